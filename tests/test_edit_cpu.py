"""Edit distance and MBR ranking, host side (no GPU): the reference (tests/edit_ref.py) against an exhaustive recursion
over all alignments and against asrx.new.train._edit_distance, the rule that fixes the counts, the kernel's blocked
wavefront schedule replayed on the host, the argument validation of asrx_edit_distance and asrx_mbr_rank, the
arithmetic of ErrorRate.compute and the Python argument errors."""
import itertools
import math
import random

import numpy as np
import pytest
import torch

from tests import edit_ref as R

ERR_ARG = -1
P0 = 0x10000   # never dereferenced: validation returns before any launch
PAIRS, GROUP, CROSS = 0, 1, 2


# ------------------------------------------------------------------------------------------------ reference

def test_reference_is_the_exhaustive_optimum():
    """Every pair of strings of length <= 4 over a 3-letter alphabet (121^2 = 14 641 pairs): the packed-key DP returns
    the lexicographic minimum of (edits, substitutions) over all alignments, with its deletions and insertions."""
    strs = [s for n in range(5) for s in itertools.product(range(3), repeat=n)]
    assert len(strs) ** 2 == 14641
    for a in strs:
        for b in strs:
            got = R.align(a, b)
            assert got[:4] == R.exhaustive(a, b), (a, b)
            assert got[4] == len(b) and got[0] == got[1] + got[2] + got[3] and got[3] - got[2] == len(a) - len(b)


def test_reference_distance_equals_the_host_metric():
    from asrx.new.train import _edit_distance
    rng = random.Random(5)
    for _ in range(200):
        V = rng.choice((2, 5, 50))
        a = [rng.randrange(V) for _ in range(rng.randrange(0, 40))]
        b = [rng.randrange(V) for _ in range(rng.randrange(0, 40))]
        assert R.align(a, b)[0] == _edit_distance(a, b) == R.plain_distance(a, b)


def test_rule_is_an_optimum_not_a_backtrace_order():
    """hyp (a, b) against ref (b, c): 2 edits either as two substitutions or as one deletion and one insertion around
    the match of b; fewest substitutions decides.  A diagonal-first backtrace would answer 2 substitutions."""
    a, b, c = 7, 8, 9
    assert R.align([a, b], [b, c]) == (2, 0, 1, 1, 2)
    assert R.align([b, c], [a, b]) == (2, 0, 1, 1, 2)
    assert R.align([a], [b]) == (1, 1, 0, 0, 1)          # nothing to match: the substitution stays
    assert R.align([], []) == (0, 0, 0, 0, 0) and R.align([a, a], []) == (2, 0, 0, 2, 0)
    assert R.align([], [a, b, c]) == (3, 0, 3, 0, 3)
    assert R.align([1] * 256, [1]) == (-2, -1, -1, -1, -1) and R.align([1] * 255, [1])[0] == 254


def test_sequence_rule():
    row = [1, 5, 4, 6, 2, 4, 4, 9]
    assert R.sequence(row) == row
    assert R.sequence(row, drop=(1, 2, 4)) == [5, 6, 9]
    assert R.sequence(row, stop=2, drop=(1, 4)) == [5, 6]
    assert R.sequence(row, stop=1) == [] and R.sequence(row, stop=-1) == row and R.sequence(row, stop=77) == row
    assert R.sequence(row, length=3) == [1, 5, 4] and R.sequence(row, length=-2) == [] and R.sequence(row, 99) == row


@pytest.mark.parametrize("V", [2, 5, 250])
def test_blocked_wavefront_schedule_equals_the_row_dp(V):
    """The kernel's decomposition (64-column blocks, one anti-diagonal per step, the boundary column carried between
    blocks) replayed lane by lane on the host."""
    rng = random.Random(V)
    lens = [0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255]
    for m, n in [(a, b) for a in lens for b in lens if (a + b) % 3 == 0 or a == b]:
        h = [rng.randrange(V) for _ in range(m)]
        r = [rng.randrange(V) for _ in range(n)]
        assert R.wavefront(h, r) == R.packed(h, r) == R.packed_rows(h, r), (m, n)


def test_reference_modes_and_absent_slots():
    hyp = np.array([[1, 2, 3], [1, 2, 0], [3, 3, 3], [1, 0, 0]])
    ref = np.array([[1, 2, 3, 0], [3, 0, 0, 0]])
    d, c = R.edit_distance(hyp, ref, drop=(0,), mode="group", W=2, n_hyp=[2, 1])
    assert d.tolist() == [0, 1, 2, -1] and c[1].tolist() == [0, 1, 0, 3] and c[3].tolist() == [-1] * 4
    d, c = R.edit_distance(hyp, drop=(0,), mode="cross", W=2, n_hyp=[2, 1])
    assert d.tolist() == [0, 1, 1, 0, 0, -1, -1, -1]
    assert c[1].tolist() == [0, 0, 1, 2] and c[2].tolist() == [0, 1, 0, 3]      # (i, j) and (j, i): del / ins swapped
    d, _ = R.edit_distance(hyp[:2], ref, drop=(0,), mode="pairs", n_hyp=[0, 0])
    assert d.tolist() == [0, 2]


def test_reference_cross_distances():
    rng = random.Random(11)
    seqs = [[rng.randrange(4) for _ in range(n)] for n in (0, 7, 7, 1, 30, 12)]
    d = R.cross_distances(seqs)
    assert d.tolist() == [[R.align(a, b)[0] for b in seqs] for a in seqs]


def test_reference_mbr():
    dist = [[0, 2, 4], [2, 0, 2], [4, 2, 0]]
    r, live = R.mbr_risk(dist, [0.0, 0.0, 0.0], scale=0.0)
    assert live.all() and np.allclose(r, [2.0, 4 / 3, 2.0]) and R.mbr_order(r) == [1, 0, 2]     # the medoid
    r, _ = R.mbr_risk(dist, [0.0, -1.0, -50.0])
    p = np.exp([0.0, -1.0, -50.0])
    p /= p.sum()
    assert np.allclose(r, np.array(dist) @ p) and R.mbr_order(r) == [0, 1, 2]
    r, live = R.mbr_risk(dist, [0.0, float("nan"), -1.0], n_hyp=3)
    assert list(live) == [True, False, True] and r[1] == math.inf and R.mbr_order(r)[-1] == 1
    r, live = R.mbr_risk(dist, [0.0, 0.0, 0.0], n_hyp=0)
    assert not live.any() and R.mbr_order(r) == [0, 1, 2]
    r32, _ = R.mbr_risk(dist, [0.3, -1.7, -2.2], dtype=np.float32)
    assert r32.dtype == np.float32
    r64, live, bnd, gap = R.mbr_check(dist, [0.3, -1.7, -2.2])
    assert (bnd >= 1e-5).all() and gap > 0 and (np.abs(r32 - r64) <= bnd).all()
    assert R.bound(0.0, 0.5) == 1e-5 and R.bound(1e-3, 1.0) == 4e-3


# ------------------------------------------------------------------------------------------------ C-ABI

def _ed(**kw):
    a = dict(hyp=P0, ld_hyp=16, hyp_cols=12, hyp_len=None, ref=P0 + 0x10000, ld_ref=8, ref_cols=8, ref_len=None, N=18,
             mode=PAIRS, W=1, n_hyp=None, drop=None, ndrop=0, stop_id=-1, dist=P0 + 0x20000, counts=None, stream=None)
    a.update(kw)
    if a["drop"] is not None:
        import ctypes
        a["drop"] = (ctypes.c_int64 * 4)(*a["drop"])
    return list(a.values())


def _mbr(**kw):
    a = dict(dist=P0, score=P0 + 0x1000, n_hyp=None, B=2, W=4, scale=1.0, risk=P0 + 0x2000, order=P0 + 0x3000,
             stream=None)
    a.update(kw)
    return list(a.values())


def test_abi_version_and_symbols():
    import asrx
    from asrx._lib import ED_CROSS, ED_GROUP, ED_PAIRS, SIGNATURES
    lib = asrx.native()
    assert lib.asrx_version() >= 9
    for name in ("asrx_edit_distance", "asrx_mbr_rank"):
        assert getattr(lib, name) is not None and name in SIGNATURES
    assert len(SIGNATURES["asrx_edit_distance"]) == len(_ed()) and len(SIGNATURES["asrx_mbr_rank"]) == len(_mbr())
    assert (ED_PAIRS, ED_GROUP, ED_CROSS) == (PAIRS, GROUP, CROSS)


@pytest.mark.parametrize("bad", [
    dict(N=0), dict(N=-4), dict(hyp_cols=0), dict(hyp_cols=-1), dict(ref_cols=0), dict(ld_hyp=11), dict(ld_ref=7),
    dict(ndrop=-1), dict(ndrop=5, drop=(1, 2, 3, 4)), dict(ndrop=1, drop=None), dict(hyp=None), dict(dist=None),
    dict(ref=None), dict(ref=None, mode=GROUP, W=3), dict(mode=GROUP, W=0), dict(mode=GROUP, W=-2),
    dict(mode=GROUP, W=4), dict(mode=CROSS, W=0), dict(mode=CROSS, W=17, N=17 * 17), dict(mode=CROSS, W=2),
    dict(mode=CROSS, W=3, hyp=None), dict(mode=3), dict(mode=-1)])
def test_edit_distance_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_edit_distance(*_ed(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(scale=-0.5), dict(scale=float("nan")), dict(W=0), dict(W=17), dict(B=0),
                                 dict(B=-1), dict(dist=None), dict(score=None), dict(risk=None), dict(order=None)])
def test_mbr_rank_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_mbr_rank(*_mbr(**bad)) == ERR_ARG


# ------------------------------------------------------------------------------------------------ Python layers

def test_error_rate_arithmetic_on_host_records():
    from asrx.score import reduce_counts
    # update 0: 1-best only, 3 samples; update 1: 3-best, 2 samples, the second with one absent slot
    d0 = torch.tensor([[0], [2], [1]])
    c0 = torch.tensor([[[0, 0, 0, 4]], [[1, 1, 0, 5]], [[0, 0, 1, 3]]])
    d1 = torch.tensor([[3, 1, 2], [0, 4, -1]])
    c1 = torch.tensor([[[2, 1, 0, 6], [1, 0, 0, 6], [0, 1, 1, 6]], [[0, 0, 0, 2], [0, 0, 4, 2], [-1, -1, -1, -1]]])
    r = reduce_counts([(d0, c0)])
    assert r["n_edits"] == 3 and r["n_ref"] == 12 and r["ter"] == 3 / 12 and r["ser"] == 2 / 3
    assert (r["n_sub"], r["n_del"], r["n_ins"]) == (1, 1, 1) and r["sub"] == 1 / 12 and "oracle_ter" not in r
    r = reduce_counts([(d0, c0), (d1, c1)])
    assert r["n_edits"] == 6 and r["n_ref"] == 20 and r["ter"] == 6 / 20 and r["n_samples"] == 5 and r["n_wrong"] == 3
    assert (r["n_sub"], r["n_del"], r["n_ins"]) == (3, 2, 1) and r["del"] == 2 / 20 and r["ins"] == 1 / 20
    assert r["n_oracle_edits"] == 3 + 1 + 0 and r["oracle_ter"] == 4 / 20 <= r["ter"] and r["ser"] == 3 / 5
    e = reduce_counts([(torch.tensor([[0]]), torch.tensor([[[0, 0, 0, 0]]]))])
    assert math.isnan(e["ter"]) and e["ser"] == 0.0                       # no reference tokens: nan, as the WER
    assert math.isnan(reduce_counts([])["ter"])
    with pytest.raises(ValueError, match="sample 4 .*255"):
        reduce_counts([(d0, c0), (torch.tensor([[1, 0], [0, -2]]), -torch.ones(2, 2, 4, dtype=torch.long))])
    with pytest.raises(ValueError, match="sample 1 .*no hypothesis"):
        reduce_counts([(torch.tensor([[1], [-1]]), torch.zeros(2, 1, 4, dtype=torch.long))])


def test_python_argument_errors_and_types():
    import asrx
    t = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="mode"):
        asrx.edit_distance(t, t, mode="all")
    with pytest.raises(ValueError, match="four"):
        asrx.edit_distance(t, t, drop=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="four"):
        asrx.ErrorRate((1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="pairs"):
        asrx.edit_distance(t, torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="cross"):
        asrx.edit_distance(t, mode="cross")
    with pytest.raises(ValueError, match="1..16"):
        asrx.edit_distance(torch.zeros(1, 17, 3, dtype=torch.int64), mode="cross")
    r = asrx.BeamResult(torch.zeros(2, 3, 4, dtype=torch.int64), torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="mbr_scale"):
        asrx.mbr_rerank(r, scale=-1.0)
    with pytest.raises(ValueError, match="mbr_scale"):
        asrx.mbr_rerank(r, scale=float("nan"))
    assert asrx.EditCounts._fields == ("dist", "sub", "dele", "ins", "ref_len")
    z = torch.zeros(1)
    assert asrx.RescoreResult(z, z, z).risks is None and asrx.RescoreResult(z, z, z, z, z, z).risks is z
    assert isinstance(asrx.MbrResult(z, z, z, z), asrx.BeamResult) and asrx.MbrResult(z, z, z, z).risks is z


def test_token_drop_ids_and_mbr_scale_validation():
    import asrx
    m = asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=True)
    assert m.token_drop_ids() == (1, 2, 4) and m.token_drop_ids(bos_token_id=3) == (3, 2, 4)
    m = asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=True, ctc_blank=0)
    assert m.token_drop_ids() == (1, 2, 4, 0)
    m2 = asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=False, ctc_blank=0)
    assert m2.token_drop_ids() == (1, 2, 4)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="mbr_scale"):
            m.decoder.rescore(torch.zeros(1, 4, 16), (torch.zeros(4, 64), 4, 0, None), mbr_scale=bad)
