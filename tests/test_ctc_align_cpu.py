"""Forced alignment, host side (no GPU): the reference Viterbi recursion (tests/ctc_align_ref.py) against brute-force
enumeration of all frame paths, its tie rule, margin and dtype parameter, the argument validation of asrx_ctc_align,
its workspace rule, frame_span against `subsampled`, and the Python argument errors."""
import math

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R

ERR_ARG, ERR_UNSUPPORTED = -1, -3
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _logits(T, V, seed, scale=2.0):
    return (scale * torch.randn(T, V, generator=torch.Generator().manual_seed(seed))).numpy()


@pytest.mark.parametrize("T,V,target", [(5, 4, (1, 2)), (5, 3, (1, 1)), (4, 4, (3, 1, 3)), (5, 4, ()), (3, 3, (2,)),
                                        (1, 3, (1,)), (5, 3, (2, 2, 1)), (4, 3, (1, 2, 1, 2))])
@pytest.mark.parametrize("seed", range(3))
def test_reference_finds_the_brute_force_maximum(T, V, target, seed):
    """Every one of the V^T paths is enumerated: the reference's score is the maximum over those that collapse to the
    target, and its path is the maximising one (random logits: the maximum is unique)."""
    x = _logits(T, V, 100 * T + 10 * V + seed)
    want, paths = R.brute_force(x, target, 0)
    r = R.viterbi(x, target, 0)
    assert r["feasible"] and abs(r["score"] - want) <= 1e-12
    assert len(paths) == 1 and R.symbols_of(r["frame_pos"], target, 0, T) == paths[0]
    assert R.path_is_valid(r["frame_pos"], target, T)
    total, flp = R.rescore(x, target, 0, r["frame_pos"], T)
    assert abs(total - want) <= 1e-12 and np.allclose(flp, r["frame_logp"], atol=1e-14)
    for u in range(len(target)):
        run = r["frame_logp"][r["start"][u]:r["end"][u]]
        assert r["end"][u] > r["start"][u] and abs(r["conf"][u] - math.exp(run.mean())) <= 1e-12
        assert u == 0 or r["start"][u] >= r["end"][u - 1]


def test_reference_infeasible_and_malformed():
    x = _logits(5, 4, 1)
    assert R.brute_force(x[:2], (1, 1), 0) == (-math.inf, [])
    r = R.viterbi(x[:2], (1, 1), 0)                    # T = 2 < L + repeats = 3
    assert not r["feasible"] and r["score"] == -math.inf
    assert (r["frame_pos"] == -1).all() and (r["frame_logp"] == 0).all() and (r["start"] == -1).all()
    assert R.viterbi(x[:3], (1, 1), 0)["feasible"]     # exactly L + repeats: the single alignment 1 blank 1
    assert R.symbols_of(R.viterbi(x[:3], (1, 1), 0)["frame_pos"], (1, 1), 0, 3) == (1, 0, 1)
    assert not R.viterbi(x, (1, 2, 3), 0, frames=2)["feasible"]
    assert not R.viterbi(x, (1,), 0, frames=0)["feasible"]
    e = R.viterbi(x, (), 0, frames=0)
    assert e["feasible"] and e["score"] == 0.0 and (e["frame_pos"] == -1).all()
    for bad in ((0,), (4,), (-1,)):                    # the blank, V, negative
        assert not R.viterbi(x, bad, 0)["feasible"]
    assert not R.viterbi(x, (1, 2), 0, lmax=1)["feasible"]
    part = R.viterbi(x, (2,), 0, frames=3, lmax=4)
    assert (part["frame_pos"][3:] == -1).all() and (part["frame_logp"][3:] == 0).all() and part["start"][1] == -1


def test_reference_tie_rule():
    """Equal logits everywhere: every reachable transition ties.  The end is the last label state (the final blank
    is not strictly greater), and going back every state stays while its own predecessor is reachable: the last label
    stretches back to the first frame it can hold, which it enters by the only finite predecessor."""
    x = np.zeros((6, 4), np.float32)
    r = R.viterbi(x, (1, 2), 0)
    assert list(r["frame_pos"]) == [0, 1, 1, 1, 1, 1] and r["margin"] == 0.0
    r = R.viterbi(x, (1, 1), 0)
    assert list(r["frame_pos"]) == [0, -1, 1, 1, 1, 1]
    # a skip that merely ties with the stay is not taken: at t = 2 label 2 stays, though the skip from label 1 and
    # the step from the blank are as good
    x = np.zeros((3, 4), np.float32)
    x[0, 1] = 1.0
    r = R.viterbi(x, (1, 2), 0)
    assert list(r["frame_pos"]) == [0, 1, 1]
    assert R.brute_force(x, (1, 2), 0)[0] == pytest.approx(r["score"], abs=1e-12)


def test_reference_dtype_parameter_margin_and_bound():
    target = [1 + (i * 7) % 29 for i in range(20)]
    x = _logits(60, 30, 7, 1.0)
    x[:, 0] += 2.0
    a = R.viterbi(x, target, 0)
    b = R.viterbi(x, target, 0, dtype=np.float32)
    err = abs(a["score"] - b["score"])
    print(f"fp32 reference error {err:.2e}, margin {a['margin']:.3e}")
    assert 0.0 < err < 1e-3 and a["margin"] > 0.0
    assert R.bound(err, a["score"]) >= 1e-5 * abs(a["score"]) and R.bound(0.0, 0.5) == 1e-5
    if a["margin"] > 100 * err:
        assert (a["frame_pos"] == b["frame_pos"]).all()
    y = R.planted(40, 12, [3, 3, 5, 7], 8.0, 0.5, 1)
    p = R.viterbi(y, [3, 3, 5, 7], 0)
    assert p["margin"] > 1.0 and R.path_is_valid(p["frame_pos"], [3, 3, 5, 7], 40)
    assert not R.path_is_valid([0, 1, -1, -1], [3, 3], 4) and not R.path_is_valid([0, -1, 0, 1], [3, 4], 4)
    assert not R.path_is_valid([0, 0, -1, -1], [3, 4], 4) and R.path_is_valid([0, -1, 1, -1], [3, 3], 3)


# ------------------------------------------------------------------------------------------------ C-ABI

def _args(**kw):
    a = dict(logits=P0, B=2, T=9, V=10, ld=16, targets=P0 + 0x1000, tgt_stride=8, input_lengths=None,
             target_lengths=P0 + 0x2000, max_target_len=7, blank=0, ws=P0 + 0x3000, ws_words=1 << 20,
             frame_pos=P0 + 0x100000, frame_logp=P0 + 0x200000, tok_start=P0 + 0x300000, tok_end=P0 + 0x400000,
             tok_conf=P0 + 0x500000, score=P0 + 0x600000, stream=None)
    a.update(kw)
    return list(a.values())


def test_abi_version_and_symbols():
    import asrx
    from asrx._lib import SIGNATURES
    lib = asrx.native()
    assert lib.asrx_version() >= 8
    for name in ("asrx_ctc_align", "asrx_ctc_align_workspace_words"):
        assert getattr(lib, name) is not None and name in SIGNATURES
    assert len(SIGNATURES["asrx_ctc_align"]) == len(_args())


@pytest.mark.parametrize("bad", [dict(blank=-1), dict(blank=10), dict(T=0), dict(T=-3), dict(B=0), dict(B=-1),
                                 dict(V=0), dict(ld=9), dict(max_target_len=-1), dict(tgt_stride=6),
                                 dict(logits=None), dict(targets=None), dict(target_lengths=None), dict(ws=None),
                                 dict(ws=P0 + 0x3002), dict(ws_words=2 * 2 * 9 - 1), dict(frame_pos=None),
                                 dict(frame_logp=None), dict(tok_start=None), dict(tok_end=None),
                                 dict(tok_conf=None), dict(score=None)])
def test_align_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_ctc_align(*_args(**bad)) == ERR_ARG


def test_align_rejects_long_targets_without_gpu():
    """max_target_len = 256 is unsupported whatever the pointers are; 255 with NULL pointers is a bad argument."""
    import asrx
    lib = asrx.native()
    null = dict(logits=None, targets=None, target_lengths=None, ws=None, frame_pos=None, score=None)
    assert lib.asrx_ctc_align(*_args(max_target_len=256, tgt_stride=256, **null)) == ERR_UNSUPPORTED
    assert lib.asrx_ctc_align(*_args(max_target_len=255, tgt_stride=255, **null)) == ERR_ARG
    assert lib.asrx_ctc_align(*_args(B=65536, ws_words=1 << 40)) == ERR_UNSUPPORTED


def test_workspace_rule():
    """2 B T words (row logsumexp, path states); above T = 1008 the backpointers leave LDS: 32 B T words more."""
    import asrx
    from asrx import kernels as K
    f = asrx.native().asrx_ctc_align_workspace_words
    assert f(3, 249, 64) == 2 * 3 * 249 and f(1, 1, 0) == 2
    assert f(2, 1008, 255) == 2 * 2 * 1008 and f(2, 1009, 255) == 34 * 2 * 1009
    big = f(65535, 8000, 255)
    assert big == 34 * 65535 * 8000 and big > 2 ** 32            # (an int64 result)
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, -1), (5, 5, 256), (-1, 5, 5)):
        assert f(*bad) == -1
    assert K.ctc_align_workspace_words(3, 249, 64) == 2 * 3 * 249
    with pytest.raises(RuntimeError):
        K.ctc_align_workspace_words(1, 10, 256)
    # the call checks the same rule on both sides of the switch
    lib = asrx.native()
    assert lib.asrx_ctc_align(*_args(T=1009, ws_words=34 * 2 * 1009 - 1)) == ERR_ARG
    assert lib.asrx_ctc_align(*_args(T=1008, ws_words=2 * 2 * 1008 - 1)) == ERR_ARG


# ------------------------------------------------------------------------------------------------ Python layers

def test_frame_span_against_subsampled():
    """Encoder frame j sees spectrogram frames 4j .. 4j + 6: with n spectrogram frames the last encoder frame
    subsampled(n) - 1 ends within n, and one more spectrogram frame is needed per ... 4 for the next."""
    import asrx
    assert asrx.frame_span(0, 1) == (0, 7) and asrx.frame_span(2, 5) == (8, 23)
    assert asrx.frame_span(-1, -1) == (-1, -1) and asrx.frame_span(3, 3) == (-1, -1)
    for n in range(7, 80):
        t = asrx.subsampled(n)
        first, last = asrx.frame_span(0, t)
        assert first == 0 and last <= n < last + 4, (n, t, last)
    # the receptive field, derived from the two convolutions: y1[i] sees x[2i .. 2i+2], y2[j] sees y1[2j .. 2j+2]
    for j in range(5):
        lo, hi = 2 * (2 * j), 2 * (2 * j + 2) + 2
        assert asrx.frame_span(j, j + 1) == (lo, hi + 1)
    s, e = asrx.frame_span(torch.tensor([[0, 2, -1]]), torch.tensor([[2, 3, -1]]))
    assert s.tolist() == [[0, 8, -1]] and e.tolist() == [[11, 15, -1]]


def test_alignment_result_type():
    import asrx
    t = torch.zeros(1)
    r = asrx.CtcAlignment(t, t, t, t, t, t)
    assert r._fields == ("frame_pos", "frame_logp", "start", "end", "conf", "score", "targets", "target_lengths")
    assert r.targets is None and r.score is t


def test_align_needs_a_ctc_head():
    import asrx
    m = asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=False)
    with pytest.raises(RuntimeError, match="no CTC head"):
        m.align(torch.zeros(2, 1, 8, 20), torch.ones(2, 4, dtype=torch.int64))
