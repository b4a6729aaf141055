"""Beam search, host side (no GPU): argument validation of the two entry points, the host backtrack and ranking,
and the test reference checked against exhaustive enumeration."""
import pytest
import torch

from oracle.ref_model import OracleConfig, det_params
from tests import beam_ref

ERR_ARG = -1
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _beam_args(**kw):
    a = dict(logits=P0, B=2, W=4, V=10, ld=16, score_in=P0 + 0x100, fin_in=P0 + 0x200, len_in=P0 + 0x300, eos=2,
             score_out=P0 + 0x400, tok_out=P0 + 0x500, cur=None, parent_out=P0 + 0x600, src_row_out=P0 + 0x700,
             fin_out=P0 + 0x800, len_out=P0 + 0x900, n_live=None, stream=None)
    a.update(kw)
    return list(a.values())


def _gather_args(**kw):
    a = dict(src=P0, dst=P0 + 0x100000, index=P0 + 0x200000, esize=2, outer=2, rows=6, count=8, row_stride=16,
             outer_stride=96, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(score_in=None), dict(fin_in=None), dict(len_in=None),
                                 dict(score_out=None), dict(tok_out=None), dict(parent_out=None),
                                 dict(src_row_out=None), dict(fin_out=None), dict(len_out=None), dict(W=0),
                                 dict(W=17), dict(V=0), dict(ld=9), dict(eos=10), dict(eos=-1), dict(B=-1),
                                 dict(score_out=P0 + 0x100)])
def test_beam_step_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_beam_step(*_beam_args(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(src=None), dict(dst=None), dict(index=None), dict(dst=P0), dict(esize=1),
                                 dict(esize=8), dict(rows=-1), dict(outer=-1), dict(count=17), dict(count=-1),
                                 dict(outer_stride=95), dict(dst=P0 + 64), dict(src=P0 + 1)])
def test_gather_rows_rejects_bad_arguments_without_gpu(bad):
    """src == dst, overlapping extents, a misaligned base, a count beyond the row stride: all refused up front."""
    import asrx
    assert asrx.native().asrx_gather_rows(*_gather_args(**bad)) == ERR_ARG


def test_empty_calls_succeed_without_gpu():
    import asrx
    lib = asrx.native()
    assert lib.asrx_beam_step(*_beam_args(B=0)) == 0
    assert lib.asrx_gather_rows(*_gather_args(rows=0)) == 0
    assert lib.asrx_gather_rows(*_gather_args(count=0)) == 0
    assert lib.asrx_version() >= 4


def test_backtrack_hand_written_history():
    """Three steps, W = 3, one sample.  Step 0: all from slot 0 with tokens 7 8 9.  Step 1: slots extend (1, 0, 1)
    with 5 6 4.  Step 2: slots extend (2, 2, 0) with 3 2 1."""
    from asrx.decode import beam_backtrack
    parents = torch.tensor([[[0, 0, 0]], [[1, 0, 1]], [[2, 2, 0]]], dtype=torch.int32)
    toks = torch.tensor([[[7, 8, 9]], [[5, 6, 4]], [[3, 2, 1]]])
    seqs = beam_backtrack(parents, toks)
    assert seqs.shape == (1, 3, 3)
    assert seqs[0].tolist() == [[8, 4, 3], [8, 4, 2], [8, 5, 1]]
    # two samples with different histories keep apart
    parents2 = torch.cat([parents, torch.tensor([[[0, 0, 0]], [[2, 2, 1]], [[0, 1, 1]]], dtype=torch.int32)], dim=1)
    toks2 = torch.cat([toks, toks + 10], dim=1)
    seqs2 = beam_backtrack(parents2, toks2)
    assert seqs2[0].tolist() == seqs[0].tolist()
    assert seqs2[1].tolist() == [[19, 15, 13], [19, 16, 12], [19, 16, 11]]


def test_rank_orders_by_normalised_score_and_puts_dead_last():
    from asrx.decode import beam_rank
    inf = float("inf")
    score = torch.tensor([[-4.0, -inf, -3.0, -6.0]])
    length = torch.tensor([[2, 1, 1, 4]])
    assert beam_rank(score, length, 0.0).tolist() == [[2, 0, 3, 1]]
    assert beam_rank(score, length, 1.0).tolist() == [[3, 0, 2, 1]]      # -1.5, -2, -3, dead
    assert beam_rank(torch.tensor([[-1.0, -1.0, float("nan")]]), torch.ones(1, 3), 0.0).tolist() == [[0, 1, 2]]


def test_reference_step_rules():
    """The reference step itself on a case small enough to check by eye: V = 3, W = 2, beam 1 finished."""
    logits = torch.log(torch.tensor([[[0.5, 0.25, 0.25], [0.1, 0.1, 0.8]]], dtype=torch.float64))
    score = torch.tensor([[-1.0, -1.2]], dtype=torch.float64)
    r = beam_ref.beam_step(logits, score, torch.tensor([[False, True]]), torch.tensor([[3, 2]]), 1, 3)
    # candidates: (0,0) -1.693, (0,1) -2.386, (0,2) -2.386, (1,eos) -1.2
    assert r["parent"].tolist() == [[1, 0]] and r["tok"].tolist() == [[1, 0]]
    assert r["fin"].tolist() == [[True, False]] and r["len"].tolist() == [[2, 4]]
    assert r["src_row"].tolist() == [[1, 0]] and r["n_live"] == 1
    assert abs(float(r["score"][0, 0]) + 1.2) < 1e-12
    assert abs(float(r["score"][0, 1]) + 1.0 + 0.6931471805599453) < 1e-12


def test_reference_beam_is_exhaustive_when_wide_enough():
    """V = 5, two steps, W = 25 = V**2 keeps every continuation, so the reference's best hypothesis must be the
    brute-force optimum over the oracle decoder (both with and without the final LayerNorm)."""
    cfg = OracleConfig(vocab_size=5, d_model=16, dec_len=4, n_enc=1, n_dec=1, n_heads=2, ff_dim=32)
    P = det_params(cfg, 11)
    P["decoder._classifier.weight"] = P["decoder._classifier.weight"] * 8
    enc = torch.randn(2, 6, cfg.d_model, generator=torch.Generator().manual_seed(2))
    prompt = torch.tensor([[1], [1]])
    for final_norm in (True, False):
        r = beam_ref.beam_search(P, cfg, enc, prompt, 25, 2, 2, final_norm=final_norm)
        for b in range(2):
            row, score = beam_ref.brute_force_best(P, cfg, enc[b], prompt[b], 2, 2, final_norm)
            assert r["tokens"][b, 0].tolist() == row.tolist()
            assert abs(float(r["scores"][b, 0]) - score) < 1e-9
            assert abs(beam_ref.sequence_score(P, cfg, enc[b], row, 1, 2, final_norm) - score) < 1e-9
            assert torch.all(r["scores"][b, :-1] >= r["scores"][b, 1:])
