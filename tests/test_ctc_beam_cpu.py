"""Two-pass decoding, host side (no GPU): the reference prefix beam search (tests/ctc_beam_ref.py) against brute-force
enumeration of all frame paths and against torch's CTC likelihood, its dtype parameter, the argument validation of
the new entry points and the Python argument errors."""
import math

import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R

ERR_ARG = -1
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _logits(T, V, seed, scale=2.0):
    return (scale * torch.randn(T, V, generator=torch.Generator().manual_seed(seed))).numpy()


@pytest.mark.parametrize("T,V,W", [(3, 3, 16), (4, 4, 200)])
def test_reference_is_exact_when_every_prefix_fits(T, V, W):
    """V = 3, T = 3: all 9 reachable prefixes fit into W = 16, so every final score is the sum over the 27 enumerated
    paths; V = 4, T = 4 with W above the prefix count likewise.  Nothing is pruned, so the scores also sum to 1."""
    x = _logits(T, V, 10 + T)
    want = R.enumerate_paths(x, 0)
    r = R.prefix_beam(x, W, 0, T)
    assert len(r["prefixes"]) == len(want) == len(set(r["prefixes"]))
    if (T, V) == (3, 3):
        assert len(want) == 9
    worst = 0.0
    for g, s in zip(r["prefixes"], r["scores"]):
        worst = max(worst, abs(math.exp(float(s)) - want[g]))
    print(f"T {T} V {V}: worst error against enumeration {worst:.2e}, merges {r['merges']}")
    assert worst <= 1e-12
    assert abs(sum(math.exp(float(s)) for s in r["scores"]) - 1.0) <= 1e-12
    assert list(r["scores"]) == sorted(r["scores"], reverse=True) and r["merges"] > 0


@pytest.mark.parametrize("seed", range(4))
def test_best_score_is_the_ctc_likelihood(seed):
    """With nothing pruned the best hypothesis's score is -F.ctc_loss of its labels in fp64."""
    T, V = 5, 4
    x = _logits(T, V, seed, 1.5)
    r = R.prefix_beam(x, 1000, 0, T)
    g = r["prefixes"][0]
    lp = torch.log_softmax(torch.from_numpy(x).double(), dim=-1).unsqueeze(1)
    tg = torch.tensor([list(g) + [0] * (T - len(g))], dtype=torch.int64)
    nll = torch.nn.functional.ctc_loss(lp, tg, torch.tensor([T]), torch.tensor([len(g)]), blank=0, reduction="sum")
    assert abs(float(r["scores"][0]) + float(nll)) <= 1e-10, (g, float(r["scores"][0]), float(nll))


def test_reference_rules_max_labels_frames_and_empty_input():
    x = _logits(6, 5, 3)
    r = R.prefix_beam(x, 8, 0, 2)
    assert max(len(g) for g in r["prefixes"]) == 2                  # the cap binds
    assert R.prefix_beam(x, 8, 0, 2, frames=3)["prefixes"] == R.prefix_beam(x[:3], 8, 0, 2)["prefixes"]
    e = R.prefix_beam(x, 8, 0, 2, frames=0)
    assert e["prefixes"] == [()] and float(e["scores"][0]) == 0.0
    one = R.prefix_beam(x[:1], 8, 0, 4)                             # first frame: 5 live candidates for 8 slots
    assert len(one["prefixes"]) == 5 and one["prefixes"][0] in [(), (1,), (2,), (3,), (4,)]


def test_reference_tie_rule_is_the_flat_index():
    """A frame of equal logits: the stay (w = 0, column blank = 2) and the extensions tie; the flat index decides."""
    x = np.zeros((1, 5))
    r = R.prefix_beam(x, 3, 2, 4)
    assert r["prefixes"] == [(0,), (1,), ()]
    assert r["boundary"] == 0.0


def test_reference_dtype_parameter_gives_the_fp32_error():
    x = _logits(40, 30, 7, 1.0)
    x[:, 0] += 2.0
    a = R.prefix_beam(x, 4, 0, 63)
    b = R.prefix_beam(x, 4, 0, 63, dtype=np.float32)
    assert b["renorm"].dtype == np.float32 and a["renorm"].dtype == np.float64
    assert a["prefixes"] == b["prefixes"]
    err = float(np.abs(a["scores"] - b["scores"]).max())
    print(f"fp32 reference error {err:.2e}")
    assert 0.0 < err < 1e-3
    sel, out = R.bounds([a], [b])
    assert sel >= 1e-5 and out(-200.0) >= 2e-3


def test_recreation_cases_need_identity_by_labels():
    """The GPU cases marked `recreate`: the reference re-creates a pruned prefix whose child stayed in the beam, and a
    search that knew prefixes by the node of their first selection (identity="node") gives other hypotheses, or
    scores further off than 10 x the case's score bound.  So those cases fail for a kernel with that shortcut."""
    from tests import test_gpu_ctc_beam_kernels as G
    assert len(G.RECREATE_CASES) >= 2
    for i in G.RECREATE_CASES:
        c, x, r64, (sel, out_bound) = G.case(i)
        assert r64[0]["recreated"] > 0
        nd = R.prefix_beam(x[0, :, :c["V"]].numpy(), c["W"], G.BLANK, c["ml"], identity="node")
        if nd["prefixes"] == r64[0]["prefixes"]:
            gap = np.abs(nd["scores"] - r64[0]["scores"])
            assert any(g > 10 * out_bound(float(v)) for g, v in zip(gap, r64[0]["scores"])), i
    plain = R.prefix_beam(_logits(6, 5, 3), 8, 0, 4)
    assert plain["prefixes"] == R.prefix_beam(_logits(6, 5, 3), 8, 0, 4, identity="node")["prefixes"]


# ------------------------------------------------------------------------------------------------ C-ABI

def _beam_args(**kw):
    a = dict(logits=P0, B=2, T=9, V=10, ld=16, input_lengths=None, blank=0, W=4, max_labels=7, ws=P0 + 0x1000,
             ws_words=1 << 20, tok=P0 + 0x100000, len=P0 + 0x200000, score=P0 + 0x300000, n_hyp=P0 + 0x400000,
             stream=None)
    a.update(kw)
    return list(a.values())


def test_abi_version_and_symbols():
    import asrx
    from asrx._lib import SIGNATURES
    lib = asrx.native()
    assert lib.asrx_version() >= 7
    for name in ("asrx_ctc_prefix_beam", "asrx_hyp_tokens", "asrx_seq_logprob", "asrx_rescore_rank"):
        assert getattr(lib, name) is not None and name in SIGNATURES
    assert lib.asrx_ctc_prefix_beam(*_beam_args(B=0)) == 0


@pytest.mark.parametrize("bad", [dict(W=0), dict(W=17), dict(T=0), dict(T=-2), dict(blank=-1), dict(blank=10),
                                 dict(max_labels=0), dict(V=0), dict(ld=9), dict(B=-1), dict(logits=None),
                                 dict(ws=None), dict(ws=P0 + 0x1002), dict(ws_words=2 * 9 * 25 - 1), dict(tok=None),
                                 dict(len=None), dict(score=None), dict(n_hyp=None)])
def test_prefix_beam_rejects_bad_arguments_without_gpu(bad):
    """Also the workspace rule: B * T * (6 W + 1) words."""
    import asrx
    assert asrx.native().asrx_ctc_prefix_beam(*_beam_args(**bad)) == ERR_ARG


def test_rescoring_kernels_reject_bad_arguments_without_gpu():
    import asrx
    lib = asrx.native()
    tok = dict(tok=P0, ld_tok=7, len=P0 + 0x100, n_hyp=None, B=2, W=4, L=8, bos=1, eos=2, pad=0, ignore=-1,
               dec_in=P0 + 0x1000, dec_tgt=P0 + 0x2000, mask=P0 + 0x3000, stream=None)
    for bad in (dict(tok=None), dict(len=None), dict(dec_in=None), dict(mask=None), dict(W=0), dict(W=17), dict(L=0),
                dict(ld_tok=0), dict(B=-1)):
        assert lib.asrx_hyp_tokens(*{**tok, **bad}.values()) == ERR_ARG, bad
    assert lib.asrx_hyp_tokens(*{**tok, **dict(B=0)}.values()) == 0
    lp = dict(logits=P0, N=8, L=4, V=10, ld=16, tgt=P0 + 0x1000, ignore=-1, n_hyp=None, W=1, out=P0 + 0x2000,
              stream=None)
    for bad in (dict(logits=None), dict(tgt=None), dict(out=None), dict(L=0), dict(V=0), dict(ld=9), dict(N=-1),
                dict(n_hyp=P0 + 0x3000, W=3), dict(n_hyp=P0 + 0x3000, W=0)):
        assert lib.asrx_seq_logprob(*{**lp, **bad}.values()) == ERR_ARG, bad
    assert lib.asrx_seq_logprob(*{**lp, **dict(N=0)}.values()) == 0
    rk = dict(att=P0, ctc=P0 + 0x100, B=2, W=4, att_weight=1.0, ctc_weight=0.5, score=P0 + 0x200, order=P0 + 0x300,
              stream=None)
    for bad in (dict(att=None), dict(ctc=None), dict(score=None), dict(order=None), dict(W=0), dict(W=17),
                dict(att_weight=float("nan")), dict(ctc_weight=float("nan")), dict(B=-1)):
        assert lib.asrx_rescore_rank(*{**rk, **bad}.values()) == ERR_ARG, bad
    assert lib.asrx_rescore_rank(*{**rk, **dict(B=0)}.values()) == 0


# ------------------------------------------------------------------------------------------------ Python arguments

def _model(ctc):
    import asrx
    return asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=ctc)


def test_two_pass_argument_errors():
    """Raised before anything touches a device: no CTC head, a beam outside 1..16, nbest above the beam, a negative
    weight."""
    spectrum = torch.zeros(2, 1, 8, 20)
    with pytest.raises(RuntimeError):
        _model(False).ctc_beam_search(spectrum)
    with pytest.raises(RuntimeError):
        _model(False).rescore(spectrum)
    with pytest.raises(ValueError):
        _model(True).rescore(spectrum, beam=17)
    with pytest.raises(ValueError):
        _model(True).rescore(spectrum, beam=4, nbest=5)
    with pytest.raises(ValueError):
        _model(True).rescore(spectrum, ctc_weight=-0.5)
    dec = _model(True).decoder
    with pytest.raises(RuntimeError):
        dec.rescore(torch.zeros(2, 4, 16), None)
    with pytest.raises(ValueError):
        dec.rescore(torch.zeros(2, 4, 16), (torch.zeros(8, 64), 4, 0, None), beam=0)


def test_rescore_result_is_a_beam_result():
    import asrx
    t = torch.zeros(1, 1, 3, dtype=torch.int64)
    r = asrx.RescoreResult(t, t[:, :, 0], t[:, :, 0].float(), "a", "c")
    assert isinstance(r, asrx.BeamResult) and len(r) == 3 and r.tokens is t
    assert r.att_scores == "a" and r.ctc_scores == "c"
    tokens, lengths, scores = r
    assert scores is r.scores
