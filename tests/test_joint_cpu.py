"""Joint CTC/attention beam search, host side (no GPU): the reference prefix scorer (tests/joint_ref.py) against
brute-force enumeration of all paths and against torch's CTC likelihood, the argument validation of the new entry
points, and the Python argument errors."""
import itertools
import math

import pytest
import torch

from tests import ctc_ref, joint_ref

INF = float("inf")
ERR_ARG = -1
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _walk(lp, Tb, labels, blank, eos):
    """(log psi, end score, state) of a label sequence by score / advance from the root (one sample, W = 1)."""
    lpb = lp.unsqueeze(0)
    st = joint_ref.root_state(lpb, [Tb], 1, blank)
    zero = torch.zeros(1, dtype=torch.uint8)
    for c in labels:
        st = joint_ref.prefix_advance(lpb, [Tb], st, 1, torch.zeros(1, dtype=torch.int64), torch.tensor([c]), zero,
                                      blank, eos)
    return st, joint_ref.prefix_score(lpb, [Tb], st, 1, blank, eos)[0]


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_prefix_scorer_matches_enumeration_of_all_paths(T):
    """V = 4 (blank 0, labels 1..3; no EOS column, the end score is taken on its own), T <= 5, every prefix of up
    to 3 labels, repeats included: psi of every prefix, of each of its continuations, and its end probability."""
    V, blank, eos = 4, 0, -1
    lp = joint_ref.log_probs(2 * torch.randn(1, T, V, generator=torch.Generator().manual_seed(T)))[0]
    psi, end = joint_ref.brute_force_prefix(lp, blank)
    worst = 0.0
    labels = (1, 2, 3)
    prefixes = [()] + [p for n in (1, 2, 3) for p in itertools.product(labels, repeat=n)]
    for g in prefixes:
        st, delta = _walk(lp, T, g, blank, eos)
        ends = joint_ref.end_score([T], st, 1)
        want_psi = psi.get(g, 0.0)
        got_psi = math.exp(float(st.logpsi[0]))
        worst = max(worst, abs(got_psi - want_psi))
        assert abs(got_psi - want_psi) <= 1e-12, (g, got_psi, want_psi)
        assert float(delta[blank]) == -INF
        if want_psi == 0.0:
            assert bool((delta == -INF).all()), g
            continue
        got_end = math.exp(float(ends[0])) * want_psi
        assert abs(got_end - end.get(g, 0.0)) <= 1e-12, (g, got_end, end.get(g, 0.0))
        for c in labels:
            got = math.exp(float(delta[c])) * want_psi
            want = psi.get(g + (c,), 0.0)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-12, (g, c, got, want)
            assert (float(delta[c]) == -INF) == (want == 0.0)
    print(f"T {T}: worst error against enumeration {worst:.2e}")


@pytest.mark.parametrize("seed", range(6))
def test_scores_telescope_to_the_ctc_likelihood(seed):
    """Random label sequences (repeats likely at V = 6): the sum of delta along the sequence plus the EOS term is
    -nll of torch's fp64 CTC, within 1e-10; one sample uses fewer frames than the table has."""
    g = torch.Generator().manual_seed(seed)
    V, blank, eos, T = 6, 0, 1, 12 + seed
    logits = 2 * torch.randn(1, T, V, generator=g)
    L = int(torch.randint(0, 7, (1,), generator=g))
    labels = (torch.randint(2, V, (L,), generator=g)).tolist()
    Tb = T - 3 if seed == 2 else T
    got = joint_ref.sequence_ctc_score(joint_ref.log_probs(logits)[0], Tb, labels, blank, eos)
    tg = torch.tensor([labels + [blank] * (7 - L)])
    nll, _ = ctc_ref.ctc_reference(logits, tg, torch.tensor([Tb]), torch.tensor([L]), blank)
    assert math.isfinite(float(nll[0]))
    assert abs(got + float(nll[0])) <= 1e-10, (labels, got, float(nll[0]))


def test_infeasible_sequence_scores_minus_infinity_not_nan():
    """Five labels with a repeat over four frames, and anything over no frames at all."""
    V, blank, eos = 5, 0, 1
    lp = joint_ref.log_probs(torch.randn(1, 4, V, generator=torch.Generator().manual_seed(0)))[0]
    assert joint_ref.sequence_ctc_score(lp, 4, [2, 3, 3, 4], blank, eos) == -INF     # needs 5 frames
    assert joint_ref.sequence_ctc_score(lp, 4, [2, 3, 4, 2, 3], blank, eos) == -INF
    assert math.isfinite(joint_ref.sequence_ctc_score(lp, 4, [2, 3, 4, 2], blank, eos))
    st, delta = _walk(lp, 0, (), blank, eos)
    assert float(delta[eos]) == 0.0 and bool((delta[[0, 2, 3, 4]] == -INF).all())
    st, delta = _walk(lp, 4, (2, 3, 3, 4), blank, eos)
    assert float(st.logpsi[0]) == -INF and bool((delta == -INF).all()) and not bool(torch.isnan(st.nb).any())


def test_joint_step_reduces_to_beam_step():
    from tests import beam_ref
    g = torch.Generator().manual_seed(4)
    B, W, V = 2, 3, 7
    logits = torch.randn(B, W, V, generator=g)
    score = torch.randn(B, W, generator=g)
    fin = torch.tensor([[False, True, False], [False, False, False]])
    length = torch.ones(B, W, dtype=torch.int64)
    a = beam_ref.beam_step(logits, score, fin, length, 2, V)
    b = joint_ref.joint_step(logits, torch.zeros(B, W, V), 1.0, 0.0, score, fin, length, 2, V)
    for k in ("score", "tok", "parent", "fin", "len"):
        assert torch.equal(a[k], b[k]), k
    extra = torch.full((B, W, V), -INF)
    extra[:, 2, 5] = 0.0
    c = joint_ref.joint_step(logits, extra, 0.5, 0.5, score, fin, length, 2, V)
    assert c["tok"][1, 0] == 5 and c["parent"][1, 0] == 2       # the one candidate the second term allows
    assert c["parent"][0].tolist()[:2] in ([1, 2], [2, 1]) and c["tok"][0, c["parent"][0].tolist().index(1)] == 2


# ------------------------------------------------------------------------------------------------ C-ABI

def _init_args(**kw):
    a = dict(logits=P0, B=2, W=4, T=9, V=10, ld=16, input_lengths=None, blank=0, logp=P0 + 0x1000, frames=P0 + 0x2000,
             state=P0 + 0x3000, logpsi=P0 + 0x4000, last=P0 + 0x5000, stream=None)
    a.update(kw)
    return list(a.values())


def _score_args(**kw):
    a = dict(logp=P0, frames=P0 + 0x1000, B=2, W=4, T=9, V=10, blank=0, eos=2, state=P0 + 0x2000, logpsi=P0 + 0x3000,
             last=P0 + 0x4000, delta=P0 + 0x5000, ld_delta=16, stream=None)
    a.update(kw)
    return list(a.values())


def _advance_args(**kw):
    a = dict(logp=P0, frames=P0 + 0x1000, B=2, W=4, T=9, V=10, blank=0, eos=2, parent=P0 + 0x2000, tok=P0 + 0x3000,
             fin_prev=P0 + 0x4000, state_in=P0 + 0x10000, logpsi_in=P0 + 0x20000, last_in=P0 + 0x30000,
             state_out=P0 + 0x40000, logpsi_out=P0 + 0x50000, last_out=P0 + 0x60000, stream=None)
    a.update(kw)
    return list(a.values())


def _joint_args(**kw):
    a = dict(logits=P0, B=2, W=4, V=10, ld=16, extra=P0 + 0x1000, ld_extra=16, att_weight=0.7, extra_weight=0.3,
             score_in=P0 + 0x100, fin_in=P0 + 0x200, len_in=P0 + 0x300, eos=2, score_out=P0 + 0x400,
             tok_out=P0 + 0x500, cur=None, parent_out=P0 + 0x600, src_row_out=P0 + 0x700, fin_out=P0 + 0x800,
             len_out=P0 + 0x900, n_live=None, stream=None)
    a.update(kw)
    return list(a.values())


BAD_COMMON = [dict(blank=-1), dict(blank=10), dict(W=0), dict(W=17), dict(T=0), dict(T=-3), dict(V=0), dict(B=-1)]


def test_abi_version_and_symbols():
    import asrx
    lib = asrx.native()
    assert lib.asrx_version() >= 6
    for name in ("asrx_ctc_prefix_init", "asrx_ctc_prefix_score", "asrx_ctc_prefix_advance", "asrx_beam_step_joint"):
        assert getattr(lib, name) is not None
    assert lib.asrx_ctc_prefix_init(*_init_args(B=0)) == 0
    assert lib.asrx_ctc_prefix_score(*_score_args(B=0)) == 0
    assert lib.asrx_ctc_prefix_advance(*_advance_args(B=0)) == 0
    assert lib.asrx_beam_step_joint(*_joint_args(B=0)) == 0


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(ld=9), dict(logits=None), dict(logp=None), dict(frames=None),
                                              dict(state=None), dict(state=P0 + 0x3004), dict(logpsi=None),
                                              dict(last=None)])
def test_prefix_init_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_ctc_prefix_init(*_init_args(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(eos=-1), dict(eos=10), dict(eos=0), dict(ld_delta=9),
                                              dict(logp=None), dict(frames=None), dict(state=None),
                                              dict(logpsi=None), dict(last=None), dict(delta=None)])
def test_prefix_score_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_ctc_prefix_score(*_score_args(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(eos=-1), dict(eos=10), dict(eos=0), dict(parent=None),
                                              dict(tok=None), dict(fin_prev=None), dict(state_in=None),
                                              dict(state_out=None), dict(logpsi_out=None), dict(last_out=None),
                                              dict(state_out=P0 + 0x10000), dict(state_out=P0 + 0x10008),
                                              dict(logpsi_out=P0 + 0x20000), dict(last_out=P0 + 0x30000)])
def test_prefix_advance_rejects_bad_arguments_without_gpu(bad):
    """Besides the ranges: the output set must not overlap the input set (the caller ping-pongs)."""
    import asrx
    assert asrx.native().asrx_ctc_prefix_advance(*_advance_args(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(extra=None), dict(ld_extra=9), dict(att_weight=float("nan")),
                                 dict(extra_weight=float("nan")), dict(W=0), dict(W=17), dict(eos=10), dict(eos=-1),
                                 dict(V=0), dict(ld=9), dict(logits=None), dict(score_out=P0 + 0x100)])
def test_beam_step_joint_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_beam_step_joint(*_joint_args(**bad)) == ERR_ARG


# ------------------------------------------------------------------------------------------------ Python arguments

def _model(ctc):
    import asrx
    return asrx.Transformer(30, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=ctc)


def test_beam_search_argument_errors():
    """Raised before anything touches a device: ctc_weight outside [0, 1], ctc_weight > 0 without a head, a prompt
    of more than one token under ctc_weight > 0."""
    spectrum = torch.zeros(2, 1, 8, 20)
    with pytest.raises(ValueError):
        _model(True).beam_search(spectrum, ctc_weight=1.5)
    with pytest.raises(ValueError):
        _model(False).beam_search(spectrum, ctc_weight=-0.1)
    with pytest.raises(RuntimeError):
        _model(False).beam_search(spectrum, ctc_weight=0.3)
    with pytest.raises(ValueError):
        _model(True).beam_search(spectrum, torch.ones(2, 3, dtype=torch.int64), ctc_weight=0.3)
    dec = _model(True).decoder
    enc = torch.zeros(2, 4, 16)
    with pytest.raises(ValueError):
        dec.beam_search(torch.ones(2, 1, dtype=torch.int64), enc, ctc_weight=2.0)
    with pytest.raises(RuntimeError):
        dec.beam_search(torch.ones(2, 1, dtype=torch.int64), enc, ctc_weight=0.5)          # no head logits given
    with pytest.raises(ValueError):
        dec.beam_search(torch.ones(2, 2, dtype=torch.int64), enc, ctc_weight=0.5, ctc=(enc, 4, 0, None))
