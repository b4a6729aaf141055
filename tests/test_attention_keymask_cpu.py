"""The key-mask cases of test_gpu_attention_keymask.py, without a GPU: for every case of its table
  (a) the profiles' preconditions hold on the float64 scores of the bf16-rounded operands;
  (b) the clipped validity word, emulated in float64 (keys >= Lk - Lk % 4 masked besides), breaks check_fwd on every
      case with Lk % 4 != 0 and an utterance that has a live key in that word;
  (c) a leak, emulated in float64 (byte n_b live), breaks check_fwd on every case with a dead key;
  (d) tail_pair: a float64 backward with P, dS and O rounded to bf16 stays within half of BWD_TOL, so the bound
      measures the kernel and not the profile.
(b) and (c) are the proof that the GPU tests can fail; the unbroken reference itself passes the same check_fwd."""
import pytest
import torch

import attn_keymask_ref as M
import test_gpu_attention_peaked as P

PARAMS = [pytest.param(*c[2:], id=c[0]) for c in M.CASES]


def _breaks(tag, emu, ref):
    with pytest.raises(AssertionError):
        P.check_fwd(tag, M.as_run(emu), ref)


@pytest.mark.parametrize("profile", ["tail_spike", "tail_pair"])
@pytest.mark.parametrize("Lq,Lk,form,n,drop", PARAMS)
def test_keymask_profiles_catch_a_dropped_and_a_leaked_key(Lq, Lk, form, n, drop, profile):
    qb, kvb, valid, ref = M.reference(profile, Lq, Lk, n, form, drop)
    keep = P.keep_of(Lq, Lk, drop)
    M.check_tail(profile, ref, n, form)                                              # (a)
    P.check_fwd("float64 reference", M.as_run(ref), ref)
    if M.clipped_word_applies(Lk, n):                                                # (b)
        _breaks("clipped word", M.emulate_clipped_word(qb, kvb, valid, Lq, form, keep), ref)
    if min(n) < Lk:                                                                  # (c)
        _breaks("leaked key", M.emulate_leak(qb, kvb, valid, n, Lq, form, keep), ref)


@pytest.mark.parametrize("Lq,Lk,form,n,drop", PARAMS)
def test_keymask_tail_pair_backward_is_not_a_rounding_measurement(Lq, Lk, form, n, drop):
    qb, kvb, valid, ref, dOb, refs = M.bwd_reference(Lq, Lk, n, form, drop)          # (d)
    dO = dOb.double().view(M.B, Lq, M.H, M.DH).transpose(1, 2)
    emu = M.emulate_bwd_bf16(ref, P.keep_of(Lq, Lk, drop), dO)
    errs = M.grad_errors(emu, refs, n)
    print(f"tail_pair bf16-rounded float64 backward ({Lq}, {Lk}) n {n} {form}: " +
          ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {P.BWD_TOL / 2:g})")
    for name, e in errs.items():
        assert e <= P.BWD_TOL / 2, (name, e)


def test_case_table_covers_what_it_claims():
    """Every streamed shape has a length pair that puts a live key into the last, partial validity word."""
    for cid, variant, Lq, Lk, form, n, drop in M.CASES:
        assert len(n) == M.B and all(1 <= x <= Lk for x in n), cid
    ids = [c[0] for c in M.CASES]
    assert len(set(ids)) == len(ids)
    for s in M.SHAPES + M.DROP_SHAPES:
        if s[3] % 4:
            assert any(M.clipped_word_applies(s[3], n) for n in M.lengths_of(s[3], s[4])), s[0]
