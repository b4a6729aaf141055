"""asrx_ctc_prefix_init / _score / _advance and asrx_beam_step_joint on the GPU against tests/joint_ref.py (fp64, CPU).

Prefix kernels.  A case walks 0-4 random selections from the empty prefix (random parents, a third of the tokens the
parent's own last label, a sixth EOS), so the root, c == last(g), finished parents and dead slots (psi = 0: more
labels than frames) all occur; before every selection delta is checked for all c, after it the state and log psi.
Tolerance, per case, step and quantity: 4 x the largest error of the reference's own formulas run in fp32 on the CPU
(over the same selections) against fp64, the rule of tests/test_gpu_ctc_kernels.py, with beam_step's tolerance
1e-5 * max(1, |value|) as the floor; -inf must match exactly.  Each case prints its worst kernel-error / bound ratios
(DESIGN §10 records them).  Padding columns of delta and every input buffer must be bitwise unchanged, and a second
run of the whole walk must give the same bits.

Joint step: test_gpu_beam_kernels.py's random cases with a random second score matrix; exact selection needs the
reference's own margins (>= 1e-4, asserted per case) to exceed the kernel's error.

End to end: score -> joint step -> advance for 6 steps from the root with random attention logits; every hypothesis
equals the reference's token for token, the reference's margin being >= 10 x the case's delta bound."""
import functools
import math

import pytest
import torch

from tests import beam_ref, joint_ref
from tests.test_gpu_beam_kernels import check as check_step, make_case

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
LN2 = math.log(2.0)
EOS = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().clone()


# ------------------------------------------------------------------------------------------------ prefix kernels

def random_walk(B, W, V, blank, steps, g):
    """steps x (parent [R], tok [R]) and the flags each selection starts from; `last` is tracked so that a third of
    the tokens repeat the parent's last label."""
    R = B * W
    labels = torch.tensor([v for v in range(V) if v not in (blank, EOS)])
    last = torch.full((R,), -1, dtype=torch.int64)
    fin = torch.zeros(R, dtype=torch.bool)
    walk = []
    for _ in range(steps):
        parent = torch.randint(0, W, (R,), generator=g)
        src = torch.arange(R) // W * W + parent
        tok = labels[torch.randint(0, labels.numel(), (R,), generator=g)]
        kind = torch.randint(0, 6, (R,), generator=g)
        tok = torch.where((kind < 2) & (last[src] >= 0), last[src], tok)
        tok = torch.where(kind == 5, torch.full_like(tok, EOS), tok)
        walk.append((parent, tok, fin.clone()))
        copied = fin[src] | (tok == EOS)
        last = torch.where(copied, last[src], tok)
        fin = copied
    return walk


def reference_walk(logits, frames, W, blank, walk, dtype):
    """[(delta before selection k, state after it)] for k < steps, then (delta of the final state, None)."""
    lp = joint_ref.log_probs(logits, dtype)
    st = joint_ref.root_state(lp, frames, W, blank)
    out = []
    for parent, tok, fin in walk:
        d = joint_ref.prefix_score(lp, frames, st, W, blank, EOS)
        st = joint_ref.prefix_advance(lp, frames, st, W, parent, tok, fin, blank, EOS)
        out.append((d, st))
    out.append((joint_ref.prefix_score(lp, frames, st, W, blank, EOS), None))
    return out


def device_walk(logits, lengths, W, ld, blank, walk):
    """The same walk through the kernels.  Returns the list reference_walk returns (natural-log fp64 on the host)
    plus the raw bits of every output; asserts on the way that padding and inputs stay untouched."""
    B, T, V = logits.shape
    R = B * W
    x = torch.full((B * T, ld), float("nan"), dtype=torch.float32)      # only columns [0, V) may be read
    x[:, :V] = logits.reshape(B * T, V).float()
    x = x.to(dev)
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    x0 = bits(x)
    pf = K().CtcPrefix(x, B, W, T, V, blank, il)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), x0)
    raw = [bits(pf.logp), bits(pf.frames)]

    def host_state():
        st, lpsi, last = pf.cur
        s = st.cpu().double() * LN2
        return joint_ref.PrefixState(s[:, :, 0], s[:, :, 1], lpsi.cpu().double() * LN2, last.cpu().long())

    def score():
        delta = torch.full((R, ld), 512.0, dtype=torch.float32, device=dev)
        keep = [bits(t) for t in (pf.logp, pf.frames) + tuple(pf.cur)]
        pf.score(EOS, delta)
        torch.cuda.synchronize()
        assert all(torch.equal(a, bits(t)) for a, t in zip(keep, (pf.logp, pf.frames) + tuple(pf.cur)))
        assert bool((delta[:, V:] == 512.0).all()), "padding columns of delta must not be written"
        raw.append(bits(delta))
        return delta[:, :V].cpu().double()

    out = []
    root = host_state()
    for parent, tok, fin in walk:
        d = score()
        src = pf.cur
        keep = [bits(t) for t in (pf.logp, pf.frames) + tuple(src)]
        pf.advance(EOS, parent.to(torch.int32).to(dev), tok.to(dev), fin.to(torch.uint8).to(dev))
        torch.cuda.synchronize()
        assert all(torch.equal(a, bits(t)) for a, t in zip(keep, (pf.logp, pf.frames) + tuple(src)))
        raw.extend(bits(t) for t in pf.cur)
        out.append((d, host_state()))
    out.append((score(), None))
    return out, raw, root


def compare(name, got, r64, r32, worst):
    """One quantity of one step: -inf exactly, finite entries within max(4 * fp32 reference error, floor)."""
    assert torch.equal(r32 == -INF, r64 == -INF), (name, "the fp32 reference must share the fp64 one's -inf pattern")
    assert not bool(torch.isnan(got).any()), (name, "NaN")
    assert torch.equal(got == -INF, r64 == -INF), (name, "-inf pattern")
    fin = r64 != -INF
    if not bool(fin.any()):
        return
    e32 = float((r32.double()[fin] - r64[fin]).abs().max())
    bound = torch.clamp(1e-5 * r64[fin].abs().clamp(min=1.0), min=4 * e32)
    err = (got[fin] - r64[fin]).abs()
    ratio = float((err / bound).max())
    worst[name.split()[0]] = max(worst.get(name.split()[0], 0.0), ratio)
    assert ratio <= 1.0, (name, ratio, float(err.max()), e32)


# (T, V, ld, W, B, steps, blank, logit scale, input lengths): every T of the frame-chunk edges (the advance stages 64
# frames at a time, the scorer splits the frames over 4 waves), every (V, ld) and W (each register tile of the scorer:
# 1, 4, 8, 16 hypotheses), one sample shorter than T, one with a single frame, one with none, peaked logits, and the
# long utterance
PREFIX_CASES = [
    (1, 5, 8, 1, 1, 2, 0, 1.0, None),
    (2, 5, 8, 3, 3, 3, 0, 1.0, [2, 0, 1]),
    (5, 250, 256, 3, 1, 4, 4, 1.0, None),
    (5, 5, 8, 16, 1, 4, 0, 1.0, None),
    (63, 257, 320, 16, 1, 3, 4, 1.0, None),
    (64, 5, 8, 16, 3, 4, 0, 1.0, [64, 40, 1]),
    (65, 250, 256, 1, 3, 4, 4, 1.0, None),
    (65, 257, 320, 8, 1, 3, 0, 1.0, [64]),
    (130, 257, 320, 3, 3, 4, 4, 1.0, [130, 77, 1]),
    (249, 250, 256, 16, 3, 4, 4, 1.0, [249, 200, 1]),
    (249, 250, 256, 3, 1, 4, 4, 30.0, None),
    (999, 257, 320, 16, 1, 2, 4, 1.0, None),
]


@pytest.mark.parametrize("T,V,ld,W,B,steps,blank,scale,lengths", PREFIX_CASES)
def test_prefix_score_and_advance(T, V, ld, W, B, steps, blank, scale, lengths):
    g = torch.Generator().manual_seed(1000 * T + 10 * W + B)
    logits = scale * torch.randn(B, T, V, generator=g)
    walk = random_walk(B, W, V, blank, steps, g)
    frames = joint_ref.frame_counts(B, T, lengths)
    r64 = reference_walk(logits, frames, W, blank, walk, torch.float64)
    r32 = reference_walk(logits, frames, W, blank, walk, torch.float32)
    got, raw, root = device_walk(logits, lengths, W, ld, blank, walk)
    worst = {}
    lp64 = joint_ref.log_probs(logits)
    lp32 = joint_ref.log_probs(logits, torch.float32)
    s64, s32 = (joint_ref.root_state(lp, frames, W, blank) for lp in (lp64, lp32))
    compare("state root", root.nb, s64.nb, s32.nb, worst)
    assert torch.equal(root.nb, root.b) and bool((root.logpsi == 0).all()) and bool((root.last == -1).all())
    dead = 0
    for k, ((d, st), (d64, st64), (d32, st32)) in enumerate(zip(got, r64, r32)):
        compare(f"delta step {k}", d, d64, d32, worst)
        if st is None:
            continue
        valid = torch.zeros(B * W, T, dtype=torch.bool)
        for r in range(B * W):
            valid[r, :frames[r // W]] = True
        assert bool((st.nb[~valid] == -INF).all()) and bool((st.b[~valid] == -INF).all())
        compare(f"state nb {k}", st.nb, st64.nb, st32.nb, worst)
        compare(f"state b {k}", st.b, st64.b, st32.b, worst)
        compare(f"logpsi step {k}", st.logpsi, st64.logpsi, st32.logpsi, worst)
        assert torch.equal(st.last, st64.last)
        dead += int((st64.logpsi == -INF).sum())
    print(f"T {T} V {V} W {W} B {B} scale {scale}: worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) + f"; dead slots met {dead}")
    again, raw2, _ = device_walk(logits, lengths, W, ld, blank, walk)
    assert len(raw) == len(raw2) and all(torch.equal(a, b) for a, b in zip(raw, raw2)), "two runs, different bits"


def test_walks_meet_every_kind_of_slot():
    """The condition on the inputs of the cases above (host only): repeats of the last label, EOS, finished parents
    and dead slots all occur somewhere."""
    seen = dict(repeat=0, eos=0, finished_parent=0, dead=0)
    for T, V, ld, W, B, steps, blank, scale, lengths in PREFIX_CASES[:6]:
        g = torch.Generator().manual_seed(1000 * T + 10 * W + B)
        logits = scale * torch.randn(B, T, V, generator=g)
        walk = random_walk(B, W, V, blank, steps, g)
        frames = joint_ref.frame_counts(B, T, lengths)
        ref = reference_walk(logits, frames, W, blank, walk, torch.float64)
        last = torch.full((B * W,), -1)
        for (parent, tok, fin), (_, st) in zip(walk, ref):
            src = torch.arange(B * W) // W * W + parent
            seen["repeat"] += int(((tok == last[src]) & ~fin[src]).sum())
            seen["eos"] += int((tok == EOS).sum())
            seen["finished_parent"] += int(fin[src].sum())
            seen["dead"] += int((st.logpsi == -INF).sum())
            last = st.last
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------ joint step

def run_joint(logits, extra, att_w, ext_w, score, fin, length, V, joint=True):
    B, W = score.shape
    R = B * W
    lg, ex = logits.to(dev), extra.to(dev)
    si, fi, li = (score.reshape(R).float().to(dev), fin.reshape(R).to(torch.uint8).to(dev),
                  length.reshape(R).to(torch.int32).to(dev))
    keep = [bits(t) for t in (lg, ex, si, fi, li)]
    so, fo, lo = torch.empty_like(si), torch.empty_like(fi), torch.empty_like(li)
    tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
    parent = torch.full((R,), -7, dtype=torch.int32, device=dev)
    src_row = torch.full((R,), -7, dtype=torch.int32, device=dev)
    cur = torch.full((R,), -7, dtype=torch.int64, device=dev)
    n_live = torch.zeros(1, dtype=torch.int32, device=dev)
    if joint:
        K().beam_step_joint(lg, V, B, W, EOS, ex, att_w, ext_w, (si, fi, li), (so, fo, lo), tok, parent, src_row,
                            cur=cur, n_live=n_live)
    else:
        K().beam_step(lg, V, B, W, EOS, (si, fi, li), (so, fo, lo), tok, parent, src_row, cur=cur, n_live=n_live)
    torch.cuda.synchronize()
    assert all(torch.equal(a, bits(t)) for a, t in zip(keep, (lg, ex, si, fi, li)))
    out = dict(score=so, tok=tok, parent=parent, src_row=src_row, fin=fo, len=lo)
    out = {k: v.cpu().view(B, W) for k, v in out.items()}
    out["n_live"] = int(n_live)
    assert torch.equal(cur.cpu().view(B, W), out["tok"])
    return out


def make_extra(V, ld, W, B, lam):
    """A second score around -3 per candidate, one in eight -inf, +inf in the padding columns."""
    g = torch.Generator().manual_seed(7000 * V + 70 * W + B + int(10 * lam))
    extra = 2 * torch.randn(B * W, ld, generator=g) - 3
    extra[torch.rand(B * W, ld, generator=g) < 0.125] = -INF
    extra[:, V:] = INF
    return extra


JOINT_SHAPES = [(5, 8), (250, 256), (1030, 1032)]       # (1030 x 16 candidates: the path that re-reads the logits)


@pytest.mark.parametrize("lam", [0.3, 1.0])
@pytest.mark.parametrize("W", [1, 3, 16])
@pytest.mark.parametrize("V,ld", JOINT_SHAPES)
def test_beam_step_joint_random(V, ld, W, lam):
    B = 3
    logits, score, fin, length = make_case(V, ld, W, B)
    extra = make_extra(V, ld, W, B, lam)
    ref = joint_ref.joint_step(logits.view(B, W, ld), extra.view(B, W, ld), 1.0 - lam, lam, score, fin, length, EOS, V)
    assert ref["gap"] >= 1e-4, f"fp64 margin {ref['gap']:.2e}: choose another seed for this case"
    check_step(run_joint(logits, extra, 1.0 - lam, lam, score, fin, length, V), ref)


@pytest.mark.parametrize("V,ld,W", [(5, 8, 3), (250, 256, 16), (1030, 1032, 16)])
def test_beam_step_joint_with_zero_weight_is_beam_step_bit_for_bit(V, ld, W):
    B = 3
    logits, score, fin, length = make_case(V, ld, W, B)
    zero = torch.zeros(B * W, ld)
    a = run_joint(logits, zero, 1.0, 0.0, score, fin, length, V)
    b = run_joint(logits, zero, 1.0, 0.0, score, fin, length, V, joint=False)
    for k in ("tok", "parent", "src_row", "fin", "len"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(bits(a["score"]), bits(b["score"])) and a["n_live"] == b["n_live"]


# ------------------------------------------------------------------------------------------------ end to end

E2E_STEPS = 6
# (T, V, ld, W, B, lam, seed): seeds chosen on the CPU so that the reference's margin clears 10 x the delta bound
E2E_CASES = [(40, 5, 8, 16, 2, 0.3, 2), (65, 250, 256, 3, 3, 0.3, 0), (130, 257, 320, 4, 2, 1.0, 0),
             (249, 250, 256, 8, 1, 0.5, 12)]


@functools.lru_cache(maxsize=None)
def e2e_reference(T, V, ld, W, B, lam, seed):
    g = torch.Generator().manual_seed(seed)
    ctc_logits = 2 * torch.randn(B, T, V, generator=g)
    ctc_logits[:, :, 0] += 5.0 + math.log(V)     # mostly blank, as a trained head is: short hypotheses are likely
    att = 3 * torch.randn(E2E_STEPS, B * W, ld, generator=g)
    att[:, :, V:] = INF
    frames = [T] * B
    lp = joint_ref.log_probs(ctc_logits)
    ref = joint_ref.joint_search(lambda rows: att[rows.shape[2]].view(B, W, ld), lp, frames, W, EOS, 0, lam, E2E_STEPS)
    # the delta bound of the case: the fp32 formulas over the reference's own selections
    walk = [(p, t, f) for p, t, f, _ in ref["history"]]
    r64 = reference_walk(ctc_logits, frames, W, 0, walk, torch.float64)
    r32 = reference_walk(ctc_logits, frames, W, 0, walk, torch.float32)
    bound = 0.0
    for (d64, _), (d32, _) in zip(r64[:-1], r32[:-1]):
        fin = d64 != -INF
        e32 = float((d32.double()[fin] - d64[fin]).abs().max())
        bound = max(bound, 4 * e32, 1e-5 * max(1.0, float(d64[fin].abs().max())))
    return ctc_logits, att, ref, bound


@pytest.mark.parametrize("T,V,ld,W,B,lam,seed", E2E_CASES)
def test_score_joint_step_advance_end_to_end(T, V, ld, W, B, lam, seed):
    ctc_logits, att, ref, bound = e2e_reference(T, V, ld, W, B, lam, seed)
    print(f"reference margin {ref['gap']:.3e}, delta bound {bound:.3e}")
    assert ref["gap"] >= 10 * bound, "choose another seed for this case"
    R = B * W
    pf = K().CtcPrefix(ctc_logits.reshape(B * T, V).float().to(dev), B, W, T, V, 0)
    score0 = torch.full((B, W), -INF)
    score0[:, 0] = 0.0
    state = (score0.reshape(R).to(dev), torch.zeros(R, dtype=torch.uint8, device=dev),
             torch.zeros(R, dtype=torch.int32, device=dev))
    other = tuple(torch.empty_like(a) for a in state)
    tok = torch.empty(E2E_STEPS, R, dtype=torch.int64, device=dev)
    par = torch.empty(E2E_STEPS, R, dtype=torch.int32, device=dev)
    src_row = torch.empty(R, dtype=torch.int32, device=dev)
    delta = torch.empty(R, ld, dtype=torch.float32, device=dev)
    att_d = att.to(dev)
    for s in range(E2E_STEPS):
        pf.score(EOS, delta)
        K().beam_step_joint(att_d[s], V, B, W, EOS, delta, 1.0 - lam, lam, state, other, tok[s], par[s], src_row)
        pf.advance(EOS, par[s], tok[s], state[1])
        state, other = other, state
    torch.cuda.synchronize()
    for s, (p, t, _, _) in enumerate(ref["history"]):
        assert torch.equal(par[s].cpu().long(), p), f"parents of step {s}"
        assert torch.equal(tok[s].cpu(), t), f"tokens of step {s}"
    from asrx.decode import beam_backtrack
    seqs = beam_backtrack(par.cpu().view(E2E_STEPS, B, W), tok.cpu().view(E2E_STEPS, B, W))
    assert torch.equal(seqs, ref["tokens"])
    got = state[0].cpu().double().view(B, W)
    assert torch.equal(got == -INF, ref["score"] == -INF)
    fin = ref["score"] != -INF
    err = float((got[fin] - ref["score"][fin]).abs().max())
    tol = 1e-5 * max(1.0, float(ref["score"][fin].abs().max())) + E2E_STEPS * lam * bound
    print(f"joint score error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    assert torch.equal(state[1].cpu().bool().view(B, W), ref["fin"])
    assert torch.equal(state[2].cpu().long().view(B, W), ref["len"])
