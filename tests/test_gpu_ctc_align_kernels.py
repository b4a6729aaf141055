"""asrx_ctc_align on the GPU against tests/ctc_align_ref.py (the recursion in fp64).

Tolerance (the rule of tests/test_gpu_ctc_beam_kernels.py): per sample 4 x the error of the reference's own fp32 run
against fp64, measured on the path's score, floored at 1e-5 * max(1, |value|); -inf must match exactly.

On every case the kernel's path must be a valid alignment whose fp64 score lies within the bound of the reference
optimum, and score, frame_logp and tok_conf must lie within the bound of their fp64 values on THAT path; the spans are
the run boundaries of frame_pos exactly.  The path itself is only comparable where fp32 cannot flip a decision on it:
a case marked exact asserts, on the input, that the reference's on-path margin is >= 10 x the bound (seeds and planted
alignments were chosen on the CPU for that), and then asserts frame_pos identical to the reference's."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
BLANK = 2
LDS_T = 1008      # the longest T whose backpointers stay in LDS (asrx.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def labels(n, V, seed, repeat_every=0):
    """n labels in [0, V) without the blank, no two adjacent equal unless repeat_every > 0 (then every
    repeat_every-th label repeats its predecessor)."""
    rng = np.random.default_rng(seed)
    out = []
    for u in range(n):
        if repeat_every and u % repeat_every == repeat_every - 1 and out:
            out.append(out[-1])
            continue
        while True:
            c = int(rng.integers(0, V))
            if c != BLANK and (not out or c != out[-1]):
                out.append(c)
                break
    return out


def _rand(c):
    g = torch.Generator().manual_seed(c["seed"])
    x = c.get("s", 1.0) * torch.randn(c["B"], c["T"], c["ld"], generator=g)
    x[:, :, BLANK] += c.get("boost_blank", 2.0) * c.get("s", 1.0)
    return x


def _planted(c):
    xs = []
    for b, tg in enumerate(c["targets"]):
        Tb = c["T"] if c["lengths"] is None else c["lengths"][b]
        x = (c["noise"] * np.random.default_rng(1000 * c["seed"] + b).standard_normal((c["T"], c["ld"]))).astype(
            np.float32)
        ok = all(0 <= t < c["V"] and t != BLANK for t in tg)
        if Tb > 0 and ok:
            x[:Tb] = R.planted(Tb, c["V"], tg, c["boost"], c["noise"], 1000 * c["seed"] + b, BLANK, c["ld"])
        xs.append(torch.from_numpy(x))
    return torch.stack(xs)


# T, (V, ld), Lmax = max_target_len (KP = ceil((Lmax + 1) / 64)), per-sample targets and input lengths (None: all T),
# the logits (random with a boosted blank | a planted alignment), and whether the path must equal the reference's
CASES = [
    # a single frame; an empty target; no frame at all for a label (no alignment)
    dict(T=1, V=5, ld=8, Lmax=1, targets=[[1], [], [3]], lengths=(1, 1, 0), gen="rand", seed=0, exact=True),
    # T_b = L + repeats - 1 (no alignment), T_b = L exactly (the single alignment), a free label
    dict(T=2, V=250, ld=256, Lmax=2, targets=[[7, 7], [7, 9], [5]], lengths=None, gen="rand", seed=1, exact=True),
    # T_b = L + repeats exactly with one label repeated (the single alignment), the same one frame short
    dict(T=5, V=257, ld=320, Lmax=3, targets=[[256, 1, 256], [4, 4, 4], [4, 4, 4]], lengths=(5, 5, 4), gen="rand",
         seed=2, exact=True),
    # KP = 1 at its limit L = 63 with one spare frame; input_lengths (T, 40, 0), the last the empty alignment
    dict(T=64, V=5, ld=8, Lmax=63, targets=[labels(63, 5, 3), labels(20, 5, 4, 4), []], lengths=(64, 40, 0),
         gen="planted", boost=6.0, noise=0.5, seed=3, exact=True),
    # KP = 2 from L = 64, a row stride that is no multiple of 4
    dict(T=65, V=250, ld=251, Lmax=64, targets=[labels(64, 250, 5), [9]], lengths=None, gen="planted", boost=6.0,
         noise=0.5, seed=4, exact=True),
    dict(T=130, V=257, ld=320, Lmax=127, targets=[labels(127, 257, 6), [9] * 40], lengths=(130, 100), gen="planted",
         boost=8.0, noise=0.5, seed=5, exact=True),
    # random logits with a boosted blank at a moderate T (the margin holds for this seed)
    dict(T=130, V=250, ld=256, Lmax=30, targets=[labels(30, 250, 7), labels(12, 250, 8, 3)], lengths=None,
         gen="rand", boost_blank=4.0, seed=25, exact=True),
    # KP = 3: L = 128 and L = 191
    dict(T=249, V=250, ld=256, Lmax=128, targets=[labels(128, 250, 9), labels(64, 250, 10)], lengths=None,
         gen="planted", boost=8.0, noise=0.5, seed=7, exact=True),
    dict(T=249, V=250, ld=256, Lmax=191, targets=[labels(191, 250, 11)], lengths=None, gen="planted", boost=8.0,
         noise=0.5, seed=8, exact=True),
    # KP = 4: L = 192, and repeated labels at T = 249
    dict(T=249, V=257, ld=320, Lmax=192, targets=[labels(192, 257, 12), labels(100, 257, 13, 5)],
         lengths=(249, 230), gen="planted", boost=8.0, noise=0.5, seed=9, exact=True),
    # random logits at T = 249: fp32 may take another path of (nearly) the same score
    dict(T=249, V=250, ld=256, Lmax=64, targets=[labels(64, 250, 14), labels(64, 250, 15, 6)], lengths=None,
         gen="rand", seed=10, exact=False),
    # both sides of the LDS / workspace switch at the longest target
    dict(T=LDS_T, V=250, ld=256, Lmax=255, targets=[labels(255, 250, 16), labels(100, 250, 17, 7)],
         lengths=(LDS_T, 700), gen="planted", boost=8.0, noise=0.5, seed=11, exact=True),
    dict(T=LDS_T + 1, V=250, ld=256, Lmax=255, targets=[labels(255, 250, 18), labels(3, 250, 19)],
         lengths=(LDS_T + 1, 600), gen="planted", boost=8.0, noise=0.5, seed=12, exact=True),
    # the other KP above the switch
    dict(T=LDS_T + 1, V=5, ld=8, Lmax=10, targets=[labels(10, 5, 20, 3)], lengths=None, gen="planted", boost=8.0,
         noise=0.5, seed=13, exact=True),
    dict(T=LDS_T + 1, V=250, ld=256, Lmax=100, targets=[labels(100, 250, 21)], lengths=None, gen="planted",
         boost=8.0, noise=0.5, seed=14, exact=True),
    dict(T=LDS_T + 1, V=250, ld=256, Lmax=150, targets=[labels(150, 250, 22, 9)], lengths=None, gen="planted",
         boost=8.0, noise=0.5, seed=15, exact=True),
    # malformed samples next to a good one: a label equal to the blank, a label equal to V, a target length above
    # max_target_len, a negative one
    dict(T=5, V=5, ld=8, Lmax=3, targets=[[1, BLANK], [1, 5], [1, 3, 4, 0], [1], [3, 1]], tlens=(2, 2, 4, -1, 2),
         lengths=None, gen="rand", seed=16, exact=True),
    # a weaker planted alignment in louder noise (hundreds of close decisions), the second target with repeats
    dict(T=249, V=250, ld=256, Lmax=64, targets=[labels(64, 250, 30), labels(64, 250, 31, 4)], lengths=None,
         gen="planted", boost=4.0, noise=1.0, seed=43, exact=True),
]
for _c in CASES:
    _c["B"] = len(_c["targets"])


@functools.lru_cache(maxsize=None)
def case(i):
    """(case, logits (B, T, ld), targets (B, W) int64, target lengths, per-sample fp64 references, per-sample fp32
    error of the reference).  Computed once, shared by the tests, never changed."""
    c = CASES[i]
    x = _rand(c) if c["gen"] == "rand" else _planted(c)
    W = max(c["Lmax"], max(len(t) for t in c["targets"]), 1)
    tg = torch.full((c["B"], W), BLANK, dtype=torch.int64)
    for b, t in enumerate(c["targets"]):
        tg[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    tl = torch.tensor(c.get("tlens", [len(t) for t in c["targets"]]), dtype=torch.int32)
    refs, errs = [], []
    for b in range(c["B"]):
        L = int(tl[b])
        Tb = c["T"] if c["lengths"] is None else c["lengths"][b]
        if L < 0 or L > c["Lmax"]:
            refs.append(R.no_alignment(c["T"], c["Lmax"]))
            errs.append(0.0)
            continue
        xb = x[b, :, :c["V"]].numpy()
        r64 = R.viterbi(xb, c["targets"][b][:L], BLANK, Tb, c["Lmax"])
        r32 = R.viterbi(xb, c["targets"][b][:L], BLANK, Tb, c["Lmax"], dtype=np.float32)
        refs.append(r64)
        errs.append(abs(r64["score"] - r32["score"]) if r64["feasible"] else 0.0)
    return c, x, tg, tl, refs, errs


GARBAGE_I, GARBAGE_F = 0x7f7f7f7f, float("nan")


def run(i):
    """The C entry point on buffers filled with garbage: every element of every output must be written."""
    from asrx._lib import call
    from asrx import kernels as K
    c, x, tg, tl, _, _ = case(i)
    B, T, ld, Lmax = c["B"], c["T"], c["ld"], c["Lmax"]
    xd = x.reshape(B * T, ld).to(dev)
    tgd, tld = tg.to(dev), tl.to(dev)
    il = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32, device=dev)
    words = K.ctc_align_workspace_words(B, T, Lmax)
    ws = torch.full((words,), GARBAGE_I, dtype=torch.int32, device=dev)
    fp = torch.full((B, T), GARBAGE_I, dtype=torch.int32, device=dev)
    fl = torch.full((B, T), GARBAGE_F, dtype=torch.float32, device=dev)
    st = torch.full((B, Lmax), GARBAGE_I, dtype=torch.int32, device=dev)
    en = torch.full((B, Lmax), GARBAGE_I, dtype=torch.int32, device=dev)
    cf = torch.full((B, Lmax), GARBAGE_F, dtype=torch.float32, device=dev)
    sc = torch.full((B,), GARBAGE_F, dtype=torch.float32, device=dev)
    call("asrx_ctc_align", xd.data_ptr(), B, T, c["V"], ld, tgd.data_ptr(), tgd.stride(0),
         None if il is None else il.data_ptr(), tld.data_ptr(), Lmax, BLANK, ws.data_ptr(), words, fp.data_ptr(),
         fl.data_ptr(), st.data_ptr(), en.data_ptr(), cf.data_ptr(), sc.data_ptr(), K.stream())
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (fp, fl, st, en, cf, sc))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("i", range(len(CASES)))
def test_align_matches_reference(i):
    c, x, tg, tl, refs, errs = case(i)
    T, Lmax = c["T"], c["Lmax"]
    got = run(i)
    fp, fl, st, en, cf, sc = got
    worst = 0.0
    for b, r in enumerate(refs):
        L = int(tl[b])
        Tb = T if c["lengths"] is None else c["lengths"][b]
        if not r["feasible"]:
            assert float(sc[b]) == -INF, (b, float(sc[b]))
            assert (fp[b] == -1).all() and (fl[b] == 0).all()
            assert (st[b] == -1).all() and (en[b] == -1).all() and (cf[b] == 0).all()
            continue
        target = c["targets"][b][:L]
        bound = R.bound(errs[b], r["score"])
        print(f"case {i} sample {b}: L {L}, T_b {Tb}, score {r['score']:.4f}, fp32 reference error {errs[b]:.2e}, "
              f"bound {bound:.2e}, on-path margin {r['margin']:.3e} = {r['margin'] / bound:.1f} x bound")
        if c["exact"]:
            assert r["margin"] >= 10 * bound, (b, r["margin"], bound)     # a condition on the input
        pos = fp[b].numpy()
        assert R.path_is_valid(pos, target, Tb), (b, pos.tolist())
        total, flp = R.rescore(x[b, :, :c["V"]].numpy(), target, BLANK, pos, Tb)
        assert total >= r["score"] - bound and total <= r["score"] + 1e-9, (b, total, r["score"])
        err = abs(float(sc[b]) - total)
        worst = max(worst, err / bound)
        assert err <= bound, (b, float(sc[b]), total, bound)
        assert (fl[b, Tb:] == 0).all()
        for t in range(Tb):
            assert abs(float(fl[b, t]) - flp[t]) <= R.bound(errs[b], flp[t]), (b, t, float(fl[b, t]), flp[t])
        ws, we, wc = R.spans_of(pos, flp, L, Lmax)
        assert st[b].tolist() == ws.tolist() and en[b].tolist() == we.tolist(), b
        for u in range(Lmax):
            assert abs(float(cf[b, u]) - wc[u]) <= R.bound(errs[b], wc[u]), (b, u, float(cf[b, u]), wc[u])
            if u < L:
                assert we[u] > ws[u] and (u == 0 or ws[u] >= we[u - 1])
        if c["exact"]:
            assert pos.tolist() == r["frame_pos"].tolist(), b
    print(f"case {i}: worst score error / bound {worst:.3f}")
    again = run(i)
    for a, b_ in zip(got, again):
        assert torch.equal(bits(a), bits(b_))      # the same inputs give the same bits


def test_cases_cover_the_code_paths():
    """An exact case per KP, on each side of the LDS / workspace switch, and with repeated labels; every (V, ld)."""
    exact = [c for c in CASES if c["exact"]]
    for kp in (1, 2, 3, 4):
        for side in (False, True):
            assert any((c["Lmax"] + 64) // 64 == kp and (c["T"] > LDS_T) == side for c in exact), (kp, side)
    assert any(c["T"] == LDS_T for c in exact) and any(c["T"] == LDS_T + 1 for c in exact)
    assert any(any(a == b for t in c["targets"] for a, b in zip(t, t[1:])) for c in exact)
    assert {(5, 8), (250, 256), (257, 320)} <= {(c["V"], c["ld"]) for c in CASES}
    assert any(c["ld"] % 4 for c in CASES)
    assert {1, 2, 5, 64, 65, 130, 249} <= {c["T"] for c in CASES}
    assert {0, 1, 63, 64, 127, 128, 191, 192, 255} <= {len(t) for c in CASES for t in c["targets"]}


def test_wrapper_and_graph_replay():
    """kernels.ctc_align gives the C call's bits; captured in a graph and replayed twice it gives them again."""
    from asrx import kernels as K
    i = 9
    c, x, tg, tl, _, _ = case(i)
    want = run(i)
    B, T, ld = c["B"], c["T"], c["ld"]
    xd = x.reshape(B * T, ld).to(dev)
    tgd, tld = tg.to(dev), tl.to(dev)
    il = torch.tensor(c["lengths"], dtype=torch.int32, device=dev)
    eager = K.ctc_align(xd, c["V"], T, tgd, tld, il, max_target_len=c["Lmax"], blank=BLANK)
    torch.cuda.synchronize()
    assert eager.targets is tgd and eager.target_lengths is tld
    for a, b in zip(eager[:6], want):
        assert torch.equal(bits(a.cpu()), bits(b))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = K.ctc_align(xd, c["V"], T, tgd, tld, il, max_target_len=c["Lmax"], blank=BLANK)
    for _ in range(2):
        for t in out[:6]:
            t.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out[:6], want):
            assert torch.equal(bits(a.cpu()), bits(b))
    with pytest.raises(RuntimeError, match="unsupported"):
        K.ctc_align(xd, c["V"], T, torch.zeros(B, 256, dtype=torch.int64, device=dev), tld, il)
