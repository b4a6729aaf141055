"""asrx_ctc_prefix_beam, asrx_hyp_tokens, asrx_seq_logprob and asrx_rescore_rank on the GPU against
tests/ctc_beam_ref.py.

Tolerances (the rule of DESIGN sections 9 and 10): per case 4 x the error of the reference's own recursion run in fp32
on the CPU against fp64, floored at 1e-5 * max(1, |value|); -inf must match exactly.  The kernel selects and ranks on
scores renormalised per frame (magnitude O(10)), so the selection margins are held against the bound of the
renormalised scores; the scores that leave carry the accumulated offset and are held against the bound at their own
magnitude (ctc_beam_ref.bounds).  Hypotheses, lengths, counts and order are only comparable where fp32 cannot flip a
selection: every case asserts that the reference's smallest boundary margin (W-th against (W+1)-th candidate over all
frames) and smallest gap of the final ranking are >= 10 x its bound; the seeds were chosen on the CPU for that."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def K():
    import asrx.kernels as k
    return k


# T, (V, ld), W, B, per-sample lengths (None: all T), max_labels, scale, seed, must merge
CASES = [
    dict(T=1, V=5, ld=8, W=3, B=1, lengths=None, ml=63, s=1, seed=0, merge=False),
    dict(T=2, V=250, ld=256, W=8, B=3, lengths=(2, 1, 0), ml=63, s=3, seed=0, merge=False),
    dict(T=5, V=257, ld=320, W=16, B=1, lengths=None, ml=2, s=1, seed=0, merge=False),
    dict(T=5, V=5, ld=8, W=16, B=1, lengths=None, ml=63, s=1, seed=0, merge=True),
    dict(T=63, V=250, ld=256, W=1, B=3, lengths=(63, 40, 1), ml=63, s=1, seed=0, merge=False),
    dict(T=64, V=5, ld=8, W=8, B=1, lengths=None, ml=63, s=3, seed=0, merge=True),
    dict(T=64, V=5, ld=8, W=3, B=1, lengths=None, ml=2, s=1, seed=0, merge=True),
    dict(T=65, V=257, ld=320, W=3, B=3, lengths=(65, 0, 17), ml=2, s=3, seed=0, merge=False),
    dict(T=130, V=250, ld=256, W=16, B=1, lengths=None, ml=63, s=1, seed=2, merge=False),
    dict(T=249, V=257, ld=320, W=8, B=1, lengths=None, ml=63, s=1, seed=0, merge=False),
    dict(T=249, V=250, ld=256, W=16, B=1, lengths=(200,), ml=63, s=3, seed=1, merge=False),
    # beyond the issue's list: a cap that never binds, so the beam keeps extending over all frames
    dict(T=249, V=250, ld=256, W=8, B=1, lengths=None, ml=254, s=3, seed=0, merge=False),
    dict(T=130, V=257, ld=320, W=16, B=1, lengths=None, ml=254, s=1, seed=0, merge=False),
    # and both sides of V = 256 and V = 512, where the prologue changes its kernel variant
    dict(T=5, V=256, ld=256, W=8, B=1, lengths=None, ml=63, s=3, seed=0, merge=False),
    dict(T=5, V=512, ld=512, W=8, B=1, lengths=None, ml=63, s=1, seed=0, merge=False),
    dict(T=5, V=600, ld=608, W=3, B=3, lengths=(5, 4, 1), ml=63, s=3, seed=0, merge=False),
    # a prefix is pruned while a child of it stays in the beam and is selected again later: the child's stay must
    # get the parent's mass again.  A search that knew prefixes by the node of their first selection returns other
    # hypotheses in the first case and scores off by 2.4e-3 in the second (tests/test_ctc_beam_cpu.py).
    dict(T=64, V=5, ld=8, W=8, B=1, lengths=None, ml=63, s=3, seed=104, merge=True, recreate=True),
    dict(T=64, V=8, ld=8, W=16, B=1, lengths=None, ml=63, s=3, seed=31, merge=True, recreate=True),
]
RECREATE_CASES = [i for i, c in enumerate(CASES) if c.get("recreate")]
BLANK = 2


def make_logits(c, seed=None):
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    x = c["s"] * torch.randn(c["B"], c["T"], c["ld"], generator=g)
    x[:, :, BLANK] += 2.0 * c["s"]
    return x


def references(c, x):
    r64 = R.batch(x, c["V"], c["W"], BLANK, c["ml"], c["lengths"])
    r32 = R.batch(x, c["V"], c["W"], BLANK, c["ml"], c["lengths"], dtype=np.float32)
    return r64, r32


@functools.lru_cache(maxsize=None)
def case(i):
    c = CASES[i]
    x = make_logits(c)
    r64, r32 = references(c, x)
    return c, x, r64, R.bounds(r64, r32)


def run(x, V, W, ml, lengths=None, blank=BLANK):
    B, T, ld = x.shape
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    tok, lens, score, n_hyp = K().ctc_prefix_beam(x.reshape(B * T, ld).to(dev), V, T, blank, W, ml, il)
    torch.cuda.synchronize()
    return tok.cpu().view(B, W, ml), lens.cpu().view(B, W), score.cpu().view(B, W), n_hyp.cpu()


def compare(got, refs, W, ml, out_bound, blank=BLANK):
    """Hypotheses, lengths, counts and order exactly; scores within out_bound(value); dead slots blank / 0 / -inf.
    Returns the worst score error / bound ratio."""
    tok, lens, score, n_hyp = got
    worst = 0.0
    for b, r in enumerate(refs):
        n = len(r["prefixes"])
        assert int(n_hyp[b]) == n, (b, int(n_hyp[b]), n)
        for j in range(W):
            if j < n:
                g = list(r["prefixes"][j])
                assert int(lens[b, j]) == len(g), (b, j)
                assert tok[b, j].tolist() == g + [blank] * (ml - len(g)), (b, j, tok[b, j].tolist(), g)
                want = float(r["scores"][j])
                err = abs(float(score[b, j]) - want)
                bound = out_bound(want)
                worst = max(worst, err / bound)
                assert err <= bound, (b, j, float(score[b, j]), want, bound)
            else:
                assert int(lens[b, j]) == 0 and float(score[b, j]) == -INF
                assert tok[b, j].tolist() == [blank] * ml
    return worst


@pytest.mark.parametrize("i", range(len(CASES)))
def test_prefix_beam_matches_reference(i):
    c, x, r64, (sel, out_bound) = case(i)
    boundary = min(r["boundary"] for r in r64)
    final = min(r["final"] for r in r64)
    merges = sum(r["merges"] for r in r64)
    print(f"case {i}: selection bound {sel:.2e}, boundary margin {boundary:.2e}, final margin {final:.2e}, "
          f"merges {merges}")
    assert boundary >= 10 * sel and final >= 10 * sel
    if c["merge"]:
        assert c["W"] > 1 and merges > 0
    if c.get("recreate"):
        assert sum(r["recreated"] for r in r64) > 0
    got = run(x, c["V"], c["W"], c["ml"], c["lengths"])
    worst = compare(got, r64, c["W"], c["ml"], out_bound)
    print(f"case {i}: worst score error / bound {worst:.3f}")
    again = run(x, c["V"], c["W"], c["ml"], c["lengths"])
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_prefix_beam_enumeration_on_the_gpu():
    """V = 3, T = 3, W = 16: all 9 reachable prefixes fit, each score is the sum over the enumerated paths."""
    x = 2.0 * torch.randn(1, 3, 3, generator=torch.Generator().manual_seed(13))
    want = R.enumerate_paths(x[0].numpy(), 0)
    tok, lens, score, n_hyp = run(x, 3, 16, 3, blank=0)
    assert int(n_hyp[0]) == 9 == len(want)
    seen = set()
    for j in range(9):
        g = tuple(tok[0, j, :int(lens[0, j])].tolist())
        seen.add(g)
        p = want[g]
        assert abs(float(score[0, j]) - math.log(p)) <= 1e-5 * max(1.0, abs(math.log(p))), (g, float(score[0, j]), p)
    assert len(seen) == 9
    assert bool((score[0, :8] >= score[0, 1:9]).all()) and bool((score[0, 9:] == -INF).all())


def _tie_cases():
    g = torch.Generator().manual_seed(3)
    equal_row = torch.zeros(1, 1, 8)                                   # T = 1: one frame of equal logits
    mid = torch.randn(1, 3, 8, generator=g)
    mid[:, 1, :] = 0.5                                                 # a row of equal logits between two others
    cols = torch.randn(1, 2, 8, generator=g)
    cols[:, :, 3] = cols[:, :, 1]                                      # two equal columns in every frame
    first = torch.randn(1, 1, 8, generator=g)                          # first frame: 5 live candidates, W = 8
    return [("equal row", equal_row, 3), ("equal row between", mid, 4), ("equal columns", cols, 8),
            ("first frame", first, 8)]


@pytest.mark.parametrize("k", range(4))
def test_prefix_beam_ties_follow_the_flat_index(k):
    """Tied candidates are the same sums of the same operands in either precision, so the flat index decides alike;
    the first three cases must really tie in the reference (a zero gap)."""
    name, x, W = _tie_cases()[k]
    V, ml = 5, 4
    r64 = R.batch(x, V, W, BLANK, ml)
    if k < 3:
        assert min(r64[0]["boundary"], r64[0]["final"]) == 0.0, name
    else:
        assert len(r64[0]["prefixes"]) == 5 < W
    got = run(x, V, W, ml)
    compare(got, r64, W, ml, lambda v: 1e-5 * max(1.0, abs(v)))


def test_hyp_tokens_exact():
    B, W, ml, L = 2, 4, 6, 7
    BOS, EOS, PAD, IGN = 1, 9, 4, -1
    hyps = [[(5, 6, 7), (), (8, 8, 3, 5, 6, 7)], [(3,), (5, 5), (6, 7, 8, 3), (7,)]]
    tok = torch.full((B * W, ml), 2, dtype=torch.int64)
    lens = torch.zeros(B * W, dtype=torch.int32)
    for b, hs in enumerate(hyps):
        for j, g in enumerate(hs):
            tok[b * W + j, :len(g)] = torch.tensor(g, dtype=torch.int64)
            lens[b * W + j] = len(g)
    n_hyp = torch.tensor([3, 4], dtype=torch.int32)
    got = K().hyp_tokens(tok.to(dev), lens.to(dev), n_hyp.to(dev), B, W, L, BOS, EOS, PAD, IGN)
    want = [torch.cat(t) for t in zip(*(R.hyp_tokens(hs, W, L, BOS, EOS, PAD, IGN) for hs in hyps))]
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b)
    assert got[0].dtype == torch.int64 and got[2].dtype == torch.float32
    assert bool((got[2][3].cpu() == 0).all()) and bool((got[0][3].cpu() == PAD).all())       # the dead slot


@pytest.mark.parametrize("V,ld", [(5, 8), (250, 256), (257, 320)])
@pytest.mark.parametrize("L", [1, 7, 64])
def test_seq_logprob_matches_fp64(V, ld, L):
    """Against the fp64 log_softmax gather; bound 4 x the fp32 torch evaluation's own error, floor 1e-5 * max(1, |v|).
    Ignored positions do not count, a row of ignored positions sums to 0, dead slots are -inf."""
    g = torch.Generator().manual_seed(V + L)
    B, W = 2, 3
    N = B * W
    x = 3 * torch.randn(N, L, ld, generator=g)
    tgt = torch.randint(0, V, (N, L), generator=g)
    tgt[0, L // 2:] = -1
    tgt[1, :] = -1
    tgt[2, 0] = V - 1
    n_hyp = torch.tensor([3, 2], dtype=torch.int32)
    want = R.seq_logprob(x[:, :, :V], tgt, -1)
    f32 = torch.where(tgt != -1, torch.log_softmax(x[:, :, :V], -1).gather(2, tgt.clamp(min=0)[..., None])[..., 0],
                      torch.zeros(N, L)).sum(1)
    e32 = float((f32.double() - want).abs().max())
    got = K().seq_logprob(x.reshape(N * L, ld).to(dev), V, tgt.to(dev), -1, n_hyp.to(dev), W).cpu()
    assert float(got[5]) == -INF and float(got[1]) == 0.0
    worst = 0.0
    for n in range(5):
        bound = max(4 * e32, 1e-5 * max(1.0, abs(float(want[n]))))
        err = abs(float(got[n]) - float(want[n]))
        worst = max(worst, err / bound)
        assert err <= bound, (n, float(got[n]), float(want[n]), bound)
    print(f"V {V} L {L}: worst error / bound {worst:.3f}")
    alive = K().seq_logprob(x.reshape(N * L, ld).to(dev), V, tgt.to(dev), -1).cpu()
    assert torch.isfinite(alive).all() and torch.equal(alive[:5], got[:5])


def test_rescore_rank_order():
    att = torch.tensor([[-3.0, -1.0, -3.0, -INF], [-2.0, -2.0, -2.0, -2.0], [-5.0, float("nan"), -4.0, -6.0]])
    ctc = torch.tensor([[-1.0, -4.0, -1.0, -1.0], [-1.0, -1.0, -1.0, -1.0], [-1.0, -1.0, -INF, -2.0]])
    B, W = att.shape
    for aw, cw in ((1.0, 0.5), (1.0, 0.0), (0.7, 0.3)):
        score, order = K().rescore_rank(att.reshape(-1).to(dev), ctc.reshape(-1).to(dev), B, W, aw, cw)
        want = aw * att.double() + cw * ctc.double()
        want[torch.isinf(att) | torch.isinf(ctc) | torch.isnan(want)] = -INF
        assert torch.equal(order.cpu().long(), R.rank(want)), (aw, cw, order.cpu(), R.rank(want))
        s = score.cpu().view(B, W)
        assert torch.equal(torch.isinf(s), torch.isinf(want))
        fin = torch.isfinite(want)
        assert float((s.double()[fin] - want[fin]).abs().max()) <= 1e-6
    assert order.cpu()[1].tolist() == [0, 1, 2, 3]                      # equal scores: by slot
