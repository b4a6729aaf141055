"""asrx_edit_distance and asrx_mbr_rank on the GPU against tests/edit_ref.py.

The distances and counts are integers and the objective is an optimum, not a tie rule: every output is compared
EXACTLY.  Every call's outputs are pre-filled with garbage, so an element the kernel leaves unwritten fails the
comparison.

MBR risks follow the project's tolerance (tests/test_gpu_ctc_beam_kernels.py): 4 x the error of the reference's own
fp32 run against fp64, floored at 1e-5 * max(1, |value|); the order is compared exactly wherever the smallest gap
between two fp64 risks is >= 10 x that bound, which must hold on at least 90 of the 100 generated cases."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import edit_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255]
GARBAGE = -123456789


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def i32(a):
    return None if a is None else torch.tensor(list(a), dtype=torch.int32, device=dev)


def run(hyp, ref=None, hl=None, rl=None, drop=(), stop=None, mode="pairs", W=1, n_hyp=None, counts=True):
    """One call on device copies of host rows (a torch tensor keeps its strides), outputs pre-filled with garbage;
    returns host (dist, counts)."""
    from asrx import kernels as K
    hd = hyp.to(dev) if torch.is_tensor(hyp) else torch.tensor(np.asarray(hyp), dtype=torch.int64, device=dev)
    rd = None if ref is None else (ref.to(dev) if torch.is_tensor(ref) else
                                   torch.tensor(np.asarray(ref), dtype=torch.int64, device=dev))
    N = hd.shape[0] * (W if mode == "cross" else 1)
    out = (torch.full((N,), GARBAGE, dtype=torch.int32, device=dev),
           torch.full((N, 4), GARBAGE, dtype=torch.int32, device=dev) if counts else None)
    d, c = K.edit_distance(hd, rd, i32(hl), i32(rl), drop, stop, mode, W, i32(n_hyp), counts, out)
    torch.cuda.synchronize()
    return d.cpu().numpy(), None if c is None else c.cpu().numpy()


def check(hyp, ref=None, hl=None, rl=None, **kw):
    """Run, and compare every output element with the reference; returns the reference outputs."""
    got_d, got_c = run(hyp, ref, hl, rl, **kw)
    kw.pop("counts", None)
    want_d, want_c = R.edit_distance(np.asarray(hyp), None if ref is None else np.asarray(ref), hl, rl, **kw)
    assert got_d.tolist() == want_d.tolist()
    if got_c is not None:
        assert got_c.tolist() == want_c.tolist()
    return want_d, want_c


def rows(n, cols, V, seed, lo=10):
    return np.random.default_rng(seed).integers(lo, lo + V, size=(n, cols))


@pytest.mark.parametrize("V", [2, 5, 250])
def test_length_grid(V):
    """All 144 pairs of lengths around every 64-column block edge, the empty sequence against itself and against 255
    included, in one launch; a small vocabulary makes almost every cell a tie."""
    pairs = [(m, n) for m in LENS for n in LENS]
    hyp, ref = rows(len(pairs), 255, V, 10 + V), rows(len(pairs), 255, V, 20 + V)
    d, c = check(hyp, ref, [m for m, _ in pairs], [n for _, n in pairs])
    k = pairs.index((0, 0))
    assert d[k] == 0 and c[k].tolist() == [0, 0, 0, 0]
    k = pairs.index((0, 255))
    assert d[k] == 255 and c[k].tolist() == [0, 255, 0, 255]
    k = pairs.index((255, 0))
    assert d[k] == 255 and c[k].tolist() == [0, 0, 255, 0]
    assert (c[:, 0] + c[:, 1] + c[:, 2] == d).all()


def test_identical_rows_and_rows_without_a_common_token():
    n = len(LENS)
    a = rows(n, 255, 250, 3)
    d, c = check(a, a.copy(), LENS, LENS)
    assert (d == 0).all() and (c[:, :3] == 0).all()
    b = rows(n, 255, 250, 4, lo=1000)                # disjoint vocabularies: max(m, n) edits, min(m, n) of them sub
    hl, rl = LENS, LENS[::-1]
    d, c = check(a, b, hl, rl)
    assert d.tolist() == [max(m, k) for m, k in zip(hl, rl)]
    assert c[:, 0].tolist() == [min(m, k) for m, k in zip(hl, rl)]


def test_the_rule_on_the_device():
    """hyp (a, b) against ref (b, c): 0 sub, 1 del, 1 ins (a diagonal-first backtrace would say 2 sub)."""
    d, c = check([[7, 8], [8, 9], [7, 7]], [[8, 9], [7, 8], [8, 7]])
    assert d.tolist() == [2, 2, 1] and c[0].tolist() == [0, 1, 1, 2] and c[2].tolist() == [1, 0, 0, 2]


def test_wide_rows_filtered_to_255_and_256_tokens():
    """cols = 300 > 255: what counts is the filtered length.  255 kept tokens are scored, 256 give -2 (counts -1)."""
    cols = 300
    hyp = rows(4, cols, 5, 30)
    ref = rows(4, cols, 5, 31)
    rng = np.random.default_rng(32)
    hyp[0, rng.permutation(cols)[:45]] = 0                 # 255 kept
    hyp[1, rng.permutation(cols)[:44]] = 0                 # 256 kept: unsupported
    ref[:, 200:] = 0                                       # 200 kept
    ref[2, :] = rows(1, cols, 5, 33)[0]
    ref[2, rng.permutation(cols)[:44]] = 0                 # the reference side too long
    hyp[2, 100:] = 0
    hyp[3, 255:] = 0                                       # exactly the first 255
    d, c = check(hyp, ref, drop=(0,))
    assert d[1] == -2 and d[2] == -2 and d[0] >= 55 and c[1].tolist() == [-1] * 4 and c[0][3] == 200
    # the same through the length and the stop id instead of the drop id
    h2 = rows(2, cols, 5, 34)
    d, _ = check(h2, h2.copy(), [255, 256], [255, 256])
    assert d.tolist() == [0, -2]
    h2[0, 255] = 3000
    h2[1, 256] = 3000
    d, _ = check(h2, h2.copy(), stop=3000)
    assert d.tolist() == [0, -2]


def test_row_strides_and_lengths_outside_the_row():
    """ld > cols on both sides (column slices of wider tensors); lengths below 0 and above cols are clamped."""
    big_h = torch.from_numpy(rows(6, 100, 5, 40))
    big_r = torch.from_numpy(rows(6, 90, 5, 41))
    hyp, ref = big_h.to(dev)[:, :70], big_r.to(dev)[:, :33]
    assert hyp.stride(0) == 100 and ref.stride(0) == 90
    hl, rl = [-5, 0, 70, 71, 1000, 2 ** 31 - 1], [33, -1, 34, 0, -2 ** 31, 12]
    got_d, got_c = run(hyp, ref, hl, rl)
    want_d, want_c = R.edit_distance(big_h[:, :70].numpy(), big_r[:, :33].numpy(), hl, rl)
    assert got_d.tolist() == want_d.tolist() and got_c.tolist() == want_c.tolist()
    assert want_c[:, 3].tolist() == [33, 0, 33, 0, 0, 12] and want_d[0] == 33 and want_d[1] == 0


@pytest.mark.parametrize("drop", [(), (11,), (11, 12, 13, 2 ** 40)])
@pytest.mark.parametrize("stop_at", [None, 0, 77])
def test_drop_and_stop(drop, stop_at):
    """ndrop 0, 1 and 4 (one id beyond 32 bits); a stop id in the first position, in the middle (after a 64-entry
    round), and absent.  The stop id also occurs after its first occurrence, and among the dropped ids' neighbours."""
    STOP = 999
    hyp, ref = rows(5, 150, 6, 50), rows(5, 140, 6, 51)
    hyp[0, 20] = 2 ** 40
    ref[1, 5] = 2 ** 40
    if stop_at is not None:
        hyp[:, stop_at] = STOP
        hyp[:, 120] = STOP
        ref[::2, stop_at + 3] = STOP
    d, c = check(hyp, ref, drop=drop, stop=STOP)
    if stop_at == 0:
        assert (c[:, 2] == 0).all() and (d == c[:, 1]).all()      # empty hypotheses: all deletions
    d2, _ = check(hyp, ref, drop=drop, stop=None)                 # no stop: the id is an ordinary token
    d3, _ = check(hyp, ref, drop=drop, stop=-7)
    assert d2.tolist() == d3.tolist()


def test_dropped_tokens_around_the_64_entry_boundaries():
    """Dropped entries on both sides of each 64-entry load round and kept counts that cross the 64-column block edge:
    the left-packing prefix carries across rounds."""
    cols = 200
    hyp, ref = rows(6, cols, 4, 60), rows(6, cols, 4, 61)
    for r, idx in enumerate(([62, 63, 64, 65], [63], [64], [0, 63, 64, 127, 128, 191, 192, 199],
                             list(range(60, 70)), list(range(0, 200, 2)))):
        hyp[r, idx] = 0
        ref[r, [i + 1 for i in idx if i + 1 < cols]] = 0
    d, c = check(hyp, ref, drop=(0,))
    assert c[:, 3].tolist() == [196, 199, 199, 193, 190, 100]
    check(hyp, ref, [130] * 6, [129] * 6, drop=(0,))


@pytest.mark.parametrize("W", [1, 3, 16])
def test_group_mode(W):
    B, cols = 4, 40
    ref = rows(B, 37, 5, 70)
    hyp = rows(B * W, cols, 5, 71)
    hyp[::2, :30] = np.repeat(ref, W, axis=0)[::2, :30]          # some close hypotheses
    n_hyp = [0, 1, W, max(W - 1, 0)]
    d, c = check(hyp, ref, mode="group", W=W, n_hyp=n_hyp, drop=(10,))
    d = d.reshape(B, W)
    assert (d[0] == -1).all() and d[1, 0] >= 0 and (d[1, 1:] == -1).all() and (d[2] >= 0).all()
    assert (c.reshape(B, W, 4)[0] == -1).all()
    check(hyp, ref, mode="group", W=W, n_hyp=None, hl=[cols - (i % 7) for i in range(B * W)], rl=[37, 0, 5, 36])


@pytest.mark.parametrize("W", [1, 3, 16])
def test_cross_mode(W):
    """All W x W pairs of each group: symmetric, zero diagonal, del and ins swapped across it; absent slots -1."""
    G, cols = 3, 70
    base = rows(G, cols, 6, 80)
    hyp = np.repeat(base, W, axis=0)
    rng = np.random.default_rng(81)
    for r in range(G * W):                                       # each hypothesis: a few edits of its group's base
        for _ in range(r % 5):
            hyp[r, rng.integers(0, cols)] = rng.integers(10, 16)
    hl = [cols - (r % 4) * 3 for r in range(G * W)]
    d, c = check(hyp, hl=hl, mode="cross", W=W)
    d, c = d.reshape(G, W, W), c.reshape(G, W, W, 4)
    for g in range(G):
        assert (d[g] == d[g].T).all() and (np.diag(d[g]) == 0).all()
        assert (c[g, :, :, 0] == c[g, :, :, 0].T).all() and (c[g, :, :, 1] == c[g, :, :, 2].T).all()
    n_hyp = [0, 1, W]
    d, c = check(hyp, hl=hl, mode="cross", W=W, n_hyp=n_hyp, drop=(12,), stop=15)
    d = d.reshape(G, W, W)
    assert (d[0] == -1).all() and d[1, 0, 0] == 0 and (d[1, 1:, :] == -1).all() and (d[1, :, 1:] == -1).all()
    assert (d[2] >= 0).all()


def test_null_counts_bitwise_repeat_and_graph_replay():
    from asrx import kernels as K
    pairs = [(m, n) for m in LENS[::2] for n in LENS[1::2]]
    hyp, ref = rows(len(pairs), 255, 3, 90), rows(len(pairs), 255, 3, 91)
    hl, rl = [m for m, _ in pairs], [n for _, n in pairs]
    want_d, want_c = check(hyp, ref, hl, rl)
    d_only, none = run(hyp, ref, hl, rl, counts=False)            # counts NULL: dist alone, the same values
    assert none is None and d_only.tolist() == want_d.tolist()
    again_d, again_c = run(hyp, ref, hl, rl)
    assert again_d.tobytes() == want_d.astype(np.int32).tobytes() and again_c.tobytes() == want_c.tobytes()
    hd, rd = torch.tensor(hyp, device=dev), torch.tensor(ref, device=dev)
    hld, rld = i32(hl), i32(rl)
    out = (torch.empty(len(pairs), dtype=torch.int32, device=dev),
           torch.empty(len(pairs), 4, dtype=torch.int32, device=dev))
    K.edit_distance(hd, rd, hld, rld, out=out)                    # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.edit_distance(hd, rd, hld, rld, out=out)
    for _ in range(2):
        out[0].fill_(GARBAGE)
        out[1].fill_(GARBAGE)
        g.replay()
        torch.cuda.synchronize()
        assert out[0].cpu().numpy().tolist() == want_d.tolist() and out[1].cpu().numpy().tolist() == want_c.tolist()


def test_python_surface():
    """asrx.edit_distance: shapes per mode, host inputs moved to the device, the reference's values."""
    import asrx
    hyp = torch.from_numpy(rows(6, 30, 5, 95))
    ref = torch.from_numpy(rows(2, 28, 5, 96))
    e = asrx.edit_distance(hyp, torch.from_numpy(rows(6, 28, 5, 97)), drop=(10,))
    assert all(t.is_cuda and t.dtype == torch.int32 and t.shape == (6,) for t in e)
    wd, wc = R.edit_distance(hyp.numpy(), rows(6, 28, 5, 97), drop=(10,))
    assert e.dist.tolist() == wd.tolist() and torch.stack(e[1:], 1).tolist() == wc.tolist()
    e = asrx.edit_distance(hyp.view(2, 3, 30), ref, mode="group", n_hyp=torch.tensor([3, 2]), stop=12)
    wd, wc = R.edit_distance(hyp.numpy(), ref.numpy(), stop=12, mode="group", W=3, n_hyp=[3, 2])
    assert e.dist.shape == (2, 3) and e.dist.reshape(-1).tolist() == wd.tolist()
    assert e.ref_len.reshape(-1).tolist() == wc[:, 3].tolist() and e.dele.reshape(-1).tolist() == wc[:, 1].tolist()
    e = asrx.edit_distance(hyp.view(2, 3, 30).to(dev), mode="cross", hyp_lengths=torch.full((2, 3), 25))
    wd, wc = R.edit_distance(hyp.numpy(), hyp_lengths=[25] * 6, mode="cross", W=3)
    assert e.dist.shape == (2, 3, 3) and e.dist.reshape(-1).tolist() == wd.tolist()
    assert e.ins.reshape(-1).tolist() == wc[:, 2].tolist()


# ------------------------------------------------------------------------------------------------ asrx_mbr_rank

def mbr(dist, score, n_hyp=None, scale=1.0):
    """dist [B][W][W], score [B][W] host arrays -> host (risk [B, W], order [B, W])."""
    from asrx import kernels as K
    dist = np.asarray(dist, dtype=np.int32)
    B, W = dist.shape[:2]
    risk, order = K.mbr_rank(torch.tensor(dist, device=dev).reshape(-1),
                             torch.tensor(np.asarray(score, dtype=np.float32), device=dev).reshape(-1), B, W, scale,
                             i32(n_hyp))
    torch.cuda.synchronize()
    return risk.cpu().numpy(), order.cpu().numpy()


@functools.lru_cache(maxsize=None)
def mbr_cases():
    """100 n-best lists: W distinct hypotheses, each 0-4 random edits of a common base of 8-40 tokens, scores
    ~ N(0, 2) sorted descending.  (dist [W][W], score [W]) with the distances from the reference."""
    rng = np.random.default_rng(2024)
    cases = []
    while len(cases) < 100:
        W = (2, 3, 8, 16)[len(cases) % 4]
        base = list(rng.integers(0, 30, size=int(rng.integers(8, 41))))
        hyps = []
        while len(hyps) < W:
            h = list(base)
            for _ in range(int(rng.integers(0, 5))):
                k = int(rng.integers(0, 3))
                p = int(rng.integers(0, len(h) + (k == 1)))
                if k == 0 and h:
                    h[p] = int(rng.integers(0, 30))
                elif k == 1:
                    h.insert(p, int(rng.integers(0, 30)))
                elif len(h) > 1:
                    del h[p]
            if h not in hyps:
                hyps.append(h)
        dist = R.cross_distances(hyps)
        score = np.sort(rng.normal(0.0, 2.0, size=W).astype(np.float32))[::-1].copy()
        cases.append((np.array(dist, dtype=np.int32), score))
    return cases


def test_mbr_rank_random_lists():
    worst, exact = 0.0, 0
    for W in (2, 3, 8, 16):
        group = [c for c in mbr_cases() if c[0].shape[0] == W]
        risk, order = mbr(np.stack([d for d, _ in group]), np.stack([s for _, s in group]))
        for b, (dist, score) in enumerate(group):
            r64, live, bnd, gap = R.mbr_check(dist, score)
            assert live.all()
            err = np.abs(risk[b].astype(np.float64) - r64)
            worst = max(worst, float((err / bnd).max()))
            assert (err <= bnd).all(), (W, b, err, bnd)
            assert sorted(order[b].tolist()) == list(range(W))
            if gap >= 10 * bnd.max():
                exact += 1
                assert order[b].tolist() == R.mbr_order(r64), (W, b)
    print(f"worst risk error / bound {worst:.3f}; order compared exactly on {exact} of 100 cases")
    assert exact >= 90


def test_mbr_rank_duplicates_medoid_dead_slots_and_one_hypothesis():
    # slots 1 and 3 are the same hypothesis: identical dist rows, bitwise-equal risks, slot order
    hyps = [[1, 2, 3, 4], [1, 2, 3], [1, 9, 3, 4, 5], [1, 2, 3], [7, 7]]
    dist = np.array([[R.align(a, b)[0] for b in hyps] for a in hyps])
    score = [0.5, -0.25, -1.0, -3.0, -0.5]
    risk, order = mbr([dist], [score])
    assert risk[0, 1].tobytes() == risk[0, 3].tobytes()
    o = order[0].tolist()
    assert o.index(1) + 1 == o.index(3)
    r64, _, bnd, _ = R.mbr_check(dist, score)
    assert (np.abs(risk[0] - r64) <= bnd).all()
    # scale 0: the posterior is uniform, the first slot is the medoid
    risk0, order0 = mbr([dist], [score], scale=0.0)
    mean = dist.mean(axis=1)
    assert (np.abs(risk0[0] - mean) <= 1e-5 * np.maximum(1.0, mean)).all()
    assert order0[0, 0] == int(np.argmin(mean)) and risk0[0, 1].tobytes() == risk0[0, 3].tobytes()
    # dead slots: by n_hyp, by a -inf and by a NaN score, and by the absent (-1) diagonal of a CROSS matrix; their
    # columns hold values that would poison a sum
    d = dist.copy()
    d[:, 4] = 10 ** 9
    d[4, :] = -1
    d[:, 2] = -1
    sc = np.array([0.5, -INF, float("nan"), -3.0, 0.1], dtype=np.float32)
    risk, order = mbr([d, d, dist], [sc, [0.5, -0.25, -1.0, -3.0, -0.5], score], n_hyp=[4, 2, 0])
    want, live, bnd, _ = R.mbr_check(d, sc, 4)
    assert list(live) == [True, False, False, True, False]
    assert np.isposinf(risk[0][[1, 2, 4]]).all() and (np.abs(risk[0][[0, 3]] - want[[0, 3]]) <= bnd[[0, 3]]).all()
    assert order[0].tolist() == R.mbr_order(want) and order[0].tolist()[2:] == [1, 2, 4]
    want, live, bnd, _ = R.mbr_check(d, [0.5, -0.25, -1.0, -3.0, -0.5], 2)
    assert list(live) == [True, True, False, False, False] and np.isposinf(risk[1][2:]).all()
    assert (np.abs(risk[1][:2] - want[:2]) <= bnd[:2]).all() and order[1].tolist() == R.mbr_order(want)
    assert np.isposinf(risk[2]).all() and order[2].tolist() == [0, 1, 2, 3, 4]        # nothing live: slot order
    # W = 1
    risk, order = mbr([[[0]], [[0]]], [[-2.5], [-INF]])
    assert risk.tolist() == [[0.0], [INF]] and order.tolist() == [[0], [0]]
