"""asrx_edit_distance_long on the GPU: sequences of up to 4095 kept tokens, compared EXACTLY (integers, an optimum).

tests/edit_ref.py's `align` stops at 255 tokens and its packing at 511 substitutions, so this file carries its own
reference: edit_ref.packed_rows' running-minimum recursion on the packed cost edits * 2^13 + substitutions
(substitutions <= 4095 < 2^13, int64), cross-checked below against edit_ref.plain_distance (unit costs, no packing)
and against edit_ref.align where that applies.  Every call's outputs are pre-filled with garbage."""
import numpy as np
import pytest
import torch

from tests import edit_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
LENS = [0, 1, 255, 256, 257, 1023, 1024, 1025, 4095]
MAXL = 4095
EDIT = 1 << 13
GARBAGE = -123456789


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def long_align(hyp, ref):
    """(edits, sub, del, ins, reference tokens) of two sequences; (-2, -1, -1, -1, -1) if either keeps more than 4095
    tokens.  With t[j] = min(diagonal, up), row i is cur[j] = min over k <= j of t[k] + EDIT * (j - k)."""
    m, n = len(hyp), len(ref)
    if m > MAXL or n > MAXL:
        return (-2, -1, -1, -1, -1)
    if n == 0 or m == 0:
        p = EDIT * (m + n)
    else:
        r = np.asarray(ref, dtype=np.int64)
        step = EDIT * np.arange(n + 1, dtype=np.int64)
        prev = step.copy()
        t = np.empty(n + 1, dtype=np.int64)
        for i, h in enumerate(hyp, 1):
            t[0] = EDIT * i
            t[1:] = np.minimum(prev[:-1] + np.where(r == h, 0, EDIT + 1), prev[1:] + EDIT)
            prev = np.minimum.accumulate(t - step) + step
        p = int(prev[-1])
    edits, sub = p >> 13, p & (EDIT - 1)
    dele = (edits - sub - (m - n)) // 2
    return (edits, sub, dele, dele + m - n, n)


def reference(hyp, ref=None, hyp_lengths=None, ref_lengths=None, drop=(), stop=None, mode="pairs", W=1, n_hyp=None):
    """edit_ref.edit_distance with long_align: (dist int32 [N], counts int32 [N, 4])."""
    hyp = np.asarray(hyp)
    hs = [R.sequence(hyp[r], None if hyp_lengths is None else hyp_lengths[r], drop, stop) for r in range(hyp.shape[0])]
    if mode == "cross":
        G = hyp.shape[0] // W
        pairs = [(g * W + i, g * W + j, g, max(i, j)) for g in range(G) for i in range(W) for j in range(W)]
        rs = hs
    else:
        ref = np.asarray(ref)
        rs = [R.sequence(ref[r], None if ref_lengths is None else ref_lengths[r], drop, stop)
              for r in range(ref.shape[0])]
        pairs = [(n, n // W, n // W, n % W) for n in range(hyp.shape[0])] if mode == "group" else \
            [(n, n, 0, -1) for n in range(hyp.shape[0])]
    dist = np.empty(len(pairs), np.int32)
    counts = np.empty((len(pairs), 4), np.int32)
    for k, (h, r, g, slot) in enumerate(pairs):
        if mode != "pairs" and n_hyp is not None and slot >= int(n_hyp[g]):
            dist[k], counts[k] = -1, -1
            continue
        a = long_align(hs[h], rs[r])
        dist[k], counts[k] = a[0], a[1:]
    return dist, counts


def i32(a):
    return None if a is None else torch.tensor(list(a), dtype=torch.int32, device=dev)


def run(hyp, ref=None, hl=None, rl=None, drop=(), stop=None, mode="pairs", W=1, n_hyp=None, long=True):
    from asrx import kernels as K
    hd = torch.tensor(np.asarray(hyp), dtype=torch.int64, device=dev)
    rd = None if ref is None else torch.tensor(np.asarray(ref), dtype=torch.int64, device=dev)
    N = hd.shape[0] * (W if mode == "cross" else 1)
    out = (torch.full((N,), GARBAGE, dtype=torch.int32, device=dev),
           torch.full((N, 4), GARBAGE, dtype=torch.int32, device=dev))
    d, c = K.edit_distance(hd, rd, i32(hl), i32(rl), drop, stop, mode, W, i32(n_hyp), True, out, long=long)
    torch.cuda.synchronize()
    return d.cpu().numpy(), c.cpu().numpy()


def check(hyp, ref=None, hl=None, rl=None, both=False, **kw):
    """Run the long kernel and compare every output element with the reference; both: the short kernel must give the
    identical integers (inputs of at most 255 kept tokens).  Returns the reference outputs."""
    got_d, got_c = run(hyp, ref, hl, rl, **kw)
    want_d, want_c = reference(hyp, ref, hl, rl, **kw)
    assert got_d.tolist() == want_d.tolist()
    assert got_c.tolist() == want_c.tolist()
    if both:
        short_d, short_c = run(hyp, ref, hl, rl, long=False, **kw)
        assert short_d.tolist() == got_d.tolist() and short_c.tolist() == got_c.tolist()
    return want_d, want_c


def rows(n, cols, V, seed, lo=10):
    return np.random.default_rng(seed).integers(lo, lo + V, size=(n, cols))


def test_the_reference_agrees_with_the_plain_distance_and_the_short_reference():
    """Host only: the wide packing's edits are the textbook distance at a few hundred tokens, and its counts are
    edit_ref.align's where that one applies."""
    rng = np.random.default_rng(5)
    for m, n, V in ((300, 280, 3), (257, 400, 30), (120, 255, 2), (255, 255, 4)):
        a, b = rng.integers(0, V, m).tolist(), rng.integers(0, V, n).tolist()
        got = long_align(a, b)
        assert got[0] == R.plain_distance(a, b) and got[1] + got[2] + got[3] == got[0] and got[4] == n
        if max(m, n) <= 255:
            assert got == R.align(a, b)
    assert long_align([1] * 4096, [1]) == (-2, -1, -1, -1, -1) and long_align([1] * 4095, [1])[0] == 4094


@pytest.mark.parametrize("V", [2, 250])
def test_length_grid(V):
    """All 81 pairs of lengths around 255 / 256 (the short kernel's bound), 1024 and the limit, in one launch; V = 2
    makes almost every cell a tie."""
    pairs = [(m, n) for m in LENS for n in LENS]
    hyp, ref = rows(len(pairs), MAXL, V, 10 + V), rows(len(pairs), MAXL, V, 20 + V)
    d, c = check(hyp, ref, [m for m, _ in pairs], [n for _, n in pairs])
    k = pairs.index((0, 0))
    assert d[k] == 0 and c[k].tolist() == [0, 0, 0, 0]
    k = pairs.index((0, 4095))
    assert d[k] == 4095 and c[k].tolist() == [0, 4095, 0, 4095]
    k = pairs.index((4095, 0))
    assert d[k] == 4095 and c[k].tolist() == [0, 0, 4095, 0]
    assert (c[:, 0] + c[:, 1] + c[:, 2] == d).all()


def test_more_substitutions_than_the_short_packing_holds():
    """Disjoint vocabularies at 1000 x 1000 tokens: 1000 substitutions, which edits * 512 + substitutions would carry
    into the edit count.  Also 4095 x 4095 (the largest packed value) and identical rows."""
    a, b = rows(3, MAXL, 250, 3), rows(3, MAXL, 250, 4, lo=1000)
    d, c = check(a, b, [1000, 4095, 600], [1000, 4095, 1000])
    assert d.tolist() == [1000, 4095, 1000] and c[:, 0].tolist() == [1000, 4095, 600]
    d, c = check(a, a.copy(), [1000, 4095, 600], [1000, 4095, 600])
    assert (d == 0).all() and (c[:, :3] == 0).all()


def test_4096_kept_tokens_are_refused():
    """cols = 5000: what counts is the filtered length.  4095 kept tokens are scored, 4096 give -2 (counts -1), through
    the drop id, the length and the stop id."""
    cols = 5000
    hyp, ref = rows(4, cols, 5, 30), rows(4, cols, 5, 31)
    rng = np.random.default_rng(32)
    hyp[0, rng.permutation(cols)[:905]] = 0                # 4095 kept
    hyp[1, rng.permutation(cols)[:904]] = 0                # 4096 kept
    ref[:, 300:] = 0                                       # 300 kept
    ref[2, :] = rows(1, cols, 5, 33)[0]
    ref[2, rng.permutation(cols)[:904]] = 0                # the reference side too long
    hyp[2, 100:] = 0
    hyp[3, 4095:] = 0                                      # exactly the first 4095
    d, c = check(hyp, ref, drop=(0,))
    assert d[1] == -2 and d[2] == -2 and d[0] >= 3795 and c[1].tolist() == [-1] * 4 and c[0][3] == 300
    h2 = rows(2, cols, 5, 34)
    d, _ = check(h2, h2.copy(), [4095, 4096], [4095, 4096])
    assert d.tolist() == [0, -2]
    h2[0, 4095] = 3000
    h2[1, 4096] = 3000
    d, _ = check(h2, h2.copy(), stop=3000)
    assert d.tolist() == [0, -2]
    d, _ = check(h2, h2.copy(), [-3, 9999], [0, 9999], stop=3000)     # lengths outside the row are clamped
    assert d.tolist() == [0, -2]


def test_group_and_cross_modes_with_long_rows_and_n_hyp():
    """W = 3 hypotheses per sample against one reference, and all 3 x 3 pairs; absent slots give -1."""
    B, W, cols = 2, 3, 700
    hyp, ref = rows(B * W, cols, 4, 50), rows(B, 650, 4, 51)
    hl = [700, 300, 0, 256, 255, 640]
    d, c = check(hyp, ref, hl, [650, 257], mode="group", W=W, n_hyp=[3, 2])
    assert d[5] == -1 and c[5].tolist() == [-1] * 4 and (d[:5] >= 0).all()
    d, c = check(hyp, None, hl, mode="cross", W=W, n_hyp=[3, 2])
    dm = d.reshape(B, W, W)
    assert (dm[0] == dm[0].T).all() and (np.diag(dm[0]) == 0).all() and (dm[1, 2] == -1).all() and (dm[1, :, 2] == -1).all()
    check(hyp, ref, hl, [650, 257], mode="group", W=W)


@pytest.mark.parametrize("V", [2, 250])
def test_both_kernels_give_identical_integers_up_to_255_tokens(V):
    lens = [0, 1, 2, 63, 64, 65, 128, 192, 255]
    pairs = [(m, n) for m in lens for n in lens]
    hyp, ref = rows(len(pairs), 255, V, 60 + V), rows(len(pairs), 255, V, 70 + V)
    check(hyp, ref, [m for m, _ in pairs], [n for _, n in pairs], both=True)
    g = rows(6, 255, V, 80 + V)
    check(g, rows(2, 200, V, 81 + V), mode="group", W=3, n_hyp=[2, 3], both=True)
    check(g, None, [255, 100, 3, 0, 254, 64], mode="cross", W=3, n_hyp=[3, 1], both=True)
    wide = rows(3, 300, 5, 90)
    wide[:, 250:] = 0
    check(wide, wide[::-1].copy(), drop=(0,), stop=13, both=True)
