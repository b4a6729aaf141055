"""Host reference for asrx_edit_distance and asrx_mbr_rank (pure Python / numpy, no GPU).

The distance minimises (edits, substitutions) lexicographically.  `align` is the ordinary min-plus recursion on the
packed cost edits * 512 + substitutions (a match costs 0, a substitution 513, an insertion or deletion 512);
`exhaustive` recurses over every alignment and keeps the lexicographic minimum of the explicit pair, so it does not
depend on the packing.  A deletion is a reference token without a hypothesis counterpart, an insertion a hypothesis
token without a reference counterpart."""
import functools
import math

import numpy as np

EDIT = 512
MAXL = 255


def sequence(row, length=None, drop=(), stop=None):
    """The sequence of a row: its first `length` entries (None: all; clamped to the row), cut before the first `stop`
    (None or negative: no stop), without the `drop` ids."""
    row = [int(t) for t in row]
    n = len(row) if length is None else min(max(int(length), 0), len(row))
    out = []
    for t in row[:n]:
        if stop is not None and stop >= 0 and t == stop:
            break
        if t not in drop:
            out.append(t)
    return out


def packed(hyp, ref):
    """The optimum as edits * 512 + substitutions: one row of the DP at a time."""
    prev = [EDIT * j for j in range(len(ref) + 1)]
    for i, h in enumerate(hyp, 1):
        cur = [EDIT * i]
        for j, r in enumerate(ref, 1):
            cur.append(min(prev[j - 1] + (0 if h == r else EDIT + 1), prev[j] + EDIT, cur[j - 1] + EDIT))
        prev = cur
    return prev[-1]


def packed_rows(hyp, ref):
    """`packed`, one numpy row at a time (the long GPU cases): with t[j] = min(diagonal, up) the row is
    cur[j] = min over k <= j of t[k] + 512 * (j - k), a running minimum of t[k] - 512 * k."""
    n = len(ref)
    if n == 0:
        return EDIT * len(hyp)
    r = np.asarray(ref, dtype=np.int64)
    step = EDIT * np.arange(n + 1, dtype=np.int64)
    prev = step.copy()
    for i, h in enumerate(hyp, 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = EDIT * i
        t[1:] = np.minimum(prev[:-1] + np.where(r == h, 0, EDIT + 1), prev[1:] + EDIT)
        prev = np.minimum.accumulate(t - step) + step
    return int(prev[-1])


def align(hyp, ref):
    """(edits, sub, del, ins, reference tokens) of two sequences; (-2, -1, -1, -1, -1) if either is longer than 255."""
    m, n = len(hyp), len(ref)
    if m > MAXL or n > MAXL:
        return (-2, -1, -1, -1, -1)
    p = packed(hyp, ref) if m * n <= 4096 else packed_rows(hyp, ref)
    edits, sub = p >> 9, p & 511
    dele = (edits - sub - (m - n)) // 2
    return (edits, sub, dele, dele + m - n, n)


def cross_distances(seqs):
    """edits[i][j] of every pair of `seqs` (each at most 255 tokens): packed_rows on all pairs at once."""
    W = len(seqs)
    lens = np.array([len(q) for q in seqs])
    n = int(lens.max()) if W else 0
    tok = np.full((W, n), -1, dtype=np.int64)
    for k, q in enumerate(seqs):
        tok[k, :len(q)] = q
    step = EDIT * np.arange(n + 1, dtype=np.int64)
    prev = np.broadcast_to(step, (W, W, n + 1)).copy()        # [hyp i][ref j][column]
    out = np.zeros((W, W), dtype=np.int64)
    for i in range(n + 1):
        if i > 0:
            t = np.empty_like(prev)
            t[:, :, 0] = EDIT * i
            cost = np.where(tok[:, i - 1][:, None, None] == tok[None, :, :], 0, EDIT + 1)
            t[:, :, 1:] = np.minimum(prev[:, :, :-1] + cost, prev[:, :, 1:] + EDIT)
            prev = np.minimum.accumulate(t - step, axis=2) + step
        done = lens == i
        if done.any():
            out[done] = prev[done][:, np.arange(W), lens]
    return out >> 9


def exhaustive(hyp, ref):
    """(edits, sub, del, ins) minimising (edits, sub) over ALL alignments, by plain recursion on explicit tuples.  For
    short sequences only."""
    hyp, ref = tuple(hyp), tuple(ref)

    @functools.lru_cache(maxsize=None)
    def go(i, j):
        # every way to align hyp[i:] with ref[j:]: the set of reachable (edits, sub, del, ins) is reduced to its
        # lexicographic minimum on (edits, sub); del and ins follow from those and the lengths
        if i == len(hyp):
            return (len(ref) - j, 0, len(ref) - j, 0)
        if j == len(ref):
            return (len(hyp) - i, 0, 0, len(hyp) - i)
        cands = []
        e, s, d, k = go(i + 1, j + 1)
        cands.append((e, s, d, k) if hyp[i] == ref[j] else (e + 1, s + 1, d, k))
        e, s, d, k = go(i + 1, j)
        cands.append((e + 1, s, d, k + 1))
        e, s, d, k = go(i, j + 1)
        cands.append((e + 1, s, d + 1, k))
        return min(cands, key=lambda c: (c[0], c[1]))

    return go(0, 0)


def plain_distance(hyp, ref):
    """The textbook Levenshtein distance (unit costs), independent of the packing."""
    prev = list(range(len(ref) + 1))
    for i, h in enumerate(hyp, 1):
        cur = [i]
        for j, r in enumerate(ref, 1):
            cur.append(min(prev[j - 1] + (h != r), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def edit_distance(hyp, ref=None, hyp_lengths=None, ref_lengths=None, drop=(), stop=None, mode="pairs", W=1,
                  n_hyp=None):
    """asrx_edit_distance on host rows: hyp (rows, cols), ref (rows', cols') array-likes.  Returns (dist int32 [N],
    counts int32 [N, 4]) with the kernel's -1 / -2 conventions."""
    hyp = np.asarray(hyp)
    hs = [sequence(hyp[r], None if hyp_lengths is None else hyp_lengths[r], drop, stop) for r in range(hyp.shape[0])]
    if mode == "cross":
        G = hyp.shape[0] // W
        pairs = [(g * W + i, g * W + j, g, max(i, j)) for g in range(G) for i in range(W) for j in range(W)]
        rs = hs
    else:
        ref = np.asarray(ref)
        rs = [sequence(ref[r], None if ref_lengths is None else ref_lengths[r], drop, stop)
              for r in range(ref.shape[0])]
        if mode == "group":
            pairs = [(n, n // W, n // W, n % W) for n in range(hyp.shape[0])]
        else:
            pairs = [(n, n, 0, -1) for n in range(hyp.shape[0])]
    dist = np.empty(len(pairs), np.int32)
    counts = np.empty((len(pairs), 4), np.int32)
    for k, (h, r, g, slot) in enumerate(pairs):
        if mode != "pairs" and n_hyp is not None and slot >= int(n_hyp[g]):
            dist[k], counts[k] = -1, -1
            continue
        a = align(hs[h], rs[r])
        dist[k], counts[k] = a[0], a[1:]
    return dist, counts


def mbr_risk(dist, score, n_hyp=None, scale=1.0, dtype=np.float64):
    """Risks of one sample: dist [W][W] ints, score [W].  Slot j is live if j < n_hyp, its score is finite and its own
    distance is >= 0; p_j = exp(scale * (s_j - max live s)) / sum, risk_i = sum over live j (ascending) of
    p_j * dist[i][j], all in `dtype`; +inf for a dead slot.  Returns (risk [W] of dtype, live [W] bool)."""
    dist = np.asarray(dist)
    W = dist.shape[0]
    s = np.asarray(score, dtype=np.float32)
    nh = W if n_hyp is None else int(n_hyp)
    live = np.array([j < nh and math.isfinite(float(s[j])) and dist[j][j] >= 0 for j in range(W)])
    risk = np.full(W, np.inf, dtype=dtype)
    if not live.any():
        return risk, live
    mx = dtype(max(float(s[j]) for j in range(W) if live[j]))
    e = np.zeros(W, dtype=dtype)
    for j in range(W):
        if live[j]:
            d = dtype(s[j]) - mx
            e[j] = dtype(1.0) if d == 0 else np.exp(dtype(scale) * d, dtype=dtype)
    tot = dtype(0.0)
    for j in range(W):
        tot = dtype(tot + e[j])
    for i in range(W):
        if not live[i]:
            continue
        acc = dtype(0.0)
        for j in range(W):
            if live[j]:
                acc = dtype(acc + dtype(e[j] / tot) * dtype(dist[i][j]))
        risk[i] = acc
    return risk, live


def mbr_order(risk):
    """Slots by (risk ascending, slot ascending); +inf (dead) slots last."""
    return sorted(range(len(risk)), key=lambda j: (float(risk[j]), j))


def bound(err, value):
    """The project's tolerance: 4 x the reference's own fp32-against-fp64 error, floored at 1e-5 * max(1, |value|)."""
    return max(4.0 * err, 1e-5 * max(1.0, abs(value)))


def mbr_check(dist, score, n_hyp=None, scale=1.0):
    """(risk fp64, live, per-slot bound, smallest gap between two live fp64 risks (inf with < 2 live slots))."""
    r64, live = mbr_risk(dist, score, n_hyp, scale, np.float64)
    r32, _ = mbr_risk(dist, score, n_hyp, scale, np.float32)
    bnd = np.array([bound(abs(float(r32[j]) - float(r64[j])), float(r64[j])) if live[j] else 0.0
                    for j in range(len(r64))])
    lv = sorted(float(r64[j]) for j in range(len(r64)) if live[j])
    gap = min((b - a for a, b in zip(lv, lv[1:])), default=math.inf)
    return r64, live, bnd, gap


def wavefront(hyp, ref):
    """The kernel's own schedule, lane by lane, on the host: 64-column blocks of the reference, lane l computing row
    s - l at step s from its previous value, lane l - 1's previous value and the value that lane delivered one step
    earlier, the last column of a block kept as the next block's boundary.  Returns the packed optimum."""
    m, n = len(hyp), len(ref)
    if m == 0 or n == 0:
        return EDIT * (m + n)
    bd = [EDIT * i for i in range(m + 1)]
    v = [0] * 64
    for c0 in range(0, n, 64):
        last = min(n - 1 - c0, 63)
        v = [EDIT * (c0 + l + 1) for l in range(64)]
        lp = [EDIT * (c0 + l) for l in range(64)]
        for s in range(m + last):
            fill = bd[min(s + 1, m)]
            left = [fill] + v[:63]
            nv = list(v)
            for l in range(64):
                i = s - l
                if 0 <= i < m:
                    rt = ref[min(c0 + l, n - 1)]
                    nv[l] = min(min(v[l], left[l]) + EDIT, lp[l] + (0 if hyp[i] == rt else EDIT + 1))
            if 0 <= s - 63 < m:
                bd[s - 63 + 1] = nv[63]
            v, lp = nv, left
    return v[(n - 1) & 63]
