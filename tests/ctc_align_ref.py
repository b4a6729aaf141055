"""Forced-alignment test reference (host only, numpy): the CTC Viterbi recursion of asrx_ctc_align with its tie rule in
fp64 (the reference) or fp32 (to measure the error of a plain single-precision run, from which the kernel tolerances
derive), the on-path decision margin, a path checker and re-scorer, and a brute-force maximum over all V^T frame paths
for tiny cases."""
import itertools
import math

import numpy as np

from tests.ctc_ref import collapse


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def no_alignment(T, lmax):
    return dict(feasible=False, score=-math.inf, frame_pos=np.full(T, -1, np.int32), frame_logp=np.zeros(T),
                start=np.full(lmax, -1, np.int32), end=np.full(lmax, -1, np.int32), conf=np.zeros(lmax),
                margin=math.inf)


def spans_of(frame_pos, frame_logp, L, lmax):
    """Run boundaries and exp(mean log-probability) per label from a frame-level path."""
    start, end, conf = np.full(lmax, -1, np.int32), np.full(lmax, -1, np.int32), np.zeros(lmax)
    for u in range(L):
        ts = np.nonzero(np.asarray(frame_pos) == u)[0]
        if len(ts):
            start[u], end[u] = ts[0], ts[-1] + 1
            s = 0.0
            for t in range(ts[0], ts[-1] + 1):
                s += float(frame_logp[t])
            conf[u] = math.exp(s / (end[u] - start[u]))
    return start, end, conf


def viterbi(logits, target, blank=0, frames=None, lmax=None, dtype=np.float64):
    """logits (T, V), target: the L labels.  The best path over the first `frames` frames (None: T) under
    asrx_ctc_align's definition and tie rule, every operation in `dtype`.  Returns a dict: feasible, score, frame_pos
    (T,) (-1: blank / past `frames`), frame_logp (T,), start / end / conf (lmax,), margin (the smallest gap, over the
    end choice and every backpointer on the path, between the chosen predecessor and the best other one)."""
    logits = np.asarray(logits)
    T, V = logits.shape
    target = [int(c) for c in target]
    L = len(target)
    lmax = L if lmax is None else lmax
    Tb = T if frames is None else max(0, min(T, int(frames)))
    if L > lmax or any(c < 0 or c >= V or c == blank for c in target):
        return no_alignment(T, lmax)
    repeats = sum(1 for u in range(1, L) if target[u] == target[u - 1])
    if Tb < L + repeats:
        return no_alignment(T, lmax)
    out = no_alignment(T, lmax)
    out["feasible"] = True
    if Tb == 0:
        out["score"] = 0.0
        return out
    lp = log_softmax(logits[:Tb], dtype)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = target
    can_skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        can_skip[s] = ext[s] != ext[s - 2]
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype)
    a[0] = lp[0, blank]
    if L:
        a[1] = lp[0, ext[1]]
    back = np.zeros((Tb, S), np.int8)
    gaps = np.full((Tb, S), np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tb):
            stay = a
            one = np.concatenate(([ninf], a))[:S]
            two = np.concatenate(([ninf, ninf], a))[:S]
            two = np.where(can_skip, two, ninf)
            best, ch = stay.copy(), np.zeros(S, np.int8)
            m1 = one > best
            best, ch = np.where(m1, one, best), np.where(m1, 1, ch)
            m2 = two > best
            best, ch = np.where(m2, two, best), np.where(m2, 2, ch)
            cands = np.stack([stay, one, two]).astype(np.float64)
            cands[ch, np.arange(S)] = -np.inf
            g = best.astype(np.float64) - cands.max(axis=0)
            gaps[t] = np.where(np.isnan(g), np.inf, g)
            back[t] = ch
            a = (best + lp[t, ext]).astype(dtype)
    if L == 0:
        s, margin = 0, math.inf
    else:
        s = 2 * L if a[2 * L] > a[2 * L - 1] else 2 * L - 1
        margin = abs(float(a[2 * L]) - float(a[2 * L - 1]))
        if math.isnan(margin):
            margin = math.inf
    score = float(a[s])
    if not score > -math.inf:
        return no_alignment(T, lmax)
    states = np.zeros(Tb, np.int64)
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        if t > 0:
            margin = min(margin, float(gaps[t, s]))
            s -= int(back[t, s])
    assert states[0] in (0, 1)
    pos = np.full(T, -1, np.int32)
    flp = np.zeros(T)
    for t in range(Tb):
        st = int(states[t])
        pos[t] = (st - 1) // 2 if st & 1 else -1
        flp[t] = float(lp[t, ext[st]])
    out.update(score=score, frame_pos=pos, frame_logp=flp, margin=margin)
    out["start"], out["end"], out["conf"] = spans_of(pos, flp, L, lmax)
    return out


def path_is_valid(frame_pos, target, frames):
    """frame_pos (T,): positions 0 .. L-1 in order over the first `frames` frames, each at least once, a blank between
    adjacent equal labels, -1 beyond."""
    pos = [int(p) for p in frame_pos]
    L = len(target)
    if any(p != -1 for p in pos[frames:]):
        return False
    prev, seen = -1, -1      # previous frame's position, highest position seen
    for p in pos[:frames]:
        if p != -1:
            if p == seen:
                if prev != p:             # came back to a label after leaving it
                    return False
            elif p == seen + 1:
                if prev == seen and seen >= 0 and target[p] == target[seen]:
                    return False          # adjacent equal labels with no blank between
                seen = p
            else:
                return False
        prev = p
    return seen == L - 1


def rescore(logits, target, blank, frame_pos, frames):
    """fp64 log-probability of the frame-level path: (total, per-frame (T,))."""
    T = np.asarray(logits).shape[0]
    flp = np.zeros(T)
    if frames:
        lp = log_softmax(np.asarray(logits)[:frames])
        for t in range(frames):
            p = int(frame_pos[t])
            flp[t] = lp[t, blank if p < 0 else int(target[p])]
    return float(flp.sum()), flp


def bound(err32, value):
    """The project's rule (tests/test_gpu_ctc_beam_kernels.py): 4 x the fp32 reference's own error, floored at
    1e-5 * max(1, |value|)."""
    return max(4.0 * err32, 1e-5 * max(1.0, abs(value)))


def brute_force(logits, target, blank=0):
    """(best log-probability, the paths that reach it) over every length-T path that collapses to `target` (fp64);
    (-inf, []) if none does."""
    logits = np.asarray(logits)
    T, V = logits.shape
    lp = log_softmax(logits)
    best, arg = -math.inf, []
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) == list(target):
            s = sum(float(lp[t, c]) for t, c in enumerate(path))
            if s > best + 1e-12:
                best, arg = s, [path]
            elif abs(s - best) <= 1e-12:
                arg.append(path)
    return best, arg


def symbols_of(frame_pos, target, blank, frames):
    return tuple(blank if int(p) < 0 else int(target[int(p)]) for p in frame_pos[:frames])


def planted(T, V, target, boost, noise, seed, blank=0, ld=None):
    """Logits (T, ld) with a monotone alignment of `target` planted: `noise` x N(0, 1) everywhere, `boost` added to
    the planted symbol of every frame.  Labels get about equal runs; adjacent equal labels are separated by a
    planted blank frame, the remaining frames are blanks spread between the labels."""
    rng = np.random.default_rng(seed)
    ld = V if ld is None else ld
    x = (noise * rng.standard_normal((T, ld))).astype(np.float32)
    L = len(target)
    if L:
        edges = np.linspace(0, T, L + 1).astype(int)
        for u in range(L):
            lo, hi = edges[u], edges[u + 1]
            rep = u > 0 and target[u] == target[u - 1]
            for t in range(lo, hi):
                first_blank = (rep and t == lo and hi - lo >= 2)
                x[t, blank if first_blank else target[u]] += boost
    else:
        x[:, blank] += boost
    return x
