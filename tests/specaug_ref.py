"""numpy restatement of asrx_specaug (asr-transformer_amd/csrc/specaug.hip; the rule is DESIGN.md §16), test oracle
only.  The plan is exact integer arithmetic over tests/rng_ref.py's rng_hash; the values are applied in float64, with
`frac` rounded to fp32 as the rule states (one fp32 division)."""
import numpy as np

from tests.rng_ref import rng_hash

U64 = (1 << 64) - 1


def step_seed(seed, step):
    """seed_at of csrc/common.h: the seed unchanged for step 0, else the three-multiply mix of the offset."""
    seed, step = int(seed) & U64, int(step) & U64
    if step == 0:
        return seed
    z = (step * 0x9E3779B97F4A7C15) & U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return seed ^ z ^ (z >> 31)


def uniform(h, n):
    return (int(h) * int(n)) >> 32


def plan(B, F, T, lengths=None, *, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_ratio=1.0,
         time_warp=0, seed=0, step=0):
    """int32 [B, 4 + 2 * (freq_masks + time_masks)]: L, w0, c (0, 0 without a warp), 0, (f0, w) pairs, (t0, w) pairs."""
    nF, nT, W = freq_masks, time_masks, time_warp
    D = 2 + 2 * (nF + nT)
    s = step_seed(seed, step)
    out = np.zeros((B, 4 + 2 * (nF + nT)), dtype=np.int32)
    for b in range(B):
        h = [int(x) for x in rng_hash(s, np.arange(b * D, (b + 1) * D, dtype=np.uint64))]
        L = T if lengths is None else min(max(int(lengths[b]), 0), T)
        w0 = c = 0
        if W > 0 and L > 2 * W:
            w0 = W + uniform(h[0], L - 2 * W)
            c = w0 - W + 1 + uniform(h[1], 2 * W)
        row = [L, w0, c, 0]
        for j in range(nF):
            w = uniform(h[2 + 2 * j], min(freq_width, F) + 1)
            row += [uniform(h[3 + 2 * j], F - w + 1), w]
        for j in range(nT):
            cap = min(time_width, int(np.floor(np.float32(time_ratio) * np.float32(L))))
            w = uniform(h[2 + 2 * nF + 2 * j], cap + 1)
            row += [uniform(h[3 + 2 * nF + 2 * j], L - w + 1), w]
        out[b] = row
    return out


def warp_sources(L, w0, c):
    """(i, i1, frac) of every output frame t < L: out = x[i] + frac * (x[i1] - x[i]); frac is the fp32 quotient."""
    t = np.arange(L, dtype=np.int64)
    first = t < c
    num = np.where(first, t * w0, (t - c) * (L - w0))
    den = np.where(first, c, L - c)
    i = np.where(first, 0, w0) + num // den
    r = num % den
    frac = (r.astype(np.float32) / den.astype(np.float32)).astype(np.float32)
    return i, np.minimum(i + 1, L - 1), frac


def apply(x, P, *, freq_masks=0, time_masks=0, mask_value=0.0):
    """The float64 result of plan P on x (B, 1, F, T) or (B, F, T); and, for the tolerance of warped frames, |a| + |b|
    of the two source samples of every element (0 where the element is copied or masked).  Both in x's shape."""
    x64 = np.asarray(x, dtype=np.float64)
    shape = x64.shape
    x64 = x64.reshape(shape[0], shape[-2], shape[-1])
    out = x64.copy()
    mag = np.zeros_like(x64)
    for b in range(x64.shape[0]):
        L, w0, c = (int(v) for v in P[b, :3])
        if c > 0:
            i, i1, frac = warp_sources(L, w0, c)
            a, bb = x64[b][:, i], x64[b][:, i1]
            out[b][:, :L] = a + frac.astype(np.float64) * (bb - a)
            mag[b][:, :L] = np.abs(a) + np.abs(bb)
        for j in range(freq_masks):
            f0, w = (int(v) for v in P[b, 4 + 2 * j:6 + 2 * j])
            out[b][f0:f0 + w, :L] = mask_value
            mag[b][f0:f0 + w, :L] = 0
        for j in range(time_masks):
            k = 4 + 2 * freq_masks + 2 * j
            t0, w = (int(v) for v in P[b, k:k + 2])
            out[b][:, t0:t0 + w] = mask_value
            mag[b][:, t0:t0 + w] = 0
    return out.reshape(shape), mag.reshape(shape)


def specaug(x, lengths=None, *, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_ratio=1.0, time_warp=0,
            mask_value=0.0, seed=0, step=0):
    """(float64 output, |a| + |b| of warped elements, plan) of the whole rule on x (B, 1, F, T) or (B, F, T)."""
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    P = plan(B, F, T, lengths, freq_masks=freq_masks, freq_width=freq_width, time_masks=time_masks,
             time_width=time_width, time_ratio=time_ratio, time_warp=time_warp, seed=seed, step=step)
    out, mag = apply(x, P, freq_masks=freq_masks, time_masks=time_masks, mask_value=mask_value)
    return out, mag, P
