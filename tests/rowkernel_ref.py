"""Float64 references, input families, per-row bounds and case tables for the row kernels (csrc/norm.hip,
csrc/ln512.h, csrc/softmax.hip).  Needs no GPU: tests/test_rowkernel_ref_cpu.py proves here that every bound holds
for a correct fp32 implementation and fails for the planted errors; the three GPU modules apply them to the kernels.

Every bound is per row or per element (never a maximum over the tensor), in units of u = 2^-24 and the row's
cond = 1 + max|x_row| rstd_ref: how much an input rounding of u |x| is magnified by the normalisation.

  y (fp32)     |y - ref| <= 8 u cond (max_row|ref - beta| + max|beta|)
  rstd         |rstd - ref| / ref <= 8 u cond
  mean         |mean - ref| <= MEAN_K u max|x_row|
  dx (fp32)    |dx - ref| <= 16 u cond (rstd_ref max_row|dy gamma| + max_row|dres|), ref from the kernel's mean / rstd
  bf16 result  |got - ref| <= half a bf16 ulp of (|ref| + b) + b, b the fp32 bound of that quantity
  softmax p    per row <= 1e-5 rowmax(ref);  dS per row <= 2e-5 scale rowmax(P) 2 rowmax|G|

MEAN_K = 16: torch's fp32 row mean on the CPU (layer_norm's saved mean) reaches 3.01 u max|x_row| over the seven
families at d in {80, 256, 512, 1024, 2048} (2100 rows each); the worst are `offset100` / `offset3000` rows, 2.1 to
3.0, where the last additions of the sum round at 2^-24 of d times the mean, every other family stays under 0.3.
4 times 3.01, rounded up to a power of two, is 16.  The model of the kernels' order (a serial sum per lane, then the
64-lane butterfly) reaches 2.78.  test_rowkernel_ref_cpu.py measures both again and asserts that MEAN_K is that
power of two.  One fp32 ulp of 300 is 1.7 u max|x_row| on an `offset3000` row: less than the error a correct fp32
mean has there, so no bound that a correct mean meets can see it.  What does see it is the order of addition itself:
IEEE addition is deterministic, so the kernels' mean equals lane_sum()'s bit for bit (mean_model_f32), which the
GPU module asserts next to the bound.

The bf16 bound: a round-to-nearest-even store of a value v is off by at most half a bf16 ulp of v,
2^(floor(log2|v|) - 8), which lies between 2^-9 |v| (top of a binade) and 2^-8 |v| (bottom).  The plain 2^-9 |ref|
rejects correct rounding in the lower part of every binade (1.0039 -> 1.0 is off by 2^-8): the CPU module shows
that it fails on 28 % of the elements of an exactly rounded float64 LayerNorm, and that the half-ulp bound takes all
of them while 28 to 35 % of a truncating store's elements break it."""
import math
import os
from typing import NamedTuple

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "asr-transformer_amd", "csrc")

U = 2.0 ** -24
EPS = 1e-5
MEAN_K = 16.0
F32, B16, F64 = torch.float32, torch.bfloat16, torch.float64

# ------------------------------------------------------------------------------------------ LayerNorm inputs

FAMILIES = ("plain", "offset100", "offset3000", "tiny", "huge", "outlier", "constant")


def family_rows(kind, n, d, g):
    """n rows of one family, fp32 [n, d]"""
    r = torch.randn(n, d, generator=g, dtype=F64)
    if kind == "plain":
        x = r * 2 + 0.5
    elif kind == "offset100":
        x = 10 + 0.1 * r
    elif kind == "offset3000":
        x = 300 + 0.1 * r
    elif kind == "tiny":
        x = 1e-4 * r
    elif kind == "huge":
        x = 1e4 * r
    elif kind == "outlier":
        x = 0.01 * r
        x[torch.arange(n), torch.randint(0, d, (n,), generator=g)] = 50.0
    elif kind == "constant":
        x = torch.full((n, d), 3.25, dtype=F64)
    else:
        raise KeyError(kind)
    return x.to(F32)


def mixed_rows(rows, d, seed, kinds=FAMILIES):
    """fp32 [rows, d], row r of family kinds[r % len(kinds)]: the families interleaved row by row, so that neighbouring
    rows (one wave's ring slots, one block's waves) differ by up to 1e8 in size"""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(rows, d, dtype=F32)
    for i, kind in enumerate(kinds):
        n = len(range(i, rows, len(kinds)))
        if n:
            x[i::len(kinds)] = family_rows(kind, n, d, g)
    return x


def ln_params(d, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return (1 + 0.1 * torch.randn(d, generator=g)).to(F32), (0.1 * torch.randn(d, generator=g)).to(F32)


def ln_grads(rows, d, seed, dtype=F32):
    """dy (rounded to `dtype`, returned in it) and dres (fp32)"""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(rows, d, generator=g).to(dtype), torch.randn(rows, d, generator=g)


def int_rows(rows, cols, lim, seed, dtype=F32):
    """integers in [-lim, lim]: exact in bf16 and fp32, and so is every partial sum below 2^24 in any order"""
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randint(-lim, lim + 1, (rows, cols), generator=g).to(dtype)


# ------------------------------------------------------------------------------------------ LayerNorm reference

class LnRef(NamedTuple):
    mean: torch.Tensor      # [rows]
    rstd: torch.Tensor      # [rows]
    y: torch.Tensor         # [rows, d]
    cond: torch.Tensor      # [rows]  1 + max|x_row| rstd
    xmax: torch.Tensor      # [rows]
    y_bound: torch.Tensor   # [rows, 1]  fp32 y
    rstd_bound: torch.Tensor  # [rows]  relative
    mean_bound: torch.Tensor  # [rows]


def ln_ref(x, gamma, beta, eps=EPS):
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    mean = xd.mean(-1)
    xc = xd - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    y = xc * rstd[:, None] * gd + bd
    xmax = xd.abs().amax(-1)
    cond = 1 + xmax * rstd
    y_bound = 8 * U * cond * ((y - bd).abs().amax(-1) + bd.abs().max())
    return LnRef(mean, rstd, y, cond, xmax, y_bound[:, None], 8 * U * cond, MEAN_K * U * xmax)


def ln_bwd_ref(x, dy, gamma, mean, rstd, dres, cond):
    """dx in float64 from the GIVEN statistics (the kernel's own mean and rstd, as the backward reads them), its
    per-row fp32 bound [rows, 1], and the dgamma | dbeta column sums with their 1e-5 bounds"""
    xd, dyd, gd = x.double(), dy.double(), gamma.double()
    m, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (xd - m) * rs
    g = dyd * gd
    dx = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    bound = rs[:, 0] * g.abs().amax(-1)
    if dres is not None:
        dx = dx + dres.double()
        bound = bound + dres.double().abs().amax(-1)
    bound = 16 * U * cond * bound
    dgamma, dbeta = (dyd * xh).sum(0), dyd.sum(0)
    return dx, bound[:, None], dgamma, dbeta, 1e-5 * (dyd * xh).abs().sum(0), 1e-5 * dyd.abs().sum(0)


# ------------------------------------------------------------------------------------------ bf16

def half_ulp_bf16(v):
    """half a bf16 ulp of |v| (float64 tensor): 2^(floor(log2|v|) - 8); bf16's smallest normal binade below 2^-126"""
    a = v.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8)


def bf16_bound(ref, f32_bound):
    """|got - ref| for a result computed in fp32 within f32_bound of ref and stored round-to-nearest-even"""
    return half_ulp_bf16(ref.abs() + f32_bound) + f32_bound


def bf16_bound_plain(ref, f32_bound):
    """the bound without the binade term, 2^-9 |ref| + fp32 bound: rejects correct rounding (module docstring)"""
    return 2.0 ** -9 * ref.abs() + f32_bound


def to_bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (the planted store error)"""
    bits = x.to(F32).contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(B16)


def worst(err, bound):
    """largest err / bound over a tensor, as a float; 0 / 0 counts as 0, x / 0 as inf, NaN as inf"""
    err, bound = torch.broadcast_tensors(err.double(), bound.double())
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------ fp32 models (CPU)

def lane_layout(d, kind):
    """column index [64, per] each lane owns, -1 = none.  `stream`: 8 consecutive columns per lane (ln512.h);
    `chnj`: CH consecutive columns at 64-lane steps (ln_fwd_kernel<CH, NJ>); `any`: columns l + 64 k"""
    if kind == "stream":
        assert d == 512
        return torch.arange(512).view(64, 8)
    if kind == "chnj":
        ch = next(c for c in (4, 2, 1) if d % (c * 64) == 0)
        nj = d // (ch * 64)
        return torch.arange(d).view(nj, 64, ch).permute(1, 0, 2).reshape(64, nj * ch)
    per = (d + 63) // 64
    idx = torch.arange(64)[:, None] + 64 * torch.arange(per)[None, :]
    return torch.where(idx < d, idx, torch.full_like(idx, -1))


def lane_sum(v, lay):
    """the kernels' order of addition in fp32: a serial sum over each lane's elements, then wave_sum's butterfly
    (common.h: lanes 2i + 2i+1, pairs of those, ... — an adjacent-pair tree)"""
    rows = v.shape[0]
    vz = torch.cat([v, torch.zeros(rows, 1, dtype=F32)], 1)
    t = vz[:, lay.reshape(-1)].view(rows, 64, -1)     # (index -1 reads the appended zero)
    s = torch.zeros(rows, 64, dtype=F32)
    for i in range(t.shape[2]):
        s = s + t[:, :, i]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def _over_d(s, d, kind):
    """the any-width kernels divide by d, the others multiply by the constant 1.f / D"""
    return s / torch.tensor(float(d), dtype=F32) if kind == "any" else s * torch.tensor(1.0 / d, dtype=F32)


def ln_kind(d, streaming=False):
    """which forward kernel a width takes with aligned operands: `stream` (d = 512, fp32 in, bf16 out, ln_pf != 8),
    `chnj` (d = CH NJ 64 of asrx_layernorm_fwd's list), else `any`"""
    if d == 512 and streaming:
        return "stream"
    return "chnj" if d in (64, 128, 256, 512, 768, 1024, 2048) else "any"


def mean_model_f32(x, kind):
    """the row mean in the kernels' own order of addition: what their `mean` output equals bit for bit"""
    return _over_d(lane_sum(x.to(F32), lane_layout(x.shape[1], kind)), x.shape[1], kind)


def ln_model_f32(x, gamma, beta, kind="any", eps=EPS, one_pass=False):
    """(mean, rstd, y) in fp32 by the kernels' formula: two-pass variance from registers, rstd = 1 / sqrt(var + eps),
    y = (x - mean) rstd gamma + beta.  one_pass: the planted variance E[x^2] - mean^2"""
    x = x.to(F32)
    d = x.shape[1]
    lay = lane_layout(d, kind)
    mean = _over_d(lane_sum(x, lay), d, kind)
    if one_pass:
        var = _over_d(lane_sum(x * x, lay), d, kind) - mean * mean
    else:
        t = x - mean[:, None]
        var = _over_d(lane_sum(t * t, lay), d, kind)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    y = (x - mean[:, None]) * rstd[:, None] * gamma.to(F32) + beta.to(F32)
    return mean, rstd, y


def ln_torch_f32(x, gamma, beta, eps=EPS):
    """torch's own fp32 CPU layer_norm with its saved statistics"""
    y, mean, rstd = torch.native_layer_norm(x.to(F32), (x.shape[1],), gamma.to(F32), beta.to(F32), eps)
    return mean.reshape(-1), rstd.reshape(-1), y


def ln_bwd_model_f32(x, dy, gamma, mean, rstd, dres, kind="any"):
    """dx in fp32 by the kernels' formula: dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres, g = dy gamma"""
    x, dy, gamma = x.to(F32), dy.to(F32), gamma.to(F32)
    lay = lane_layout(x.shape[1], kind)
    inv_d = torch.tensor(1.0 / x.shape[1], dtype=F32)
    xh = (x - mean.to(F32)[:, None]) * rstd.to(F32)[:, None]
    g = dy * gamma
    sg = lane_sum(g, lay) * inv_d
    sgx = lane_sum(g * xh, lay) * inv_d
    dx = rstd.to(F32)[:, None] * (g - sg[:, None] - xh * sgx[:, None])
    return dx + dres.to(F32) if dres is not None else dx


# ------------------------------------------------------------------------------------------ softmax inputs

LN2 = math.log(2.0)
SM_KINDS = ("ramp", "descending", "last_key", "all_negative", "shared_top", "randn3")
SM_SCALE = 0.125


def softmax_scores(rows, Lk, seed, scale=SM_SCALE):
    """float64 [rows, Lk] scores (before the kernel's `scale`), row r of kind SM_KINDS[r % 6]: the peaked families of
    test_gpu_attention_peaked.softmax_rows in log2 units over 8 key steps, and randn * 3"""
    g = torch.Generator().manual_seed(4000 + seed)
    r = torch.arange(rows)
    step = (torch.arange(Lk) // ((Lk + 7) // 8)).double()
    gain = (1.0 + 0.2 * (r % 37).double() / 37)[:, None]
    off = (((r * 3) % 5) - 2.0).double()[:, None]
    noise = torch.rand(rows, Lk, generator=g, dtype=F64)
    x = torch.empty(rows, Lk, dtype=F64)
    kind = r % len(SM_KINDS)
    ramp = gain * 12.0 * (step - step.max())[None, :] + off + noise
    desc = -gain * 6.0 * step[None, :] + off + noise
    last = torch.zeros(rows, Lk, dtype=F64)
    last[:, Lk - 1] = 30.0
    last = last + off + noise
    neg = -35.0 + off + noise
    top = torch.full((rows, Lk), -27.0, dtype=F64)
    for key, lvl in zip(sorted({min(1, Lk - 1), Lk // 2, Lk - 1}), (0.0, 0.4, -0.3)):
        top[:, key] = lvl + 1.0
    top = top + 0.2 * noise
    logs = torch.stack([ramp, desc, last, neg, top], 0) * LN2 / scale
    rnd = torch.randn(rows, Lk, generator=g, dtype=F64) * 3
    for k in range(5):
        x[kind == k] = logs[k][kind == k]
    x[kind == 5] = rnd[kind == 5]
    return x


def softmax_ref(s, scale=SM_SCALE, masked=None):
    """float64 softmax of scale * s over the last axis; masked (bool, True = -inf) positions and fully masked rows
    give 0 (nan_to_num)"""
    x = s.double() * scale
    if masked is not None:
        x = x.masked_fill(masked, float("-inf"))
    return torch.nan_to_num(torch.softmax(x, -1))


def softmax_p_bound(ref):
    return 1e-5 * ref.amax(-1, keepdim=True)


def softmax_ds_ref(P, G, scale=SM_SCALE):
    """dS = P (G - rowsum(P G)) scale from the STORED probabilities P, and its per-row fp32 bound"""
    P, G = P.double(), G.double()
    ds = P * (G - (P * G).sum(-1, keepdim=True)) * scale
    return ds, 2e-5 * scale * P.amax(-1, keepdim=True) * 2 * G.abs().amax(-1, keepdim=True)


def softmax_model_f32(s, scale=SM_SCALE, drop_last=False):
    """the kernel's formula in fp32: exp2((s scale log2 e) - max) / sum.  drop_last: the planted error, a row
    reduced over keys [0, Lk - 1)"""
    x = s.to(F32) * torch.tensor(scale * 1.4426950408889634, dtype=F32)
    n = x.shape[-1] - (1 if drop_last else 0)
    e = torch.exp2(x - x[..., :n].amax(-1, keepdim=True))
    p = e / e[..., :n].sum(-1, keepdim=True)
    if drop_last:
        p[..., n:] = 0
    return p


# ------------------------------------------------------------------------------------------ softmax dispatch mirror

SM_LPR_SHORT = (16, 32, 64)     # dispatch_u: try_launch<V, 16 | 32 | 64, 1, U>
SM_NJ_LONG = (2, 4, 8, 16)      # dispatch<V>: try_launch<V, 64, 2 | 4 | 8 | 16, 1>
SM_STREAM_MIN, SM_STREAM_MAX = 128, 256   # try_stream: lk <= 128 || lk > 256 refused


def softmax_kernel_name(dtype, ld, Lk, mode=0, pd=False, u=0, bwd=False):
    """The instantiation asrx_softmax_fwd / asrx_softmax_bwd launch, or None for ASRX_ERR_UNSUPPORTED.  Mirrors
    csrc/softmax.hip: run() (lines 390-399: V = 4 for fp32 with ld % 4 == 0, 8 for bf16 with ld % 8 == 0, else 1),
    dispatch<V>() (377-388), dispatch_u (356-360), softmax_u (362-364), try_stream (368-375) and try_launch's
    capacity test lk <= NJ * LPR * V (344-345)."""
    V = (4 if ld % 4 == 0 else 1) if dtype == F32 else (8 if ld % 8 == 0 else 1)
    stem = "softmax_bwd_kernel" if bwd else "softmax_fwd_kernel"
    if V == 8 and not bwd and dtype == B16 and mode == 0 and not pd and SM_STREAM_MIN < Lk <= SM_STREAM_MAX:
        return "softmax_fwd_stream_kernel<2>"
    U = u if u in (2, 4) else 1
    if not bwd and V == 8 and Lk > 128 and Lk <= 2 * 16 * V:
        return f"{stem}<{V},16,2,1>"
    for lpr in SM_LPR_SHORT:
        if Lk <= lpr * V:
            return f"{stem}<{V},{lpr},1,{U}>"
    for nj in SM_NJ_LONG:
        if Lk <= nj * 64 * V:
            return f"{stem}<{V},64,{nj},1>"
    return None


def softmax_reachable():
    """every name the mirror can return: the instantiations that can run at all (softmax_fwd_kernel<8,32,1,U> cannot:
    the forward's 129..256 keys go to <8,16,2,1> or the streaming kernel first)"""
    names = set()
    for dtype, lds in ((B16, (8, 1)), (F32, (4, 1))):
        for al in lds:
            V = al if al > 1 else 1
            edges = sorted({c for k in SM_LPR_SHORT + tuple(64 * n for n in SM_NJ_LONG) for c in (k * V, k * V + 1)}
                           | {1, 128, 129, 256, 257})
            for Lk in edges:
                ld = -(-Lk // 8) * 8 if al > 1 else (Lk if Lk % 2 else Lk + 1)
                for mode in (0, 1):
                    for pd in (False, True):
                        for u in (0, 2, 4):
                            for bwd in (False, True):
                                names.add(softmax_kernel_name(dtype, ld, Lk, mode, pd and not bwd, u, bwd))
    names.discard(None)
    return names


class SmCase(NamedTuple):
    dtype: torch.dtype
    Lk: int
    ld: int
    u: int = 0
    Lq: int = 9
    drop: float = 0.0

    @property
    def id(self):
        return f"{'bf16' if self.dtype == B16 else 'fp32'}-Lk{self.Lk}-ld{self.ld}-u{self.u}" + \
               (f"-p{self.drop}" if self.drop else "")

    def names(self):
        """the instantiations the case runs: the forward (with the dropped copy when drop), and the backward"""
        return {softmax_kernel_name(self.dtype, self.ld, self.Lk, 0, self.drop > 0, self.u, False),
                softmax_kernel_name(self.dtype, self.ld, self.Lk, 0, False, self.u, True)}


def ceil8(n):
    return (n + 7) // 8 * 8


def odd_ld(Lk):
    """an unaligned row stride: Lk when odd, else Lk + 1 (ld % 4 != 0 and ld % 8 != 0: the V = 1 family)"""
    return Lk if Lk % 2 else Lk + 1


SM_SHORT_U = (0, 2, 4)
SM_BF16_ALIGNED = (24, 100, 200, 300, 512, 999, 1025, 2048, 2049, 4096, 4097, 8192)
SM_F32_ALIGNED = (24, 100, 200, 300, 512, 999, 1025, 2048, 2049, 4096)
SM_UNALIGNED = (5, 16, 17, 33, 64, 100, 249, 300, 600, 1024)   # (300: <1,64,8>, which 249 and 600 step over)
SM_UNSUPPORTED = ((B16, 8193, 8200), (F32, 4097, 4100), (B16, 1025, 1025), (F32, 1025, 1025))


def _is_short(dtype, ld, Lk):
    name = softmax_kernel_name(dtype, ld, Lk, 0, False, 0, True)
    return name is not None and name.split(",")[2] == "1"


def softmax_cases():
    """Forward + backward cases, no mask: every aligned and unaligned length above in both dtypes; softmax_u in
    {0, 2, 4} where the row is short (one step per lane: the instantiations that take U); Lq = 3 at the extreme
    lengths; p = 0.3 dropout at one V = 1 case and at bf16 Lk = 2049 (and at bf16 Lk = 200: the forward's
    <8,16,2,1>, which plain rows of that length leave to the streaming kernel)."""
    cases = []
    for dtype, lks, ldf in ((B16, SM_BF16_ALIGNED, ceil8), (F32, SM_F32_ALIGNED, ceil8),
                            (B16, SM_UNALIGNED, odd_ld), (F32, SM_UNALIGNED, odd_ld)):
        for Lk in lks:
            ld = ldf(Lk)
            for u in (SM_SHORT_U if _is_short(dtype, ld, Lk) else (0,)):
                cases.append(SmCase(dtype, Lk, ld, u, 3 if Lk >= 4096 else 9))
    cases += [SmCase(B16, 33, 33, 0, 9, 0.3), SmCase(F32, 600, 601, 0, 9, 0.3), SmCase(B16, 2049, 2056, 0, 9, 0.3),
              SmCase(B16, 200, 200, 0, 9, 0.3)]
    return cases


def softmax_declared():
    names = set()
    for c in softmax_cases():
        names |= c.names()
    return names


# ------------------------------------------------------------------------------------------ constants of the sources

def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


LNA_MAXD = 2048      # norm.hip: the any-width kernels' widest row
RG_MAX = 64          # norm.hip: groups per asrx_reduce_rows_grouped launch
LNB_W = 8            # norm.hip: waves per block of ln_bwd512_kernel
LN_FWD_BLOCKS_PER_CU, LN_CUS = 4, 256   # norm.hip ln_bpc() default, asrx_layernorm_fwd's 256 * ln_bpc() blocks


def ln_fwd_waves(rows, bpc=0):
    """nw of ln_fwd512_rows as asrx_layernorm_fwd launches it: 4 waves x min(ceil(rows / 4), 256 bpc) blocks"""
    return 4 * max(1, min((rows + 3) // 4, LN_CUS * (bpc if bpc > 0 else LN_FWD_BLOCKS_PER_CU)))


def ring_trips(rows, pf, nw):
    """(whole trips of a wave's PF-slot ring over all nw waves, rows left for a ragged last trip)"""
    return rows // (pf * nw), rows % (pf * nw)


# ------------------------------------------------------------------------------------------ column sums

RR_ROWS = (0, 1, 59, 60, 61, 63, 64, 65, 124, 125, 128, 1000)
RR_COLS = (1, 63, 64, 65, 70)
RR_NBLOCKS = (1, 3, 512)
RR_GROUPS = (64, 65)


GUARD = 256          # sentinel elements either side of a guarded buffer (keeps the inside 512-B aligned)
SENTINEL = -1280.0   # exact in bf16 and fp32, and no value any test here computes


def guarded(n, dtype, device, fill=SENTINEL):
    """(whole buffer, its n inside elements): the inside sits between GUARD sentinels and starts out as sentinels too"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, fill=SENTINEL):
    want = torch.full((GUARD,), fill, dtype=buf.dtype, device=buf.device)
    return same_bits(buf[:GUARD], want) and same_bits(buf[GUARD + n:], want)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))
