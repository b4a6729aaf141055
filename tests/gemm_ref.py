"""Exact reference and case table of the GEMM families (asrx_gemm, csrc/gemm.hip and gemm_ws.hip); no GPU needed.

bf16 holds small integers exactly and an fp32 sum of their products is exact in any order, so a correct kernel
reproduces an int64 reference bit for bit, whatever its tiling, split or epilogue.  Every case of the table is a
GEMM on integer operands (uniform in [-3, 3]; bias / row-add / residual / old C in [-8, 8]; gates in {-1, 0, 1};
alpha in {1, 0.5, 2}, beta in {0, 1}; dropout p = 0.5, scale 2) whose operands sit inside larger NaN-filled buffers
and whose outputs sit inside sentinel-filled ones: a read of padding turns a valid output into NaN, a stray store
changes a guard.

A case DECLARES the kernel it is meant to reach (family, layout, epilogue number, operand alignment); the CPU test
compares the declaration with asrx_gemm_kernel_name for the real descriptor, so no case runs another kernel than
the one it names.  The epilogue order and the ASRX_BITS / mask_out layout are restated from include/asrx.h."""
import dataclasses
import zlib
from typing import Optional

import numpy as np
import torch

import rng_ref

# epilogue flags (csrc/gemm_common.h) as they appear in the kernel names
E_BIAS, E_RELU, E_DROP, E_GATE, E_RESID, E_BETA, E_F32, E_ALPHA = 1, 2, 4, 8, 16, 32, 64, 128
E_ROWADD, E_GBITS, E_MASKOUT, E_GENERIC = 256, 512, 1024, 1 << 30
E_NAMES = dict(E_BIAS=E_BIAS, E_RELU=E_RELU, E_DROP=E_DROP, E_GATE=E_GATE, E_RESID=E_RESID, E_BETA=E_BETA,
               E_F32=E_F32, E_ALPHA=E_ALPHA, E_ROWADD=E_ROWADD, E_GBITS=E_GBITS, E_MASKOUT=E_MASKOUT)

GUARD_ROWS = 64                 # poisoned / sentinel rows before and after every operand and output
SENTINEL = -8192.0              # exact in bf16 and fp32
MASK_SENTINEL = 0x5A5A5A5A      # guard words of mask_out
WS_GUARD = 1024                 # NaN elements before and after the split-K workspaces
DROP_P = 0.5
SEED = 0x9E3779B100000000 | 0x1234567   # high 32 bits non-zero
ROWADD_MOD = 5

FAMILY_PREFIX = {"reg64": "gemm_bf16_kernel<64, 64, ", "reg128": "gemm_bf16_kernel<128, 128, ",
                 "p3": "gemm_bf16_p3_kernel<", "p4": "gemm_bf16_p4_kernel<",
                 "ring": "gemm_bf16_ring_kernel<64, 64, ", "ring128": "gemm_bf16_ring_kernel<128, 64, ",
                 "ws": "gemm_bf16_ws_kernel<", "ws64": "gemm_bf16_ws_kernel<", "tallk": "gemm_bf16_tallk_kernel",
                 "f32": "gemm_f32_kernel<"}
FAMILIES = tuple(f for f in FAMILY_PREFIX if f != "f32")   # the nine bf16 families


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    family: str                    # DECLARED: the kernel family the case reaches
    m: int
    n: int
    k: int
    at: bool = False
    bt: bool = False
    kernel: str = "auto"           # requested asrx_gemm_desc.kernel
    tile: int = 0
    epi: int = E_GENERIC           # DECLARED epilogue number in the kernel name (ring / ws families)
    vec: bool = True               # DECLARED operand alignment flag in the name (register families)
    fallback: bool = False         # the request cannot be honoured: planned on the register kernel, on purpose
    in_f32: bool = False
    c_f32: bool = True
    lda_pad: int = 8               # ld - row length
    ldb_pad: int = 8
    ldc_pad: int = 8
    off_a: int = 0                 # element offset of the base inside its buffer (1: unaligned)
    off_b: int = 0
    off_c: int = 0
    alpha: float = 1.0
    beta: float = 0.0
    bias: bool = False
    rowadd: bool = False
    relu: bool = False
    drop: bool = False
    gate: Optional[str] = None     # "bf16" | "f32" | "bits"
    resid: Optional[str] = None    # "f32" | "bf16"
    mask_out: bool = False
    splitk: int = 1
    rowsum: bool = False
    attn: Optional[str] = None     # section F: one of ATTN_SHAPES (batched, two-level strides)
    batch: int = 1                 # plain batch (batch_inner = 1, slab strides)


def expected_family(case):
    """(kernel-name prefix, epilogue number or None) the case is meant to reach."""
    numbered = case.family in ("p3", "p4", "ring", "ring128", "ws", "ws64")
    return FAMILY_PREFIX[case.family], (case.epi if numbered else None)


def expected_name(case):
    """The full instantiation name asrx_gemm_kernel_name must report for the case's descriptor."""
    tf = ("false", "true")
    at, bt = tf[case.at], tf[case.bt]
    f = case.family
    if f in ("reg64", "reg128"):
        return f"{FAMILY_PREFIX[f]}{at}, {bt}, {tf[case.vec]}>"
    if f in ("p3", "p4", "ring", "ring128"):
        return f"{FAMILY_PREFIX[f]}{at}, {bt}, {case.epi}>"
    if f in ("ws", "ws64"):
        return f"{FAMILY_PREFIX[f]}{bt}, {case.epi}, {256 if f == 'ws' else 64}>"
    if f == "f32":
        return f"{FAMILY_PREFIX[f]}{at}, {bt}>"
    return FAMILY_PREFIX[f]


def parse_name(name):
    """(family, epilogue number or None) of a kernel name as asrx_gemm_kernel_name reports it"""
    for fam, prefix in FAMILY_PREFIX.items():
        if name.startswith(prefix) and (fam not in ("ws", "ws64") or name.endswith(", 256>" if fam == "ws" else ", 64>")):
            if fam in ("p3", "p4", "ring", "ring128"):
                return fam, int(name[:-1].rsplit(", ", 1)[1])
            if fam in ("ws", "ws64"):
                return fam, int(name[:-1].split(", ")[1])
            return fam, None
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ layouts

class Lay:
    """A [rows][cols] matrix per batch index z = zo * ni + zi inside a flat buffer: element (z, r, c) at
    off + zo * so + zi * si + r * ld + c.  GUARD_ROWS rows of ld elements lie before `off` and after the last
    element."""

    def __init__(self, rows, cols, ld, off=0, no=1, ni=1, so=0, si=0):
        self.rows, self.cols, self.ld, self.no, self.ni, self.so, self.si = rows, cols, ld, no, ni, so, si
        self.off = GUARD_ROWS * ld + off
        last = self.off + (no - 1) * so + (ni - 1) * si + (rows - 1) * ld + cols
        self.size = last + GUARD_ROWS * ld

    def index(self):
        zo = np.arange(self.no, dtype=np.int64)[:, None, None, None] * self.so
        zi = np.arange(self.ni, dtype=np.int64)[None, :, None, None] * self.si
        r = np.arange(self.rows, dtype=np.int64)[None, None, :, None] * self.ld
        c = np.arange(self.cols, dtype=np.int64)[None, None, None, :]
        return (self.off + zo + zi + r + c).reshape(self.no * self.ni, self.rows, self.cols)


# Section F: the six batched GEMMs of the unfused attention (asrx/blocks.py attn_fwd / attn_bwd) at B = 2, H = 3,
# Lq = 37, Lk = 41, dh = 32: token-major operands [B][L][H * dh] (head stride dh) and score slabs [B * H][Lq][ld],
# ld = Lk rounded up to 8.  name -> (m, n, k, at, bt, A, B, C) with "q" / "k" = token-major with Lq / Lk rows,
# "s" = score slab
ATTN_B, ATTN_H, ATTN_LQ, ATTN_LK, ATTN_DH = 2, 3, 37, 41, 32
ATTN_SHAPES = {
    "scores": (ATTN_LQ, ATTN_LK, ATTN_DH, False, False, "q", "k", "s"),    # S = Q K^T
    "out": (ATTN_LQ, ATTN_DH, ATTN_LK, False, True, "s", "k", "q"),        # O = P V
    "dprob": (ATTN_LQ, ATTN_LK, ATTN_DH, False, False, "q", "k", "s"),     # dP = dO V^T
    "dv": (ATTN_LK, ATTN_DH, ATTN_LQ, True, True, "s", "q", "k"),          # dV = P^T dO
    "dq": (ATTN_LQ, ATTN_DH, ATTN_LK, False, True, "s", "k", "q"),         # dQ = dS K
    "dk": (ATTN_LK, ATTN_DH, ATTN_LQ, True, True, "s", "q", "k"),          # dK = dS^T Q
}


def _attn_lay(kind, cols, packed):
    d = ATTN_H * ATTN_DH
    if kind == "s":
        ld = (ATTN_LK + 7) // 8 * 8
        return Lay(ATTN_LQ, cols, ld, 0, ATTN_B, ATTN_H, ATTN_H * ATTN_LQ * ld, ATTN_LQ * ld)
    rows = ATTN_LQ if kind == "q" else ATTN_LK
    ld = 3 * d if packed else d + 8    # rows of a packed Q|K|V projection, or of a tensor of its own
    return Lay(rows, cols, ld, 0, ATTN_B, ATTN_H, rows * ld, ATTN_DH)


def layouts(case):
    """(A, B, C) layouts.  A is stored [K][M] when a_trans, B [K][N] when b_trans."""
    ar, ac = (case.k, case.m) if case.at else (case.m, case.k)
    br, bc = (case.k, case.n) if case.bt else (case.n, case.k)
    if case.attn:
        _, _, _, _, _, ka, kb, kc = ATTN_SHAPES[case.attn]
        packed = case.attn in ("scores", "dq")
        return _attn_lay(ka, ac, packed), _attn_lay(kb, bc, packed), _attn_lay(kc, case.n, False)
    nb = case.batch
    la, lb, lc = ac + case.lda_pad, bc + case.ldb_pad, case.n + case.ldc_pad
    # plain batches: slabs 8 rows apart, rounded to 8 elements (keeps the operand alignment flag)
    sa, sb, sc = (((r + 8) * ld + 7) // 8 * 8 if nb > 1 else 0 for r, ld in ((ar, la), (br, lb), (case.m, lc)))
    return (Lay(ar, ac, la, case.off_a, nb, 1, sa, 0), Lay(br, bc, lb, case.off_b, nb, 1, sb, 0),
            Lay(case.m, case.n, lc, case.off_c, nb, 1, sc, 0))


def nbatch(case):
    return ATTN_B * ATTN_H if case.attn else case.batch


# ------------------------------------------------------------------------------------------------ the builder

def mask_bit_pos(c):
    """include/asrx.h mask_out / ASRX_BITS: column c = n % 32 sits at bit 8*((c & 15) >> 2) + 4*(c >> 4) + (c & 3)"""
    return 8 * ((c & 15) >> 2) + 4 * (c >> 4) + (c & 3)


def pack_bits(pos, words_per_row, fill):
    """bool [m][n] -> uint32 words [m][words_per_row] in the ASRX_BITS layout; bits of columns >= n and the padding
    words take `fill`'s bits."""
    m, n = pos.shape
    out = np.full((m, words_per_row), fill, dtype=np.uint64)
    col = np.arange(n)
    bit = np.uint64(1) << mask_bit_pos(col % 32).astype(np.uint64)
    for w in range((n + 31) // 32):
        sel = (col // 32) == w
        word = out[:, w] & ~np.bitwise_or.reduce(bit[sel])
        word |= (pos[:, sel].astype(np.uint64) * bit[sel]).sum(1).astype(np.uint64)
        out[:, w] = word
    return out.astype(np.uint32)


def _exact(x, what):
    """every intermediate is an integer multiple of 0.5 whose fp32 image is exact"""
    assert np.isfinite(x).all(), what
    assert (x * 2 == np.round(x * 2)).all(), what
    assert np.abs(x * 2).max(initial=0) < 2 ** 24, what
    return x


class Built:
    """Host buffers, descriptor recipe and expected results of one case (see make_case)."""


def bf16_round(x):
    """float32 image of x rounded to bfloat16, round-to-nearest-even (what v_cvt_pk_bf16_f32 and torch's
    .to(torch.bfloat16) do), in numpy; NaN stays NaN"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def as_tensor(x, dtype):
    """numpy values -> host tensor of `dtype` (fp32 exactly; bf16 by bf16_round), without a torch compute op: the
    builders leave torch's thread pool alone"""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.float32:
        return torch.from_numpy(x32.copy())
    hi = (bf16_round(x32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    return torch.from_numpy(hi).view(torch.bfloat16)


def _filled(size, dtype, fill=float("nan"), lay=None, values=None, span=None):
    """flat host tensor of `fill` (NaN: poison) with `values` at the elements of `lay` ([batch, rows, cols]) or at
    the flat range `span`"""
    buf = np.full(size, fill, dtype=np.float32)
    if lay is not None:
        buf[lay.index().reshape(-1)] = np.asarray(values, dtype=np.float32).reshape(-1)
    if span is not None:
        buf[span[0]:span[1]] = np.asarray(values, dtype=np.float32).reshape(-1)
    return as_tensor(buf, dtype)


def make_case(case):
    """Everything a launch of `case` needs plus its expected result.

    .bufs: name -> flat host tensor (operands NaN-poisoned around the logical matrix, outputs sentinel-filled);
    .ptr: name -> byte offset of the descriptor pointer inside its buffer; .desc(base): the asrx_gemm_desc for
    buffer base addresses base[name]; .c_index: flat indices of the logical C elements [batch, m, n];
    .expect_c: the exact C in the C dtype; .expect_mask / .expect_rowsum likewise; .pre_drop / .keep: the
    pre-dropout value and the keep mask of dropout cases; .gate_pos: gate > 0; .addend: what is added after the
    dropout and the gate (residual + beta * C_old)."""
    rs = np.random.RandomState(zlib.crc32(case.id.encode()) & 0x7FFFFFFF)
    nb, m, n, k = nbatch(case), case.m, case.n, case.k
    in_dt = torch.float32 if case.in_f32 else torch.bfloat16
    c_dt = torch.float32 if case.c_f32 else torch.bfloat16
    la, lb, lc = layouts(case)
    A = rs.randint(-3, 4, size=(nb, m, k)).astype(np.float64)
    B = rs.randint(-3, 4, size=(nb, n, k)).astype(np.float64)
    b = Built()
    b.case, b.bufs, b.ptr, b.lay = case, {}, {}, dict(a=la, b=lb, c=lc)
    for name, lay, val, tr in (("a", la, A, case.at), ("b", lb, B, case.bt)):
        buf = _filled(lay.size, in_dt, lay=lay, values=val.transpose(0, 2, 1) if tr else val)
        b.bufs[name], b.ptr[name] = buf, lay.off * buf.element_size()

    # ---- reference, in the epilogue order of include/asrx.h; float64 holds every value exactly
    acc = np.matmul(A, B.transpose(0, 2, 1))
    assert (acc == np.round(acc)).all() and np.abs(acc).max(initial=0) < 2 ** 24
    v = _exact(case.alpha * acc, "alpha")
    if case.bias:
        bias = rs.randint(-8, 9, size=n).astype(np.float64)
        buf = _filled(n + 128, torch.float32, values=bias, span=(64, 64 + n))
        b.bufs["bias"], b.ptr["bias"] = buf, 64 * 4
        v = _exact(v + bias, "bias")
    if case.rowadd:
        ra = rs.randint(-8, 9, size=(ROWADD_MOD, n)).astype(np.float64)
        lr = Lay(ROWADD_MOD, n, n + 4)
        buf = _filled(lr.size, torch.float32, lay=lr, values=ra)
        b.bufs["rowadd"], b.ptr["rowadd"], b.lay["rowadd"] = buf, lr.off * 4, lr
        v = _exact(v + ra[np.arange(m) % ROWADD_MOD][None], "rowadd")
    if case.relu:
        v = np.maximum(v, 0.0)
    b.pre_drop = b.keep = None
    if case.drop:
        b.pre_drop = v.copy()
        b.keep = rng_ref.elem_keep(SEED, nb * m * n, DROP_P).reshape(nb, m, n)
        v = _exact(np.where(b.keep, v * 2.0, 0.0), "dropout")
    if case.gate:
        assert nb == 1
        gate = rs.randint(-1, 2, size=(m, n)).astype(np.float64)
        if case.gate == "bits":
            words = (n + 31) // 32 + 3
            lg = Lay(m, words, words)
            raw = np.full(lg.size, 0xFFFFFFFF, dtype=np.uint32)     # padding reads as "keep": a stray read shows
            raw[lg.index().reshape(-1)] = pack_bits(gate > 0, words, 0xFFFFFFFF).reshape(-1)
            buf = torch.from_numpy(raw.view(np.int32))
            b.bufs["gate"], b.ptr["gate"], b.lay["gate"] = buf, lg.off * 4, lg
        else:
            gdt = torch.bfloat16 if case.gate == "bf16" else torch.float32
            lg = Lay(m, n, n + 4)
            buf = _filled(lg.size, gdt, lay=lg, values=gate)
            b.bufs["gate"], b.ptr["gate"], b.lay["gate"] = buf, lg.off * buf.element_size(), lg
        v = np.where(gate[None] > 0, v, 0.0)
    b.before_add = v.copy()          # what the residual and beta * C_old are added to
    b.gate_pos = (gate[None] > 0) if case.gate else None
    b.resid = None
    if case.resid:
        assert nb == 1
        resid = rs.randint(-8, 9, size=(m, n)).astype(np.float64)
        rdt = torch.float32 if case.resid == "f32" else torch.bfloat16
        lr = Lay(m, n, n + 4)
        buf = _filled(lr.size, rdt, lay=lr, values=resid)
        b.bufs["resid"], b.ptr["resid"], b.lay["resid"] = buf, lr.off * buf.element_size(), lr
        b.resid = resid
        v = _exact(v + resid[None], "resid")
    # C: sentinel everywhere, old C (beta = 1) or NaN (beta = 0: C is not read) in the logical elements
    if case.beta != 0.0:
        c_old = rs.randint(-8, 9, size=(nb, m, n)).astype(np.float64)
        v = _exact(v + case.beta * c_old, "beta")
    else:
        c_old = np.full((nb, m, n), np.nan)
    cbuf = _filled(lc.size, c_dt, SENTINEL, lc, c_old)
    b.bufs["c"], b.ptr["c"] = cbuf, lc.off * cbuf.element_size()
    b.c_index = torch.from_numpy(lc.index())
    b.exact = v
    b.addend = v - b.before_add      # residual + beta * C_old, exact
    assert np.isfinite(v).all()                              # the poison never enters the reference
    b.expect_c = as_tensor(v, c_dt)                          # fp32 is exact; bf16 rounds to nearest even
    b.expect_mask = None
    if case.mask_out:
        assert nb == 1 and n % 32 == 0
        words = n // 32 + 3
        lm = Lay(m, n // 32, words)
        b.bufs["mask_out"] = torch.from_numpy(np.full(lm.size, MASK_SENTINEL, dtype=np.uint32).view(np.int32).copy())
        b.ptr["mask_out"], b.lay["mask_out"] = lm.off * 4, lm
        pos = bf16_round(v[0]) > 0                            # the bits C > 0 as stored
        b.expect_mask = torch.from_numpy(pack_bits(pos, n // 32, 0).view(np.int32).copy())
    b.expect_rowsum = None
    if case.rowsum:
        assert nb == 1 and case.at
        old = rs.randint(-8, 9, size=m).astype(np.float64)
        buf = _filled(m + 128, torch.float32, SENTINEL, values=old, span=(64, 64 + m))
        b.bufs["rowsum"], b.ptr["rowsum"] = buf, 64 * 4
        b.expect_rowsum = as_tensor(_exact(old + A[0].sum(1), "rowsum"), torch.float32)
    if case.splitk > 1:
        b.bufs["ws"] = _filled(case.splitk * m * n + 2 * WS_GUARD, torch.float32)
        b.ptr["ws"] = WS_GUARD * 4
        if case.rowsum:
            b.bufs["rowsum_ws"] = _filled(case.splitk * m + 2 * WS_GUARD, torch.float32)
            b.ptr["rowsum_ws"] = WS_GUARD * 4
    b.desc = lambda base: _desc(b, base)
    return b


def _desc(b, base):
    from asrx._lib import BF16, BITS, F32, GemmDesc
    from asrx.kernels import KERNEL_CODES
    c = b.case
    la, lb, lc = b.lay["a"], b.lay["b"], b.lay["c"]
    p = {name: base[name] + off for name, off in b.ptr.items()}
    d = GemmDesc()
    d.m, d.n, d.k, d.in_dtype = c.m, c.n, c.k, (F32 if c.in_f32 else BF16)
    d.a, d.lda, d.a_trans = p["a"], la.ld, int(c.at)
    d.b, d.ldb, d.b_trans = p["b"], lb.ld, int(c.bt)
    d.c, d.ldc, d.c_dtype = p["c"], lc.ld, (F32 if c.c_f32 else BF16)
    d.batch, d.batch_inner = nbatch(c), la.ni
    d.sa_outer, d.sa_inner, d.sb_outer, d.sb_inner = la.so, la.si, lb.so, lb.si
    d.sc_outer, d.sc_inner = lc.so, lc.si
    d.alpha, d.beta = c.alpha, c.beta
    if c.bias:
        d.bias = p["bias"]
    if c.rowadd:
        d.rowadd, d.ld_rowadd, d.rowadd_mod = p["rowadd"], b.lay["rowadd"].ld, ROWADD_MOD
    d.relu = int(c.relu)
    if c.drop:
        d.dropout_p, d.seed = DROP_P, SEED
    if c.gate:
        d.gate, d.ld_gate = p["gate"], b.lay["gate"].ld
        d.gate_dtype = {"bf16": BF16, "f32": F32, "bits": BITS}[c.gate]
    if c.resid:
        d.resid, d.ld_resid, d.resid_dtype = p["resid"], b.lay["resid"].ld, (F32 if c.resid == "f32" else BF16)
    d.splitk = c.splitk
    if c.splitk > 1:
        d.workspace, d.workspace_elems = p["ws"], c.splitk * c.m * c.n
    d.tile = c.tile
    if c.rowsum:
        d.rowsum_a = p["rowsum"]
        if c.splitk > 1:
            d.rowsum_ws = p["rowsum_ws"]
    if c.mask_out:
        d.mask_out, d.ld_mask = p["mask_out"], b.lay["mask_out"].ld
    d.kernel = KERNEL_CODES[c.kernel]
    return d


def fake_bases(b):
    """Buffer addresses with the alignment of a real device allocation (host-only plan checks)."""
    return {name: (i + 1) << 28 for i, name in enumerate(sorted(b.bufs))}


# ------------------------------------------------------------------------------------------------ the case table

LAYOUTS4 = [(False, False), (False, True), (True, False), (True, True)]


def _lname(at, bt):
    """the sources' names of the layouts: NT = x . W^T (both k-contiguous), NN = B stored [K][N], TT = both operands
    k-strided (weight gradients); TN = A stored [K][M] with a k-contiguous B"""
    return {(False, False): "NT", (False, True): "NN", (True, True): "TT", (True, False): "TN"}[(bool(at), bool(bt))]


def _vec_pad(row):
    """a pad that makes ld = row + pad a multiple of 8 larger than the row"""
    return (row // 8 + 1) * 8 - row


def _flags(epi):
    """case fields that make the planner arrive at the fast epilogue `epi`"""
    return dict(bias=bool(epi & E_BIAS), relu=bool(epi & E_RELU), drop=bool(epi & E_DROP),
                gate="bf16" if epi & E_GATE else "bits" if epi & E_GBITS else None,
                resid="f32" if epi & E_RESID else None, beta=1.0 if epi & E_BETA else 0.0,
                c_f32=bool(epi & E_F32), alpha=0.5 if epi & E_ALPHA else 1.0, rowadd=bool(epi & E_ROWADD),
                mask_out=bool(epi & E_MASKOUT))


def _odd_pad(row):
    """a pad that leaves ld = row + pad odd"""
    return 3 if (row + 3) % 2 else 4


def cases_reg():
    """A. register kernels, both tiles and both VEC values, all four layouts, K across the 64-deep step and the
    8-element vector, with and without alignment."""
    shapes = [(1, 1), (7, 5), (33, 17), (65, 129), (2, 136), (130, 72)]
    ks = [1, 7, 8, 9, 40, 63, 64, 65, 100, 129]
    out = []

    vec_pad = _vec_pad

    def add(tag, i, m, n, k, at, bt, **kw):
        tile = kw.pop("tile")
        ar, br = (m if at else k), (n if bt else k)
        aligned = kw.pop("aligned")
        pads = dict(lda_pad=vec_pad(ar), ldb_pad=vec_pad(br)) if aligned else {}
        out.append(Case(f"reg-{tag}-{m}x{n}x{k}-{_lname(at, bt)}", "reg64" if tile == 64 else "reg128", m, n, k, at,
                        bt, kernel="reg", tile=tile, vec=aligned and not (kw.get("off_a") or kw.get("off_b")),
                        **pads, **kw))

    i = 0
    for (m, n) in shapes:
        for k in ks:
            for li, (at, bt) in enumerate(LAYOUTS4):
                ar, br = (m if at else k), (n if bt else k)
                # every (shape, K, layout): 64 x 64 tiles, aligned operands, fp32 C with 16-byte rows
                add("t64v", i, m, n, k, at, bt, tile=64, aligned=True, ldc_pad=vec_pad(n) + 4 if n % 4 else 4)
                # the other configurations take one layout per (shape, K), rotating
                if li == i % 4:
                    add("t64odd", i, m, n, k, at, bt, tile=64, aligned=False, lda_pad=_odd_pad(ar),
                        ldb_pad=_odd_pad(br), ldc_pad=_odd_pad(n), c_f32=False)
                    add("t128v", i, m, n, k, at, bt, tile=128, aligned=True, c_f32=False,
                        ldc_pad=(n // 4 + 1) * 4 - n)
                if li == (i + 1) % 4:
                    add("t128offa", i, m, n, k, at, bt, tile=128, aligned=True, off_a=1, off_c=1)
                    add("t64offb", i, m, n, k, at, bt, tile=64, aligned=True, off_b=1, c_f32=False, off_c=1,
                        ldc_pad=_odd_pad(n))
            i += 1
    return out


# family -> (kernel request, ragged shapes: one full tile plus a remainder, minimum shape, layouts it takes)
DMA_FAMILIES = {
    "p3": ("p3", [(264, 136)], (8, 8), LAYOUTS4),
    "p4": ("p4", [(264, 264)], (8, 8), [(False, False), (False, True), (True, True)]),
    "ring": ("ring", [(72, 72)], (8, 8), LAYOUTS4[:2]),
    "ring128": ("ring128", [(136, 72)], (8, 8), LAYOUTS4[:2]),
    "ws": ("ws", [(264, 128), (264, 256)], (8, 128), LAYOUTS4[:2]),
    "ws64": ("ws64", [(72, 128)], (8, 128), LAYOUTS4[:2]),
}


def _plain_epi(family, at, bt, c_f32):
    """the epilogue number of a GEMM without epilogue operands"""
    if at and not bt:
        return E_GENERIC            # no fast epilogue is instantiated for A^T with a k-contiguous B
    if at:
        return E_F32                # the weight-gradient layout has fp32 epilogues only
    return E_F32 if c_f32 else 0


def cases_dma_edges():
    """B. LDS-DMA families: 1 to 5 K-steps (below, at and above the 2-, 3- and 4-stage rings) on a full tile plus a
    ragged remainder, and the 8 x 8 minimum; ld = row + 8."""
    out = []
    for fam, (kern, shapes, mn, lays) in DMA_FAMILIES.items():
        for (m, n) in shapes + [mn]:
            for k in ([64, 128, 192, 256, 320] if (m, n) != mn else [64, 192]):
                for at, bt in lays:
                    c_f32 = at or (k // 64) % 2 == 0
                    out.append(Case(f"edge-{fam}-{m}x{n}x{k}-{_lname(at, bt)}", fam, m, n, k, at, bt, kernel=kern,
                                    epi=_plain_epi(fam, at, bt, c_f32), c_f32=c_f32))
    for n in (64, 576):
        for sk in (64, 256):
            for k in (64 * 32, 64 * 32 + 37):
                out.append(Case(f"edge-tallk-64x{n}x{k}-s{sk}", "tallk", 64, n, k, True, True, splitk=sk,
                                rowsum=(n == 576) == (sk == 64), beta=float(k % 2), ldc_pad=4))
    return out


# The fast epilogues instantiated per family and layout (csrc/gemm_common.h ASRX_EPI_*, gemm.hip ASRX_EPI4_*,
# gemm_ws.hip ASRX_EPIWS_*), restated; test_gemm_ref_cpu.py compares them with the lists in the sources.
EPI_NT = [1, 3, 7, 81, 85, 64, 321, 0, 1027, 1031]
EPI_NN = [0, 8, 136, 64, 512, 640]
EPI_TT = [96, 64]
EPI4_NT = [1, 7, 64, 0, 1031]
EPI4_NN = [0, 64, 512, 640]
EPI4_TT = [96, 64]
EPIWS_NT = [0, 1, 64, 65, 81, 85, 321]
EPIWS_NN = [0, 64]
FAMILY_EPIS = {   # family -> layout name -> epilogue numbers
    "p3": {"NT": EPI_NT, "NN": EPI_NN, "TT": EPI_TT},
    "p4": {"NT": EPI4_NT, "NN": EPI4_NN, "TT": EPI4_TT},
    "ring": {"NT": EPI_NT, "NN": EPI_NN},
    "ring128": {"NT": EPI_NT, "NN": EPI_NN},
    "ws": {"NT": EPIWS_NT, "NN": EPIWS_NN},
    "ws64": {"NT": EPIWS_NT, "NN": EPIWS_NN},
}
_LAY = {"NT": (False, False), "NN": (False, True), "TT": (True, True)}   # (a_trans, b_trans)
# the ragged shape of section B, and its N rounded so that mask_out's N % 32 == 0 holds
EPI_SHAPE = {"p3": (264, 136, 160), "p4": (264, 264, 288), "ring": (72, 72, 96), "ring128": (136, 72, 96),
             "ws": (264, 256, 256), "ws64": (72, 128, 128)}


def cases_epilogues():
    """C / D. every instantiated fast epilogue on every family that has it, at the family's ragged shape, K = 192;
    the dropout ones are section D's fast-path cases."""
    out = []
    for fam, per_layout in FAMILY_EPIS.items():
        m, n, n32 = EPI_SHAPE[fam]
        for lname, epis in per_layout.items():
            at, bt = _LAY[lname]
            for epi in epis:
                nn = n32 if epi & E_MASKOUT else n
                out.append(Case(f"epi-{fam}-{lname}-{epi}", fam, m, nn, 192, at, bt, kernel=DMA_FAMILIES[fam][0],
                                epi=epi, **_flags(epi)))
        if fam in ("p3", "ring"):
            # bf16 C whose rows are 8- but not 16-byte aligned: the fast epilogue without the paired stores
            for epi in (1, 7, 8, 512):
                at, bt = _LAY["NT" if epi in (1, 7) else "NN"]
                out.append(Case(f"epi-{fam}-unpaired-{epi}", fam, m, n, 192, at, bt, kernel=fam, epi=epi, ldc_pad=4,
                                **_flags(epi)))
    # p4 has no bias + ReLU (+ mask bits) instantiation without dropout: the plan runs the dropout one, keeping all
    m, n, n32 = EPI_SHAPE["p4"]
    out.append(Case("epi-p4-NT-3as7", "p4", m, n, 192, kernel="p4", epi=7, **_flags(3)))
    out.append(Case("epi-p4-NT-1027as1031", "p4", m, n32, 192, kernel="p4", epi=1031, **_flags(1027)))
    # N > 4096: the p3 / p4 bias epilogues run as column chunks of their LDS bias stage
    out.append(Case("epi-p3-chunks-1", "p3", 8, 4104, 64, kernel="p3", epi=1, **_flags(1)))
    out.append(Case("epi-p4-chunks-1", "p4", 8, 4104, 64, kernel="p4", epi=1, **_flags(1)))
    out.append(Case("epi-p4-chunks-3as7", "p4", 8, 4104, 64, kernel="p4", epi=7, **_flags(3)))
    # the generic epilogue with everything at once: bf16 C, odd N
    for gate, resid in (("bf16", "f32"), ("f32", "bf16"), ("bits", "f32")):
        for drop in (False, True):
            out.append(Case(f"epi-generic-{gate}-{resid}-{'drop' if drop else 'keep'}", "reg64", 33, 37, 100,
                            kernel="reg", tile=64, c_f32=False, lda_pad=4, ldb_pad=4, ldc_pad=_odd_pad(37), alpha=2.0,
                            beta=1.0, bias=True,
                            rowadd=True, relu=True, drop=drop, gate=gate, resid=resid))
    out.append(Case("epi-generic-f32c", "reg128", 65, 129, 72, kernel="reg", tile=128, ldc_pad=_odd_pad(129),
                    alpha=0.5, beta=1.0, bias=True, rowadd=True, gate="f32", resid="bf16", vec=True))
    return out


def cases_dropout():
    """D. the generic dropout path: odd N (a hash pair straddles two rows) and z > 0 of the index (z M + m) N + n."""
    out = []
    for m, n in ((7, 5), (33, 17), (65, 129)):
        out.append(Case(f"drop-generic-{m}x{n}", "reg64", m, n, 40, kernel="reg", tile=64, drop=True, bias=True,
                        resid="f32", ldc_pad=_odd_pad(n)))
    out.append(Case("drop-generic-relu", "reg64", 33, 17, 40, kernel="reg", tile=64, drop=True, bias=True, relu=True,
                    c_f32=False, ldc_pad=_odd_pad(17)))
    for at, bt in ((False, False), (True, True)):
        out.append(Case(f"drop-batch2-{_lname(at, bt)}", "reg64", 33, 17, 40, at, bt, kernel="reg", tile=64,
                        drop=True, bias=True, batch=2, ldc_pad=_odd_pad(17), lda_pad=_vec_pad(33 if at else 40),
                        ldb_pad=_vec_pad(17 if bt else 40)))
    out.append(Case("drop-batch2-p3", "p3", 264, 136, 64, kernel="p3", epi=E_GENERIC, drop=True, batch=2))
    return out


SPLITS = [(320, 5), (576, 7), (320, 4), (640, 8)]   # the last three leave trailing splits without a K range


def empty_splits(k, splitk, bk=64):
    steps = -(-k // bk)
    per = -(-steps // splitk)
    return [s for s in range(splitk) if s * per >= steps]


def cases_splitk():
    """E. split-K into fp32 C on every family that splits, beta 0 and 1, with the fused row sums where A is
    k-strided; splits without a K range included."""
    out = []
    fams = [("reg64", "reg", 64, (65, 129), [(False, False), (True, True)]),
            ("reg128", "reg", 128, (130, 72), [(False, True), (True, True)]),
            ("p3", "p3", 0, (264, 136), [(False, False), (True, True)]),
            ("ring", "ring", 0, (72, 72), [(False, False)]),
            ("ring128", "ring128", 0, (136, 72), [(False, True)])]
    for fam, kern, tile, (m, n), lays in fams:
        for at, bt in lays:
            for k, sk in SPLITS:
                for beta in (0.0, 1.0):
                    out.append(Case(f"split-{fam}-{_lname(at, bt)}-k{k}s{sk}-b{int(beta)}", fam, m, n, k, at, bt,
                                    kernel=kern, tile=tile, splitk=sk, beta=beta, rowsum=at, ldc_pad=4,
                                    lda_pad=_vec_pad(m if at else k), ldb_pad=_vec_pad(n if bt else k)))
    for tile, fam in ((64, "reg64"), (128, "reg128")):
        for beta in (0.0, 1.0):   # ragged last split
            out.append(Case(f"split-{fam}-k200s3-b{int(beta)}", fam, 65, 129, 200, True, True, kernel="reg",
                            tile=tile, splitk=3, beta=beta, rowsum=True, ldc_pad=_odd_pad(129),
                            lda_pad=_vec_pad(65), ldb_pad=_vec_pad(129)))
    # fp32 operands, 16-deep K-steps: 80 = 5 steps over 5 splits; 144 = 9 steps over 7 splits of 2 (splits 5, 6 empty)
    assert not empty_splits(80, 5, 16) and empty_splits(144, 7, 16) == [5, 6]
    for k, sk in ((80, 5), (144, 7)):
        for at, bt in ((False, False), (True, True)):
            out.append(Case(f"split-f32-{_lname(at, bt)}-k{k}s{sk}", "f32", 65, 33, k, at, bt, in_f32=True, splitk=sk,
                            beta=1.0, ldc_pad=4))
    # K of one step under many splits: a single split has a K range
    out.append(Case("split-p3-NT-k64s2-b0", "p3", 264, 136, 64, kernel="p3", splitk=2, ldc_pad=4))
    out.append(Case("split-p3-TT-k64s3-b1", "p3", 264, 136, 64, True, True, kernel="p3", splitk=3, beta=1.0,
                    rowsum=True, ldc_pad=4))
    return out


def cases_attention():
    """F. the six batched GEMMs of the unfused attention, bf16 and fp32."""
    out = []
    for name, (m, n, k, at, bt, _, _, _) in ATTN_SHAPES.items():
        out.append(Case(f"attn-{name}-bf16", "reg64", m, n, k, at, bt, attn=name, c_f32=False))
        out.append(Case(f"attn-{name}-f32", "f32", m, n, k, at, bt, attn=name, in_f32=True))
    return out


def cases_plan():
    """Requests the planner cannot honour (it plans the register kernel, and the table says so), the decode-step
    GEMMs (M < 8) and what the auto plan picks at small sizes."""
    out = []
    fb = dict(kernel="p3", fallback=True, tile=64)
    out.append(Case("plan-p3-k100", "reg64", 72, 72, 100, lda_pad=4, ldb_pad=4, **fb))          # K % 64 != 0
    out.append(Case("plan-p3-at-m68", "reg64", 68, 72, 128, True, True, lda_pad=4, **fb))      # a_trans, M % 8 != 0
    out.append(Case("plan-p4-bt-n68", "reg64", 72, 68, 128, False, True, kernel="p4", fallback=True, tile=64,
                    ldb_pad=4))                                                                # b_trans, N % 8 != 0
    out.append(Case("plan-ring-lda", "reg64", 72, 72, 128, kernel="ring", fallback=True, tile=64, lda_pad=4,
                    vec=False))
    out.append(Case("plan-ring128-offb", "reg64", 72, 72, 128, kernel="ring128", fallback=True, tile=64, off_b=1,
                    vec=False))
    out.append(Case("plan-ring-at", "reg64", 72, 72, 128, True, False, kernel="ring", fallback=True, tile=64))
    out.append(Case("plan-ws-m4", "reg64", 4, 128, 128, kernel="ws", fallback=True, tile=64, bias=True, c_f32=False))
    # decode steps: M < 8 never takes an LDS-DMA family
    for m in (1, 4, 7):
        out.append(Case(f"plan-decode-m{m}", "reg64", m, 512, 512, bias=True, c_f32=False, fallback=True))
        out.append(Case(f"plan-decode-m{m}-NN", "reg64", m, 96, 512, False, True, c_f32=False, fallback=True))
    # the auto plan at small grids: the 64 x 64 ring for k-contiguous A, the register kernel for A^T
    out.append(Case("plan-auto-ring", "ring", 72, 72, 128, epi=1, bias=True, c_f32=False))
    out.append(Case("plan-auto-ring-NN", "ring", 72, 136, 192, False, True, epi=E_F32))
    out.append(Case("plan-auto-reg-TN", "reg64", 72, 136, 192, True, True))
    return out


def all_cases():
    out = (cases_reg() + cases_dma_edges() + cases_epilogues() + cases_dropout() + cases_splitk() +
           cases_attention() + cases_plan())
    ids = [c.id for c in out]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    return out


# ------------------------------------------------------------------------------------------------ G. grouped

GROUP_KINDS = {   # kind -> (asrx.kernels WGRAD_KIND, WGRAD_QUEUE, kernel names for beta 0 / 1)
    "reg": ("reg", False, ("gemm_bf16_grouped_dev_kernel<true, true>",) * 2),
    "p3": ("p3", False, ("gemm_bf16_p3g_kernel<64>", "gemm_bf16_p3g_kernel<96>")),
    "p4": ("p4", False, ("gemm_bf16_p4g_kernel<64>", "gemm_bf16_p4g_kernel<96>")),
    "ws": ("ws", False, ("gemm_bf16_wsg_kernel<64>", "gemm_bf16_wsg_kernel<96>")),
    "wsq": ("ws", True, ("gemm_bf16_wsgq_kernel<64>", "gemm_bf16_wsgq_kernel<96>")),
}
# (rows, n, k): dW[n][k] (+)= dY[rows][n]^T X[rows][k]
GROUPS = [(1, 8, 64), (63, 136, 72), (65, 264, 264), (200, 136, 64), (264, 8, 264)]


def make_groups(beta, seed):
    """The five weight gradients of section G: per group the host buffers (dY and X NaN-poisoned around the matrix,
    ld = row + 8; dW and the bias gradient sentinel-guarded), the views' geometry and the exact results."""
    rs = np.random.RandomState(seed)
    out = []
    for gi, (rows, n, k) in enumerate(GROUPS):
        g = Built()
        dy = rs.randint(-3, 4, size=(rows, n)).astype(np.float64)
        x = rs.randint(-3, 4, size=(rows, k)).astype(np.float64)
        old = rs.randint(-8, 9, size=(n, k)).astype(np.float64)
        g.lay = dict(dy=Lay(rows, n, n + 8), x=Lay(rows, k, k + 8), w=Lay(n, k, k + 4))
        g.bufs = dict(dy=_filled(g.lay["dy"].size, torch.bfloat16, lay=g.lay["dy"], values=dy),
                      x=_filled(g.lay["x"].size, torch.bfloat16, lay=g.lay["x"], values=x),
                      w=_filled(g.lay["w"].size, torch.float32, SENTINEL, g.lay["w"],
                                old if beta else np.full((n, k), np.nan)))
        g.expect_w = as_tensor(_exact(dy.T @ x + (old if beta else 0.0), "dW"), torch.float32)
        g.expect_b = None
        if gi % 2 == 0:   # bias-gradient row sums on every other group (always accumulated)
            bold = rs.randint(-8, 9, size=n).astype(np.float64)
            g.bufs["bg"] = _filled(n + 128, torch.float32, SENTINEL, values=bold, span=(64, 64 + n))
            g.expect_b = as_tensor(_exact(bold + dy.sum(0), "db"), torch.float32)
        out.append(g)
    return out
