"""The conv front-end kernels (frontend.hip, the tall-K gather of gemm.hip) beyond the benchmark geometry, against
the fp64 CPU references of frontend_ref.py: a sweep of tiny geometries through all eight entry points, exact integer
cases, the persistent multi-tile / multi-row paths at one larger shape, and the accepted limits.

Error measures.  Forwards and data gradients per element: |got - ref| <= tol * S + r * |ref| with S the same
convolution of the operands' absolute values, tol = 1e-5 for fp32 operands and 1e-2 for bf16 operands, r = 2^-8 for a
bf16 output.  Weight / bias gradients: the max-normalised relerr of test_gpu_kernels.py with its bounds.  Every test
prints its worst error/bound ratio before asserting.

r = 2^-8 is the largest relative error of a correct round-to-nearest-even to bf16 (half an ulp at the bottom of a
binade), so a bf16 output sits close to its bound by construction.  Worst error/bound over every case of this file on
an MI355X: conv1_fwd 0.023 (fp32) / 0.993 (bf16, the rounding), conv2_fwd 0.107, col2im 0.013, conv2_wgrad 0.029,
conv1_bwd_w 0.019, conv1_bwd_fused 0.0017, conv_bwd_implicit 0.023 (bf16-operand reference) / 0.26 (exact operands);
im2col and the integer cases are bit-exact.  Launches with 73,152 and 81,920 B of dynamic LDS are accepted by the
runtime as they are (no function attribute) and compute correctly."""
import math
import zlib

import pytest
import torch

from tests import frontend_ref as R
from tests.frontend_ref import BF16, F32

pytestmark = pytest.mark.gpu

dev = "cuda"
U8 = torch.uint8
DT = [F32, BF16]
DTID = {F32: "f32", BF16: "bf16"}.get


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def tol_for(dt):
    return 1e-5 if dt == F32 else 1e-2


def out_r(dt):
    return 0.0 if dt == F32 else 2.0 ** -8


# ------------------------------------------------------------------------------------------------ helpers

GUARD = 512   # guard elements before and after a payload (keeps the payload 16-byte aligned for every dtype)
_BITS = {F32: torch.int32, BF16: torch.int16, U8: torch.uint8}


def guarded(shape, dt):
    """(buffer, payload view): the payload lies between two guard runs, everything filled with a sentinel (NaN for
    floats, 0xA5 for bytes)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), 0xA5 if dt == U8 else float("nan"), dtype=dt, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def put(t):
    """An input tensor on the device between NaN (0xA5) guards: a read one row out of range is poisoned, not lucky."""
    _, v = guarded(tuple(t.shape), t.dtype)
    v.copy_(t)
    return v


def check_guards(buf, what):
    """Guards bit-identical to the sentinel, no sentinel left in a float payload.  (A byte payload is compared bit
    for bit with its reference by the caller: 0xA5 is a legal mask byte.)"""
    torch.cuda.synchronize()
    bits = buf.view(_BITS[buf.dtype]).cpu()
    sent = torch.full((1,), 0xA5 if buf.dtype == U8 else float("nan"), dtype=buf.dtype).view(_BITS[buf.dtype])
    assert bool((bits[:GUARD] == sent).all()), f"{what}: wrote before the tensor"
    assert bool((bits[-GUARD:] == sent).all()), f"{what}: wrote past the tensor"
    if buf.dtype != U8:
        assert not bool(torch.isnan(buf[GUARD:-GUARD]).any()), f"{what}: elements never written"


def check_elem(what, got, ref, S, tol, r=0.0, where=None):
    """Per element |got - ref| <= tol * S + r * |ref|; `where(idx)` adds to the failure message."""
    got, ref, S = got.detach().double().cpu(), ref.double(), S.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = tol * S + r * ref.abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    idx = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)) if ratio.numel() else ()
    print(f"{what}: worst error/bound {worst:.3g} at {idx}")
    assert worst <= 1.0, (f"{what}: error/bound {worst:.3g} at {idx}: got {float(got[idx])!r}, ref {float(ref[idx])!r}"
                          + (where(idx) if where else ""))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_rel(what, got, ref, bound):
    e = relerr(got, ref)
    print(f"{what}: relerr {e:.3g}, error/bound {e / bound:.3g}")
    assert e < bound, f"{what}: relerr {e:.3g} >= {bound:g}"   # (a NaN fails too)


def grad_init(ref_w, ref_b, gen):
    """Random starting values of a gradient pair, a quarter of the gradient's own scale so that neither the start
    nor the increment hides under the other in the max-normalised error."""
    sw = float(ref_w.abs().max().clamp_min(1e-3)) * 0.25
    sb = float(ref_b.abs().max().clamp_min(1e-3)) * 0.25
    w0 = (torch.randn(ref_w.shape, generator=gen) * sw).float()
    return w0, (torch.randn(ref_b.shape, generator=gen) * sb).float()


def gen_for(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ the kernels

def run_conv1_fwd(c, dt):
    ybuf, y1 = guarded((c.B, c.F1, c.T1, 64), dt)
    mbuf, y1m = guarded((c.B, c.F1, c.T1, 8), U8)
    K().conv1_fwd(put(c.x), put(c.w1.reshape(64, 9)), put(c.b1), y1, mask=y1m)
    check_guards(ybuf, "y1")
    check_guards(mbuf, "y1_mask")
    check_elem(f"conv1_fwd {DTID(dt)}", R.nchw(y1.float().cpu()), c.ref1, c.S1, 1e-5, out_r(dt))   # fp32 operands
    assert torch.equal(R.unpack_mask(y1m.cpu()), y1.float().cpu() > 0), "y1_mask bits != (y1 > 0) as stored"


def run_conv2_fwd(c):
    obuf, out = guarded((c.M, 64), BF16)
    K().conv2_fwd(put(c.y1(BF16)), put(R.w2_phys(c.w2).to(BF16)), put(c.b2), out)
    check_guards(obuf, "conv2 out")
    pre, S = c.ref2(BF16)
    b = c.b2.double().view(1, 64, 1, 1)

    def where(idx):   # the persistent walk: tile -> workgroup tile % 256, walk step tile // 256
        row = (idx[0] * c.T2 + idx[3]) * c.F2 + idx[2]
        ntiles = (c.M + 255) // 256
        grid = min(ntiles, 256)
        return (f"; row {row} = row {row % 256} of tile {row // 256} of {ntiles}, walk step {row // 256 // grid} of "
                f"workgroup {row // 256 % grid}")
    check_elem("conv2_fwd", R.from_rows(out.float().cpu(), c.B, c.F2, c.T2), torch.relu(pre + b), S + b.abs(), 1e-2,
               2.0 ** -8, where)


def run_conv2_wgrad(c, splitk, with_db):
    rw, rb = c.conv2_grads
    w0, b0 = grad_init(rw, rb, gen_for("w2", c.B, c.F, c.T, splitk))
    dw, db = put(w0), put(b0)
    K().conv2_wgrad(put(c.dy2(BF16)), put(c.y1(BF16)), dw, db if with_db else None, splitk=splitk)
    check_rel(f"conv2_wgrad dw splitk={splitk}", dw, w0.double() + rw, 1e-5)
    if with_db:
        check_rel(f"conv2_wgrad db splitk={splitk}", db, b0.double() + rb, 1e-5)
    else:
        assert torch.equal(db.cpu(), b0), "db written although None was passed"


def run_implicit(c):
    (rw3, rb3), (rw2, rb2) = c.implicit_grads
    w0, b0 = grad_init(rw2, rb2, gen_for("imp", c.B, c.F, c.T))
    dw, db = put(w0), put(b0)
    K().conv_bwd_implicit(put(c.dy2(BF16)), put(R.w2_phys(c.w2).to(BF16)), put(R.pack_mask(c.y1(BF16))), put(c.x),
                          dw, db)
    # against the fp64 gradient of the bf16-rounded MFMA operands (dy1, x), and the unrounded one at bf16 level
    check_rel("conv_bwd_implicit dw (bf16 operands)", dw, w0.double() + rw3, 1e-3)
    check_rel("conv_bwd_implicit db (bf16 operands)", db, b0.double() + rb3, 1e-3)
    check_rel("conv_bwd_implicit dw (exact operands)", dw, w0.double() + rw2, 1e-2)
    check_rel("conv_bwd_implicit db (exact operands)", db, b0.double() + rb2, 1e-2)


# ------------------------------------------------------------------------------------------------ 1. geometry sweep

SHAPES = [
    (1, 7, 7),     # F1 = T1 = 3, F2 = T2 = 1: the smallest legal input; T1 < 8 (6 of 8 fused segments empty), one row
    (2, 9, 10),    # F1 = T1 = 4 (both even: a dead conv1 row and column), F2 = T2 = 1, an x column nobody reads
    (2, 11, 27),   # F1 = 5, T1 = 13 (< 16: idle implicit waves), F2 = 2, T2 = 6 (five carries inside one tall-K stage)
    (3, 15, 63),   # T1 = 31 (n0 = 16, n1 = 15), T2 = 15 (not a divisor of 32), 45 rows per utterance: one conv2 tile
                   #   and one tall-K stage span all three utterances
    (2, 12, 66),   # T1 = 32 (n0 = n1 = 16: both parities end on a chunk edge; dead column), F1 = 5
    (4, 23, 68),   # T1 = 33 (n0 = 17: one position into a second chunk), F1 = 11, T2 = 16, M = 320: two conv2 tiles
                   #   (the second ragged), utterance boundaries at rows 80/160/240, ten tall-K steps at splitk = 1
    (1, 10, 70),   # T1 = 34 (n0 = n1 = 17), F1 = 4 (dead row and column), F2 = 1
]
SID = [f"{b}x{f}x{t}" for b, f, t in SHAPES]


@pytest.mark.parametrize("dt", DT, ids=DTID)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv1_fwd(shape, dt):
    run_conv1_fwd(R.case(*shape), dt)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv2_fwd(shape):
    run_conv2_fwd(R.case(*shape))


@pytest.mark.parametrize("dt", DT, ids=DTID)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_im2col(shape, dt):
    """A gather: the image must equal the reference unfold of the same y1 bit for bit."""
    c = R.case(*shape)
    cbuf, cols = guarded((c.M, 576), dt)
    K().im2col_conv2(put(c.y1(dt)), cols)
    check_guards(cbuf, "cols")
    ref = R.rows_of_cols(R.nchw(c.y1(dt).double()), c.F2, c.T2)
    assert torch.equal(cols.cpu().double(), ref)


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("splitk", [1, 3, 7, 256])   # 256 (and mostly 7) exceed the 64-row K blocks: empty splits
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv2_wgrad(shape, splitk, with_db):
    """Against the fp64 autograd weight gradient of conv2d (no GPU-made im2col image), += on random gradients."""
    run_conv2_wgrad(R.case(*shape), splitk, with_db)


@pytest.mark.parametrize("yd", DT, ids=DTID)
@pytest.mark.parametrize("dd", DT, ids=DTID)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_col2im(shape, dd, yd):
    c = R.case(*shape)
    dbuf, dy1 = guarded((c.B, c.F1, c.T1, 64), F32)
    K().col2im_conv2(put(c.dcols(dd)), put(c.y1(yd)), dy1)
    check_guards(dbuf, "dy1")
    ref, S = c.dy1(dd, yd)
    got = R.nchw(dy1.cpu())
    check_elem(f"col2im dcols {DTID(dd)} y1 {DTID(yd)}", got, ref, S, tol_for(dd))
    # a conv1 row / column that conv2 never reads (F1 / T1 even) has exactly no gradient
    if c.F1 % 2 == 0:
        assert not bool(got[:, :, c.F1 - 1].any()), "gradient on the conv1 row conv2 never reads"
    if c.T1 % 2 == 0:
        assert not bool(got[:, :, :, c.T1 - 1].any()), "gradient on the conv1 column conv2 never reads"


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv1_bwd_w(shape):
    c = R.case(*shape)
    dy1 = R.cl(c.dy1(F32, F32)[0]).float()                      # the kernel's input: an fp32 dy1
    rw, rb = R.conv1_wgrad(c.x, R.nchw(dy1))
    w0, b0 = grad_init(rw, rb, gen_for("w1", *shape))
    dw, db = put(w0), put(b0)
    K().conv1_bwd_w(put(c.x), put(dy1), dw, db)
    check_rel("conv1_bwd_w dw", dw, w0.double() + rw, 1e-5)
    check_rel("conv1_bwd_w db", db, b0.double() + rb, 1e-5)


@pytest.mark.parametrize("yd", DT, ids=DTID)
@pytest.mark.parametrize("dd", DT, ids=DTID)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv1_bwd_fused(shape, dd, yd):
    """All four (dcols, y1) dtype pairs: the v8 kernel and the three conv1_bwd_fused_kernel<DT, YT> in use, each operand
    rounded to its own dtype in the reference."""
    c = R.case(*shape)
    rw, rb = c.conv1_grads(dd, yd)
    w0, b0 = grad_init(rw, rb, gen_for("fu", *shape, dd, yd))
    dw, db = put(w0), put(b0)
    K().conv1_bwd_fused(put(c.dcols(dd)), put(c.y1(yd)), put(c.x), dw, db)
    check_rel(f"conv1_bwd_fused dw {DTID(dd)}/{DTID(yd)}", dw, w0.double() + rw, 1e-4)
    check_rel(f"conv1_bwd_fused db {DTID(dd)}/{DTID(yd)}", db, b0.double() + rb, 1e-4)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_conv_bwd_implicit(shape):
    run_implicit(R.case(*shape))


# ------------------------------------------------------------------------------------------------ 2. exact integers

def same(got, ref, dt):
    """got equals the exact integer result rounded to dt, bit for bit (the sign of a zero aside: the fp64 reference
    gates by multiplication and keeps -0 where the kernels store +0)."""
    want = ref.to(dt) + 0
    torch.cuda.synchronize()
    return torch.equal((got.cpu() + 0).view(_BITS[dt]), want.view(_BITS[dt]))


def test_exact_conv2_fwd_and_im2col():
    e = R.exact_case()
    obuf, out = guarded((e.M, 64), BF16)
    K().conv2_fwd(put(e.y1.to(BF16)), put(R.w2_phys(e.w2).to(BF16)), put(e.b2.float()), out)
    check_guards(obuf, "conv2 out")
    assert same(out, e.out, BF16)
    for dt in DT:
        cbuf, cols = guarded((e.M, 576), dt)
        K().im2col_conv2(put(e.y1.to(dt)), cols)
        check_guards(cbuf, "cols")
        assert same(cols, e.cols, dt)


@pytest.mark.parametrize("splitk", [1, 2, 256])
def test_exact_conv2_wgrad(splitk):
    e = R.exact_case()
    dw, db = put(e.dw2_0.float()), put(e.db2_0.float())
    K().conv2_wgrad(put(e.dy2.to(BF16)), put(e.y1.to(BF16)), dw, db, splitk=splitk)
    assert same(dw, e.dw2, F32)
    assert same(db, e.db2, F32)


@pytest.mark.parametrize("yd", DT, ids=DTID)
@pytest.mark.parametrize("dd", DT, ids=DTID)
def test_exact_col2im_and_conv1_bwd_fused(dd, yd):
    e = R.exact_case()
    dbuf, dy1 = guarded((e.B, e.F1, e.T1, 64), F32)
    K().col2im_conv2(put(e.dcols.to(dd)), put(e.y1.to(yd)), dy1)
    check_guards(dbuf, "dy1")
    assert same(dy1, e.dy1, F32)
    dw, db = put(e.dw1_0.float()), put(e.db1_0.float())
    K().conv1_bwd_fused(put(e.dcols.to(dd)), put(e.y1.to(yd)), put(e.x.float()), dw, db)
    assert same(dw, e.dw1_f, F32)
    assert same(db, e.db1_f, F32)


def test_exact_conv1_bwd_w():
    e = R.exact_case()
    dw, db = put(e.dw1_0.float()), put(e.db1_0.float())
    K().conv1_bwd_w(put(e.x.float()), put(e.dy1_in.float()), dw, db)
    assert same(dw, e.dw1_w, F32)
    assert same(db, e.db1_w, F32)


# ------------------------------------------------------------------------------------------------ 3. persistent paths

# 136,800 conv2 rows = 535 tiles of 256 (the last holds 96 rows) over 256 persistent workgroups: workgroups 0-22 walk
# three tiles, the others two.  9360 conv1 rows over 512 persistent workgroups of the implicit backward.  2138 K blocks
# in the weight gradient: 576 rows = 18 ring steps per split at splitk = 256, utterance boundaries (570 rows) inside
# every split.
BIG = (240, 80, 125)


@pytest.fixture(scope="module")
def big():
    c = R.Case(*BIG)
    assert (c.F1, c.T1, c.F2, c.T2, c.M) == (39, 62, 19, 30, 136800)
    return c


def test_big_conv1_fwd(big):
    run_conv1_fwd(big, BF16)


def test_big_conv2_fwd(big):
    """A failure names the tile and the walk step of the worst element (run_conv2_fwd's `where`)."""
    run_conv2_fwd(big)


@pytest.mark.parametrize("splitk", [256, 37])
def test_big_conv2_wgrad(big, splitk):
    run_conv2_wgrad(big, splitk, True)


def test_big_conv_bwd_implicit(big):
    run_implicit(big)


# ------------------------------------------------------------------------------------------------ 4. limits

def test_conv1_fwd_longest_row():
    """T = 5120 is the longest accepted input (three fp32 lines = 60 KiB of dynamic LDS); 5121 is refused."""
    run_conv1_fwd(R.Case(1, 7, 5120), F32)
    x = torch.zeros(1, 1, 7, 5121, device=dev)
    y1 = torch.empty(1, 3, 2560, 64, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        K().conv1_fwd(x, torch.zeros(64, 9, device=dev), torch.zeros(64, device=dev), y1)


@pytest.mark.parametrize("T", [1500, 2048])
def test_conv_bwd_implicit_above_64k_lds(T):
    """73,152 B and (T = 2048, T1 = 1023: the longest accepted input) exactly 81,920 B of dynamic LDS."""
    assert K().conv_bwd_implicit_fits(T) and not K().conv_bwd_implicit_fits(2049)
    run_implicit(R.Case(1, 7, T))


@pytest.mark.parametrize("T", [2049, 2050, 2051])
def test_frontend_module_past_the_implicit_limit(T):
    """asrx.FrontEnd forward + backward (bf16 compute) where the implicit backward no longer fits its LDS (T = 2049,
    2050: T1 = 1024 passes the T1 cap but not the LDS sum) and past the cap (2051): all take linear_dgrad +
    conv1_bwd_fused.  Integer weights, input and gradients keep every bf16 intermediate exact (y1 <= 10, features
    <= 91, one conv2 weight per (tap, output channel, input channel)), so the fp64 nn.Sequential of the same weights is
    the reference of the bf16 path itself and the conv1_bwd_fused bound applies to every gradient."""
    import asrx
    from torch import nn
    g = torch.Generator().manual_seed(T)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    w1, b1, b2 = ri(-1, 1, 64, 1, 3, 3), ri(-1, 1, 64), ri(-1, 1, 64)
    w2 = torch.zeros(64, 64, 3, 3, dtype=torch.float64)
    for tap in range(9):
        for co in range(64):
            w2[co, (5 * co + 7 * tap + 3) % 64, tap // 3, tap % 3] = (-1) ** (co + tap)
    x = ri(-1, 1, 1, 1, 7, T)
    ref = nn.Sequential(nn.Conv2d(1, 64, 3, stride=2), nn.ReLU(), nn.Conv2d(64, 64, 3, stride=2), nn.ReLU()).double()
    fe = asrx.FrontEnd()
    with torch.no_grad():
        for m in (ref, fe):
            m[0].weight.copy_(w1), m[0].bias.copy_(b1), m[2].weight.copy_(w2), m[2].bias.copy_(b2)
    fe = fe.cuda()
    out = fe(x.float().cuda())
    want = ref(x)
    gy = ri(-2, 2, *want.shape)
    out.backward(gy.float().cuda())
    want.backward(gy)
    torch.cuda.synchronize()
    assert float(want.max()) <= 256 and relerr(out.float(), want) < 1e-2
    for name, p, q in [("conv1.weight", fe[0].weight, ref[0].weight), ("conv1.bias", fe[0].bias, ref[0].bias),
                       ("conv2.weight", fe[2].weight, ref[2].weight), ("conv2.bias", fe[2].bias, ref[2].bias)]:
        check_rel(f"FrontEnd T={T} {name}.grad", p.grad, q.grad, 1e-4)


def _offset(t):
    """The same values one element off the allocation's alignment."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("entry,which", [("conv2_fwd", "y1"), ("conv2_wgrad", "dy2"), ("conv2_wgrad", "y1"),
                                         ("conv_bwd_implicit", "dy2"), ("conv_bwd_implicit", "y1_mask"),
                                         ("conv_bwd_implicit", "F<7")])
def test_refusals_raise(entry, which):
    """Arguments the C entry points refuse before any launch (their pointer-alignment guards and
    asrx_conv_bwd_implicit's F >= 7) surface as exceptions.  Every buffer is real and fully sized."""
    c = R.case(2, 11, 27) if which != "F<7" else R.Case(1, 6, 9)
    y1, dy2 = c.y1(BF16).to(dev), torch.zeros(max(c.M, 1), 64, dtype=BF16, device=dev)
    w2 = R.w2_phys(c.w2).to(BF16).to(dev)
    y1m = R.pack_mask(c.y1(BF16)).to(dev)
    dw2, db2 = torch.zeros(64, 576, device=dev), torch.zeros(64, device=dev)
    dw1, db1 = torch.zeros(64, 9, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        if entry == "conv2_fwd":
            K().conv2_fwd(_offset(y1), w2, c.b2.to(dev), torch.empty(c.M, 64, dtype=BF16, device=dev))
        elif entry == "conv2_wgrad":
            K().conv2_wgrad(_offset(dy2) if which == "dy2" else dy2, _offset(y1) if which == "y1" else y1, dw2, db2)
        else:
            K().conv_bwd_implicit(_offset(dy2) if which == "dy2" else dy2, w2,
                                  _offset(y1m) if which == "y1_mask" else y1m, c.x.to(dev), dw1, db1)
    torch.cuda.synchronize()
    assert not bool(dw2.any()) and not bool(dw1.any())
