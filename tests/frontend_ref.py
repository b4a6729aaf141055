"""fp64 CPU references of the conv front-end (frontend.hip, the tall-K gather of gemm.hip) for test_gpu_frontend.py.

Forwards are torch.nn.functional.conv2d in fp64, gradients its autograd; operands are rounded to the kernel's
storage dtype exactly where the kernel reads them rounded.  Nothing here touches the GPU: every tensor a kernel
under test is given (y1, the sign-bit mask, dcols, dy1) is made here, never by another kernel."""
import functools

import torch
import torch.nn.functional as Fn

F32, BF16 = torch.float32, torch.bfloat16


def memo(fn):
    """Per-instance cache of a method's results (the references die with their case)."""
    @functools.wraps(fn)
    def wrapped(self, *args):
        key = (fn.__name__, args)
        if key not in self.__dict__.setdefault("_memo", {}):
            self._memo[key] = fn(self, *args)
        return self._memo[key]
    return wrapped


def dims(F, T):
    F1, T1 = (F - 3) // 2 + 1, (T - 3) // 2 + 1
    return F1, T1, (F1 - 3) // 2 + 1, (T1 - 3) // 2 + 1


def cl(t):
    """(B, C, H, W) -> channels-last (B, H, W, C), contiguous."""
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def rows_of(t):
    """(B, 64, F2, T2) -> the conv2 GEMM rows [(b, t2, f2)][64]."""
    return t.permute(0, 3, 2, 1).reshape(-1, t.shape[1]).contiguous()


def from_rows(r, B, F2, T2):
    return r.view(B, T2, F2, -1).permute(0, 3, 2, 1)


def w2_phys(w2):
    """(co, ci, kh, kw) -> the [64][576] operand with columns (kh, kw, ci)."""
    return w2.permute(0, 2, 3, 1).reshape(64, 576).contiguous()


def pack_mask(y1_cl):
    """conv1_fwd's sign bits of a channels-last y1: byte q of a position holds channels 8q..8q+7, bit c = y1 > 0."""
    bits = (y1_cl > 0).view(*y1_cl.shape[:3], 8, 8).to(torch.int32)
    return (bits << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def unpack_mask(m):
    return torch.stack([(m >> i) & 1 for i in range(8)], -1).reshape(*m.shape[:3], 64).bool()


def fold_cols(dcols, B, F1, T1):
    """col2im of conv2: dcols [(b, t2, f2)][(kh, kw, c)] -> (B, 64, F1, T1), the sum of the taps that read a position."""
    F2, T2 = (F1 - 3) // 2 + 1, (T1 - 3) // 2 + 1
    u = dcols.view(B, T2, F2, 3, 3, 64).permute(0, 5, 3, 4, 2, 1).reshape(B, 576, F2 * T2)
    return Fn.fold(u, (F1, T1), 3, stride=2)


def conv1_wgrad(x, dy1):
    """fp64 autograd gradients of conv1 (weight (64, 9), bias (64)) for the output gradient dy1 (B, 64, F1, T1)."""
    w = torch.zeros(64, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    Fn.conv2d(x.double(), w, b, stride=2).backward(dy1.double())
    return w.grad.reshape(64, 9), b.grad


def conv2_wgrad(y1_nchw, dy2_nchw):
    """fp64 autograd gradients of conv2 in the kernel's layout: weight [64][(kh, kw, ci)], bias [64]."""
    w = torch.zeros(64, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    Fn.conv2d(y1_nchw.double(), w, b, stride=2).backward(dy2_nchw.double())
    return w2_phys(w.grad), b.grad


def conv2_dgrad(dy2_nchw, w2, shape):
    """fp64 autograd data gradient of conv2 for an input of `shape` (B, 64, F1, T1)."""
    y = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    Fn.conv2d(y, w2.double(), stride=2).backward(dy2_nchw.double())
    return y.grad


class Case:
    """One random front-end problem and its fp64 references, computed lazily and once."""

    def __init__(self, B, F, T, seed=5):
        self.B, self.F, self.T = B, F, T
        self.F1, self.T1, self.F2, self.T2 = dims(F, T)
        self.M = B * self.T2 * self.F2
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(B, 1, F, T, generator=g)
        self.w1 = torch.randn(64, 1, 3, 3, generator=g) * 0.3
        self.b1 = torch.randn(64, generator=g) * 0.1
        self.w2 = torch.randn(64, 64, 3, 3, generator=g) * 0.05
        self.b2 = torch.randn(64, generator=g) * 0.1
        self.gy = torch.randn(B, 64, self.F2, self.T2, generator=g)
        self.g = g

    @functools.cached_property
    def ref1(self):
        """relu(conv1(x)) in fp64, (B, 64, F1, T1)."""
        return torch.relu(Fn.conv2d(self.x.double(), self.w1.double(), self.b1.double(), stride=2))

    @functools.cached_property
    def S1(self):
        return Fn.conv2d(self.x.double().abs(), self.w1.double().abs(), self.b1.double().abs(), stride=2)

    @memo
    def y1(self, dt):
        """The y1 every later kernel is given: the fp64 conv1 output rounded to dt, channels-last."""
        return cl(self.ref1).to(dt)

    @memo
    def w2r(self, dt):
        return self.w2.to(dt).double()

    @memo
    def dy2(self, dt):
        """conv2 output gradient rows [(b, t2, f2)][64] in dt."""
        return rows_of(self.gy).to(dt)

    def dy2_nchw(self, dt):
        return from_rows(self.dy2(dt).double(), self.B, self.F2, self.T2)

    @memo
    def ref2(self, dt):
        """conv2(y1(dt)) with dt-rounded weights, no bias: (value, scale)."""
        y = nchw(self.y1(dt).double())
        return Fn.conv2d(y, self.w2r(dt), stride=2), Fn.conv2d(y.abs(), self.w2r(dt).abs(), stride=2)

    @memo
    def dcols(self, dt):
        """The conv2 column gradient dy2 . W2 as the GEMM stores it: fp64 product of the dt operands, rounded to dt."""
        return (self.dy2(dt).double() @ w2_phys(self.w2r(dt))).to(dt)

    @memo
    def dy1(self, dd, yd):
        """col2im of dcols(dd) gated by y1(yd) > 0: (value, scale), both (B, 64, F1, T1) fp64."""
        gate = nchw(self.y1(yd) > 0)
        d = self.dcols(dd).double()
        return (fold_cols(d, self.B, self.F1, self.T1) * gate, fold_cols(d.abs(), self.B, self.F1, self.T1) * gate)

    @memo
    def conv1_grads(self, dd, yd):
        return conv1_wgrad(self.x, self.dy1(dd, yd)[0])

    @functools.cached_property
    def conv2_grads(self):
        return conv2_wgrad(nchw(self.y1(BF16).double()), self.dy2_nchw(BF16))

    @functools.cached_property
    def implicit_grads(self):
        """conv_bwd_implicit's two references (bf16 path): the conv1 gradients of dy1 = gate * conv2^T(dy2) with dy1
        and x rounded to bf16 (the kernel's MFMA operands), and the unrounded ones."""
        dy1 = conv2_dgrad(self.dy2_nchw(BF16), self.w2r(BF16), (self.B, 64, self.F1, self.T1))
        dy1 = dy1 * nchw(self.y1(BF16) > 0)
        rounded = conv1_wgrad(self.x.to(BF16), dy1.to(BF16))
        return rounded, conv1_wgrad(self.x, dy1)


@functools.lru_cache(maxsize=None)
def case(B, F, T):
    return Case(B, F, T)


class ExactCase:
    """Small non-negative integer y1 (given, conv1 bypassed), a sparse integer W2 with a different input channel per
    (tap, output channel), integer dy2 / dcols / x / dy1: every sum below is an exact integer well under 2^24 and
    every bf16 value at most 256, so each kernel must reproduce the integer result bit for bit."""
    B, F, T = 2, 14, 17   # F1 = 6 (dead trailing row), T1 = 8 (dead trailing column), F2 = 2, T2 = 3

    def __init__(self):
        B, F, T = self.B, self.F, self.T
        self.F1, self.T1, self.F2, self.T2 = dims(F, T)
        self.M = B * self.T2 * self.F2
        g = torch.Generator().manual_seed(11)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
        self.x = ri(-3, 3, B, 1, F, T)
        self.y1 = ri(0, 3, B, self.F1, self.T1, 64)              # channels-last; zeros are gated off
        w2 = torch.zeros(64, 64, 3, 3, dtype=torch.float64)
        for tap in range(9):
            for co in range(64):
                w2[co, (5 * co + 7 * tap + 3) % 64, tap // 3, tap % 3] = (1 + (co + tap) % 3) * (-1) ** (co + tap // 2)
        self.w2 = w2
        self.b2 = ri(-4, 4, 64)
        self.dy2 = ri(-3, 3, self.M, 64)
        self.dcols = ri(-4, 4, self.M, 576)
        self.dy1_in = ri(-8, 8, B, self.F1, self.T1, 64)         # conv1_bwd_w's input, channels-last
        self.dw2_0, self.db2_0 = ri(-9, 9, 64, 576), ri(-9, 9, 64)
        self.dw1_0, self.db1_0 = ri(-9, 9, 64, 9), ri(-9, 9, 64)
        y = nchw(self.y1)
        self.out = rows_of(torch.relu(Fn.conv2d(y, w2, self.b2, stride=2)))
        self.cols = rows_of_cols(y, self.F2, self.T2)
        gw, gb = conv2_wgrad(y, from_rows(self.dy2, B, self.F2, self.T2))
        self.dw2, self.db2 = self.dw2_0 + gw, self.db2_0 + gb
        self.dy1 = cl(fold_cols(self.dcols, B, self.F1, self.T1) * (y > 0))
        gw, gb = conv1_wgrad(self.x, nchw(self.dy1_in))
        self.dw1_w, self.db1_w = self.dw1_0 + gw, self.db1_0 + gb
        gw, gb = conv1_wgrad(self.x, nchw(self.dy1))
        self.dw1_f, self.db1_f = self.dw1_0 + gw, self.db1_0 + gb
        self.check_magnitudes()

    def check_magnitudes(self):
        """The references are integers; accumulators stay below 2^24 and everything stored as bf16 is at most 256."""
        for name in ("out", "cols", "dw2", "db2", "dy1", "dw1_w", "db1_w", "dw1_f", "db1_f"):
            v = getattr(self, name)
            assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 24, name
        # absolute-value bounds of the accumulators themselves (partial sums in any order)
        assert 9 * 3 * 3 + 4 <= 256 and float(self.out.max()) <= 256                       # conv2_fwd, bf16 output
        assert self.M * 3 * 3 < 2 ** 24 and self.B * self.F1 * self.T1 * 16 * 3 < 2 ** 24   # wgrad sums
        for name in ("x", "y1", "dy2", "dcols", "dy1_in"):
            assert float(getattr(self, name).abs().max()) <= 256, name
        assert float(self.w2.abs().max()) <= 3 and int((self.w2 != 0).sum()) == 9 * 64
        return True


def rows_of_cols(y_nchw, F2, T2):
    """im2col of conv2: (B, 64, F1, T1) -> [(b, t2, f2)][(kh, kw, c)]."""
    B = y_nchw.shape[0]
    u = Fn.unfold(y_nchw, 3, stride=2).view(B, 64, 3, 3, F2, T2)      # (b, c, kh, kw, f2, t2)
    return u.permute(0, 5, 4, 2, 3, 1).reshape(B * T2 * F2, 576).contiguous()


@functools.lru_cache(maxsize=None)
def exact_case():
    return ExactCase()


def implicit_fits(T):
    """The acceptance rule of asrx_conv_bwd_implicit written out independently: T1 <= 1024 and 48 KiB of weights +
    the row's sign bits (rounded up to 16 B) + three fp32 input lines within 80 KiB of LDS."""
    T1 = (T - 3) // 2 + 1
    return T1 <= 1024 and 6 * 64 * 64 * 2 + (T1 * 8 + 15) // 16 * 16 + 12 * T <= 80 * 1024
