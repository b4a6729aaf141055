"""asrx_ctc_loss / asrx_ctc_targets / asrx_ctc_greedy and asrx.CTCLoss on the GPU against tests/ctc_ref.py.

Reference: torch's CPU log_softmax + ctc_loss in fp64 with autograd.  Tolerances come from the reference itself: every
case also runs the same torch path in fp32 and measures its error against fp64 on the very quantity compared (the
weighted gradient, the per-sample nll); the kernel gets 4x that error (its summation order differs from torch's), with
a floor of 1e-6 absolute for gradients and 1e-6 relative for nll.  A bf16 gradient gets the fp32 bound plus 2^-8 |g|
(one bf16 rounding).  Each case prints its worst ratio (kernel error / bound); DESIGN §9 records them.

Shapes are the smallest at which the kernel can go wrong: T = 1; empty and one-label targets; repeats at the only
feasible length and one frame short; every lane-layout edge of the state row (L + 1 = 32 .. 256 pairs over 64 lanes x
1..4 pairs); vector and element-wise rows (ld % 4); padded columns (filled with NaN in the logits: only [0, V) may be
read)."""
import functools

import pytest
import torch

from tests import ctc_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rand_targets(Ls, V, blank, g, width=None):
    """Random labels != blank, (B, width) padded with blank; also the frames the longest-needing sample needs."""
    width = max(1, max(Ls)) if width is None else width
    tg = torch.full((len(Ls), width), blank, dtype=torch.int64)
    need = 1
    for b, L in enumerate(Ls):
        lab = torch.randint(0, V - 1, (L,), generator=g)
        lab = lab + (lab >= blank).long()
        tg[b, :L] = lab
        need = max(need, L + int((lab[1:] == lab[:-1]).sum()) if L else 1)
    return tg, need


class Case:
    """Inputs on the host plus the fp64 reference and torch's own fp32 error, computed once."""

    def __init__(self, logits, targets, Ls, blank, input_lengths=None, infeasible=()):
        self.logits, self.targets, self.blank = logits, targets, blank
        self.B, self.T, self.V = logits.shape
        self.tl = torch.tensor(Ls, dtype=torch.int32)
        self.il = None if input_lengths is None else torch.tensor(input_lengths, dtype=torch.int32)
        self.nll64, self.g64 = ctc_ref.ctc_reference(logits, targets, self.il, self.tl, blank, torch.float64)
        self.nll32, self.g32 = ctc_ref.ctc_reference(logits, targets, self.il, self.tl, blank, torch.float32)
        # the condition on the inputs: every sample has an alignment, except the stated ones
        for b in range(self.B):
            assert bool(torch.isinf(self.nll64[b])) == (b in infeasible), (b, float(self.nll64[b]))
        self.infeasible = set(infeasible)


def launch(case, ld=None, reduction="mean", dtype=torch.float32, grad_scale=1.0, zero_infinity=False, loss_add=None,
           loss_add_scale=0.0, loss_scale=1.0, max_target_len=None, tgt_stride=None):
    """One asrx_ctc_loss call on buffers this test owns: logits rows of stride ld whose padding is NaN, outputs
    pre-filled with NaN.  Returns (loss, nll, dlogits [B*T, ld]) on the host."""
    from asrx import kernels as K
    from asrx._lib import call
    B, T, V = case.B, case.T, case.V
    ld = V if ld is None else ld
    x = torch.full((B * T, ld), float("nan"), dtype=torch.float32)
    x[:, :V] = case.logits.reshape(B * T, V).float()
    x = x.to(dev)
    width = case.targets.shape[1] if tgt_stride is None else tgt_stride
    tg = torch.full((B, width), case.blank, dtype=torch.int64)
    tg[:, :case.targets.shape[1]] = case.targets
    tg = tg.to(dev)
    mtl = case.targets.shape[1] if max_target_len is None else max_target_len
    tl = case.tl.to(dev)
    il = None if case.il is None else case.il.to(dev)
    nll = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    dl = torch.full((B * T, ld), float("nan"), device=dev, dtype=dtype)
    n = K.ctc_workspace_elems(B, T, mtl)
    ws = torch.full((n,), float("nan"), device=dev)
    la = None if loss_add is None else torch.tensor([loss_add], dtype=torch.float32, device=dev)
    call("asrx_ctc_loss", x.data_ptr(), B, T, V, ld, tg.data_ptr(), width, None if il is None else il.data_ptr(),
         tl.data_ptr(), mtl, case.blank, K.CTC_REDUCTIONS[reduction], int(zero_infinity), grad_scale, nll.data_ptr(),
         loss.data_ptr(), dl.data_ptr(), K.code(dl), None if la is None else la.data_ptr(), loss_add_scale, loss_scale,
         ws.data_ptr(), n, K.stream())
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), dl.cpu()


def check(case, out, label, ld=None, reduction="mean", dtype=torch.float32, grad_scale=1.0, zero_infinity=False,
          loss_add=None, loss_add_scale=0.0, loss_scale=1.0):
    """Compare one launch with the reference under the derived bounds; returns the worst ratios."""
    loss, nll, dl = out
    B, T, V = case.B, case.T, case.V
    ld = V if ld is None else ld
    feas = [b for b in range(B) if b not in case.infeasible]
    # nll: 4x torch's fp32 relative error, floor 1e-6 relative
    r_nll = 0.0
    for b in range(B):
        if b in case.infeasible:
            assert float(nll[b]) == INF, (label, b, float(nll[b]))
            continue
        ref = float(case.nll64[b])
        tol = max(4 * abs(float(case.nll32[b]) - ref), 1e-6 * abs(ref))
        err = abs(float(nll[b]) - ref)
        print(f"{label}: nll[{b}] {float(nll[b]):.9g} ref {ref:.9g} err {err:.3g} tol {tol:.3g}")
        assert err <= tol, (label, b, float(nll[b]), ref, err, tol)
        r_nll = max(r_nll, err / tol if tol > 0 else 0.0)
    # gradient: the weighted quantity the kernel writes
    w = ctc_ref.sample_weights(case.tl, B, reduction) * grad_scale
    g64 = case.g64 * w.view(B, 1, 1)
    g32 = case.g32.double() * w.view(B, 1, 1)
    tol_g = max(4 * float((g32 - g64).abs().max()), 1e-6)
    g = dl.view(B, T, ld).double()
    assert torch.equal(g[:, :, V:], torch.zeros_like(g[:, :, V:])), (label, "padded columns must be written as zero")
    r_g = 0.0
    for b in range(B):
        gb = g[b, :, :V]
        if b in case.infeasible:
            if zero_infinity:
                assert torch.equal(gb, torch.zeros_like(gb)), (label, b, "gradient rows of an infeasible sample")
            continue
        if case.il is not None:
            tail = gb[int(case.il[b]):]
            assert torch.equal(tail, torch.zeros_like(tail)), (label, b, "rows past the input length")
        bound = tol_g + (2.0 ** -8 * g64[b].abs() if dtype == torch.bfloat16 else 0.0)
        ratio = float(((gb - g64[b]).abs() / bound).max())
        assert ratio <= 1.0, (label, b, ratio, tol_g, float((gb - g64[b]).abs().max()))
        r_g = max(r_g, ratio)
    # loss
    terms = case.nll64 * ctc_ref.sample_weights(case.tl, B, reduction)
    if zero_infinity or not case.infeasible:
        ctc = float(terms[feas].sum()) if feas else 0.0
        want = loss_scale * ctc + (loss_add_scale * loss_add if loss_add is not None else 0.0)
        mag = abs(loss_scale * ctc) + (abs(loss_add_scale * loss_add) if loss_add is not None else 0.0)
        rel = max([4 * abs(float(case.nll32[b]) - float(case.nll64[b])) / abs(float(case.nll64[b])) for b in feas
                   if float(case.nll64[b]) != 0.0] + [1e-6])
        assert abs(float(loss) - want) <= rel * mag + 1e-7 * mag + 1e-30, (label, float(loss), want)
    else:
        assert float(loss) == INF, (label, float(loss))
    print(f"{label}: worst ratio nll {r_nll:.3f} grad {r_g:.3f} (grad bound {tol_g:.3g})")
    return r_nll, r_g


def randn_case(B, T, V, Ls, blank=0, seed=0, scale=1.0, input_lengths=None, extra=2):
    g = torch.Generator().manual_seed(seed)
    tg, need = rand_targets(Ls, V, blank, g)
    T = need + extra if T is None else T
    return Case(torch.randn(B, T, V, generator=g) * scale, tg, Ls, blank, input_lengths)


# ---------------------------------------------------------------------------------------------- the loss kernel

@functools.lru_cache(maxsize=None)
def small_case(name):
    if name == "T1":             # one frame: the empty target and one-label targets are the only feasible ones
        return randn_case(3, 1, 5, [0, 1, 1], seed=1)
    if name == "L0":             # all-blank path only
        return randn_case(2, 4, 5, [0, 0], seed=2)
    if name == "L1":
        return randn_case(2, 3, 5, [1, 1], seed=3)
    if name == "mixed":          # empty, short and longer targets in one batch
        return randn_case(4, 30, 20, [0, 3, 8, 12], seed=4)
    raise KeyError(name)


@pytest.mark.parametrize("name,ld", [("T1", 5), ("L0", 5), ("L1", 5), ("L1", 8), ("mixed", 20), ("mixed", 24),
                                     ("mixed", 21)])
def test_small_shapes(name, ld):
    """ld = V unaligned (element accesses), ld % 4 == 0 (16-B accesses) and ld = 21 (padded and unaligned)."""
    c = small_case(name)
    check(c, launch(c, ld=ld), f"{name}/ld{ld}", ld=ld)


def _repeat_case(T):
    """Sample 0: a a b b b (3 repeats: exactly L + 3 = 8 frames align, one way per blank placement); sample 1 has an
    alignment at either length."""
    g = torch.Generator().manual_seed(50 + T)
    tg = torch.tensor([[2, 2, 3, 3, 3], [1, 2, 3, 0, 0]], dtype=torch.int64)
    return Case(torch.randn(2, T, 6, generator=g), tg, [5, 3], 0, infeasible=(0,) if T < 8 else ())


def test_repeats_at_the_only_feasible_length():
    c = _repeat_case(8)
    check(c, launch(c), "repeat/T8")
    check(c, launch(c, reduction="sum", dtype=torch.bfloat16), "repeat/T8/sum/bf16", reduction="sum",
          dtype=torch.bfloat16)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_one_frame_short_is_infeasible(reduction):
    """nll = +inf; with zero_infinity the sample adds 0 to the loss, its gradient rows are exactly 0 and the other
    sample is what it is alone; without, the loss is +inf and the other sample's rows are still right."""
    c = _repeat_case(7)
    check(c, launch(c, reduction=reduction, zero_infinity=True), f"short/{reduction}/zi", reduction=reduction,
          zero_infinity=True)
    out = launch(c, reduction=reduction, zero_infinity=False)
    check(c, out, f"short/{reduction}", reduction=reduction, zero_infinity=False)
    assert bool(torch.isnan(out[2].view(2, 7, 6)[0]).all())     # documented: NaN rows, as torch's


def test_malformed_samples_have_no_alignment_and_touch_nothing_else():
    """What the host cannot see: a label equal to blank, outside [0, V), negative, and a length beyond
    max_target_len.  Each such sample is infeasible (+inf; zero rows with zero_infinity); the good one is unchanged."""
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(5, 9, 6, generator=g)
    good = torch.tensor([1, 2, 3, 0], dtype=torch.int64)
    ref = Case(logits[:1], good.view(1, 4), [3], 0)
    tg = torch.stack([good, torch.tensor([1, 0, 3, 0]), torch.tensor([1, 6, 3, 0]), torch.tensor([1, -5, 3, 0]),
                      good])
    from asrx import kernels as K
    x = logits.reshape(45, 6).to(dev)
    tl = torch.tensor([3, 3, 3, 3, 9], dtype=torch.int32, device=dev)
    loss, nll, dl = K.ctc_loss(x, 6, 9, tg.to(dev), tl, max_target_len=4, blank=0, reduction="sum",
                               zero_infinity=True, grad_dtype=torch.float32)
    torch.cuda.synchronize()
    nll, dl = nll.cpu(), dl.cpu().view(5, 9, 6)
    assert nll[1:].tolist() == [INF] * 4
    assert torch.equal(dl[1:], torch.zeros_like(dl[1:]))
    tol = max(4 * abs(float(ref.nll32[0] - ref.nll64[0])), 1e-6 * float(ref.nll64[0]))
    assert abs(float(nll[0]) - float(ref.nll64[0])) <= tol
    assert abs(float(loss) - float(ref.nll64[0])) <= tol
    assert float((dl[0].double() - ref.g64[0]).abs().max()) <= max(4 * float((ref.g32 - ref.g64).abs().max()), 1e-6)


def test_input_lengths_shorter_than_T():
    c = randn_case(3, 12, 9, [4, 3, 0], seed=6, input_lengths=[12, 7, 5])
    check(c, launch(c, ld=12), "input_lengths", ld=12)
    check(c, launch(c, ld=12, dtype=torch.bfloat16, reduction="sum"), "input_lengths/bf16", ld=12, dtype=torch.bfloat16,
          reduction="sum")


@functools.lru_cache(maxsize=None)
def edge_case(L):
    """Two samples, L and L // 2 labels, V = 250; T = the frames the repeats need + 2."""
    return randn_case(2, None, 250, [L, L // 2], seed=1000 + L)


@pytest.mark.parametrize("L", [31, 32, 33, 63, 64, 95, 127, 128, 255])
def test_state_row_lane_layout_edges(L):
    """S = 2L + 1 = 63 .. 511 extended states: L + 1 pairs fill 64 lanes x 1, 2, 3, 4 pairs exactly, one short, one
    over.  max_target_len = L picks the kernel; ld = 256 (V = 250)."""
    c = edge_case(L)
    check(c, launch(c, ld=256), f"edge/L{L}", ld=256)


def test_max_target_len_above_the_lengths():
    """A wider bound (more pairs per lane, a wider target row) changes the layout, not the result."""
    c = edge_case(33)
    for mtl in (64, 130, 255):
        check(c, launch(c, ld=256, max_target_len=mtl, tgt_stride=260), f"edge/L33/bound{mtl}", ld=256)


@pytest.mark.parametrize("V,ld", [(5, 5), (5, 8), (250, 256), (257, 320), (257, 257)])
def test_vocabulary_sizes_and_padded_columns(V, ld):
    c = randn_case(2, 12, V, [5, 2], seed=V)
    check(c, launch(c, ld=ld), f"V{V}/ld{ld}", ld=ld)
    check(c, launch(c, ld=ld, dtype=torch.bfloat16), f"V{V}/ld{ld}/bf16", ld=ld, dtype=torch.bfloat16)


@pytest.mark.parametrize("blank", [0, 3, 6])
def test_blank_first_middle_last(blank):
    c = randn_case(3, 10, 7, [4, 0, 6], blank=blank, seed=20 + blank)
    check(c, launch(c), f"blank{blank}")


@pytest.mark.parametrize("L", [40, 130])
def test_one_label_fills_the_target(L):
    """The longest run of the ordered occupancy sum: every position carries the same label (T = 2L - 1 + 2)."""
    g = torch.Generator().manual_seed(L)
    tg = torch.full((1, L), 7, dtype=torch.int64)
    c = Case(torch.randn(1, 2 * L + 1, 12, generator=g), tg, [L], 0)
    out = launch(c)
    check(c, out, f"onelabel/L{L}")
    out2 = launch(c)
    assert torch.equal(out[2], out2[2])


def test_peaked_logits():
    """randn x 30: nll in the thousands, exp(x) overflows without the row maximum."""
    c = randn_case(2, 100, 250, [20, 7], seed=30, scale=30.0)
    assert float(c.nll64.min()) > 1e3
    check(c, launch(c, ld=256), "peaked", ld=256)
    check(c, launch(c, ld=256, dtype=torch.bfloat16, reduction="sum"), "peaked/bf16", ld=256, dtype=torch.bfloat16,
          reduction="sum")


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reductions_dtypes_scale_and_loss_add(reduction, dtype):
    c = small_case("mixed")
    kw = dict(ld=24, reduction=reduction, dtype=dtype)
    check(c, launch(c, **kw), f"mixed/{reduction}/{dtype}", **kw)
    kw.update(grad_scale=0.3)
    check(c, launch(c, **kw), f"mixed/{reduction}/{dtype}/gs", **kw)
    kw.update(loss_add=2.5, loss_add_scale=0.7, loss_scale=0.3)
    check(c, launch(c, **kw), f"mixed/{reduction}/{dtype}/add", **kw)


@pytest.mark.parametrize("which", ["edge64", "edge255", "mixed"])
def test_two_calls_are_bit_identical(which):
    c, ld = (small_case("mixed"), 24) if which == "mixed" else (edge_case(int(which[4:])), 256)
    for dtype in (torch.float32, torch.bfloat16):
        a = launch(c, ld=ld, dtype=dtype)
        b = launch(c, ld=ld, dtype=dtype)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16),
                               y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16))


# ---------------------------------------------------------------------------------------------- targets, best path

def test_ctc_targets_against_the_python_loop():
    from asrx import kernels as K
    g = torch.Generator().manual_seed(8)
    for B, n in ((6, 9), (3, 65), (3, 130), (5, 1)):
        text = torch.randint(0, 12, (B, n), generator=g)
        mask = (torch.rand(B, n, generator=g) > 0.2).float()
        if n >= 9:
            text[0] = 4                                     # nothing kept: all PAD
            text[1, 0], text[1, 1:] = 1, torch.randint(5, 12, (n - 1,), generator=g)   # no EOS, kept to the end
            mask[1] = 1.0
            text[2, :3] = torch.tensor([1, 2, 4])           # BOS EOS PAD ... then more
        for drop in ((1, 2, 4), (1, 2, 4, 0), (), (7,)):
            want_t, want_l = ctc_ref.targets_loop(text, mask, drop, 4)
            got_t, got_l = K.ctc_targets(text.to(dev), mask.to(dev), list(drop), 4)
            assert torch.equal(got_t.cpu(), want_t) and torch.equal(got_l.cpu(), want_l), (B, n, drop)
    # a strided view of a wider token matrix (row stride > n)
    wide = torch.randint(0, 12, (4, 20), generator=g).to(dev)
    wmask = torch.ones(4, 20, device=dev)
    got_t, got_l = K.ctc_targets(wide[:, :11], wmask[:, :11], [1, 2, 4], 4)
    want_t, want_l = ctc_ref.targets_loop(wide[:, :11].cpu(), wmask[:, :11].cpu(), (1, 2, 4), 4)
    assert torch.equal(got_t.cpu(), want_t) and torch.equal(got_l.cpu(), want_l)


def test_ctc_greedy_against_the_python_collapse():
    from asrx import kernels as K
    g = torch.Generator().manual_seed(12)
    for B, T, V, ld, blank in ((3, 7, 5, 5, 0), (2, 70, 250, 256, 4), (4, 130, 9, 12, 8), (1, 1, 3, 3, 1)):
        x = torch.randn(B, T, V, generator=g)
        # ties (first index wins), a repeat separated by a blank, an all-blank row
        x[0] = torch.round(x[0])
        if T >= 7:
            x[0, :5] = -5.0
            for t, s in enumerate([1, 1, blank, 1, 2] if blank != 1 else [0, 0, blank, 0, 2]):
                x[0, t, s] = 5.0
        if B > 1:
            x[1] = 0.0
            x[1, :, blank] = 1.0
        buf = torch.full((B * T, ld), float("nan"))
        buf[:, :V] = x.reshape(B * T, V)
        for il in (None, torch.randint(0, T + 1, (B,), generator=g).int()):
            tok, n = K.ctc_greedy(buf.to(dev), V, T, blank, None if il is None else il.to(dev))
            want_tok, want_n = ctc_ref.greedy_loop(x, blank, il)
            assert torch.equal(n.cpu(), want_n), (B, T, V, il)
            assert torch.equal(tok.cpu(), want_tok), (B, T, V, il)
    # an exact tie between two columns: the first index, and it collapses with its neighbour
    x = torch.zeros(1, 3, 4)
    x[0, :, 2] = 1.0
    x[0, :, 3] = 1.0
    tok, n = K.ctc_greedy(x.reshape(3, 4).to(dev), 4, 3, 0)
    assert tok.cpu().tolist() == [[2, 0, 0]] and n.cpu().tolist() == [1]


# ---------------------------------------------------------------------------------------------- the module

@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_ctc_loss_module_autograd(reduction):
    """asrx.CTCLoss through torch.autograd.grad against the reference with the same upstream gradient."""
    import asrx
    c = small_case("mixed")
    B, T, V = c.B, c.T, c.V
    x = c.logits.float().to(dev).requires_grad_(True)
    crit = asrx.CTCLoss(blank=0, reduction=reduction)
    out = crit(x, c.targets.to(dev), None, c.tl.to(dev))
    up = torch.linspace(0.5, 2.0, B, dtype=torch.float64) if reduction == "none" else torch.tensor(1.7).double()
    (g,) = torch.autograd.grad(out, x, up.float().to(dev))
    w = ctc_ref.sample_weights(c.tl, B, "sum" if reduction == "none" else reduction)
    want_out = c.nll64 if reduction == "none" else (c.nll64 * w).sum()
    rel = max(4 * float(((c.nll32 - c.nll64).abs() / c.nll64.abs()).max()), 1e-6)
    assert float(((out.detach().cpu().double() - want_out).abs() / want_out.abs()).max()) <= rel + 2e-7
    wg = c.g64 * (w * up).view(-1, 1, 1) if reduction == "none" else c.g64 * w.view(-1, 1, 1) * up
    wg32 = c.g32.double() * ((w * up).view(-1, 1, 1) if reduction == "none" else w.view(-1, 1, 1) * up)
    tol = max(4 * float((wg32 - wg).abs().max()), 1e-6)
    assert float((g.cpu().double() - wg).abs().max()) <= tol + 1e-7 * float(wg.abs().max())
    # input lengths and zero_infinity pass through; integer lengths of any dtype are taken
    crit = asrx.CTCLoss(blank=0, reduction="sum", zero_infinity=True)
    il = torch.tensor([30, 20, 30, 5])                       # sample 3: 12 labels in 5 frames
    out = crit(x, c.targets.to(dev), il.to(dev), c.tl.long().to(dev))
    nll, _ = ctc_ref.ctc_reference(c.logits, c.targets, il, c.tl, 0)
    nll32, _ = ctc_ref.ctc_reference(c.logits, c.targets, il, c.tl, 0, torch.float32)
    assert torch.isinf(nll[3]) and torch.isfinite(nll[:3]).all()
    want = float(nll[:3].sum())
    assert abs(float(out.detach()) - want) <= max(4 * float((nll32[:3].double() - nll[:3]).abs().sum()), 1e-6 * want)
