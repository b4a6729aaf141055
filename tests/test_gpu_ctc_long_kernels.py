"""asrx_ctc_loss_long on the GPU against tests/ctc_ref.py: targets of up to 4095 labels, a workgroup of NW =
ceil((Lmax + 1) / 256) waves per sample.

Reference, tolerances and the printed worst ratios are those of tests/test_gpu_ctc_kernels.py, whose Case / check are
used as they stand: torch's CPU fp64 path is the reference, and the kernel gets 4x the error of torch's own fp32 path
on the quantity compared, floors of 1e-6, plus 2^-8 |g| for a bf16 gradient.  DESIGN §20 records the ratios.

Shapes: every wave-seam edge of the pair row (L + 1 = 256 pairs fill one wave, 257 need a second, ... 4096 fill
sixteen); equal labels on both sides of a seam at the only feasible length and one frame short; waves that own no
live pair (short samples under a long bound); long runs of one label in the ordered occupancy sum; malformed labels
beyond the first wave."""
import functools

import pytest
import torch

from tests.test_gpu_ctc_kernels import Case, check, launch as launch_short, rand_targets, randn_case

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def launch(case, ld=None, reduction="mean", dtype=torch.float32, grad_scale=1.0, zero_infinity=False, loss_add=None,
           loss_add_scale=0.0, loss_scale=1.0, max_target_len=None, tgt_stride=None):
    """One asrx_ctc_loss_long call on buffers this test owns: logits rows of stride ld whose padding is NaN, outputs and
    workspace pre-filled with NaN.  Returns (loss, nll, dlogits [B*T, ld]) on the host."""
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
    n = K.ctc_workspace_elems(B, T, mtl, long=True)
    ws = torch.full((n,), float("nan"), device=dev)
    la = None if loss_add is None else torch.tensor([loss_add], dtype=torch.float32, device=dev)
    call("asrx_ctc_loss_long", x.data_ptr(), B, T, V, ld, tg.data_ptr(), width, None if il is None else il.data_ptr(),
         tl.data_ptr(), mtl, case.blank, K.CTC_REDUCTIONS[reduction], int(zero_infinity), grad_scale, nll.data_ptr(),
         loss.data_ptr(), dl.data_ptr(), K.code(dl), None if la is None else la.data_ptr(), loss_add_scale, loss_scale,
         ws.data_ptr(), n, K.stream())
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), dl.cpu()


def same_bits(a, b):
    for x, y in zip(a, b):
        if not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16),
                           y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16)):
            return False
    return True


# ---------------------------------------------------------------------------------------------- seam edges

@functools.lru_cache(maxsize=None)
def edge_case(L):
    """edge_case of tests/test_gpu_ctc_kernels.py, extended: two samples, L and L // 2 labels, V = 250; T = the frames
    the repeats need + 2."""
    return randn_case(2, None, 250, [L, L // 2], seed=1000 + L)


@pytest.mark.parametrize("L", [255, 256, 257, 511, 512, 767, 1023, 1024, 2047, 4095])
def test_wave_seam_edges(L):
    """L + 1 pairs fill 1, 2, 3, 4, 8 and 16 waves exactly, one short, or one over.  max_target_len = L picks NW; at
    255 the long entry runs as one wave (NW = 1).  ld = 256 (V = 250)."""
    c = edge_case(L)
    check(c, launch(c, ld=256), f"long/edge/L{L}", ld=256)


def test_both_kernels_lie_within_the_reference_bounds_on_a_short_case():
    """L = 255 is inside both kernels' range: each lies within the bounds (no bit equality is asked)."""
    c = edge_case(255)
    check(c, launch_short(c, ld=256), "short-kernel/edge/L255", ld=256)
    check(c, launch(c, ld=256), "long-kernel/edge/L255", ld=256)
    check(c, launch(c, ld=256, max_target_len=700, tgt_stride=704), "long-kernel/edge/L255/bound700", ld=256)


# ---------------------------------------------------------------------------------------------- repeats across a seam

def _seam_repeat_case(at, short):
    """Sample 0: L = at + 45 labels without adjacent repeats except target[at - 1] == target[at], whose pairs sit in
    different waves (at = 256, 512): exactly L + 1 frames align.  Sample 1 (20 labels) aligns at either length."""
    V, L = 20, at + 45
    g = torch.Generator().manual_seed(at)
    lab = torch.randint(1, V, (L,), generator=g)
    for u in range(1, L):
        while lab[u] == lab[u - 1]:
            lab[u] = 1 + (int(lab[u]) % (V - 1))
    lab[at] = lab[at - 1]
    while lab[at + 1] == lab[at]:
        lab[at + 1] = 1 + (int(lab[at + 1]) % (V - 1))
    assert int((lab[1:] == lab[:-1]).sum()) == 1 and lab[at - 1] == lab[at]
    other, _ = rand_targets([20], V, 0, g, width=L)
    tg = torch.cat([lab.view(1, L), other])
    T = L + 1 - (1 if short else 0)
    return Case(torch.randn(2, T, V, generator=g), tg, [L, 20], 0, infeasible=(0,) if short else ())


@pytest.mark.parametrize("at", [256, 512])
def test_equal_labels_across_a_seam(at):
    """target[255] == target[256] and target[511] == target[512]: the skip flag of the seam pair is read from the
    targets.  At the only feasible T the sample aligns; one frame short it gives +inf, zero rows with zero_infinity, and
    the other sample is what it is."""
    c = _seam_repeat_case(at, short=False)
    check(c, launch(c), f"long/seam-repeat{at}/feasible")
    c = _seam_repeat_case(at, short=True)
    check(c, launch(c, zero_infinity=True), f"long/seam-repeat{at}/short/zi", zero_infinity=True)
    out = launch(c, reduction="sum", zero_infinity=False)
    check(c, out, f"long/seam-repeat{at}/short", reduction="sum", zero_infinity=False)
    assert bool(torch.isnan(out[2].view(2, c.T, c.V)[0]).all())     # NaN rows, as torch's


# ---------------------------------------------------------------------------------------------- idle waves

@functools.lru_cache(maxsize=None)
def idle_case(with_lengths):
    """Ls = [0, 3, 300, 700]: under the bound 700 (NW = 3) samples 0 and 1 leave two waves without a live pair, sample
    2 one.  with_lengths: input lengths below T, one of them 0.  torch's ctc_loss reads frame 0 and frame T_b - 1
    whatever T_b is, so the reference of the T_b = 0 sample (an empty target: nll 0, zero rows) is written down."""
    g = torch.Generator().manual_seed(4321)
    Ls = [0, 3, 300, 700]
    tg, need = rand_targets(Ls, 12, 0, g)
    T = need + 2
    logits = torch.randn(4, T, 12, generator=g)
    if not with_lengths:
        return Case(logits, tg, Ls, 0)
    il = [0, 40, T - 60, T - 1]
    sub = Case(logits[1:], tg[1:], Ls[1:], 0, input_lengths=il[1:])
    c = Case.__new__(Case)
    c.logits, c.targets, c.blank = logits, tg, 0
    c.B, c.T, c.V = logits.shape
    c.tl = torch.tensor(Ls, dtype=torch.int32)
    c.il = torch.tensor(il, dtype=torch.int32)
    zero = torch.zeros(1, dtype=sub.nll64.dtype)
    c.nll64, c.nll32 = torch.cat([zero, sub.nll64]), torch.cat([zero.to(sub.nll32.dtype), sub.nll32])
    c.g64 = torch.cat([torch.zeros_like(sub.g64[:1]), sub.g64])
    c.g32 = torch.cat([torch.zeros_like(sub.g32[:1]), sub.g32])
    c.infeasible = set()
    return c


@pytest.mark.parametrize("with_lengths", [False, True])
def test_waves_without_a_live_pair(with_lengths):
    """Every wave of a workgroup runs the sample's T_b frames, whether or not it owns a pair; a wider bound (NW = 16)
    and a wider target row change the layout, not the result."""
    c = idle_case(with_lengths)
    check(c, launch(c), f"long/idle/il{int(with_lengths)}")
    check(c, launch(c, max_target_len=4095, tgt_stride=4095), f"long/idle/il{int(with_lengths)}/bound4095")
    check(c, launch(c, ld=16, dtype=torch.bfloat16, reduction="sum"), f"long/idle/il{int(with_lengths)}/bf16", ld=16,
          dtype=torch.bfloat16, reduction="sum")


# ---------------------------------------------------------------------------------------------- runs, vocabularies

@functools.lru_cache(maxsize=None)
def mid_case(V):
    """600 and 40 labels; at V = 5 every one of the four labels occurs about 150 times: the gradient's run sums."""
    return randn_case(2, None, V, [600, 40], seed=2000 + V)


@pytest.mark.parametrize("V,ld", [(5, 5), (5, 8), (257, 320), (257, 257)])
def test_long_label_runs_vocabularies_and_padded_columns(V, ld):
    c = mid_case(V)
    check(c, launch(c, ld=ld), f"long/V{V}/ld{ld}", ld=ld)
    check(c, launch(c, ld=ld, dtype=torch.bfloat16), f"long/V{V}/ld{ld}/bf16", ld=ld, dtype=torch.bfloat16)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_reductions_dtypes_scale_and_loss_add(reduction):
    c = mid_case(5)
    for dtype in (torch.float32, torch.bfloat16):
        kw = dict(ld=8, reduction=reduction, dtype=dtype)
        check(c, launch(c, **kw), f"long/mid/{reduction}/{dtype}", **kw)
        kw.update(grad_scale=0.3)
        check(c, launch(c, **kw), f"long/mid/{reduction}/{dtype}/gs", **kw)
        kw.update(loss_add=2.5, loss_add_scale=0.7, loss_scale=0.3)
        check(c, launch(c, **kw), f"long/mid/{reduction}/{dtype}/add", **kw)


# ---------------------------------------------------------------------------------------------- malformed, repeats

def test_malformed_labels_beyond_the_first_wave_touch_nothing_else():
    """A blank id at position 300, an id >= V at position 600, a length above the bound: each such sample is
    infeasible (+inf; zero rows with zero_infinity) and the good one is unchanged."""
    from asrx import kernels as K
    V, L = 20, 650
    g = torch.Generator().manual_seed(99)
    good, need = rand_targets([L], V, 0, g)
    T = need + 2
    logits = torch.randn(4, T, V, generator=g)
    ref = Case(logits[:1], good, [L], 0)
    tg = good.repeat(4, 1)
    tg[1, 300] = 0
    tg[2, 600] = V
    tl = torch.tensor([L, L, L, L + 5], dtype=torch.int32, device=dev)
    x = logits.reshape(4 * T, V).to(dev)
    loss, nll, dl = K.ctc_loss(x, V, T, tg.to(dev), tl, max_target_len=L, blank=0, reduction="sum", zero_infinity=True,
                               grad_dtype=torch.float32, long=True)
    torch.cuda.synchronize()
    nll, dl = nll.cpu(), dl.cpu().view(4, T, V)
    assert nll[1:].tolist() == [INF] * 3
    assert torch.equal(dl[1:], torch.zeros_like(dl[1:]))
    tol = max(4 * abs(float(ref.nll32[0] - ref.nll64[0])), 1e-6 * float(ref.nll64[0]))
    assert abs(float(nll[0]) - float(ref.nll64[0])) <= tol
    assert abs(float(loss) - float(ref.nll64[0])) <= tol
    assert float((dl[0].double() - ref.g64[0]).abs().max()) <= max(4 * float((ref.g32 - ref.g64).abs().max()), 1e-6)
    with pytest.raises(RuntimeError, match="unsupported"):
        K.ctc_loss(x, V, T, torch.zeros(4, 4096, dtype=torch.int64, device=dev), tl, long=True)


@pytest.mark.parametrize("which", ["edge256", "edge1024", "idle", "mid"])
def test_two_calls_are_bit_identical(which):
    c, ld = {"idle": (idle_case(True), 12), "mid": (mid_case(5), 8)}.get(which) or (edge_case(int(which[4:])), 256)
    for dtype in (torch.float32, torch.bfloat16):
        assert same_bits(launch(c, ld=ld, dtype=dtype), launch(c, ld=ld, dtype=dtype))
