"""asrx_cross_entropy_ls on the GPU (csrc/xent.hip) against the fp64 formulas of tests/xent_ref.py: every register
template, the scalar path, the streamed rows, label smoothing, both gradient dtypes, ties, ignored rows, statistics.

Tolerances are those of the existing cross-entropy test (test_gpu_kernels.py, _ce_check): loss 1e-5 relative, bf16
dlogits 1e-2 of grad_scale x the fp64 gradient; fp32 dlogits and stats[0] 1e-5; argmax and stats[1] exact."""
import pytest
import torch

from tests import xent_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
B16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# (V, ld): smallest; small padded; the old limit; the first shape the old kernel refuses; unaligned rows (scalar path);
# the 4-float4 template's last row and the first past it; a BPE vocabulary; the last register-resident row; the first
# streamed row; a streamed row of 40 chunks (rows <= 5 only)
SIZES = [(2, 2), (250, 256), (1000, 1024), (1025, 1088), (1031, 1031), (4096, 4096), (4097, 4160), (5000, 5056),
         (16384, 16384), (16385, 16448), (40000, 40000)]


def _tied_logits(rows, V, ld):
    """Logits on a grid of 0.5 with planted ties of the row maximum: row 0 at columns V // 3 and V - 1 (other lanes,
    waves, register rounds or stream chunks), row 1 at two adjacent columns (one thread's float4, or neighbouring
    lanes); the padded copy [rows, ld] has +inf in columns [V, ld): a kernel that reads one fails loudly."""
    g = torch.Generator().manual_seed(V + 3 * rows)
    x = (torch.randn(rows, V, generator=g) * 6).round() / 2
    x[0, V // 3] = x[0, V - 1] = x[0].max() + 0.5
    if rows > 1 and V > 2:
        a = V // 2
        x[1, a] = x[1, a + 1] = x[1].max() + 0.5
        assert int(x[1].argmax()) == a
    assert int(x[0].argmax()) == V // 3
    full = torch.full((rows, ld), float("inf"))
    full[:, :V] = x
    return x, full


def _targets(rows, V):
    g = torch.Generator().manual_seed(V + rows)
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[0] = 0
    tgt[-1] = V - 1
    if rows > 2:
        tgt[1] = V - 1
    return tgt


def _check(x, fulld, V, tgt, ignore_index, eps, grad_scale, grad_dtype, ref=None, want_grad=True, want_argmax=True):
    """One call against the reference (computed at grad_scale 1: the gradient is linear in it)."""
    rows, ld = fulld.shape
    ref = ref if ref is not None else R.cross_entropy(x, tgt, ignore_index=ignore_index, eps=eps)
    loss, dl, am, stats = K().cross_entropy(fulld, V, tgt.to(dev), ignore_index=ignore_index, grad_scale=grad_scale,
                                            want_grad=want_grad, want_argmax=want_argmax, label_smoothing=eps,
                                            grad_dtype=grad_dtype, want_stats=True)
    loss, stats = float(loss), stats.cpu()
    print(f"V {V} ld {ld} rows {rows} eps {eps} gs {grad_scale} {grad_dtype}: loss {loss:.7f} "
          f"ref {float(ref.loss):.7f}")
    if want_argmax:
        assert torch.equal(am.cpu(), ref.argmax)
    else:
        assert am is None
    assert abs(loss - float(ref.loss)) <= 1e-5 * abs(float(ref.loss))
    assert abs(float(stats[0]) - float(ref.nll)) <= 1e-5 * abs(float(ref.nll))
    assert float(stats[1]) == float(torch.tensor(ref.acc, dtype=torch.float32))
    if not want_grad:
        assert dl is None
        return ref
    assert dl.shape == (rows, ld) and dl.dtype == grad_dtype
    dl = dl.cpu()
    assert bool((dl[:, V:] == 0).all())
    assert bool((dl[tgt == ignore_index] == 0).all())
    if bool((tgt == ignore_index).all()):
        assert loss == 0.0 and bool((dl == 0).all()) and float(stats[0]) == 0.0 and float(stats[1]) == 0.0
        return ref
    err = relerr(dl[:, :V].float(), grad_scale * ref.grad)
    print(f"    dlogits relerr {err:.3e}")
    assert err < (1e-2 if grad_dtype == B16 else 1e-5)
    return ref


@pytest.mark.parametrize("V,ld", SIZES)
def test_sizes_smoothing_ties_and_ignored_rows(V, ld):
    """Every path of the dispatcher at its boundaries, rows 1 / 5 / 130 (130: a ragged last block where four rows
    share a workgroup), eps 0 and 0.1, grad_scale 1, 0.125 and 64 in both gradient dtypes; targets at columns 0 and
    V - 1, a stride of ignored rows, all rows ignored, ignore_index = 0; without gradient, without argmax."""
    for rows in ([1, 5] if V >= 40000 else [1, 5, 130]):
        x, full = _tied_logits(rows, V, ld)
        fulld = full.to(dev)
        tgt = _targets(rows, V)
        some = tgt.clone()
        some[3::7] = -100
        zero = tgt.clone()
        zero[2::5] = 0                                   # ignore_index = 0: the class-0 rows are the ignored ones
        for eps in (0.0, 0.1):
            ref = R.cross_entropy(x, some, eps=eps)
            for gs, gd in ((1.0, B16), (1.0, F32), (0.125, F32), (0.125, B16), (64.0, B16), (64.0, F32)):
                _check(x, fulld, V, some, -100, eps, gs, gd, ref=ref)
            _check(x, fulld, V, some, -100, eps, 64.0, B16, ref=ref, want_grad=False)
            _check(x, fulld, V, some, -100, eps, 1.0, F32, ref=ref, want_argmax=False)
            _check(x, fulld, V, some, -100, eps, 1.0, B16, ref=ref, want_grad=False, want_argmax=False)
            if rows > 1:                                  # (rows = 1: its one target is class 0)
                _check(x, fulld, V, zero, 0, eps, 1.0, B16)
                _check(x, fulld, V, zero, 0, eps, 0.125, F32)
            none = torch.full((rows,), -100)
            r0 = R.cross_entropy(x, none, eps=eps)
            assert float(r0.loss) == 0.0 and r0.acc == 0.0
            _check(x, fulld, V, none, -100, eps, 1.0, B16, ref=r0)
            _check(x, fulld, V, none, -100, eps, 64.0, F32, ref=r0)
            _check(x, fulld, V, torch.zeros(rows, dtype=torch.int64), 0, eps, 1.0, B16)   # all ignored as class 0


@pytest.mark.parametrize("V,ld", [(250, 256), (1025, 1088), (1031, 1031), (5000, 5056), (16385, 16448)])
def test_sharp_rows(V, ld):
    """Logits x 30: one class holds nearly all the mass, exp underflows for most others, lse is far from the mean."""
    for rows in (5, 130):
        g = torch.Generator().manual_seed(V)
        x = torch.randn(rows, V, generator=g) * 30
        full = torch.full((rows, ld), float("inf"))
        full[:, :V] = x
        tgt = _targets(rows, V)
        tgt[2::3] = x.argmax(-1)[2::3]                    # some rows right (tiny nll), the rest wrong (large nll)
        tgt[3::7] = -100
        for eps in (0.0, 0.1):
            ref = R.cross_entropy(x, tgt, eps=eps)
            _check(x, full.to(dev), V, tgt, -100, eps, 1.0, F32, ref=ref)
            _check(x, full.to(dev), V, tgt, -100, eps, 64.0, B16, ref=ref)


def _ordered(bits):
    """bf16 bit patterns as integers in value order (one step = one ulp; -0 and +0 coincide)."""
    b = bits.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


@pytest.mark.parametrize("V,ld", [(2, 2), (250, 256), (500, 512), (1000, 1024)])
def test_agrees_with_the_old_entry_point_where_both_apply(V, ld, monkeypatch):
    """ld <= 1024, eps = 0, bf16: the wrapper calls asrx_cross_entropy; forced through asrx_cross_entropy_ls (by asking
    for stats) the loss agrees to 1e-6 relative, dlogits to one bf16 ulp, argmax exactly."""
    names = []
    real = K().call
    monkeypatch.setattr(K(), "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for rows in (1, 5, 130):
        x, full = _tied_logits(rows, V, ld)
        tgt = _targets(rows, V)
        tgt[3::7] = -100
        fulld, tgtd = full.to(dev), tgt.to(dev)
        for gs in (1.0, 64.0):
            del names[:]
            l0, d0, a0 = K().cross_entropy(fulld, V, tgtd, grad_scale=gs, want_argmax=True)
            assert names == ["asrx_cross_entropy"]
            l1, d1, a1, _ = K().cross_entropy(fulld, V, tgtd, grad_scale=gs, want_argmax=True, want_stats=True)
            assert names == ["asrx_cross_entropy", "asrx_cross_entropy_ls"]
            assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0))
            assert torch.equal(a0, a1)
            assert int((_ordered(d0.cpu()) - _ordered(d1.cpu())).abs().max()) <= 1


def test_every_other_request_takes_the_new_entry_point(monkeypatch):
    names = []
    real = K().call
    monkeypatch.setattr(K(), "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    x = torch.randn(6, 256, device=dev)
    t = torch.randint(0, 250, (6,), device=dev)
    K().cross_entropy(x, 250, t, label_smoothing=0.1)
    K().cross_entropy(x, 250, t, grad_dtype=F32)
    K().cross_entropy(x, 250, t, want_stats=True)
    K().cross_entropy(torch.randn(6, 1088, device=dev), 1025, t)       # refused before this entry point existed
    assert names == ["asrx_cross_entropy_ls"] * 4
    with pytest.raises(ValueError):
        K().cross_entropy(x, 250, t, label_smoothing=1.0)


@pytest.mark.parametrize("V,ld", [(1025, 1088), (1031, 1031), (16385, 16448)])
def test_loss_is_bit_reproducible(V, ld):
    x, full = _tied_logits(130, V, ld)
    fulld = full.to(dev)
    tgt = _targets(130, V).to(dev)
    runs = [K().cross_entropy(fulld, V, tgt, label_smoothing=0.1, want_stats=True) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][3].view(torch.int32), runs[1][3].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))


def test_no_rows():
    """rows == 0 at the C ABI (live pointers, as for any call): loss 0, stats 0, nothing else written."""
    from asrx._lib import BF16
    x, t = torch.zeros(4, 1088, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    out = torch.full((3,), 7.0, device=dev)
    dl = torch.full((4, 1088), 7.0, device=dev, dtype=B16)
    ws = torch.empty(K().xent_workspace_elems(0), device=dev)
    K().call("asrx_cross_entropy_ls", x.data_ptr(), 0, 1025, 1088, t.data_ptr(), -100, 0.1, 1.0, out.data_ptr(),
             out[1:].data_ptr(), BF16, dl.data_ptr(), None, ws.data_ptr(), K().stream())
    assert out.tolist() == [0.0, 0.0, 0.0] and bool((dl == 7.0).all())


def test_row_strided_view_is_read_in_place():
    """A [rows, V] view of a [rows, ld] buffer: the stride is the kernel's ld, the columns past V are never read."""
    V, ld, rows = 1500, 1536, 7
    x, full = _tied_logits(rows, V, ld)
    tgt = _targets(rows, V)
    view = full.to(dev)[:, :V]
    with pytest.raises(AssertionError):                    # (not by accident: the caller says so)
        K().cross_entropy(view, V, tgt.to(dev), label_smoothing=0.1)
    loss, dl, _ = K().cross_entropy(view, V, tgt.to(dev), label_smoothing=0.1, grad_dtype=F32, strided=True)
    ref = R.cross_entropy(x, tgt, eps=0.1)
    assert dl.shape == (rows, ld)
    assert abs(float(loss) - float(ref.loss)) <= 1e-5 * abs(float(ref.loss))
    assert relerr(dl[:, :V].cpu(), ref.grad) < 1e-5 and bool((dl[:, V:] == 0).all())
