"""The GEMM families of libasrx.so against the exact integer reference of tests/gemm_ref.py, bit for bit.

Every case asserts (a) that the kernel it declares is the one the plan launches, (b) that C equals the exact
result (torch.equal, all finite: the operands' padding is NaN), (c) that no byte outside the logical outputs
changed (C, mask_out, row sums, the split-K workspaces' surroundings), and (d) for dropout cases that the elements
dropped are exactly those the counter-based RNG drops.  No tolerance anywhere.

Split-K with splits that have no K range (k_per_split is rounded up to whole 64-deep steps): the p3 family left
such a split's partial slab and row-sum row unwritten while the reduction summed every slab.  With this file's
NaN-filled workspaces all of C came out NaN, first at element (0, 0), in the 14 cases split-p3-{NT,TT}-k576s7,
-k320s4, -k640s8 (beta 0 and 1), split-p3-NT-k64s2-b0 and split-p3-TT-k64s3-b1; the four -k320s5 cases (no empty
split) passed.  asrx_gemm now launches and reduces only p3's non-empty splits, and all of them pass."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
CASES = R.all_cases()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _first_diff(got, want):
    ne = (_bits(got.contiguous()) != _bits(want.contiguous())).reshape(-1)
    if not bool(ne.any()):
        return "equal"
    i = int(ne.nonzero()[0])
    idx = np.unravel_index(i, tuple(got.shape))
    return f"{int(ne.sum())} of {ne.numel()} differ, first at {tuple(int(x) for x in idx)}: " \
           f"got {float(got.reshape(-1)[i])}, want {float(want.reshape(-1)[i])}"


def _guards_unchanged(after, before, inside_index, what):
    """every element of the buffer outside `inside_index` keeps its bit pattern"""
    outside = torch.ones(before.numel(), dtype=torch.bool)
    outside[inside_index.reshape(-1)] = False
    a, b = _bits(after)[outside], _bits(before)[outside]
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} guard elements changed, first at flat index " \
                              f"{int(outside.nonzero().reshape(-1)[(a != b).nonzero()[0]])}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_gemm_exact(case):
    k = K()
    k.set_seed_offset(0)
    b = R.make_case(case)
    d_bufs = {name: t.to(dev) for name, t in b.bufs.items()}
    base = {name: t.data_ptr() for name, t in d_bufs.items()}
    assert all(p % 256 == 0 for p in base.values())       # the alignment the host-only plan test assumed
    d = b.desc(base)
    assert k.kernel_name(d) == R.expected_name(case)       # (a)
    k.call("asrx_gemm", ctypes.byref(d), k.stream())
    torch.cuda.synchronize()
    out = {name: d_bufs[name].cpu() for name in ("c", "mask_out", "rowsum", "ws", "rowsum_ws") if name in d_bufs}

    got = out["c"][b.c_index]                              # (b)
    exact = bool(torch.isfinite(got.float()).all()) and torch.equal(got, b.expect_c)
    assert exact, _first_diff(got, b.expect_c)
    _guards_unchanged(out["c"], b.bufs["c"], b.c_index, "C")   # (c)
    if case.mask_out:
        idx = torch.from_numpy(b.lay["mask_out"].index())
        got_mask = out["mask_out"][idx][0]
        assert torch.equal(got_mask, b.expect_mask), _first_diff(got_mask, b.expect_mask)
        _guards_unchanged(out["mask_out"], b.bufs["mask_out"], idx, "mask_out")
    if case.rowsum:
        idx = torch.arange(64, 64 + case.m)
        assert torch.equal(out["rowsum"][idx], b.expect_rowsum), _first_diff(out["rowsum"][idx], b.expect_rowsum)
        _guards_unchanged(out["rowsum"], b.bufs["rowsum"], idx, "rowsum")
    for name, elems in (("ws", case.splitk * case.m * case.n), ("rowsum_ws", case.splitk * case.m)):
        if name in out:
            _guards_unchanged(out[name], b.bufs[name], torch.arange(R.WS_GUARD, R.WS_GUARD + elems), name)
    if case.drop:                                          # (d)
        # what the residual and beta * C_old were added to is zero exactly where the RNG drops (or where nothing
        # was there to drop: a zero before the dropout, a closed gate)
        dropped = (got.double().numpy() - b.addend) == 0
        live = b.pre_drop != 0
        if b.gate_pos is not None:
            live = live & b.gate_pos
        assert np.array_equal(~dropped, b.keep & live)
        assert np.array_equal(dropped[live], ~b.keep[live])


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("kind", list(R.GROUP_KINDS))
def test_grouped_wgrad_exact(kind, beta, monkeypatch):
    """G. grouped weight gradients (asrx_gemm_grouped_xcd through linear_wgrad_grouped), five groups whose reduction
    is 1, 63, 65, 200 and 264 rows long, bias-gradient row sums on every other group: exact, guarded outputs."""
    k = K()
    wkind, queue, names = R.GROUP_KINDS[kind]
    monkeypatch.setattr(k, "WGRAD_KIND", wkind)
    monkeypatch.setattr(k, "WGRAD_QUEUE", queue)
    monkeypatch.setattr(k, "WGRAD_XCD", True)
    groups = R.make_groups(beta, 11 + int(beta))
    items, held = [], []
    for g in groups:
        dbuf = {name: t.to(dev) for name, t in g.bufs.items()}
        held.append(dbuf)

        def view(name):
            lay = g.lay[name]
            return torch.as_strided(dbuf[name], (lay.rows, lay.cols), (lay.ld, 1), lay.off)
        bg = dbuf["bg"][64:64 + g.lay["dy"].cols] if "bg" in dbuf else None
        items.append((view("dy"), view("x"), view("w"), bg))
    assert all(k.wgrad_groupable(dy, x, w) for dy, x, w, _ in items)
    kname = k.linear_wgrad_grouped(items, beta=beta)
    torch.cuda.synchronize()
    assert kname == names[int(beta)]
    for g, dbuf in zip(groups, held):
        w = dbuf["w"].cpu()
        idx = torch.from_numpy(g.lay["w"].index())
        got = w[idx][0]
        exact = bool(torch.isfinite(got).all()) and torch.equal(got, g.expect_w)
        assert exact, _first_diff(got, g.expect_w)
        _guards_unchanged(w, g.bufs["w"], idx, "dW")
        if g.expect_b is not None:
            bgh = dbuf["bg"].cpu()
            idx = torch.arange(64, 64 + g.expect_b.numel())
            assert torch.equal(bgh[idx], g.expect_b), _first_diff(bgh[idx], g.expect_b)
            _guards_unchanged(bgh, g.bufs["bg"], idx, "bias gradient")
