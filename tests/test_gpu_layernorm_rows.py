"""LayerNorm (csrc/norm.hip, csrc/ln512.h) row by row against float64, with the bounds of tests/rowkernel_ref.py.

Seven input families interleaved row by row (plain, mean / sigma of 100 and 3000, variance far below eps, 1e4 sigma,
one outlier, constant), so no row hides behind a tensor-wide maximum: y in fp32 and bf16, mean, rstd, dx and dx_drop
per row; the mean also bit for bit against the kernels' own order of addition; constant rows give beta exactly.
Every launch here goes through the C ABI with its outputs (y, mean, rstd, dx, dx_drop, part of exactly
nblocks * 2 d) inside sentinel buffers, and every launch checks that no sentinel changed.

Paths no other test walks: the forward ring's refill at ln_pf = 4 (9219 rows at ln_bpc = 1: two whole trips and a
ragged third), the backward rings at nblocks 1..3 (100 rows: four trips of a PF = 4 ring), the grid-stride loops of
the CH x NJ and any-width backward at nblocks 1 and 3, dbeta exact on integer gradients, rows permuted and one row
NaN (a ring slot read for the wrong row moves bits), zero rows.

Measured on the MI355X with the kernels of commit ef27a9a (worst ratio to the bound over the module, as printed):
y fp32 0.089, y bf16 1.000 (a tie: half an ulp exactly, the fp32 part unused), mean 0.144, rstd 0.162, dx 0.131,
dx_drop fp32 0.107, dx_drop bf16 0.999, dgamma 0.016, dbeta 0.011.  All 110 cases passed on their first run: nothing
was found wrong and no bound was touched afterwards."""
import pytest
import torch

import rowkernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, B16 = R.F32, R.B16
WORST = {}   # quantity -> worst ratio to its bound seen in this run (printed by every test that adds to it)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


@pytest.fixture
def tuning():
    """Set a kernel-variant switch (asrx_set_tuning) for one test and restore the default afterwards."""
    used = []

    def set_(name, value):
        used.append(name)
        K().set_tuning(name, value)
    yield set_
    for name in used:
        K().set_tuning(name, 0)


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    return ratio


def _report(label):
    print(f"{label}: worst ratio to the bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------ guarded launches

def fwd(x, gam, bet, ydt, rows=None):
    """asrx_layernorm_fwd on device tensors; y / mean / rstd inside sentinels -> (y, mean, rstd), guards checked"""
    k = K()
    n, d = x.shape
    rows = n if rows is None else rows
    ybuf, y = R.guarded(rows * d, ydt, dev)
    mbuf, mean = R.guarded(rows, F32, dev)
    rbuf, rstd = R.guarded(rows, F32, dev)
    k.call("asrx_layernorm_fwd", k.code(x), x.data_ptr(), k.code(y), y.data_ptr(), gam.data_ptr(), bet.data_ptr(),
           mean.data_ptr(), rstd.data_ptr(), rows, d, R.EPS, k.stream())
    torch.cuda.synchronize()
    assert R.guards_intact(ybuf, rows * d) and R.guards_intact(mbuf, rows) and R.guards_intact(rbuf, rows)
    return y.view(rows, d), mean, rstd


def wrapper_nblocks(rows, d):
    """the grid kernels.layernorm_bwd chooses"""
    wpb = R.LNB_W if d == 512 else 4
    return max(1, min(512 * 4 // wpb, (rows + 2 * wpb - 1) // (2 * wpb)))


def bwd(x, dy, gam, mean, rstd, dres, drop_dt, nblocks, rows=None):
    """asrx_layernorm_bwd (p = 0) -> (dx, dx_drop or None, part [nblocks, 2 d]); guards of all three checked"""
    k = K()
    n, d = x.shape
    rows = n if rows is None else rows
    dbuf, dx = R.guarded(rows * d, F32, dev)
    pbuf, part = R.guarded(nblocks * 2 * d, F32, dev)
    qbuf, drop = R.guarded(rows * d, drop_dt, dev) if drop_dt is not None else (None, None)
    k.call("asrx_layernorm_bwd", k.code(x), x.data_ptr(), k.code(dy), dy.data_ptr(), gam.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), None if dres is None else dres.data_ptr(), dx.data_ptr(),
           None if drop is None else drop.data_ptr(), k.code(drop) if drop is not None else 0, 0.0, 0,
           part.data_ptr(), nblocks, rows, d, k.stream())
    torch.cuda.synchronize()
    assert R.guards_intact(dbuf, rows * d), "dx guards"
    assert R.guards_intact(pbuf, nblocks * 2 * d), "part guards"
    assert qbuf is None or R.guards_intact(qbuf, rows * d), "dx_drop guards"
    return dx.view(rows, d), None if drop is None else drop.view(rows, d), part.view(nblocks, 2 * d)


def reduce_part(part, dgb):
    """dgb += column sums of part, as kernels.layernorm_bwd reduces them (defer = None)"""
    k = K()
    nblocks, cols = part.shape
    nb2 = max(1, (nblocks + 63) // 64)
    p2buf, p2 = R.guarded(nb2 * cols, F32, dev)
    k.call("asrx_reduce_rows", k.F32, part.data_ptr(), nblocks, cols, cols, dgb.data_ptr(), 1, p2.data_ptr(), nb2,
           k.stream())
    torch.cuda.synchronize()
    assert R.guards_intact(p2buf, nb2 * cols)


# ------------------------------------------------------------------------------------------ inputs and checks

_inputs = {}


def inputs(rows, d, kinds=R.FAMILIES):
    """(x, gamma, beta on the host, the float64 reference): made once per shape and left unchanged"""
    key = (rows, d, kinds)
    if key not in _inputs:
        x = R.mixed_rows(rows, d, rows + d, kinds)
        gam, bet = R.ln_params(d, d)
        _inputs[key] = (x, gam, bet, R.ln_ref(x, gam, bet))
    return _inputs[key]


def check_fwd(label, x, gam, bet, ref, y, mean, rstd, kind, kinds=R.FAMILIES):
    """per-row bounds on y (fp32 or bf16), mean and rstd; the mean bit for bit in the kernel's order of addition;
    constant rows exactly beta"""
    yh, mh, rh = y.cpu(), mean.cpu(), rstd.cpu()
    assert bool(torch.isfinite(yh.float()).all()) and bool(torch.isfinite(mh).all()) and bool(torch.isfinite(rh).all())
    yb = ref.y_bound if yh.dtype == F32 else R.bf16_bound(ref.y, ref.y_bound)
    name = "y_fp32" if yh.dtype == F32 else "y_bf16"
    ry = _note(name, R.worst((yh.double() - ref.y).abs(), yb))
    rm = _note("mean", R.worst((mh.double() - ref.mean).abs(), ref.mean_bound))
    rr = _note("rstd", R.worst(((rh.double() - ref.rstd) / ref.rstd).abs(), ref.rstd_bound))
    print(f"{label}: {name} {ry:.3f} mean {rm:.3f} rstd {rr:.3f} of the bound")
    assert ry <= 1 and rm <= 1 and rr <= 1, (label, ry, rm, rr)
    model = R.mean_model_f32(x, kind)
    assert R.same_bits(mh, model), f"{label}: mean differs from the {kind} order of addition in " \
                                   f"{int((R.bits(mh) != R.bits(model)).sum())} rows"
    if "constant" in kinds:
        c = slice(kinds.index("constant"), None, len(kinds))
        want = bet.to(yh.dtype).expand_as(yh[c])
        assert R.same_bits(yh[c].contiguous(), want.contiguous()), f"{label}: constant rows are not beta"


def check_bwd(label, x, dy, gam, mean, rstd, dres, ref, dx, drop):
    dxr, bound, *_ = R.ln_bwd_ref(x, dy.cpu(), gam, mean.cpu(), rstd.cpu(), dres, ref.cond)
    dxh = dx.cpu()
    assert bool(torch.isfinite(dxh).all())
    r = _note("dx", R.worst((dxh.double() - dxr).abs(), bound))
    out = f"{label}: dx {r:.3f}"
    assert r <= 1, (label, r)
    if drop is not None:
        dh = drop.cpu()
        name = "dx_drop_bf16" if dh.dtype == B16 else "dx_drop_fp32"
        bd = R.bf16_bound(dxr, bound) if dh.dtype == B16 else bound
        rd = _note(name, R.worst((dh.double() - dxr).abs(), bd))
        out += f" {name} {rd:.3f}"
        assert rd <= 1, (label, rd)
        assert R.same_bits(dh, dxh.to(dh.dtype)), f"{label}: dx_drop at p = 0 is not dx rounded to nearest even"
    print(out + " of the bound")


# ------------------------------------------------------------------------------------------ widths and variants

VARIANTS = [(80, 0, 0)] + [(d, 0, rw) for d in (256, 1024) for rw in (1, 2, 4)] + \
           [(512, pf, 0) for pf in (1, 2, 4)] + [(512, 8, rw) for rw in (1, 2, 4)]


@pytest.mark.parametrize("d,pf,rw", VARIANTS)
def test_layernorm_rows(d, pf, rw, tuning):
    """37 rows of the seven families: the any-width kernel (80), CH x NJ (256; 1024 = <4, 4>; 512 at ln_pf = 8) at
    1, 2 and 4 rows per wave, the d = 512 streaming kernels at 1, 2 and 4 rows in flight"""
    tuning("ln_pf", pf)
    tuning("ln_rw", rw)
    rows = 37
    x, gam, bet, ref = inputs(rows, d)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    label = f"d {d} pf {pf} rw {rw}"
    for ydt in (B16, F32):
        y, mean, rstd = fwd(xd, gd, bd, ydt)
        check_fwd(label, x, gam, bet, ref, y, mean, rstd, R.ln_kind(d, ydt == B16 and pf != 8))
    for dyt in (B16, F32):   # (dx_drop in the gradient's dtype: the d = 512 kernels write it in bf16 only)
        dy, dres = R.ln_grads(rows, d, d, dyt)
        dx, drop, _ = bwd(xd, dy.to(dev), gd, mean, rstd, dres.to(dev), dyt, wrapper_nblocks(rows, d))
        check_bwd(f"{label} dy {dyt}", x, dy, gam, mean, rstd, dres, ref, dx, drop)
    _report(label)


# ------------------------------------------------------------------------------------------ forward ring

@pytest.mark.parametrize("pf,rows", [(4, 9219), (2, 5123)])
def test_layernorm_forward_ring(pf, rows, tuning):
    """d = 512 at ln_bpc = 1 (nw = 1024 waves): two whole trips of the PF-slot ring and a ragged third (1027 rows).
    Per-row bounds on every row, and y / mean / rstd bit-equal to ln_pf = 1 at the default grid, where no slot is
    ever refilled (ln_fwd512_rows: the arithmetic of a row does not depend on PF or the grid)."""
    assert R.ln_fwd_waves(rows, 1) == 1024 and R.ring_trips(rows, pf, 1024) == (2, 1027)
    x, gam, bet, ref = inputs(rows, 512)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    tuning("ln_pf", 1)
    y1, m1, r1 = fwd(xd, gd, bd, B16)
    tuning("ln_pf", pf)
    tuning("ln_bpc", 1)
    y, mean, rstd = fwd(xd, gd, bd, B16)
    check_fwd(f"ring pf {pf} rows {rows}", x, gam, bet, ref, y, mean, rstd, "stream")
    assert R.same_bits(y, y1) and R.same_bits(mean, m1) and R.same_bits(rstd, r1)
    _report(f"forward ring pf {pf}")


# ------------------------------------------------------------------------------------------ backward rings

_stats = {}


def stats(rows, d, kinds=R.FAMILIES):
    """the kernel's own mean / rstd of inputs(rows, d, kinds), from the default forward (device tensors)"""
    key = (rows, d, kinds)
    if key not in _stats:
        x, gam, bet, _ = inputs(rows, d, kinds)
        k = K()
        for name in ("ln_pf", "ln_rw", "ln_bpc"):
            k.set_tuning(name, 0)
        _, mean, rstd = fwd(x.to(dev), gam.to(dev), bet.to(dev), B16)
        _stats[key] = (mean, rstd)
    return _stats[key]


_base = {}


def check_dgb(label, x, dy, gam, mean, rstd, part):
    """dgamma | dbeta from `part` through asrx_reduce_rows, per column against float64"""
    d = x.shape[1]
    dgb = torch.zeros(2 * d, device=dev)
    reduce_part(part, dgb)
    _, _, dg, db, bg, bb = R.ln_bwd_ref(x, dy.cpu(), gam, mean.cpu(), rstd.cpu(), None, torch.ones(x.shape[0]))
    got = dgb.cpu().double()
    rg = _note("dgamma", R.worst((got[:d] - dg).abs(), bg))
    rb = _note("dbeta", R.worst((got[d:] - db).abs(), bb))
    print(f"{label}: dgamma {rg:.3f} dbeta {rb:.3f} of the bound")
    assert rg <= 1 and rb <= 1, (label, rg, rb)


def ring_case(d, nblocks, pf, rows, dyt, tuning):
    label = f"bwd d {d} nblocks {nblocks} pf {pf} rows {rows} dy {dyt}"
    x, gam, bet, ref = inputs(rows, d)
    mean, rstd = stats(rows, d)
    mp, rp = stats(rows, d, ("plain",))
    tuning("ln_pf", pf)   # (after stats(), which restores the defaults)
    dy, dres = R.ln_grads(rows, d, d + rows, dyt)
    xd, gd, dyd, dresd = x.to(dev), gam.to(dev), dy.to(dev), dres.to(dev)
    drop_dt = B16 if d == 512 else dyt
    dx, drop, _ = bwd(xd, dyd, gd, mean, rstd, dresd, drop_dt, nblocks)
    check_bwd(label, x, dy, gam, mean, rstd, dres, ref, dx, drop)
    key = (d, rows, dyt)
    if key not in _base:
        _base[key] = (label, dx.clone(), drop.clone())
    else:   # one dx for every grid and ring depth
        assert R.same_bits(dx, _base[key][1]), f"{label}: dx differs from {_base[key][0]}"
        assert R.same_bits(drop, _base[key][2]), f"{label}: dx_drop differs from {_base[key][0]}"
    # dgamma | dbeta on plain rows
    xp, _, _, _ = inputs(rows, d, ("plain",))
    _, _, part = bwd(xp.to(dev), dyd, gd, mp, rp, None, None, nblocks)
    check_dgb(label, xp, dy, gam, mp, rp, part)


@pytest.mark.parametrize("dyt", [B16, F32], ids=["dy_bf16", "dy_fp32"])
@pytest.mark.parametrize("rows", [5, 37, 100])
@pytest.mark.parametrize("pf", [1, 2, 4])
@pytest.mark.parametrize("nblocks", [1, 2, 3])
def test_layernorm_backward_ring_512(nblocks, pf, rows, dyt, tuning):
    """ln_bwd512_kernel<PF, DYF> at its smallest grids: nblocks = 1 is 8 waves, so 100 rows are four trips of a
    PF = 4 ring with a ragged last (PF nw = 32).  dx and dx_drop bit-equal across every nblocks and ln_pf."""
    assert R.ring_trips(100, 4, R.LNB_W) == (3, 4)
    ring_case(512, nblocks, pf, rows, dyt, tuning)
    _report("backward ring 512")


@pytest.mark.parametrize("dyt", [B16, F32], ids=["dy_bf16", "dy_fp32"])
@pytest.mark.parametrize("nblocks", [1, 3])
@pytest.mark.parametrize("d", [256, 80])
def test_layernorm_backward_grid_stride(d, nblocks, dyt, tuning):
    """ln_bwd_kernel<4, 1> (256) and ln_bwd_any_kernel (80) at 37 rows on 1 and 3 blocks of 4 waves: 10 and 4 trips
    of the grid-stride loop, the last ragged"""
    ring_case(d, nblocks, 0, 37, dyt, tuning)
    _report("backward grid stride")


# ------------------------------------------------------------------------------------------ exact dbeta

@pytest.mark.parametrize("rows", [37, 15936])
@pytest.mark.parametrize("d,nblocks", [(512, 1), (512, 2), (512, 3), (256, 1), (256, 3), (80, 1), (80, 3), (512, 0),
                                       (256, 0), (80, 0)])
def test_layernorm_dbeta_exact(d, nblocks, rows):
    """dy integers in [-8, 8] (exact in bf16; every partial sum stays below 2^24): dbeta equals the integer column
    sums bit for bit.  nblocks 0: kernels.layernorm_bwd with defer = None at its own grid."""
    k = K()
    x = R.mixed_rows(rows, d, 7, ("plain",)).to(dev)
    gam, bet = (t.to(dev) for t in R.ln_params(d, d))
    dy = R.int_rows(rows, d, 8, rows + d, B16)
    want = dy.double().sum(0).to(F32)
    _, mean, rstd = fwd(x, gam, bet, B16)
    dgb = torch.zeros(2 * d, device=dev)
    if nblocks == 0:
        k.layernorm_bwd(x, dy.to(dev), gam, mean, rstd, dgb, defer=None)
    else:
        _, _, part = bwd(x, dy.to(dev), gam, mean, rstd, None, None, nblocks)
        reduce_part(part, dgb)
    torch.cuda.synchronize()
    got = dgb[d:].cpu()
    assert R.same_bits(got, want), f"{int((got != want).sum())} of {d} columns differ, first " \
                                   f"{int((got != want).nonzero()[0])}"


# ------------------------------------------------------------------------------------------ row independence

def _independence(label, run, nrows, outs_nan_row):
    """run(perm or None, nan_row or None) -> tuple of per-row outputs (dim 0 = rows)"""
    base = run(None, None)
    g = torch.Generator().manual_seed(nrows)
    perm = torch.randperm(nrows, generator=g)
    got = run(perm, None)
    pd = perm.to(dev)
    for i, (a, b) in enumerate(zip(got, base)):
        assert R.same_bits(a, b[pd]), f"{label}: output {i} of the permuted rows is not the permuted output"
    r = outs_nan_row
    got = run(None, r)
    keep = torch.ones(nrows, dtype=torch.bool, device=dev)
    keep[r] = False
    for i, (a, b) in enumerate(zip(got, base)):
        assert bool(torch.isnan(a[r].float()).all()), f"{label}: output {i} of the NaN row is not NaN"
        assert R.same_bits(a[keep], b[keep]), f"{label}: output {i}: a NaN in row {r} moved another row"


@pytest.mark.parametrize("d,rows,pf,bpc,rw", [(512, 9219, 4, 1, 0), (256, 37, 0, 0, 4)])
def test_layernorm_forward_rows_are_independent(d, rows, pf, bpc, rw, tuning):
    tuning("ln_pf", pf)
    tuning("ln_bpc", bpc)
    tuning("ln_rw", rw)
    x, gam, bet, _ = inputs(rows, d)
    gd, bd = gam.to(dev), bet.to(dev)

    def run(perm, nan_row):
        xx = x.clone() if perm is None else x[perm]
        if nan_row is not None:
            xx[nan_row, d // 3] = float("nan")
        return fwd(xx.to(dev), gd, bd, B16)
    # (row 2051 of 9219: second trip of its wave's ring, with neighbours in flight on both sides)
    _independence(f"fwd d {d}", run, rows, 2051 if rows > 2051 else 17)


@pytest.mark.parametrize("d,rows,pf", [(512, 100, 4), (256, 37, 0)])
def test_layernorm_backward_rows_are_independent(d, rows, pf, tuning):
    x, gam, bet, _ = inputs(rows, d)
    mean, rstd = stats(rows, d)
    tuning("ln_pf", pf)
    dy, dres = R.ln_grads(rows, d, d, B16)
    gd = gam.to(dev)

    def run(perm, nan_row):
        sel = torch.arange(rows) if perm is None else perm
        xx = x[sel].clone()
        if nan_row is not None:
            xx[nan_row] = float("nan")
        sd = sel.to(dev)
        dx, drop, _ = bwd(xx.to(dev), dy[sel].to(dev), gd, mean[sd].contiguous(), rstd[sd].contiguous(),
                          dres[sel].to(dev), B16, 1)
        return dx, drop
    _independence(f"bwd d {d}", run, rows, 41 if rows > 41 else 17)


# ------------------------------------------------------------------------------------------ guards, zero rows

@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("d", [80, 512])
def test_layernorm_guards(d, rows):
    """every output between sentinels at the smallest row counts (fwd() and bwd() assert that none changed), part of
    exactly nblocks * 2 d at the wrapper's grid and at 3 blocks, most of whose waves have no row"""
    x, gam, bet, ref = inputs(rows, d)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    for ydt in (B16, F32):
        y, mean, rstd = fwd(xd, gd, bd, ydt)
        check_fwd(f"guards d {d} rows {rows}", x, gam, bet, ref, y, mean, rstd, R.ln_kind(d, ydt == B16))
    for dyt, nblocks in ((B16, wrapper_nblocks(rows, d)), (F32, 3)):
        dy, dres = R.ln_grads(rows, d, d, dyt)
        dx, drop, part = bwd(xd, dy.to(dev), gd, mean, rstd, dres.to(dev), dyt, nblocks)
        check_bwd(f"guards d {d} rows {rows} dy {dyt}", x, dy, gam, mean, rstd, dres, ref, dx, drop)
        assert bool(torch.isfinite(part).all())   # every block wrote its whole slab


@pytest.mark.parametrize("d", [80, 256, 512])
def test_layernorm_zero_rows(d):
    """rows = 0: the forward returns ASRX_OK and writes nothing; the backward writes zero partials (its reduce leaves
    dgamma | dbeta as they were) and nothing else"""
    x, gam, bet, _ = inputs(5, d)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    k = K()
    sent = torch.full((5 * d,), R.SENTINEL, device=dev)
    y, mean, rstd = sent.to(B16), sent[:5].clone(), sent[:5].clone()
    k.call("asrx_layernorm_fwd", k.F32, xd.data_ptr(), k.BF16, y.data_ptr(), gd.data_ptr(), bd.data_ptr(),
           mean.data_ptr(), rstd.data_ptr(), 0, d, R.EPS, k.stream())
    torch.cuda.synchronize()
    assert bool((y == R.SENTINEL).all()) and bool((mean == R.SENTINEL).all()) and bool((rstd == R.SENTINEL).all())
    dy = torch.ones(5, d, device=dev, dtype=B16)
    dx, drop = sent.clone(), sent.to(B16)
    nblocks = 3
    pbuf, part = R.guarded(nblocks * 2 * d, F32, dev)
    k.call("asrx_layernorm_bwd", k.F32, xd.data_ptr(), k.BF16, dy.data_ptr(), gd.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), None, dx.data_ptr(), drop.data_ptr(), k.BF16, 0.0, 0, part.data_ptr(), nblocks, 0, d,
           k.stream())
    torch.cuda.synchronize()
    assert bool((dx == R.SENTINEL).all()) and bool((drop == R.SENTINEL).all())
    assert R.guards_intact(pbuf, nblocks * 2 * d) and bool((part == 0).all())
    dgb = torch.randn(2 * d, generator=torch.Generator().manual_seed(d)).to(dev)
    before = dgb.clone()
    reduce_part(part.view(nblocks, 2 * d), dgb)
    assert R.same_bits(dgb, before)
