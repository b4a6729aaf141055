"""The unfused softmax (csrc/softmax.hip) row by row against float64, with the bounds of tests/rowkernel_ref.py.

Rows of six kinds in one launch (ramp, descending, last key, all negative, shared top, randn * 3): p per row within
1e-5 of the row maximum (bf16: half an ulp more), dS per row from the stored p, pd and dS under dropout against
rng_ref.attn_keep.  The case table (rowkernel_ref.softmax_cases) runs every instantiation the dispatch can launch,
forward and backward: the whole V = 1 family of unaligned row strides, the long-row kernels up to 8192 (bf16) and
4096 (fp32) keys, softmax_u 2 and 4 on every short-row kernel; and the three ASRX_ERR_UNSUPPORTED returns beyond.

Every buffer (s, p, pd, dS) is allocated as exactly rows * ld - (ld - Lk) elements between sentinels: the last
row's padding and everything after it must keep the sentinel, the padding of every other row must be 0 up to the
instantiation's capacity and untouched beyond it, and the scores' padding holds NaN, which must not reach a result.

Measured on the MI355X with the kernels of commit ef27a9a (worst ratio to the bound over the module, as printed):
p fp32 0.160, pd fp32 0.141, masked p fp32 0.220, dS fp32 0.003; bf16 p 0.997, pd 0.996, masked p 0.995, dS 0.988
(half an ulp is reached, the fp32 part is not).  All 138 cases passed on their first run: nothing was found wrong
and no bound was touched afterwards."""
import pytest
import torch

import rowkernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, B16 = R.F32, R.B16
SCALE = R.SM_SCALE
SEED = 0x5EED1234ABCD
WORST = {}


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


# ------------------------------------------------------------------------------------------ buffers

class Buf:
    """rows of ld elements of which the last has only Lk: n = rows * ld - (ld - Lk) elements between sentinels.  The
    trailing sentinels are at least ld long, so the [rows, ld] view exists; its last row's padding is guard."""

    def __init__(self, rows, Lk, ld, dtype, values=None, pad=float("nan")):
        self.rows, self.Lk, self.ld = rows, Lk, ld
        self.n = rows * ld - (ld - Lk)
        self.tail = max(R.GUARD, ld)
        host = torch.full((R.GUARD + self.n + self.tail,), R.SENTINEL, dtype=dtype)
        if values is not None:
            full = torch.full((rows, ld), pad, dtype=dtype)
            full[:, :Lk] = values.to(dtype)
            host[R.GUARD:R.GUARD + self.n] = full.reshape(-1)[:self.n]
        self.t = host.to(dev)

    def ptr(self):
        return self.t.data_ptr() + R.GUARD * self.t.element_size()

    def rows_host(self):
        """[rows, ld] on the host (the last row's padding comes from the trailing guard)"""
        return self.t[R.GUARD:R.GUARD + self.rows * self.ld].view(self.rows, self.ld).cpu()

    def values(self):
        return self.rows_host()[:, :self.Lk]

    def check_layout(self, what, cap, written=True):
        """guards and the last row's padding keep the sentinel; other rows' padding is 0 below the instantiation's
        capacity `cap` and sentinel from it on; written = False: the whole inside is still sentinel"""
        sent = torch.full((1,), R.SENTINEL, dtype=self.t.dtype, device=dev)
        assert bool((self.t[:R.GUARD] == sent).all()), f"{what}: leading guard changed"
        assert bool((self.t[R.GUARD + self.n:] == sent).all()), f"{what}: last row's padding or trailing guard changed"
        if not written:
            assert bool((self.t == sent).all()), f"{what}: written by a refused call"
            return
        pad = self.rows_host()[:-1, self.Lk:]
        zero_to = max(0, min(self.ld, cap) - self.Lk)
        assert bool((pad[:, :zero_to] == 0).all()), f"{what}: padding below column {cap} is not 0"
        assert bool((pad[:, zero_to:] == R.SENTINEL).all()), f"{what}: padding beyond the kernel's reach was written"


def capacity(name):
    """columns an instantiation covers: NJ LPR V (the streaming kernel: 256)"""
    if "stream" in name:
        return 256
    v, lpr, nj, _ = (int(t) for t in name[name.index("<") + 1:-1].split(","))
    return v * lpr * nj


def code(dtype):
    return K().BF16 if dtype == B16 else K().F32


def sm_fwd(s, p, pd, nbh, heads, Lq, Lk, ld, dtype, mode=0, causal=0, kvalid=None, qvalid=None, vb=0, mask=None,
           strides=(0, 0, 0), drop=0.0):
    k = K()
    k.call("asrx_softmax_fwd", code(dtype), s.ptr(), p.ptr(), None if pd is None else pd.ptr(), nbh, heads, Lq, Lk, ld,
           SCALE, mode, causal, kvalid, qvalid, vb, mask, strides[0], strides[1], strides[2], drop, SEED, k.stream())
    torch.cuda.synchronize()


def sm_bwd(p, g, ds, nbh, Lq, Lk, ld, dtype, drop=0.0):
    k = K()
    k.call("asrx_softmax_bwd", code(dtype), p.ptr(), g.ptr(), ds.ptr(), nbh, Lq, Lk, ld, SCALE, drop, SEED, k.stream())
    torch.cuda.synchronize()


def check_rows(label, what, got, ref, f32_bound, dtype):
    assert bool(torch.isfinite(got.float()).all()), f"{label}: {what} is not finite"
    bound = f32_bound if dtype == F32 else R.bf16_bound(ref, f32_bound)
    name = f"{what}_{'fp32' if dtype == F32 else 'bf16'}"
    r = _note(name, R.worst((got.double() - ref).abs(), bound))
    print(f"{label}: {name} {r:.3f} of the bound")
    assert r <= 1, (label, name, r)


def run_case(label, dtype, nbh, Lq, Lk, ld, u=0, drop=0.0, heads=3, scores=None):
    """forward (+ dropped copy) and backward with no mask, everything checked per row; returns the stored p"""
    from rng_ref import attn_keep
    rows = nbh * Lq
    x = R.softmax_scores(rows, Lk, Lk + rows) if scores is None else scores
    s = Buf(rows, Lk, ld, dtype, x)
    sv = s.values()
    ref = R.softmax_ref(sv)
    p = Buf(rows, Lk, ld, dtype)
    pd = Buf(rows, Lk, ld, dtype) if drop else None
    fname = R.softmax_kernel_name(dtype, ld, Lk, 0, drop > 0, u, False)
    bname = R.softmax_kernel_name(dtype, ld, Lk, 0, False, u, True)
    sm_fwd(s, p, pd, nbh, heads, Lq, Lk, ld, dtype, drop=drop)
    P = p.values()
    check_rows(label, "p", P, ref, R.softmax_p_bound(ref), dtype)
    p.check_layout(f"{label} p", capacity(fname))
    keep = None
    if drop:
        keep = torch.from_numpy(attn_keep(SEED, nbh, Lq, Lk, drop)).reshape(rows, Lk)
        assert abs(float(keep.double().mean()) - (1 - drop)) < 0.05
        PD = pd.values()
        check_rows(label, "pd", PD, ref * keep / (1 - drop), R.softmax_p_bound(ref) / (1 - drop), dtype)
        # exactly the dropped elements are zero (where p itself is not: a key 30 log2 units down underflows bf16's
        # product with no help from the RNG)
        live = P != 0
        assert torch.equal((PD == 0)[live], ~keep[live]), f"{label}: pd is not dropped where the RNG drops"
        pd.check_layout(f"{label} pd", capacity(fname))
    g = torch.randn(rows, Lk, generator=torch.Generator().manual_seed(Lk)).to(dtype)
    gb = Buf(rows, Lk, ld, dtype, g)
    ds = Buf(rows, Lk, ld, dtype)
    sm_bwd(p, gb, ds, nbh, Lq, Lk, ld, dtype, drop=drop)
    G = g.double() * keep / (1 - drop) if drop else g.double()
    dsr, dbound = R.softmax_ds_ref(P, G)
    check_rows(label, "dS", ds.values(), dsr, dbound, dtype)
    ds.check_layout(f"{label} dS", capacity(bname))
    return p


# ------------------------------------------------------------------------------------------ every instantiation

@pytest.mark.parametrize("case", R.softmax_cases(), ids=lambda c: c.id)
def test_softmax_instantiations(case, tuning):
    tuning("softmax_u", case.u)
    run_case(case.id, case.dtype, 6, case.Lq, case.Lk, case.ld, case.u, case.drop)
    _report(case.id)


@pytest.mark.parametrize("dtype,Lk,ld", R.SM_UNSUPPORTED,
                         ids=[f"{'bf16' if d == B16 else 'fp32'}-Lk{k}-ld{l}" for d, k, l in R.SM_UNSUPPORTED])
def test_softmax_unsupported_lengths(dtype, Lk, ld):
    """one key beyond the longest instantiation: ASRX_ERR_UNSUPPORTED from both entry points, nothing written"""
    nbh, Lq = 2, 3
    rows = nbh * Lq
    assert R.softmax_kernel_name(dtype, ld, Lk) is None and R.softmax_kernel_name(dtype, ld, Lk - 1) is not None
    s = Buf(rows, Lk, ld, dtype, torch.zeros(rows, Lk))
    p, ds = Buf(rows, Lk, ld, dtype), Buf(rows, Lk, ld, dtype)
    with pytest.raises(RuntimeError, match="unsupported"):
        sm_fwd(s, p, None, nbh, 1, Lq, Lk, ld, dtype)
    with pytest.raises(RuntimeError, match="unsupported"):
        sm_bwd(s, s, ds, nbh, Lq, Lk, ld, dtype)
    torch.cuda.synchronize()
    p.check_layout("p", 0, written=False)
    ds.check_layout("dS", 0, written=False)


# ------------------------------------------------------------------------------------------ masks

B_, H_ = 2, 3
MASKS = ["dense_k", "dense_qk", "dense_bqk", "causal", "kvalid_offset"]


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("Lq,Lk,ld", [(9, 40, 40), (9, 33, 33), (9, 5, 8), (9, 5, 5)],
                         ids=["aligned", "unaligned", "aligned_Lq>Lk", "unaligned_Lq>Lk"])
@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_softmax_masks(dtype, Lq, Lk, ld, kind):
    """Masks through asrx_softmax_fwd itself: mode 2 (dense bytes) with the broadcast strides (0, 0, 1), (0, Lk, 1)
    and (Lq Lk, Lk, 1); mode 1 causal with Lq < Lk and Lq > Lk plus key and query validity; key validity from a
    nonzero base offset with a batch stride beyond Lk.  Fully masked rows are exactly 0."""
    nbh, rows = B_ * H_, B_ * H_ * Lq
    g = torch.Generator().manual_seed(Lq * Lk + len(kind))
    x = R.softmax_scores(rows, Lk, Lk + 7)
    s = Buf(rows, Lk, ld, dtype, x)
    p = Buf(rows, Lk, ld, dtype)
    m = torch.zeros(B_, Lq, Lk, dtype=torch.bool)
    kw = {}
    if kind.startswith("dense"):
        shape = {"dense_k": (1, 1, Lk), "dense_qk": (1, Lq, Lk), "dense_bqk": (B_, Lq, Lk)}[kind]
        dense = (torch.rand(shape, generator=g) < 0.3)
        if kind != "dense_k":
            dense[-1, 2] = True         # a fully masked row
            dense[0, 5, :Lk - 1] = True   # a row with one key left
        else:
            dense[0, 0, 0] = False
        m = dense.expand(B_, Lq, Lk).clone()
        md = dense.to(torch.uint8).to(dev)
        strides = {"dense_k": (0, 0, 1), "dense_qk": (0, Lk, 1), "dense_bqk": (Lq * Lk, Lk, 1)}[kind]
        kw = dict(mode=2, mask=md.data_ptr(), strides=strides)
    else:
        vb = max(Lq, Lk) + 5
        base = 3 if kind == "kvalid_offset" else 0
        kval = torch.ones(base + B_ * vb, dtype=torch.uint8)
        kv = kval[base:].view(B_, vb)
        kv[1, Lk // 3 + 1:Lk] = 0
        kv[1, 0] = 0
        kv[:, Lk:] = 0 if kind == "kvalid_offset" else 1   # (beyond Lk: never read as a key)
        kd = kval.to(dev)
        m = m | ~kv[:, None, :Lk].bool()
        kw = dict(mode=1, kvalid=kd.data_ptr() + base, vb=vb)
        if kind == "causal":
            qval = torch.ones(B_, vb, dtype=torch.uint8)
            qval[0, Lq - 1] = 0
            qd = qval.to(dev)
            m = m | torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)[None] | ~qval[:, :Lq, None].bool()
            kw.update(causal=1, qvalid=qd.data_ptr())
    sm_fwd(s, p, None, nbh, H_, Lq, Lk, ld, dtype, **kw)
    mm = m[:, None].expand(B_, H_, Lq, Lk).reshape(rows, Lk)
    ref = R.softmax_ref(s.values(), masked=mm)
    dead = mm.all(-1)
    assert bool(dead.any()) or kind in ("dense_k", "kvalid_offset")
    P = p.values()
    label = f"mask {kind} Lq {Lq} Lk {Lk} ld {ld}"
    check_rows(label, "p_masked", P, ref, R.softmax_p_bound(ref), dtype)
    assert bool((P[dead] == 0).all()) and bool((P[mm] == 0).all()), f"{label}: a masked probability is not exactly 0"
    p.check_layout(label, capacity(R.softmax_kernel_name(dtype, ld, Lk, kw["mode"])))
    _report(label)


# ------------------------------------------------------------------------------------------ the last row

STREAM_TRIPS = 4 * 1024 * 2 * 4 + 5   # rows: 4 per group x 1024 blocks x 4 waves x PF 2 ring slots, then 5 rows more


@pytest.mark.parametrize("dtype,Lk,ld,rows", [(B16, 200, 208, 1), (B16, 200, 208, 7), (B16, 200, 208, STREAM_TRIPS),
                                              (B16, 249, 256, 7), (F32, 30, 32, 7), (B16, 30, 32, 7), (B16, 34, 35, 7),
                                              (F32, 34, 35, 1), (B16, 100, 512, 7), (F32, 100, 512, 7)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_softmax_last_row_untouched(dtype, Lk, ld, rows):
    """The last row's padding may not be allocated (softmax.hip loadable()): run_case allocates no more and checks the
    sentinels behind it.  Streaming kernel (bf16, 128 < Lk <= 256) at 1 and 7 rows and where its persistent waves use
    both ring slots and refill one for a ragged third pass; aligned and unaligned short rows; a row stride wider than
    the instantiation (Lk 100 in ld 512: columns [100, 128) are 0, [128, 512) stay untouched)."""
    if rows == STREAM_TRIPS:
        assert R.softmax_kernel_name(dtype, ld, Lk) == "softmax_fwd_stream_kernel<2>"
        assert (rows + 3) // 4 == 2 * 4096 + 2   # row groups: both ring slots of all 4096 waves, then two more
    run_case(f"last row {Lk}/{ld} rows {rows}", dtype, rows, 1, Lk, ld, heads=1)
    _report("last row")


# ------------------------------------------------------------------------------------------ row independence

@pytest.mark.parametrize("Lk,ld,u", [(24, 24, 4), (200, 208, 0)], ids=["u4", "stream"])
def test_softmax_rows_are_independent(Lk, ld, u, tuning):
    """rows permuted within each (b, h): p permutes bit for bit; one row of NaN scores: that row is NaN, every other
    row keeps its bits (rows share a wave: 4 or 16 of them, 4 lane groups x U)"""
    tuning("softmax_u", u)
    nbh, Lq = 6, 9
    rows = nbh * Lq
    x = R.softmax_scores(rows, Lk, 11)
    base = run_case(f"independence Lk {Lk}", B16, nbh, Lq, Lk, ld, u, scores=x).values()
    perm = torch.randperm(Lq, generator=torch.Generator().manual_seed(Lk))
    full = (torch.arange(nbh)[:, None] * Lq + perm[None, :]).reshape(-1)

    def fwd(scores):
        s, p = Buf(rows, Lk, ld, B16, scores), Buf(rows, Lk, ld, B16)
        sm_fwd(s, p, None, nbh, 3, Lq, Lk, ld, B16)
        return p.values()
    assert R.same_bits(fwd(x[full]), base[full])
    xn = x.clone()
    xn[22] = float("nan")
    got = fwd(xn)
    keep = torch.arange(rows) != 22
    assert bool(torch.isnan(got[22].float()).all())
    assert R.same_bits(got[keep], base[keep])
