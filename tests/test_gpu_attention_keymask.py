"""asrx_attention_fwd / asrx_attention_bwd under key-validity masks at any key count, validity stride and base,
called below blocks.attn_fwd (asrx.kernels.attention_fwd / attention_bwd), row by row against float64.

The cases, the profiles tail_spike (forward) and tail_pair (backward) and why they see a dropped or a leaked key are
in tests/attn_keymask_ref.py; tests/test_attention_keymask_cpu.py proves, without a GPU, that the clipped validity
word of DESIGN.md §18 and a leaked dead key break the bounds used here.  Bounds are the peaked file's FWD_TOL, LSE_TOL
(per row) and BWD_TOL (per (b, h)); outputs are pre-filled with NaN by run_fwd / run_bwd.

Layouts of the validity bytes (each a view into a larger uint8 buffer, 8 spare bytes before row 0 and after the last):
  tight     rows Lk bytes apart (Lk % 4 != 0: rows off a word boundary, the kernels that read bytes one by one)
  padded    rows ceil4(Lk) + 4 apart from a word-aligned base (what kernels.length_mask allocates, plus a word): the
            streamed forward and the kernels of the table in attn_keymask_ref.SHAPES
  offset1-3 the tight layout starting 1, 2, 3 bytes into the buffer
Live keys are marked 1, 2, 0x80 or 0xFF (the header's contract: == 0 is invalid).  Every forward runs with all bytes
outside the rows' [0, Lk) at 0x00 and at 0xFF: o and lse are bit-identical, and each passes check_fwd.
"""
import pytest
import torch

import attn_keymask_ref as M
import test_gpu_attention_peaked as P
from test_gpu_attention_peaked import _need_gpu, _stop_after_gpu_fault, attn_variant  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

dev = P.dev
DH, D, B, H = M.DH, M.D, M.B, M.H
LIVE_CODES = torch.tensor([1, 2, 0x80, 0xFF], dtype=torch.uint8)


def valid_view(valid, layout, fill):
    """(device uint8 view [B, Lk], row stride) of the validity bytes in `layout`, every other byte of the buffer `fill`."""
    Lk = valid.shape[1]
    stride = (Lk + 3) // 4 * 4 + 4 if layout == "padded" else Lk
    start = 8 + (int(layout[-1]) if layout.startswith("offset") else 0)
    buf = torch.full((start + B * stride + 8,), fill, dtype=torch.uint8)
    codes = LIVE_CODES[(torch.arange(Lk)[None, :] * 5 + torch.arange(B)[:, None]) % 4]
    buf.as_strided((B, Lk), (stride, 1), start).copy_(torch.where(valid, codes, torch.zeros_like(codes)))
    view = buf.to(dev).as_strided((B, Lk), (stride, 1), start)
    assert (view.data_ptr() - start) % 256 == 0          # the buffer's base is aligned: `start` decides the rows'
    return view, stride


def spec_of(valid, layout, form, fill=0):
    from asrx.kernels import MaskSpec
    view, stride = valid_view(valid, layout, fill)
    return MaskSpec(1, True, view, view, stride) if form == "decoder" else MaskSpec(1, False, view, None, stride)


def case_params(layouts_of):
    return [pytest.param(c[1], *c[2:], lay, id=f"{c[0]}-{lay}") for c in M.CASES for lay in layouts_of(c)]


def fwd_layouts(c):
    offs = ["offset1", "offset2", "offset3"] if c[0].startswith(("self-249-", "cross-16x257-")) else []
    return ["tight", "padded"] + offs


def bwd_layouts(c):
    """tight, as the case table asks; past 256 keys in padded too: rows Lk apart are off the word boundary at every
    Lk of the table, and such a call takes the tiled pair — the key-block backward is reached from aligned rows."""
    return ["tight"] + (["padded"] if c[3] > 256 else [])


@pytest.mark.parametrize("attn_variant,Lq,Lk,form,n,drop,layout", case_params(fwd_layouts), indirect=["attn_variant"])
def test_keymask_forward(attn_variant, Lq, Lk, form, n, drop, layout, request):
    qb, kvb, valid, ref = M.reference("tail_spike", Lq, Lk, n, form, drop)
    runs = [P.run_fwd(qb, kvb, DH, spec_of(valid, layout, form, fill), drop) for fill in (0x00, 0xFF)]
    for fill, run in zip(("00", "ff"), runs):
        P.check_fwd(f"{request.node.callspec.id} outside bytes {fill}", run, ref)
    assert torch.equal(runs[0]["o"], runs[1]["o"]) and torch.equal(runs[0]["lse"], runs[1]["lse"])


def fwd_bwd(qb, kvb, spec, ref, dOb, drop):
    run = P.run_fwd(qb, kvb, DH, spec, drop, with_lo=drop)   # dropout carries o_lo, as a training step does
    return run, dict(zip(("dQ", "dK", "dV"), P.run_bwd(run, ref, DH, dOb)))


@pytest.mark.parametrize("attn_variant,Lq,Lk,form,n,drop,layout", case_params(bwd_layouts), indirect=["attn_variant"])
def test_keymask_backward(attn_variant, Lq, Lk, form, n, drop, layout, request):
    qb, kvb, valid, ref, dOb, refs = M.bwd_reference(Lq, Lk, n, form, drop)
    run, got = fwd_bwd(qb, kvb, spec_of(valid, layout, form), ref, dOb, drop)
    P.check_fwd(request.node.callspec.id, run, ref)
    errs = M.grad_errors(got, refs, n)
    print(f"keymask bwd {request.node.callspec.id}: per-head err / max|ref| " +
          ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" (bound {P.BWD_TOL:g})")
    dead = (~valid)[:, None, :].expand(B, H, Lk)
    for name in refs:
        assert bool(torch.isfinite(got[name]).all()), name
        assert errs[name] <= P.BWD_TOL, (name, errs[name])
    assert bool((got["dK"][dead] == 0).all()) and bool((got["dV"][dead] == 0).all())   # §18's contract: exactly zero


def assert_same_bits(name, x, y):
    """torch.equal with the first differing positions in the message (NaN differs from itself: outputs are finite)."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    diff = (x != y) | torch.isnan(x) | torch.isnan(y)
    where = diff.nonzero()[:6].tolist()
    assert not bool(diff.any()), (name, int(diff.sum()), where, [(float(x[tuple(i)]), float(y[tuple(i)])) for i in where])


INVARIANCE = [(Lq, Lk, form, n) for Lq, Lk, form in [(249, 249, "keys"), (386, 386, "keys"), (16, 257, "keys"),
                                                     (249, 249, "decoder"), (386, 386, "decoder"),
                                                     (100, 100, "decoder")]   # (the last: attn_fwd_res_kernel<1>)
              for n in M.lengths_of(Lk, form)]


@pytest.mark.parametrize("Lq,Lk,form,n", [pytest.param(*c, id=f"{c[0]}x{c[1]}-{c[2]}-n{c[3][0]}_{c[3][1]}")
                                          for c in INVARIANCE])
def test_keymask_padding_invariance(Lq, Lk, form, n):
    """Other finite garbage (1e3 * randn) in the K / V rows of dead keys — and, in the decoder's form, in the Q rows of
    dead queries — changes no bit of o, lse, dQ and the live rows of dK / dV; the dead rows stay exactly zero.
    (Found by this test at (386, 386) with lengths (384, 193): the forwards' lazy rescale was decided per wave, so
    the garbage of dead queries 193 .. 223 moved the reference maximum of live query 192 and with it the bf16
    rounding of its probabilities, 45 elements of one row by an ulp.  The decision is per row now.)"""
    qb, kvb, valid, ref, dOb, _ = M.bwd_reference(Lq, Lk, n, form, False)
    g = torch.Generator().manual_seed(Lq + Lk + n[0])
    kv2, q2 = kvb.clone(), qb.clone()
    kv2[~valid] = (1e3 * torch.randn(int((~valid).sum()), 2 * D, generator=g)).bfloat16()
    if form == "decoder":
        q2[~valid] = (1e3 * torch.randn(int((~valid).sum()), D, generator=g)).bfloat16()
    assert bool((~valid).any())
    r1, g1 = fwd_bwd(qb, kvb, spec_of(valid, "padded", form), ref, dOb, False)
    r2, g2 = fwd_bwd(q2, kv2, spec_of(valid, "padded", form), ref, dOb, False)
    assert bool(torch.isfinite(r1["o"].float()).all())
    assert_same_bits("o", r1["o"].view(B, Lq, D), r2["o"].view(B, Lq, D))
    assert_same_bits("lse", r1["lse"].view(B, H, Lq), r2["lse"].view(B, H, Lq))
    assert_same_bits("dQ", g1["dQ"], g2["dQ"])
    live = valid[:, None, :].expand(B, H, Lk)
    for name in ("dK", "dV"):
        assert_same_bits(name, g1[name][live], g2[name][live])
        assert bool((g1[name][~live] == 0).all()) and bool((g2[name][~live] == 0).all()), name


@pytest.mark.parametrize("L", [249, 274])
def test_blocks_attn_fwd_keeps_key_masks_fused(L):
    """The model's own path: kernels.length_mask's validity rows (a multiple of 4 bytes apart) under MaskSpec.keys go
    to the fused kernels at key counts that are no multiple of 4, and the result is the reference's."""
    from asrx import blocks, kernels
    n = (L, L - 1)
    qb, kvb, valid, ref = M.reference("tail_spike", L, L, n, "keys", False)
    _, dvalid = kernels.length_mask(torch.tensor(n, dtype=torch.int32, device=dev), L)
    assert torch.equal(dvalid.cpu().bool(), valid)
    spec = kernels.MaskSpec.keys(dvalid)
    assert spec.valid_bstride % 4 == 0 and dvalid.data_ptr() % 4 == 0
    C = blocks.Ctx(None, torch.bfloat16, False, 0.0, blocks.Seeds(1))
    qd, kvd = qb.to(dev), kvb.to(dev)
    o = torch.full((B * L, D), float("nan"), device=dev, dtype=torch.bfloat16)
    S = blocks.attn_fwd(C, qd, kvd, kvd[..., D:], o, B, H, L, L, DH, P.strides(L, L, D), D ** -0.5, spec)
    assert S["impl"] == "fused"
    P.check_fwd(f"blocks.attn_fwd keys {L}", {"o": o, "lse": S["lse"]}, ref)
