"""Fused attention (and the unfused softmax) on PEAKED score rows, checked row by row against float64.

Every other attention test draws q, k, v from randn with the model's scale d_model**-0.5: the log2-domain scores then
spread by about one unit, every softmax row is flat, and the online softmax's rescale, the short-query kernel's
cross-wave combine, the saved lse and the masking of large scores cannot show an error.  Here Q and K are built so
that their scaled product follows a prescribed profile (tens of log2 units between keys, the regime of a trained
alignment), the profile's preconditions are asserted on the float64 scores of the bf16-rounded operands, and output
and lse are compared per row and head.

Profiles (log2 units; a "tile" is 32 keys, the forwards' key tile):
  ramp_small    the tile maximum rises by 3 .. 7 per tile: accumulation against a stale maximum, a rescale now and then
  ramp_big      rise of 12 .. 16 per tile: a rescale with alpha << 1 on every tile
  threshold     rises alternating under / over 8: the lazy-rescale compare itself
  descending    fall of 6 .. 8 per tile: no rescale after tile 0, the tail underflows
  last_key      flat, key Lk - 1 raised by 30: the last valid key next to the padding of the tail tile
  row_spike     query q raised at key (7 q + 3) % Lk: rows of one wave rescale at different tiles; key indexing
  all_negative  every score <= -30: a phantom key past Lk (score 0) would take the row
  quarter_skew  the four 64-key quarters at 0 / -25 / +25 / -50 (rotated per head): the kq kernel's combine weights
  shared_top    (backward) 2 - 3 keys within 1 unit hold >= 0.999 of a row, the rest >= 25 below: dS is not ~0
Masks hide scores >= 20 above every live score of their row (exact integer codes in the leading dimensions).

Which kernels asrx_attention_fwd / asrx_attention_bwd launch for each case of FWD_CASES and BWD_CASES below (B = H = 2)
is the table PEAKED_FWD / PEAKED_BWD of tests/test_attn_plan_table.py, asserted there on the CPU through
asrx_attn_kernel_name together with "every instantiation is reached by some case".  Mode 1 here has L = 300, a multiple
of 4, Lq == Lk and validity rows L bytes apart; key-only masks with Lq != Lk, key counts that are no multiple of 4 on
either side of 256, validity rows at other strides and bases, and the backward under a key-only mask are
tests/test_gpu_attention_keymask.py's, with this file's Ref, check_fwd, run_fwd / run_bwd and bounds.

Bounds: per (b, h, q) max_d |O - ref| <= 1e-2 max |V(b, h)| (the project's forward bound, per row and head);
|lse - log2 sum 2^s| <= 1e-3 on live rows, lse = +inf and an exactly zero output on fully masked rows; per (b, h)
max |g - ref| <= 2e-2 max |ref(b, h)| for dQ, dK, dV.
"""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
B, H = 2, 2
LN2 = math.log(2.0)
P_DROP, SEED = 0.3, 4321
FWD_TOL, LSE_TOL, BWD_TOL = 1e-2, 1e-3, 2e-2
NEG = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


@pytest.fixture(autouse=True)
def _stop_after_gpu_fault():
    """A device fault ends the module: nothing more is launched on a GPU that has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def K():
    from asrx import kernels
    return kernels


@pytest.fixture
def attn_variant(request):
    """ASRX_ATTN_KERNEL for one test: auto (the dispatch's choice) / tiled / resident."""
    old = os.environ.get("ASRX_ATTN_KERNEL")
    os.environ["ASRX_ATTN_KERNEL"] = request.param
    yield request.param
    if old is None:
        os.environ.pop("ASRX_ATTN_KERNEL", None)
    else:
        os.environ["ASRX_ATTN_KERNEL"] = old


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


def scale2_of(dh):
    """log2-domain score scale of the kernels: d_model**-0.5 * log2(e)."""
    return (H * dh) ** -0.5 / LN2


# ------------------------------------------------------------------------------------------------ score profiles

def _row_gain(Lq):
    return 1.0 + 0.03 * ((torch.arange(Lq, dtype=torch.float64) * 5) % 7) / 7


def _row_offset(Lq, idx):
    return ((torch.arange(Lq, dtype=torch.float64) * 3) % 5) - 2.0 + 2.0 * idx - 3.0


def n_tiles(Lk):
    return (Lk + 31) // 32


def profile_applies(profile, Lq, Lk):
    """Profiles whose precondition cannot hold at a key length are left out there (too few 32-key tiles)."""
    nt = n_tiles(Lk)
    return {"ramp_small": nt >= 4, "ramp_big": nt >= 2, "threshold": nt >= 3, "descending": nt >= 2,
            "last_key": Lk >= 2, "row_spike": Lk > 32, "all_negative": True,
            "quarter_skew": 64 < Lk <= 256, "shared_top": Lk >= 8}[profile]


def target(profile, idx, Lq, Lk):
    """Target log2-domain scores T[q][key] of head idx = b * H + h (low rank: a few outer products)."""
    tile = (torch.arange(Lk) // 32).double()
    nt = n_tiles(Lk)
    gain = _row_gain(Lq)[:, None]
    if profile == "ramp_small":      # rises in (0, 8), total above 16
        rise = max(3.0, 19.0 / (nt - 1)) * (1 + 0.03 * idx)
        T = gain * rise * (tile - (nt - 1) / 2)[None, :]
    elif profile == "ramp_big":
        T = gain * (12.0 + idx) * (tile - (nt - 1) / 2)[None, :]
    elif profile == "threshold":     # rises 6.5, 9.5, 6.5, ...
        steps = torch.tensor([0.0] + [6.5 if i % 2 == 0 else 9.5 for i in range(nt - 1)], dtype=torch.float64)
        lvl = torch.cumsum(steps, 0) * (1 + 0.02 * idx)
        T = gain * (lvl - lvl[-1] / 2)[tile.long()][None, :]
    elif profile == "descending":
        T = -gain * (6.0 + 0.5 * idx) * tile[None, :]
    elif profile == "last_key":
        T = torch.zeros(Lq, Lk, dtype=torch.float64)
        T[:, Lk - 1] = 30.0 + idx
    elif profile == "all_negative":
        return torch.full((Lq, Lk), -40.0 - 3.0 * idx, dtype=torch.float64) - ((torch.arange(Lq) * 3) % 5).double()[:, None]
    elif profile == "quarter_skew":
        lv = torch.tensor([0.0, -25.0, 25.0, -50.0], dtype=torch.float64).roll(idx)
        T = (1 + 0.05 * ((torch.arange(Lq) * 5) % 7).double() / 7)[:, None] * lv[(torch.arange(Lk) // 64)][None, :]
    else:
        raise KeyError(profile)
    return T + _row_offset(Lq, idx)[:, None]


def shared_top_groups(Lq, Lk, causal):
    """(group, rows, top keys).  Without a causal mask group g = q % 4 and its keys lie in the first 128-key block,
    the middle and the last (partial) tile; with one, groups are query ranges and their keys lie below the range
    (range 0 has no visible key to share and stays flat)."""
    G = 4
    q = torch.arange(Lq)
    out = []
    for g in range(G):
        if causal:
            s = g * Lq // G
            rows = (q >= s) & (q < (g + 1) * Lq // G)
            keys = sorted({min(g, s - 1), s // 2, s - 1}) if s >= 3 else []
        else:
            rows = (q % G) == g
            keys = sorted({(5 + 2 * g) % Lk, (Lk // 2 + 5 * g) % Lk, Lk - 1 - 3 * g})
        if len(keys) >= 2 and bool(rows.any()):
            out.append((g, rows, keys))
    return out


def qk_from_target(T, scale2, dh, g, first=0, k_norm=None):
    """Q [Lq, dh], K [Lk, dh] (float64, rounded to bf16 by the caller) with Q K^T * scale2 ~ T: the SVD factors
    U sqrt(S), V sqrt(S) of T / scale2 in dimensions first .. dh - 9, randn in the last 8 (rows are not exactly
    collinear).  k_norm (the backward cases): K = V c, Q = U S / c instead, c such that the longest K row has that
    norm.  The keys that share a row's mass then differ by about as much as they have in common; with the balanced
    split they are one long common vector plus the 8 random dimensions, dQ = sum_key dS K cancels to a small
    remainder (sum_key dS = 0) and measures the bf16 rounding of dS against |K|, not the softmax."""
    Lq, Lk = T.shape
    Q = torch.zeros(Lq, dh, dtype=torch.float64)
    Kk = torch.zeros(Lk, dh, dtype=torch.float64)
    U, S, Vh = torch.linalg.svd(T / scale2, full_matrices=False)
    n = min(dh - 8 - first, S.numel())
    if k_norm is None:
        Q[:, first:first + n] = U[:, :n] * S[:n].sqrt()
        Kk[:, first:first + n] = Vh[:n].T * S[:n].sqrt()
    else:
        c = k_norm / float(Vh[:n].T.norm(dim=1).max())
        Q[:, first:first + n] = U[:, :n] * S[:n] / c
        Kk[:, first:first + n] = Vh[:n].T * c
    Q[:, dh - 8:] = torch.randn(Lq, 8, generator=g, dtype=torch.float64)
    Kk[:, dh - 8:] = torch.randn(Lk, 8, generator=g, dtype=torch.float64)
    return Q, Kk


def qk_shared_top(Lq, Lk, dh, g, scale2, causal, idx):
    """shared_top is full rank (the shared keys change from row to row), so like row_spike it starts from random keys:
    the shared keys are randn rows, every other key randn / 4, and the rows of a group get the shortest Q that scores
    its shared keys at S + (0, 0.25, -0.15) log2 units and the other groups' shared keys at 0, S from the largest
    score that Q gives any other key (31 units below), plus randn * 3 made orthogonal to all shared keys (it moves
    the other keys' scores by up to ~4 units).  Without that part the rows of a group are one common vector, dK of a
    shared key is (sum_q dS) times it, and a head where those sums happen to cancel measures the bf16 rounding of P
    and dS, not the softmax: a float64 emulation with only P, dS and O rounded to bf16 gave 2.4e-2 for such a head."""
    groups = shared_top_groups(Lq, Lk, causal)
    Kk = torch.randn(Lk, dh, generator=g, dtype=torch.float64) * 0.25
    for _, rows, keys in groups:
        Kk[keys] = torch.randn(len(keys), dh, generator=g, dtype=torch.float64)
    Kk = Kk.bfloat16().double()
    Q = torch.randn(Lq, dh, generator=g, dtype=torch.float64) * 0.3
    gain = _row_gain(Lq)
    allk = [key for _, _, keys in groups for key in keys]
    Ka = Kk[allk]
    Ginv = torch.linalg.inv(Ka @ Ka.T)
    for _, rows, keys in groups:
        own = torch.tensor([key in keys for key in allk])
        lv = torch.zeros(len(allk), dtype=torch.float64)
        lv[own] = torch.tensor([0.0, 0.25, -0.15][:len(keys)], dtype=torch.float64) + 0.1 * idx
        x1 = Ka.T @ (Ginv @ own.double())          # scores 1 on the group's keys, 0 on the other groups' keys
        xl = Ka.T @ (Ginv @ (lv / scale2))
        other = Kk @ x1
        other[allk] = 0.0
        s_raw = (31.0 / scale2) / (1.0 - float(other.max()))
        noise = torch.randn(int(rows.sum()), dh, generator=g, dtype=torch.float64) * 3.0
        noise = noise - (noise @ Ka.T) @ (Ginv @ Ka)
        Q[rows] = gain[rows][:, None] * (s_raw * x1)[None, :] + xl[None, :] + noise
    return Q, Kk


def spike_key(q, Lk, causal):
    return (7 * q + 3) % ((q + 1) if causal else Lk)


def qk_row_spike(Lq, Lk, dh, g, scale2, causal):
    """K random, Q[q] = beta K[j(q)] / |K[j(q)]| with beta from the smallest gap between |K[j]| and the other keys'
    projections on K[j], for a score gap of 25 log2 units."""
    Kk = torch.randn(Lk, dh, generator=g, dtype=torch.float64).bfloat16().double()
    j = torch.tensor([spike_key(q, Lk, causal) for q in range(Lq)])
    unit = Kk[j] / Kk[j].norm(dim=1, keepdim=True)
    proj = unit @ Kk.T
    top = proj.gather(1, j[:, None])
    proj.scatter_(1, j[:, None], NEG)
    if causal:
        proj = proj.masked_fill(torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1), NEG)
    gap = (top - proj.amax(1, keepdim=True)).clamp_max(1e9)
    live = torch.isfinite(gap)
    beta = 25.0 / (scale2 * float(gap[live].min())) if bool(live.any()) else 1.0
    return unit * beta, Kk


@functools.lru_cache(maxsize=None)
def make_qkv(profile, Lq, Lk, dh, causal, k_norm=None):
    """bf16 q [B, Lq, H dh], kv [B, Lk, 2 H dh] (K | V) following `profile`; V of head idx is scaled by 2^(idx - 1),
    so a per-head bound is tighter than the global one for three heads of four."""
    d = H * dh
    g = torch.Generator().manual_seed(sum(map(ord, profile)) * 1000003 + Lq * 4099 + Lk * 17 + dh + int(causal))
    sc2 = scale2_of(dh)
    q = torch.zeros(B, Lq, H, dh, dtype=torch.float64)
    k = torch.zeros(B, Lk, H, dh, dtype=torch.float64)
    v = torch.zeros(B, Lk, H, dh, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            idx = b * H + h
            if profile == "row_spike":
                Q, Kk = qk_row_spike(Lq, Lk, dh, g, sc2, causal)
            elif profile == "shared_top":
                Q, Kk = qk_shared_top(Lq, Lk, dh, g, sc2, causal, idx)
            else:
                Q, Kk = qk_from_target(target(profile, idx, Lq, Lk), sc2, dh, g, k_norm=k_norm)
            q[b, :, h], k[b, :, h] = Q, Kk
            v[b, :, h] = torch.randn(Lk, dh, generator=g, dtype=torch.float64) * 2.0 ** (idx - 1)
    qb = q.reshape(B, Lq, d).bfloat16()
    kvb = torch.cat([k.reshape(B, Lk, d), v.reshape(B, Lk, d)], -1).bfloat16()
    return qb, kvb


# ------------------------------------------------------------------------------------------------ reference

class Ref:
    """float64 attention on the bf16-rounded operands: s2 (unmasked log2 scores), p, out, lse (log2; -inf = dead)."""

    def __init__(self, qb, kvb, dh, masked, keep=None, grad=False):
        Bq, Lq, d = qb.shape
        Lk = kvb.shape[1]
        self.Lq, self.Lk, self.dh = Lq, Lk, dh
        self.qh = qb.double().view(B, Lq, H, dh).transpose(1, 2).contiguous().requires_grad_(grad)
        self.kh = kvb[..., :d].double().reshape(B, Lk, H, dh).transpose(1, 2).contiguous().requires_grad_(grad)
        self.vh = kvb[..., d:].double().reshape(B, Lk, H, dh).transpose(1, 2).contiguous().requires_grad_(grad)
        s2 = (self.qh @ self.kh.transpose(-1, -2)) * scale2_of(dh)
        self.masked = masked.expand(B, H, Lq, Lk)
        sm = s2.masked_fill(self.masked, NEG)
        self.s2 = s2.detach()
        self.sm = sm.detach()
        self.lse = torch.logsumexp(self.sm * LN2, -1) / LN2
        p = torch.nan_to_num(torch.softmax(sm * LN2, -1))
        self.p = p.detach()
        self.out = (p if keep is None else p * keep) @ self.vh
        self.vmax = self.vh.detach().abs().amax((-1, -2))   # [B, H]


def no_mask(Lq, Lk):
    return torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)


def decoder_valid(L):
    """Batch 0 ends in L // 4 padded positions, batch 1 is full."""
    valid = torch.ones(B, L)
    valid[0, L - L // 4:] = 0
    return valid


def decoder_masked(valid, Lq, Lk):
    pad = valid[:, :Lk].lt(1).unsqueeze(1).expand(-1, Lq, -1)
    qpad = valid[:, :Lq].lt(1).unsqueeze(2).expand(-1, -1, Lk)
    return (pad | qpad | torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)).unsqueeze(1)


def mask_and_spec(kind, Lq, Lk):
    from asrx.kernels import MaskSpec
    if kind == "none":
        return no_mask(Lq, Lk), MaskSpec()
    valid = decoder_valid(Lq)
    masked = decoder_masked(valid, Lq, Lk)
    if kind == "decoder":
        return masked, MaskSpec.decoder(valid.to(dev))
    return masked, MaskSpec.from_attention_mask(masked[:, 0].to(dev), B, Lq, Lk)   # "dense"


def keep_of(Lq, Lk, drop):
    if not drop:
        return None
    from rng_ref import attn_keep
    return torch.from_numpy(attn_keep(SEED, B * H, Lq, Lk, P_DROP)).view(B, H, Lq, Lk).double() / (1 - P_DROP)


# ------------------------------------------------------------------------------------------------ preconditions

def tile_rises(s2):
    """Tile-to-tile rise of the row maximum over 32-key tiles, [..., nt - 1]."""
    Lk = s2.shape[-1]
    nt = n_tiles(Lk)
    pad = torch.full(s2.shape[:-1] + (nt * 32 - Lk,), NEG, dtype=s2.dtype)
    tm = torch.cat([s2, pad], -1).view(*s2.shape[:-1], nt, 32).amax(-1)
    return tm[..., 1:] - tm[..., :-1]


def check_profile(profile, ref, causal=False):
    """The profile's precondition on the reference's own scores (conditions, not measurements)."""
    s2, Lq, Lk = ref.s2, ref.Lq, ref.Lk
    p_un = torch.softmax(s2 * LN2, -1)
    if profile == "ramp_small":
        r = tile_rises(s2)
        assert bool(((r > 0) & (r < 8)).all()), (float(r.min()), float(r.max()))
        assert float(r.sum(-1).min()) > 16
    elif profile == "ramp_big":
        assert float(tile_rises(s2).min()) > 8
    elif profile == "threshold":
        r = tile_rises(s2)
        assert bool((r < 8).any(-1).all()) and bool((r > 8).any(-1).all())
        assert float(r.min()) > 0
    elif profile == "descending":
        assert float(tile_rises(s2).max()) < 0
    elif profile == "last_key":
        assert float(p_un[..., Lk - 1].min()) >= 0.999
    elif profile == "row_spike":
        j = torch.tensor([spike_key(q, Lk, causal) for q in range(Lq)])
        pj = (p_un if not causal else ref.p).gather(-1, j.view(1, 1, Lq, 1).expand(B, H, Lq, 1))[..., 0]
        live = ref.lse > NEG
        assert float(pj[live].min()) >= 0.999
        top2 = s2.masked_fill(ref.masked if causal else torch.zeros_like(ref.masked), NEG).topk(2, -1).values
        assert float((top2[..., 0] - top2[..., 1])[live & (torch.arange(Lq) > 0 if causal else live)].min()) >= 20
        if not causal:   # the spiked keys of one 16-query sub-tile fall into different key tiles
            for q0 in range(0, Lq - 4, 16):
                assert len({int(t) // 32 for t in j[q0:q0 + 16]}) >= 2
    elif profile == "all_negative":
        assert float(s2.max()) <= -30
    elif profile == "quarter_skew":
        qm = [s2[..., 64 * i:64 * (i + 1)] for i in range((Lk + 63) // 64)]
        lv = torch.stack([x.amax(-1) for x in qm], -1).sort(-1).values
        lo = torch.stack([x.amin(-1) for x in qm], -1)
        hi = torch.stack([x.amax(-1) for x in qm], -1)
        assert float((lv[..., 1:] - lv[..., :-1]).min()) >= 20          # quarter levels 20 apart ...
        assert float((hi - lo).max()) < 10                               # ... each quarter well inside its level
    elif profile == "shared_top":
        for grp, rows, keys in shared_top_groups(Lq, Lk, causal):
            live = rows[None, None, :] & (ref.lse > NEG)
            pk = ref.p[..., keys]
            assert float(pk.sum(-1)[live].min()) >= 0.999
            sk = ref.sm[..., keys]
            assert float((sk.amax(-1) - sk.amin(-1))[live].max()) <= 1.0
            rest = ref.sm.clone()
            rest[..., keys] = NEG
            assert float((sk.amin(-1) - rest.amax(-1))[live].min()) >= 25
    else:
        raise KeyError(profile)


# ------------------------------------------------------------------------------------------------ GPU runs

def strides(Lq, Lk, d):
    return ((d, Lq * d), (2 * d, Lk * 2 * d), (2 * d, Lk * 2 * d), (d, Lq * d))


def run_fwd(qb, kvb, dh, spec, drop=False, keep_words=True, with_lo=False):
    Lq, Lk, d = qb.shape[1], kvb.shape[1], H * dh
    qd, kvd = qb.to(dev), kvb.to(dev)
    o = torch.full((B * Lq, d), float("nan"), device=dev, dtype=torch.bfloat16)
    o_lo = torch.empty_like(o) if with_lo else None
    dm = K().dropmask_buffer(B, H, Lq, Lk, dh, P_DROP, dev) if (drop and keep_words) else None
    lse = K().attention_fwd(qd, kvd, kvd[..., d:], o, B, H, Lq, Lk, dh, strides(Lq, Lk, d), d ** -0.5, spec,
                            P_DROP if drop else 0.0, SEED, dropmask=dm, o_lo=o_lo)
    return dict(qd=qd, kvd=kvd, o=o, o_lo=o_lo, dm=dm, lse=lse, spec=spec, drop=drop)


def check_fwd(tag, run, ref):
    """Per-row output error against max |V(b, h)|, lse on live rows, exact zeros / +inf on dead rows."""
    Lq, dh = ref.Lq, ref.dh
    out = run["o"].float().cpu().view(B, Lq, H, dh).transpose(1, 2).double()
    lse = run["lse"].cpu().view(B, H, Lq).double()
    live = ref.lse > NEG
    row_err = (out - ref.out.detach()).abs().amax(-1) / ref.vmax[:, :, None]
    lse_err = (lse - ref.lse).abs()[live]
    e_out = float(row_err.max())
    e_lse = float(lse_err.max()) if lse_err.numel() else 0.0
    print(f"peaked fwd {tag}: row err / max|V| {e_out:.3e} (bound {FWD_TOL:g}), lse err {e_lse:.3e} "
          f"(bound {LSE_TOL:g}), dead rows {int((~live).sum())}")
    assert bool(torch.isfinite(out).all())
    assert e_out <= FWD_TOL
    assert e_lse <= LSE_TOL
    if bool((~live).any()):
        assert bool((lse[~live] == float("inf")).all())
        assert bool((out[~live] == 0).all())


def run_bwd(run, ref, dh, dOb, keep_words=True):
    Lq, Lk, d = ref.Lq, ref.Lk, H * dh
    dq = torch.full((B * Lq, d), float("nan"), device=dev, dtype=torch.bfloat16)
    dkv = torch.full((B * Lk, 2 * d), float("nan"), device=dev, dtype=torch.bfloat16)
    gst = ((d, Lq * d), (d, Lq * d), (2 * d, Lk * 2 * d), (2 * d, Lk * 2 * d))
    K().attention_bwd(run["qd"], run["kvd"], run["kvd"][..., d:], run["o"], run["lse"], dOb.to(dev), dq, dkv,
                      dkv[:, d:], B, H, Lq, Lk, dh, strides(Lq, Lk, d), gst, d ** -0.5, run["spec"],
                      P_DROP if run["drop"] else 0.0, SEED, dropmask=run["dm"] if keep_words else None,
                      o_lo=run["o_lo"])
    return (dq.float().cpu().view(B, Lq, H, dh).transpose(1, 2).double(),
            dkv[:, :d].float().cpu().view(B, Lk, H, dh).transpose(1, 2).double(),
            dkv[:, d:].float().cpu().view(B, Lk, H, dh).transpose(1, 2).double())


# ------------------------------------------------------------------------------------------------ 2. forward

PROFILES = ["ramp_small", "ramp_big", "threshold", "descending", "last_key", "row_spike", "all_negative",
            "quarter_skew"]

# (id, ASRX_ATTN_KERNEL, Lq, Lk, dh, mask, dropout, keep words) -> kernel: test_attn_plan_table.PEAKED_FWD
FWD_CASES = [
    ("kq-64x249", "auto", 64, 249, 64, "none", False, True),
    ("kq-5x17", "auto", 5, 17, 64, "none", False, True),
    ("kq-33x256", "auto", 33, 256, 64, "none", False, True),
    ("kq-64x100", "auto", 64, 100, 64, "none", False, True),
    ("kqdrop-64x249", "auto", 64, 249, 64, "none", True, True),
    ("res0-100x200", "resident", 100, 200, 64, "none", False, True),
    ("res0-249x249", "resident", 249, 249, 64, "none", False, True),
    ("res0drop-64x100", "auto", 64, 100, 64, "none", True, True),
    ("res0w8drop-249x249", "resident", 249, 249, 64, "none", True, True),
    ("res1-70x70", "auto", 70, 70, 64, "decoder", False, True),
    ("res1-33x33", "auto", 33, 33, 64, "decoder", False, True),
    ("res2-40x40", "auto", 40, 40, 64, "dense", False, True),
    ("stream0-57x1031", "auto", 57, 1031, 64, "none", False, True),
    ("stream0-300x300", "auto", 300, 300, 64, "none", False, True),
    ("stream0-64x257", "auto", 64, 257, 64, "none", False, True),
    ("stream0-100x200", "auto", 100, 200, 64, "none", False, True),
    ("stream0drop-57x1031", "auto", 57, 1031, 64, "none", True, True),
    ("stream0drop-300x300", "auto", 300, 300, 64, "none", True, True),
    ("stream1-300x300", "auto", 300, 300, 64, "decoder", False, True),
    ("stream1drop-300x300", "auto", 300, 300, 64, "decoder", True, True),
    ("tiled64-64x249", "tiled", 64, 249, 64, "none", False, True),
    ("tiled64-300x300", "tiled", 300, 300, 64, "none", False, True),
    ("tiled64drop-64x249", "auto", 64, 249, 64, "none", True, False),
    ("tiled64dense-300x300", "auto", 300, 300, 64, "dense", False, True),
    ("tiled32-64x249", "auto", 64, 249, 32, "none", False, True),
]

FWD_PARAMS = [pytest.param(c[1], *c[2:], prof, id=f"{c[0]}-{prof}") for c in FWD_CASES for prof in PROFILES
              if profile_applies(prof, c[2], c[3])]


@pytest.mark.parametrize("attn_variant,Lq,Lk,dh,mask,drop,keep_words,profile", FWD_PARAMS, indirect=["attn_variant"])
def test_attention_peaked_forward(attn_variant, Lq, Lk, dh, mask, drop, keep_words, profile, request):
    causal = mask != "none"
    qb, kvb = make_qkv(profile, Lq, Lk, dh, causal and profile == "row_spike")
    masked, spec = mask_and_spec(mask, Lq, Lk)
    ref = Ref(qb, kvb, dh, masked, keep_of(Lq, Lk, drop))
    check_profile(profile, ref, causal)
    run = run_fwd(qb, kvb, dh, spec, drop, keep_words)
    check_fwd(request.node.callspec.id, run, ref)


# ------------------------------------------------------------------------------------------------ 3. masks

G_RAISE = 320.0   # raw score step of the mask codes: 320 * scale2(dh = 64) = 40.8 log2 units (bf16-exact)


def coded_qkv(L, kind, g):
    """Q, K (dh = 64) whose masked positions score >= 20 log2 units above every live score of their row, and the
    boolean mask [B, 1, L, L].  The raise is an exact integer code in the leading dimensions (every factor is
    bf16-exact and every partial sum below 2^24, so the fp32 scores are exact); the live part is a gentle ramp (10
    units over the key range) in dimensions 32 .. 55 plus the random last 8.
      causal    raw = 320 (key - q) from key = 16 khi + klo, q = 16 qhi + qlo in four dimensions
      key_*     raw = 320 invalid[b][key]: trailing padding, leading padding (the first 64 keys of batch 0, 32 of batch
                1), one invalid key in the middle of a 128-key chunk
      irregular raw = 320 M[q % P][key % P], M random 30 %, P = min(L, 47): one dimension per residue"""
    dh, d = 64, H * 64
    sc2 = scale2_of(dh)
    q = torch.zeros(B, L, H, dh, dtype=torch.float64)
    k = torch.zeros(B, L, H, dh, dtype=torch.float64)
    v = torch.zeros(B, L, H, dh, dtype=torch.float64)
    ar = torch.arange(L)
    masked = torch.zeros(B, 1, L, L, dtype=torch.bool)
    invalid = torch.zeros(B, L, dtype=torch.bool)
    if kind == "causal":
        masked[:] = torch.triu(torch.ones(L, L, dtype=torch.bool), 1)
    elif kind == "key_trailing":
        invalid[0, L - L // 4:] = True
        invalid[1, L - 3:] = True
    elif kind == "key_leading":
        lead = 64 if L > 64 else L * 3 // 5   # (40 keys: the first 24 / 12, so that the sequence keeps live keys)
        invalid[0, :lead] = True
        invalid[1, :lead // 2] = True
    elif kind == "key_single":
        invalid[0, (L // 2) // 128 * 128 + min(64, L // 2) - 3] = True
        invalid[1, L - 1 - (L % 128) // 2] = True
    elif kind == "irregular":
        P = min(L, 47)
        M = torch.rand(B, P, P, generator=g) < 0.3
        M[:, ar[:P], ar[:P]] = False   # every row keeps a live key
        masked[:, 0] = M[:, ar % P][:, :, ar % P]
    if kind.startswith("key_"):
        masked[:] = invalid[:, None, None, :]
    # (the live part starts at dimension 32: every kernel multiplies dimensions 0 .. 31 first, so the integer code has
    #  cancelled exactly — to 0 on a causal row's diagonal, from terms near 10^5 — before a fraction is added to it)
    first = 47 if kind == "irregular" else 32
    ramp = 10.0 * (ar.double() / max(L - 1, 1))
    for b in range(B):
        for h in range(H):
            idx = b * H + h
            T = (1 + 0.1 * idx) * ramp[None, :].expand(L, L) + _row_offset(L, idx)[:, None]
            if kind == "irregular":
                T = torch.zeros(L, L, dtype=torch.float64)   # (no room beside 47 code dimensions: flat + jitter)
            Q, Kk = qk_from_target(T, sc2, dh, g, first=first)
            if kind == "irregular":
                Q[:, 47:56], Kk[:, 47:56] = 0, 0
                Q[:, :P] = G_RAISE * M[b][ar % P].double()
                Kk[:, :P] = torch.nn.functional.one_hot(ar % P, P).double()
            elif kind == "causal":
                Q[:, 0], Kk[:, 0] = 16 * G_RAISE, (ar // 16).double()
                Q[:, 1], Kk[:, 1] = G_RAISE, (ar % 16).double()
                Q[:, 2], Kk[:, 2] = -(16 * (ar // 16)).double(), G_RAISE
                Q[:, 3], Kk[:, 3] = -(ar % 16).double(), G_RAISE
            else:
                Q[:, 0], Kk[:, 0] = G_RAISE, invalid[b].double()
            q[b, :, h], k[b, :, h] = Q, Kk
            v[b, :, h] = torch.randn(L, dh, generator=g, dtype=torch.float64) * 2.0 ** (idx - 1)
    qb = q.reshape(B, L, d).bfloat16()
    kvb = torch.cat([k.reshape(B, L, d), v.reshape(B, L, d)], -1).bfloat16()
    return qb, kvb, masked, invalid


def check_hidden_scores(ref):
    """Every masked score is >= 20 log2 units above every live score of its row (rows with both kinds)."""
    hid = ref.s2.masked_fill(~ref.masked, float("inf")).amin(-1)
    live = ref.sm.amax(-1)
    both = torch.isfinite(hid) & torch.isfinite(live)
    assert bool(both.any())
    assert float((hid - live)[both].min()) >= 20


MASK_PARAMS = (
    [pytest.param(v, L, "causal", "vectors", id=f"{v}-{L}-causal-vectors") for v, L in
     [("auto", 33), ("auto", 70), ("auto", 300), ("tiled", 33), ("tiled", 70), ("tiled", 300)]] +
    [pytest.param(v, L, kind, "vectors", id=f"{v}-{L}-{kind}-vectors") for v, L in
     [("auto", 300), ("auto", 70), ("tiled", 300)] for kind in ["key_trailing", "key_leading", "key_single"]] +
    [pytest.param("auto", L, kind, "dense", id=f"auto-{L}-{kind}-dense") for L in [40, 300]
     for kind in ["causal", "key_trailing", "key_leading", "key_single", "irregular"]])


@pytest.mark.parametrize("attn_variant,L,kind,form", MASK_PARAMS, indirect=["attn_variant"])
def test_attention_masks_hide_largest_scores(attn_variant, L, kind, form, request):
    """A single unmasked position anywhere takes its row: auto = resident <1> / <2> up to 256 keys, streamed <1>
    (vectors) or tiled (dense) past that."""
    from asrx.kernels import MaskSpec
    g = torch.Generator().manual_seed(L * 31 + len(kind))
    qb, kvb, masked, invalid = coded_qkv(L, kind, g)
    ref = Ref(qb, kvb, 64, masked)
    check_hidden_scores(ref)
    if form == "dense":
        spec = MaskSpec.from_attention_mask(masked[:, 0].to(dev), B, L, L)
    elif kind == "causal":
        ones = torch.ones(B, L, dtype=torch.uint8, device=dev)
        spec = MaskSpec(1, True, ones, ones, ones.stride(0))
    else:
        kv = (~invalid).to(torch.uint8).to(dev)
        spec = MaskSpec(1, False, kv, None, kv.stride(0))
    check_fwd(request.node.callspec.id, run_fwd(qb, kvb, 64, spec), ref)


@pytest.mark.parametrize("attn_variant,L,form", [("auto", 70, "vectors"), ("auto", 300, "vectors"),
                                                 ("tiled", 300, "vectors"), ("auto", 40, "dense"),
                                                 ("auto", 300, "dense")], indirect=["attn_variant"])
def test_attention_invalid_queries_among_peaked_rows(attn_variant, L, form, request):
    """Invalid queries (no key of theirs is live) give an exactly zero row and lse = +inf while their neighbours in
    the same 16-query sub-tile are peaked (ramp_big) and live."""
    from asrx.kernels import MaskSpec
    qb, kvb = make_qkv("ramp_big", L, L, 64, False)
    qvalid = torch.ones(B, L, dtype=torch.bool)
    qvalid[0, [5, 17, 18, L - 1]] = False
    qvalid[1, [0, 31, 32]] = False
    masked = (~qvalid)[:, None, :, None].expand(B, 1, L, L)
    ref = Ref(qb, kvb, 64, masked)
    check_profile("ramp_big", ref)
    if form == "dense":
        spec = MaskSpec.from_attention_mask(masked[:, 0].to(dev), B, L, L)
    else:
        qv = qvalid.to(torch.uint8).to(dev)
        spec = MaskSpec(1, False, torch.ones_like(qv), qv, qv.stride(0))
    run = run_fwd(qb, kvb, 64, spec)
    check_fwd(request.node.callspec.id, run, ref)
    assert int((ref.lse == NEG).sum()) == 7 * H


@pytest.mark.parametrize("L", [40, 200, 300])
def test_attention_dense_mask_at_allocation_end(L):
    """The dense byte mask as the LAST bytes of its own device allocation (12 MiB: torch gives such a request a
    segment of exactly that size), L % 32 != 0.  The resident kernels' last query chunk covers rows up to 31 past Lq;
    the forward <2> and the backward <2, *> used to read mask bytes for them — for the last batch up to 31 L bytes
    past the end of the mask (found by this module: an illegal memory access at (40, 40) when the mask happened to
    end its segment).  Results equal those of an ordinary allocation bit for bit, and the reference.  L = 300 is the
    tiled pair of kernels, which always guarded the read."""
    from asrx.kernels import MaskSpec
    dh, d = 64, H * 64
    qb, kvb = make_qkv("shared_top", L, L, dh, True, K_NORM_BWD)
    masked = decoder_masked(decoder_valid(L), L, L)
    ref = Ref(qb, kvb, dh, masked)
    check_profile("shared_top", ref, True)
    dOb = torch.randn(B, L, d, generator=torch.Generator().manual_seed(L)).bfloat16()
    mb = masked[:, 0].to(torch.uint8).to(dev)

    def run(at_end):
        m = mb
        if at_end:
            m = torch.empty(12 << 20, device=dev, dtype=torch.uint8)[-mb.numel():].view_as(mb)
            m.copy_(mb)
        r = run_fwd(qb, kvb, dh, MaskSpec(2, dense=m, strides=tuple(m.stride())))
        grads = run_bwd(r, ref, dh, dOb)
        return r, grads

    r0, g0 = run(False)
    r1, g1 = run(True)
    check_fwd(f"dense-mask-at-end-{L}", r1, ref)
    assert torch.equal(r0["o"], r1["o"]) and torch.equal(r0["lse"], r1["lse"])
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. backward

K_NORM_BWD = 2.0   # longest K row of the SVD part in the backward's ramp_big inputs (see qk_from_target)

# (id, ASRX_ATTN_KERNEL, Lq, Lk, dh, mask, dropout, keep words, o_lo, profile)
BWD_CASES = [
    ("res0n2-64x64", "auto", 64, 64, 64, "none", False, True, False, "shared_top"),
    ("res0n4-64x100", "auto", 64, 100, 64, "none", False, True, False, "shared_top"),
    ("res0n8-64x249", "auto", 64, 249, 64, "none", False, True, False, "shared_top"),
    ("res0n8-64x249-drop", "auto", 64, 249, 64, "none", True, True, False, "shared_top"),
    ("res0n8-64x249-drop-lo", "auto", 64, 249, 64, "none", True, True, True, "shared_top"),
    ("res1n2-33x33", "auto", 33, 33, 64, "decoder", False, True, False, "shared_top"),
    ("res1n4-70x70", "auto", 70, 70, 64, "decoder", False, True, True, "shared_top"),
    ("res1n8-249x249", "auto", 249, 249, 64, "decoder", False, True, False, "shared_top"),
    ("res2n2-40x40", "auto", 40, 40, 64, "dense", False, True, False, "shared_top"),
    ("res2n4-100x100", "auto", 100, 100, 64, "dense", False, True, False, "shared_top"),
    ("res2n8-200x200", "auto", 200, 200, 64, "dense", False, True, False, "shared_top"),
    ("multi0-57x1031", "auto", 57, 1031, 64, "none", False, True, False, "shared_top"),
    ("multi0-57x1031-drop-lo", "auto", 57, 1031, 64, "none", True, True, True, "shared_top"),
    ("multi0-300x300", "auto", 300, 300, 64, "none", False, True, True, "shared_top"),
    ("multi0-300x300-drop", "auto", 300, 300, 64, "none", True, True, False, "shared_top"),
    ("multi0-300x300-ramp", "auto", 300, 300, 64, "none", False, True, False, "ramp_big"),
    ("multi1-300x300", "auto", 300, 300, 64, "decoder", False, True, False, "shared_top"),
    ("multi1-300x300-drop-lo", "auto", 300, 300, 64, "decoder", True, True, True, "shared_top"),
    ("multi1-300x300-ramp", "auto", 300, 300, 64, "decoder", False, True, False, "ramp_big"),
    ("tiled64-64x249", "tiled", 64, 249, 64, "none", False, True, False, "shared_top"),
    ("tiled64-300x300", "tiled", 300, 300, 64, "decoder", False, True, True, "shared_top"),
    ("tiled64-300x300-ramp", "tiled", 300, 300, 64, "none", False, True, False, "ramp_big"),
    ("tiled64-64x249-drop-nowords", "auto", 64, 249, 64, "none", True, False, False, "shared_top"),
    ("tiled64-300x300-drop-nowords", "auto", 300, 300, 64, "decoder", True, False, True, "shared_top"),
    ("tiled32-64x249", "auto", 64, 249, 32, "none", False, True, False, "shared_top"),
    ("tiled32-300x300-drop", "auto", 300, 300, 32, "decoder", True, False, False, "shared_top"),
]


@pytest.mark.parametrize("attn_variant,Lq,Lk,dh,mask,drop,keep_words,with_lo,profile",
                         [pytest.param(*c[1:], id=c[0]) for c in BWD_CASES], indirect=["attn_variant"])
def test_attention_peaked_backward(attn_variant, Lq, Lk, dh, mask, drop, keep_words, with_lo, profile, request):
    """Forward (which supplies lse, checked here too) then backward on rows that are peaked but not one-hot."""
    causal = mask != "none"
    qb, kvb = make_qkv(profile, Lq, Lk, dh, causal and profile == "shared_top", K_NORM_BWD)
    masked, spec = mask_and_spec(mask, Lq, Lk)
    ref = Ref(qb, kvb, dh, masked, keep_of(Lq, Lk, drop), grad=True)
    check_profile(profile, ref, causal)
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    dOb = torch.randn(B, Lq, H * dh, generator=g).bfloat16()
    ref.out.backward(dOb.double().view(B, Lq, H, dh).transpose(1, 2))
    refs = {"dQ": ref.qh.grad, "dK": ref.kh.grad, "dV": ref.vh.grad}
    for name, r in refs.items():
        assert float(r.abs().amax((-1, -2)).min()) > 0, name   # every head has a gradient to get wrong
    run = run_fwd(qb, kvb, dh, spec, drop, keep_words, with_lo)
    check_fwd(request.node.callspec.id, run, ref)
    got = dict(zip(("dQ", "dK", "dV"), run_bwd(run, ref, dh, dOb, keep_words)))
    errs = {n: float(((got[n] - refs[n]).abs().amax((-1, -2)) / refs[n].abs().amax((-1, -2))).max()) for n in refs}
    print(f"peaked bwd {request.node.callspec.id}: per-head err / max|ref| " +
          ", ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f" (bound {BWD_TOL:g})")
    for n in refs:
        assert bool(torch.isfinite(got[n]).all()), n
        assert errs[n] <= BWD_TOL, (n, errs[n])


# ------------------------------------------------------------------------------------------------ 5. softmax

def softmax_rows(Lk, g):
    """[5, 37, Lk] rows in log2 units over 8 key steps: ramp_big, descending, last_key, all_negative, shared_top.
    Each row's maximum is near 0 (row offsets of a few units; all_negative apart), so the fp32 rounding of the
    scaled score, |x| 2^-24, stays far below the 1e-5 bound for the entries that carry the row."""
    Lq = 37
    step = (torch.arange(Lk) // ((Lk + 7) // 8)).double()
    gain = (1.0 + 0.2 * torch.arange(Lq).double() / Lq)[:, None]
    off = (((torch.arange(Lq) * 3) % 5) - 2.0).double()[:, None]
    noise = torch.rand(5, Lq, Lk, generator=g, dtype=torch.float64)
    x = torch.zeros(5, Lq, Lk, dtype=torch.float64)
    x[0] = gain * 12.0 * (step - step.max())[None, :] + off
    x[1] = -gain * 6.0 * step[None, :] + off
    x[2, :, Lk - 1] = 30.0
    x[2] += off
    x[3] = -35.0 + off
    tops = sorted({1, Lk // 2, Lk - 1})
    x[4] = -27.0
    for key, lvl in zip(tops, (0.0, 0.4, -0.3)):
        x[4, :, key] = lvl + 1.0   # (+ noise in [0, 1) below stays under the other tops' reach of 1 unit: see assert)
    x += noise * torch.tensor([1.0, 1.0, 1.0, 1.0, 0.2], dtype=torch.float64)[:, None, None]
    return x, tops


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lk", [24, 200, 249, 999])
@pytest.mark.parametrize("u", [0, 4])
def test_softmax_peaked(dtype, Lk, u, tuning):
    """The unfused softmax on ramp_big / descending / last_key / all_negative rows (scores given directly), p per row
    against float64 at the existing tolerances on the row maximum; dS on a shared_top row at twice that.  Lk = 200 in
    bf16 is the streaming forward."""
    from asrx.kernels import MaskSpec
    tuning("softmax_u", u)
    g = torch.Generator().manual_seed(Lk)
    x, tops = softmax_rows(Lk, g)
    nbh, Lq, _ = x.shape
    ld = (Lk + 7) // 8 * 8
    scale = 0.125
    s = torch.zeros(nbh, Lq, ld, dtype=torch.float64)
    s[..., :Lk] = x * LN2 / scale
    sd = s.to(dev, dtype)
    p = torch.full_like(sd, float("nan"))
    K().softmax_fwd(sd, p, None, nbh, 1, Lq, Lk, ld, scale, MaskSpec())
    xr = sd[..., :Lk].double().cpu() * scale
    ref = torch.softmax(xr, -1)
    # preconditions on the rounded scores
    assert float(ref[2, :, Lk - 1].min()) >= 0.999
    assert float((xr[3] / LN2).max()) <= -30
    assert float(ref[4][:, tops].sum(-1).min()) >= 0.999
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    got = p[..., :Lk].double().cpu()
    err = ((got - ref).abs().amax(-1) / ref.amax(-1))
    print(f"peaked softmax {dtype} Lk {Lk} u {u}: per-row p err / row max {float(err.max()):.3e} (bound {tol:g})")
    assert float(err.max()) <= tol
    assert bool((p.reshape(-1, ld)[:-1, Lk:] == 0).all())
    dpd = torch.randn(nbh, Lq, ld, generator=g).to(dev, dtype)
    ds = torch.empty_like(sd)
    K().softmax_bwd(p, dpd, ds, nbh, Lq, Lk, ld, scale)
    G = dpd[..., :Lk].double().cpu()
    ref_ds = got * (G - (got * G).sum(-1, keepdim=True)) * scale
    assert float(ref_ds[4].abs().amax(-1).min()) > 0
    derr = (ds[..., :Lk].double().cpu() - ref_ds).abs().amax(-1)[4] / ref_ds.abs().amax(-1)[4]
    print(f"peaked softmax {dtype} Lk {Lk} u {u}: shared_top dS err / row max {float(derr.max()):.3e} "
          f"(bound {2 * tol:g})")
    assert float(derr.max()) <= 2 * tol
