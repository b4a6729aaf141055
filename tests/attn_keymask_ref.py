"""Key-validity masks of the fused attention at ANY key count: the cases, two score profiles that put a row's mass
on the LAST live keys of its utterance, and float64 emulations of the two ways such a mask goes wrong (no GPU).

The structured mask (mode 1) marks key j of utterance b live iff kvalid[b][j] != 0; here j < n_b for per-utterance
key counts n = (n0, n1).  The streamed forward moves those bytes as 4-byte words, and once clipped the word that
holds byte Lk - 1: the last Lk % 4 keys of a full-length utterance counted as padding.  Flat random
scores hide that (one key in 249 moves a row by 0.4 % of max |V|), so both profiles make the tail keys carry the row:

  tail_spike (forward)   query q has >= 0.999 of its mass on key max(n_b - 1 - q % 4, 0) (qk_row_spike's rule, a gap
                         of 25 log2 units to every other visible key)
  tail_pair  (backward)  query q shares >= 0.999 between a = n_b - 1 - q % 3 and a - 1, 0.4 units apart (the 2-key
                         analogue of shared_top, solved through the Gram matrix of the keys that serve as a pair),
                         every other live key >= 25 below, plus a random part orthogonal to the pair keys

and every DEAD key scores >= 20 units above every live score of its row: dimension 0 of K is nonzero on dead keys
only, and the product of the two dimensions 0 is a power of two R.  A dropped live key and a leaked dead key are then
each an O(1) error on some row.  R is a property of the construction (how far the raise must clear the live scores:
261 units at R = 2048; R = 1024 left the causal tail_spike at 257 keys under the 20 units — its many distinct spike
keys need a larger beta — and, in the issue's sketch, tail_pair at (303, 303) at 12), not a tolerance.
tail_spike has K[dead][0] = 1 and Q[:, 0] = R.  tail_pair has K[dead][0] = R and Q[:, 0] = 1: with R on the query
side, dK[key][0] = R scale sum_q dS[q][key] is the largest entry of dK by two orders of magnitude, a sum over rows
that are one common number, and the float64 backward with dS rounded to bf16 — check (d) of the CPU test — read up
to 1.5e-2 of it on heads where that sum happens to cancel: the bf16 rounding of dS, not the softmax (what
qk_shared_top's docstring describes).  The scores are the same either way.

Under the decoder's form (causal, kvalid = qvalid) a row sees keys <= q only, so the rules take visible keys: the
spike sits on min(q, n_b - 1) - q % 4; the last three live rows q >= n_b - 3 — the ones that see the tail — share
their own key q and q - 1, every row below them keys 1 and 0.  A pair needs two visible keys: with fewer (n_b = 1,
causal row 0) the row has the one key, and key-only rows of an utterance of 2 or 3 keys share what there is.

test_attention_keymask_cpu.py asserts the preconditions and that the emulated clipped word and the emulated leak break
check_fwd's bounds; test_gpu_attention_keymask.py runs the kernels.
"""
import functools

import torch

import test_gpu_attention_peaked as P

B, H, DH = P.B, P.H, 64
D = H * DH
NEG = P.NEG
R_RAISE = {"tail_spike": 2048.0, "tail_pair": 2048.0}

# (id, ASRX_ATTN_KERNEL, Lq, Lk, form).  The kernels each case reaches once its validity rows are word-aligned are the
# table KEYMASK of tests/test_attn_plan_table.py, asserted there through asrx_attn_kernel_name (rows off a word boundary
# take attn_fwd_res_kernel<1, false> up to 256 keys, the tiled pair past it)
SHAPES = [
    ("self-249", "auto", 249, 249, "keys"),
    ("self-129", "auto", 129, 129, "keys"),
    ("self-190", "auto", 190, 190, "keys"),
    ("self-255", "auto", 255, 255, "keys"),
    ("self-257", "auto", 257, 257, "keys"),
    ("self-386", "auto", 386, 386, "keys"),
    ("self-999", "auto", 999, 999, "keys"),
    ("cross-16x249", "auto", 16, 249, "keys"),
    ("cross-70x249", "auto", 70, 249, "keys"),
    ("cross-16x257", "auto", 16, 257, "keys"),
    ("cross-16x999", "auto", 16, 999, "keys"),
    ("dec-249", "auto", 249, 249, "decoder"),
    ("dec-257", "auto", 257, 257, "decoder"),
    ("dec-302", "auto", 302, 302, "decoder"),
    ("dec-303", "auto", 303, 303, "decoder"),
    ("ctl-252", "auto", 252, 252, "keys"),   # controls: Lk % 4 == 0; the tiled and the resident kernels
    ("ctl-tiled-259", "tiled", 259, 259, "keys"),
    ("ctl-resident-249", "resident", 249, 249, "keys"),
]
# dropout 0.3 with keep words (attn_fwd_stream_kernel<1, true> is a separate copy of the loop)
DROP_SHAPES = [
    ("drop-self-249", "auto", 249, 249, "keys"),
    ("drop-self-259", "auto", 259, 259, "keys"),
    ("drop-cross-16x257", "auto", 16, 257, "keys"),
    ("drop-dec-303", "auto", 303, 303, "decoder"),
]


def lengths_of(Lk, form):
    """The per-utterance key counts every shape runs with (the decoder's form, kvalid = qvalid: the first two)."""
    pairs = [(Lk, Lk - 1), (Lk - 2, (Lk // 2) | 1), (Lk - 3, 1)]
    return pairs[:2] if form == "decoder" else pairs


# (id, variant, Lq, Lk, form, n, drop)
CASES = [(f"{s[0]}-n{n[0]}_{n[1]}", *s[1:], n, drop) for shapes, drop in ((SHAPES, False), (DROP_SHAPES, True))
         for s in shapes for n in lengths_of(s[3], s[4])]


def valid_of(Lk, n):
    return torch.arange(Lk)[None, :] < torch.tensor(n)[:, None]      # [B, Lk] bool


def masked_of(valid, Lq, form):
    """[B, 1, Lq, Lk] bool, True = -inf.  keys: dead keys; decoder: causal | dead key | dead query (Lq == Lk)."""
    Lk = valid.shape[1]
    if form == "decoder":
        return P.decoder_masked(valid.double(), Lq, Lk)
    return (~valid)[:, None, None, :].expand(B, 1, Lq, Lk)


def _visible(Lq, Lk, n_b, causal):
    vis = (torch.arange(Lk) < n_b)[None, :].expand(Lq, Lk)
    return vis & ~torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1) if causal else vis


def spike_keys(Lq, n_b, causal):
    q = torch.arange(Lq)
    last = q.clamp_max(n_b - 1) if causal else torch.full_like(q, n_b - 1)
    return (last - q % 4).clamp_min(0)


def pair_of(q, n_b, causal):
    if causal:   # the last three live rows share their own key and the one below it, every other row keys 1 and 0
        a = min(q if n_b - 3 <= q else 1, q, n_b - 1)
    else:
        a = max(n_b - 1 - q % 3, min(1, n_b - 1))
    return (a, a - 1) if a >= 1 else (0,)


def qk_tail_spike(Lq, Lk, n_b, causal, g, sc2):
    Kk = torch.randn(Lk, DH, generator=g, dtype=torch.float64)
    Kk[:, 0] = 0.0
    Kk = Kk.bfloat16().double()
    j = spike_keys(Lq, n_b, causal)
    unit = Kk[j] / Kk[j].norm(dim=1, keepdim=True)
    proj = unit @ Kk.T
    top = proj.gather(1, j[:, None])
    proj = proj.masked_fill(~_visible(Lq, Lk, n_b, causal), NEG)
    proj.scatter_(1, j[:, None], NEG)
    gap = top - proj.amax(1, keepdim=True)
    some = torch.isfinite(gap)
    beta = 25.0 / (sc2 * float(gap[some].min())) if bool(some.any()) else 1.0
    Q = unit * beta
    Q[:, 0] = R_RAISE["tail_spike"]
    Kk[n_b:, 0] = 1.0
    return Q, Kk


def qk_tail_pair(Lq, Lk, n_b, causal, g, sc2, idx):
    """As qk_shared_top: the keys that serve as a pair are randn rows, every other key randn / 4; a row gets the
    shortest Q that scores its pair at S + (0, -0.4) and the other pair keys at 0, S from the largest score that Q
    gives any other live key (41 units below), plus randn * 6 orthogonal to all pair keys (it moves the other keys by
    up to ~8 units; without it the rows of a pair are one common vector and measure the bf16 rounding of dS)."""
    pairs = [pair_of(q, n_b, causal) for q in range(Lq)]
    special = sorted({key for p in pairs for key in p})
    Kk = torch.randn(Lk, DH, generator=g, dtype=torch.float64) * 0.25
    Kk[special] = torch.randn(len(special), DH, generator=g, dtype=torch.float64)
    Kk[:, 0] = 0.0
    Kk = Kk.bfloat16().double()
    Ka = Kk[special]
    Ginv = torch.linalg.inv(Ka @ Ka.T)
    gain = P._row_gain(Lq)
    Q = torch.zeros(Lq, DH, dtype=torch.float64)
    for pair in sorted(set(pairs)):
        rows = torch.tensor([p == pair for p in pairs])
        own = torch.tensor([key in pair for key in special])
        lv = torch.zeros(len(special), dtype=torch.float64)
        for key, level in zip(pair, (0.0, -0.4)):
            lv[special.index(key)] = level + 0.1 * idx
        x1 = Ka.T @ (Ginv @ own.double())
        xl = Ka.T @ (Ginv @ (lv / sc2))
        other = Kk @ x1
        other[special] = 0.0
        other[n_b:] = 0.0
        s_raw = (41.0 / sc2) / (1.0 - float(other.max()))
        noise = torch.randn(int(rows.sum()), DH, generator=g, dtype=torch.float64) * 6.0
        noise[:, 0] = 0.0
        noise = noise - (noise @ Ka.T) @ (Ginv @ Ka)
        Q[rows] = gain[rows][:, None] * (s_raw * x1)[None, :] + xl[None, :] + noise
    Q[:, 0] = 1.0
    Kk[n_b:, 0] = R_RAISE["tail_pair"]
    return Q, Kk


@functools.lru_cache(maxsize=4)
def make_case(profile, Lq, Lk, n, form):
    """bf16 q [B, Lq, D], kv [B, Lk, 2 D] (K | V), masked [B, 1, Lq, Lk], valid [B, Lk] bool.  V of head idx is scaled
    by 2^(idx - 1) as in make_qkv; the V rows of dead keys are as large as the live ones."""
    causal = form == "decoder"
    g = torch.Generator().manual_seed(sum(map(ord, profile + form)) * 1000003 + Lq * 4099 + Lk * 17 + n[0] * 7 + n[1])
    sc2 = P.scale2_of(DH)
    q = torch.zeros(B, Lq, H, DH, dtype=torch.float64)
    k = torch.zeros(B, Lk, H, DH, dtype=torch.float64)
    v = torch.zeros(B, Lk, H, DH, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            idx = b * H + h
            if profile == "tail_spike":
                Q, Kk = qk_tail_spike(Lq, Lk, n[b], causal, g, sc2)
            else:
                Q, Kk = qk_tail_pair(Lq, Lk, n[b], causal, g, sc2, idx)
            q[b, :, h], k[b, :, h] = Q, Kk
            v[b, :, h] = torch.randn(Lk, DH, generator=g, dtype=torch.float64) * 2.0 ** (idx - 1)
    qb = q.reshape(B, Lq, D).bfloat16()
    kvb = torch.cat([k.reshape(B, Lk, D), v.reshape(B, Lk, D)], -1).bfloat16()
    valid = valid_of(Lk, n)
    return qb, kvb, masked_of(valid, Lq, form), valid


@functools.lru_cache(maxsize=4)
def reference(profile, Lq, Lk, n, form, drop, grad=False):
    """(qb, kvb, valid, Ref) of a case, computed once and shared by the layouts that run it (left unchanged)."""
    qb, kvb, masked, valid = make_case(profile, Lq, Lk, n, form)
    return qb, kvb, valid, P.Ref(qb, kvb, DH, masked, P.keep_of(Lq, Lk, drop), grad=grad)


# ------------------------------------------------------------------------------------------------ preconditions

def check_tail(profile, ref, n, form):
    """The profile's conditions on the float64 scores of the bf16-rounded operands (conditions, not measurements)."""
    Lq, Lk = ref.Lq, ref.Lk
    causal = form == "decoder"
    live = ref.lse > NEG                                             # [B, H, Lq]
    assert bool(live.any(-1).all())
    dead = ~valid_of(Lk, n)[:, None, None, :].expand(B, H, Lq, Lk)
    if bool(dead.any()):
        hid = ref.s2.masked_fill(~dead, float("inf")).amin(-1)
        both = torch.isfinite(hid) & live
        assert bool(both.any())
        assert float((hid - ref.sm.amax(-1))[both].min()) >= 20
    for b in range(B):
        if profile == "tail_spike":
            j = spike_keys(Lq, n[b], causal)
            pj = ref.p[b].gather(-1, j.view(1, Lq, 1).expand(H, Lq, 1))[..., 0]
            assert float(pj[live[b]].min()) >= 0.999
            continue
        for q in range(Lq):
            if not bool(live[b, 0, q]):
                continue
            pair = list(pair_of(q, n[b], causal))
            sk = ref.sm[b, :, q][:, pair]
            assert float(ref.p[b, :, q][:, pair].sum(-1).min()) >= 0.999, (b, q)
            assert float((sk.amax(-1) - sk.amin(-1)).max()) <= 1.0, (b, q)
            rest = ref.sm[b, :, q].clone()
            rest[:, pair] = NEG
            assert float((sk.amin(-1) - rest.amax(-1)).min()) >= 25, (b, q)


# ------------------------------------------------------------------------------------------------ emulations

def as_run(ref):
    """A float64 reference in the layout check_fwd reads from a kernel run: o [B * Lq, D], lse (+inf = dead row)."""
    lse = ref.lse.masked_fill(ref.lse == NEG, float("inf"))
    return {"o": ref.out.detach().transpose(1, 2).reshape(B * ref.Lq, D), "lse": lse.reshape(-1)}


def clipped_word_applies(Lk, n):
    return Lk % 4 != 0 and max(n) > Lk - Lk % 4


def emulate_clipped_word(qb, kvb, valid, Lq, form, keep):
    """The known bug: the word that holds byte Lk - 1 reads as zero, keys >= Lk - Lk % 4 are masked besides."""
    Lk = valid.shape[1]
    clipped = valid & (torch.arange(Lk) < Lk - Lk % 4)[None, :]
    masked = masked_of(valid, Lq, form) | (~clipped)[:, None, None, :]
    return P.Ref(qb, kvb, DH, masked, keep)


def emulate_leak(qb, kvb, valid, n, Lq, form, keep):
    """Byte n_b counts as live.  keys: the dead key takes every row of its utterance; decoder (the one vector is
    kvalid and qvalid): the causal mask hides key n_b from every live row, and query n_b comes alive instead of
    returning an exactly zero row and lse = +inf."""
    Lk = valid.shape[1]
    leaky = valid | (torch.arange(Lk)[None, :] == torch.tensor(n)[:, None])
    return P.Ref(qb, kvb, DH, masked_of(leaky, Lq, form), keep)


def emulate_bwd_bf16(ref, keep, dO):
    """The fused backward's arithmetic in float64 with only P, dS and O rounded to bf16 (dO [B, H, Lq, DH]).  With
    dropout the cases carry o_lo, the rounding residual of O, as every training step does (include/asrx.h): delta is
    then formed from O + o_lo, here the unrounded O.  (Without it a head with one live key has dS = dP keep - dO
    bf16(O), nothing but the rounding of O.)"""
    def bf(t):
        return t.bfloat16().double()
    scale = D ** -0.5
    qh, kh, vh = ref.qh.detach(), ref.kh.detach(), ref.vh.detach()
    p = ref.p
    pd = p if keep is None else p * keep
    O = pd @ vh
    delta = (dO * (bf(O) if keep is None else O)).sum(-1, keepdim=True)
    dP = dO @ vh.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep
    dS = bf(p * (dP - delta))
    return {"dQ": dS @ kh * scale, "dK": dS.transpose(-1, -2) @ qh * scale, "dV": bf(pd).transpose(-1, -2) @ dO}


def grad_reference(ref, dOb):
    """float64 dQ, dK, dV [B, H, L, DH] of a Ref built with grad=True (called once per Ref)."""
    ref.out.backward(dOb.double().view(B, ref.Lq, H, DH).transpose(1, 2))
    return {"dQ": ref.qh.grad, "dK": ref.kh.grad, "dV": ref.vh.grad}


@functools.lru_cache(maxsize=2)
def bwd_reference(Lq, Lk, n, form, drop):
    """(qb, kvb, valid, Ref, dOb, {dQ, dK, dV}) of a tail_pair case, computed once."""
    qb, kvb, masked, valid = make_case("tail_pair", Lq, Lk, n, form)
    ref = P.Ref(qb, kvb, DH, masked, P.keep_of(Lq, Lk, drop), grad=True)
    dOb = dO_of(Lq, Lk)
    return qb, kvb, valid, ref, dOb, grad_reference(ref, dOb)


def grad_errors(got, refs, n):
    """Per (b, h) max |g - ref| / max |ref(b, h)| -> the worst head, per gradient.  A head with ONE live key has a
    constant softmax: its reference dQ and dK are zero (to float64 rounding) while a kernel returns the difference of
    two fp32 dot products; such a head's dQ and dK are held against the tensor's largest head instead."""
    errs = {}
    for name, r in refs.items():
        norm = r.abs().amax((-1, -2))                                   # [B, H]
        if name != "dV":
            single = torch.tensor([nb < 2 for nb in n])[:, None].expand(B, H)
            norm = torch.where(single, norm.max().expand(B, H), norm)
        assert float(norm.min()) > 0, name
        errs[name] = float(((got[name] - r).abs().amax((-1, -2)) / norm).max())
    return errs


def dO_of(Lq, Lk):
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    return torch.randn(B, Lq, D, generator=g).bfloat16()
