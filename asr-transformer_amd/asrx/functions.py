"""Autograd glue: each drop-in module's forward is one torch.autograd.Function whose forward and backward run
the explicit native programs of asrx.blocks.  Weight gradients are written by the kernels straight into the
flat gradient buffer that `p.grad` views (asrx.params); the Functions return None for parameters.

`model_forward` / `model_backward` are also used directly (no autograd) by the fused trainer (asrx.train).
"""
import math
import os
from typing import NamedTuple

import torch

from . import blocks as Bk
from . import kernels as K
from .kernels import MaskSpec
from .params import FlatParams


# ------------------------------------------------------------------------------------------- store / context

def root_of(m):
    r = m.__dict__.get("_asrx_root")
    r = r() if r is not None else None
    return r if r is not None else m


def param_order(root):
    """Module order, except that the decoder's per-layer cross-attention K/V projections are grouped into one
    contiguous [n_layers*2d, d] block (+ bias block): the all-layer K/V GEMM reads them as one matrix."""
    from .model import Decoder
    ps = list(root.parameters())
    decs = [m for m in root.modules() if isinstance(m, Decoder)]
    for dec in decs:
        wkv = [l._cross_attention.wkv for l in dec._layers]
        bkv = [l._cross_attention.bkv for l in dec._layers]
        if not wkv:
            continue
        ids = {id(p) for p in wkv + bkv}
        pos = min(i for i, p in enumerate(ps) if id(p) in ids)
        rest = [p for p in ps if id(p) not in ids]
        ps = rest[:pos] + wkv + bkv + rest[pos:]
    return ps


def get_store(m):
    root = root_of(m)
    st = root.__dict__.get("_asrx_store")
    try:
        dev = next(root.parameters()).device
    except StopIteration:
        raise RuntimeError("asrx: module has no parameters")
    if dev.type != "cuda":
        raise RuntimeError("asrx modules compute on the GPU only (libasrx.so, gfx950); move the model with .cuda()")
    if st is None or st.device != dev or not st.valid():
        st = FlatParams(param_order(root), dev)
        root.__dict__["_asrx_store"] = st
    return st


_SEED_FALLBACK = {}   # device index -> (initial seed, counter) when the CUDA generator cannot be read (capture)


def draw_seed(device):
    """Dropout seed base of one training call, taken where the reference's nn.Dropout takes its masks on the GPU:
    torch's CUDA generator of `device` — its seed and Philox offset, the offset advanced by 4 as a dropout kernel
    of torch would.  Runs are reproducible under torch.manual_seed / torch.cuda.manual_seed, and neither torch's
    CPU generator (DataLoader shuffling, other CPU RNG users) nor eval / no-dropout calls consume anything."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed = gen.initial_seed()
    if torch.cuda.is_current_stream_capturing():
        base, n = _SEED_FALLBACK.get(idx, (seed, 0))
        if base != seed:
            n = 0
        _SEED_FALLBACK[idx] = (seed, n + 1)
        off = (1 << 40) + n
    else:
        off = gen.get_offset()
        gen.set_offset(off + 4)
    return int((seed * 0x9E3779B97F4A7C15 + off * 0xBF58476D1CE4E5B9) & ((1 << 62) - 1))


def make_ctx(m, p_drop):
    root = root_of(m)
    st = get_store(m)
    prec = getattr(root, "precision", "bf16")
    cd = torch.bfloat16 if prec == "bf16" else torch.float32
    if cd == torch.bfloat16:
        st.refresh_shadow()
    train = m.training
    seeds = Bk.Seeds(draw_seed(st.device) if train and p_drop > 0 else 0)
    return Bk.Ctx(st, cd, train, p_drop, seeds, getattr(root, "attention", "fused"))


def _prepare_grads(C):
    st = C.store
    unbound = [p for p in st.params if p.grad is None or p.grad.data_ptr() != st._view(st.grad, p).data_ptr()]
    if not unbound:
        return
    if len(unbound) == len(st.params):
        st.zero_grad()
        for p in st.params:
            p.grad = st._view(st.grad, p)
    else:
        for p in unbound:
            st.ensure_grad(p)


def _params(m):
    return tuple(p for p in m.parameters())


# ------------------------------------------------------------------------------------------- programs

def encoder_input(C, x):
    """Accepts the FrontEnd's logical (B, 64, F'', T'') tensor (ideally the permuted view of its (B, T'', F'', 64)
    buffer) and returns (feats [B*T'', F''*64] compute dtype, B, T'')."""
    if x.dim() != 4:
        raise ValueError("Encoder expects the input_layer output (B, 64, F'', T'')")
    B, Cc, F2, T2 = x.shape
    buf = x.permute(0, 3, 2, 1)
    if not buf.is_contiguous() or buf.dtype != C.cd:
        buf = buf.to(C.cd).contiguous()
    return buf.reshape(B * T2, F2 * Cc), B, T2


def key_spec(lengths, B, T, dev, subsample=0):
    """Padded batches: (rows int32 [B], MaskSpec.keys(valid [B, T])) of per-utterance lengths, one
    asrx_length_mask launch; (None, None) without lengths.  subsample = 0: the lengths count the T rows themselves
    (encoder frames); 2: spectrogram frames in front of the two k3/s2 convolutions."""
    if lengths is None:
        return None, None
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if lengths.numel() != B:
        raise ValueError(f"asrx: {lengths.numel()} lengths for a batch of {B}")
    rows, valid = K.length_mask(lengths, T, subsample)
    return rows, MaskSpec.keys(valid)


def pad_lengths(model, input_lengths, dev=None):
    """The lengths a Transformer entry point masks its attention with: input_lengths where the model was built (or
    set) with mask_padding, else None — the call then runs launch for launch as without the feature.  dev: return
    them as the int32 vector on that device that key_spec hands to the kernel (the Trainer's static graph input)."""
    if input_lengths is None or not getattr(model, "mask_padding", False):
        return None
    if dev is None:
        return input_lengths
    return torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()


def encoder_fwd(C, enc, feats, B, T, spec=None):
    """spec: MaskSpec.keys over the T rows of each utterance, for every layer's self-attention (None: no mask)."""
    d = enc.emb_dim
    H = enc.num_heads
    x = torch.empty(B * T, d, dtype=torch.float32, device=feats.device)
    pe = enc._pe.pe[0]
    if T > pe.shape[0]:
        raise ValueError(f"encoder length {T} exceeds the PE table ({pe.shape[0]}) as in layers.py:73")
    K.linear(feats, C.W(enc._lin_in.weight), x, bias=enc._lin_in.bias.data, rowadd=pe, rowadd_mod=T, ld_rowadd=d)
    Ss = []
    for layer in enc._layers:
        x, S = Bk.enc_layer_fwd(C, x, layer, B, T, H, spec)
        Ss.append(S)
    y, mean, rstd = Bk.ln_fwd(C, x, enc._norm_out)
    return y, dict(feats=feats, x=x, mean=mean, rstd=rstd, layers=Ss)


def _spans(C, params):
    """Maximal [start, end) element ranges of the flat gradient buffer covered by `params` (a module's params
    need not be adjacent: e.g. Encoder._norm_out is registered before the layers).  Two params merge only if
    the second starts at the first aligned offset after the first, so no other parameter lies in between."""
    from .params import ALIGN
    st = C.store
    iv = sorted((st.offset(p), st.offset(p) + p.numel()) for p in params)
    out = []
    for a, b in iv:
        if out and a == -(-out[-1][1] // ALIGN) * ALIGN:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [tuple(x) for x in out]


def _release(C, ready, params):
    """Flush the queued weight-gradient / LayerNorm reductions, hand the finished ranges to the all-reduce and
    re-open the queues (multi-GPU backward only)."""
    if ready is None or C.wq is None:
        return
    C.flush_wgrad()
    if C.fresh is not None:   # unwritten (unzeroed) weight gradients must not reach the all-reduce
        C.fresh.drain(params, C.store)
    for a, b in _spans(C, params):
        ready(a, b)
    boundary = getattr(ready, "boundary", None)   # graph capture: the released ranges end a captured segment
    if boundary is not None:
        boundary()
    C.defer_wgrad()


# encoder layers per gradient release of the multi-GPU backward (ASRX_DP_RELEASE_LAYERS; 0 = by tile rounds, below).
# Every release ends a grouped weight-gradient launch, so finer releases trade all-reduce overlap for fuller launches.
RELEASE_LAYERS = int(os.environ.get("ASRX_DP_RELEASE_LAYERS", "0"))


def _wgrad_tile():
    """(rows, cols) of one weight-gradient tile of the grouped launch's kernel (kernels.WGRAD_KIND)."""
    return K._TILE_CODE.get(K.WGRAD_KIND, ((256, 256), 0))[0]


def _tiles(m, n):
    tm, tn = _wgrad_tile()
    return -(-m // tm) * -(-n // tn)


def _queued_tiles(C, start=0):
    """Output tiles of the weight gradients queued since queue position `start` (one tile per workgroup in the
    grouped launch, one workgroup per CU)."""
    return sum(_tiles(dy.shape[1], x.shape[1]) for (dy, x, _, _) in (C.wq or [])[start:])


def _num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else 256


def release_groups(n, every=None):
    """The encoder layer ranges [lo, hi) released together, in backward order: groups of `every` layers from the
    top; the lowest group (with _lin_in and the front-end) is left to the reducer's finish()."""
    every = RELEASE_LAYERS if every is None else every
    k = every if every > 0 else max(1, n // 2)
    out, hi = [], n
    while hi - k > 0:
        out.append((hi - k, hi))
        hi -= k
    return out


def encoder_bwd(C, enc, S, dy, gate_feats, ready=None, release_every=None, carry=None, with_norm_out=None):
    """dy: grad of the encoder output (fp32 or compute dtype). Returns dfeats (compute dtype).  With `ready`, the
    layers are released to the gradient all-reduce in groups (release_groups; the first with _norm_out) as soon as
    their gradients are final.  carry: parameters (the decoder's) released with the first group (else at finish).
    with_norm_out: further parameters released with _norm_out (the CTC head on the encoder output)."""
    x = S["x"]
    dx_c = torch.empty(x.shape, dtype=C.cd, device=x.device)
    dx = Bk.ln_bwd(C, x, dy, enc._norm_out, S["mean"], S["rstd"], drop_out=dx_c)
    n = len(S["layers"])
    # by tile rounds (the default): ONE release, at the highest layer i whose lower layers 0..i-1 plus _lin_in fit
    # one round of weight-gradient tiles (one workgroup per CU).  The released launch carries the decoder's weight
    # gradients and layers n-1..i (c3: 7 layers; modelled makespan 626 K-steps), the finish() launch the rest (250
    # tiles, 249 K-steps): 875 in all, the single-GPU launch's makespan.  (Releases every 5 layers — one round each —
    # overlapped more of the all-reduce but made 505 + 249 + 249 K-steps.)
    by_rounds = ready is not None and C.wq is not None and release_every is None and RELEASE_LAYERS == 0
    groups = {} if by_rounds else {lo: hi for lo, hi in release_groups(n, release_every)}
    hi, q0, cus = n, len(C.wq or []), _num_cus(x.device)
    lw = enc._lin_in.weight
    tail = _tiles(lw.shape[0], lw.shape[1])
    for i, layer_S in reversed(list(enumerate(S["layers"]))):
        nxt = torch.empty(x.shape, dtype=C.cd, device=x.device)
        dx = Bk.enc_layer_bwd(C, layer_S, dx, dx_c, nxt)
        dx_c = nxt
        if by_rounds and i > 0 and C.wq is not None and hi == n:
            per = _queued_tiles(C, q0) // (n - i)
            if i * per + tail <= cus:
                groups[i] = hi
        if i in groups:
            extra = list(enc._norm_out.parameters()) + list(with_norm_out or []) if groups[i] == n else []
            _release(C, ready, [p for l in enc._layers[i:groups[i]] for p in l.parameters()] + extra + (carry or []))
            carry = None
            hi, q0 = i, len(C.wq or [])
    feats = S["feats"]
    dfeats = torch.empty(feats.shape, dtype=C.cd, device=x.device)
    w = enc._lin_in.weight
    if gate_feats:
        K.linear_dgrad(dx_c, C.W(w), dfeats, gate=feats, ld_gate=feats.shape[1])
    else:
        K.linear_dgrad(dx_c, C.W(w), dfeats)
    C.wgrad(dx_c, feats, C.G(w), C.G(enc._lin_in.bias))
    return dfeats


def _kv_block(C, dec):
    st = C.store
    n = len(dec._layers)
    first_w = dec._layers[0]._cross_attention.wkv
    first_b = dec._layers[0]._cross_attention.bkv
    d = dec.emb_dim
    buf = st.shadow if C.cd == torch.bfloat16 else st.flat
    W = st.span(first_w, n, buf)
    bias = st.span(first_b, n, st.flat)
    gW = st.span(first_w, n, st.grad)
    gb = st.span(first_b, n, st.grad)
    if W is None or bias is None:
        raise RuntimeError("asrx: cross-attention K/V parameters are not contiguous in the flat store")
    return W.view(n * 2 * d, d), bias, gW.view(n * 2 * d, d), gb


def decoder_fwd(C, dec, text, mask, enc_c, B, L, Te, final_norm=True, spec=None, group=1, xspec=None):
    """Decoder.forward as one native program over B token rows of length L.  group > 1 (eval only): every `group`
    consecutive rows decode against ONE encoder output, enc_c [(B / group) * Te, d]: self-attention runs as batch B,
    cross-attention as batch B / group with group * L queries over the once-projected K/V (blocks.cross_attn_fwd).
    xspec: MaskSpec.keys over the Te rows of each encoder output, for every layer's cross-attention (None: no mask)."""
    d, H, n = dec.emb_dim, dec.num_heads, len(dec._layers)
    dev = enc_c.device
    Md = B * L
    text = text.to(device=dev, dtype=torch.int64).contiguous()
    if spec is None:
        spec = MaskSpec.decoder(mask.to(dev))
    pe = dec._pe.pe[0]
    if L > pe.shape[0]:
        raise ValueError(f"decoder length {L} exceeds the PE table ({pe.shape[0]})")
    x = torch.empty(Md, d, dtype=torch.float32, device=dev)
    s_emb = C.seed()
    K.embed_fwd(text, dec._embedding.weight.data, pe, x, L, C.p, s_emb)
    Wkv, bkv, _, _ = _kv_block(C, dec)
    kv = torch.empty(B // group * Te, n * 2 * d, dtype=C.cd, device=dev)
    K.linear(enc_c, Wkv, kv, bias=bkv)
    Ss = []
    for l, layer in enumerate(dec._layers):
        x, S = Bk.dec_layer_fwd(C, x, layer, B, L, H, spec, kv[:, l * 2 * d:], n * 2 * d, Te, group, xspec)
        Ss.append(S)
    cls = dec._classifier
    if final_norm:
        h, mean, rstd = Bk.ln_fwd(C, x, dec._norm_layer)
    else:
        h, mean, rstd = x.to(C.cd), None, None
    logits = torch.empty(Md, cls.Vp, dtype=torch.float32, device=dev)
    K.linear(h, C.W(cls.weight), logits)
    return logits, dict(text=text, x=x, h=h, mean=mean, rstd=rstd, kv=kv, enc=enc_c, layers=Ss, s_emb=s_emb,
                        dims=(B, L, Te))


def decoder_bwd(C, dec, S, dlogits_c):
    """dlogits_c: [B*L, Vp] compute dtype (padded columns zero). Returns d(encoder output) fp32 [B*Te, d]."""
    B, L, Te = S["dims"]
    d, n = dec.emb_dim, len(dec._layers)
    x, h = S["x"], S["h"]
    dev = x.device
    cls = dec._classifier
    dh = torch.empty(B * L, d, dtype=C.cd, device=dev)
    K.linear_dgrad(dlogits_c, C.W(cls.weight), dh)
    C.wgrad(dlogits_c, h, C.G(cls.weight))
    dx_c = torch.empty(B * L, d, dtype=C.cd, device=dev)
    dx = Bk.ln_bwd(C, x, dh, dec._norm_layer, S["mean"], S["rstd"], drop_out=dx_c)
    dkv = torch.empty(B * Te, n * 2 * d, dtype=C.cd, device=dev)
    for l in reversed(range(n)):
        nxt = torch.empty(B * L, d, dtype=C.cd, device=dev)
        dx = Bk.dec_layer_bwd(C, S["layers"][l], dx, dx_c, dkv[:, l * 2 * d:], nxt)
        dx_c = nxt
    K.embed_bwd(S["text"], dx, C.G(dec._embedding.weight), L, dec.pad_token_id if dec.pad_token_id is not None else -1,
                C.p, S["s_emb"])
    Wkv, _, gW, gb = _kv_block(C, dec)
    denc = torch.empty(B * Te, d, dtype=torch.float32, device=dev)
    K.linear_dgrad(dkv, Wkv, denc)
    C.wgrad(dkv, S["enc"], gW, gb)
    return denc


def ctc_head_fwd(C, model, enc_c):
    """fp32 CTC logits [B*T', Vp] of the compute-dtype encoder output [B*T', d] (Transformer.ctc_head)."""
    head = getattr(model, "ctc_head", None)
    if head is None:
        raise RuntimeError("asrx: the model has no CTC head (build it with Transformer(..., ctc=True))")
    logits = torch.empty(enc_c.shape[0], head.Vp, dtype=torch.float32, device=enc_c.device)
    K.linear(enc_c, C.W(head.weight), logits)
    return logits


def model_forward(C, model, spectrum, text, mask, spec=None, ctc=False, enc_spec=None):
    """Transformer.forward (model.py:194-198) as one native program. Returns (logits [B*L, Vp] fp32, S).  spec:
    the decoder's self-attention mask when the caller already built it (mask is then unused).  ctc: also run the CTC
    head on the encoder output, S["ctc_logits"] (fp32 [B*T', Vp]).  enc_spec: MaskSpec.keys over the T' encoder rows
    of each utterance; it masks the encoder's self-attention and the decoder's cross-attention."""
    dev = C.store.device
    spectrum = spectrum.to(dev)
    feats, Sf = Bk.frontend_fwd(C, spectrum, model.input_layer[0], model.input_layer[2])
    B = spectrum.shape[0]
    T2 = Sf["dims"][-1]
    enc, Se = encoder_fwd(C, model.encoder, feats, B, T2, enc_spec)
    L = text.shape[1]
    logits, Sd = decoder_fwd(C, model.decoder, text, mask, enc, B, L, T2, spec=spec, xspec=enc_spec)
    S = dict(f=Sf, e=Se, d=Sd)
    if ctc:
        S["ctc_logits"] = ctc_head_fwd(C, model, enc)
    return logits, S


def model_backward(C, model, S, dlogits_c, ready=None, dctc_c=None):
    """Backward of model_forward.  ready(start, end): optional callback that receives flat-gradient ranges as
    they become final (decoder, then upper encoder half) so their all-reduce overlaps the rest of the backward;
    whatever is not released that way is final when this returns.  dctc_c: gradient of S["ctc_logits"] ([B*T', Vp]
    compute dtype, padded columns zero): the head's data gradient is added to the encoder-output gradient before the
    encoder's backward, its weight gradient joins the queued ones, its range is released with Encoder._norm_out."""
    _prepare_grads(C)
    own = C.defer_wgrad()
    denc = decoder_bwd(C, model.decoder, S["d"], dlogits_c)
    head_params = None
    if dctc_c is not None:
        head = model.ctc_head
        # denc + dctc . W_head in the GEMM's fp32-residual epilogue (as FFN2 adds its residual stream)
        dsum = torch.empty_like(denc)
        K.linear_dgrad(dctc_c, C.W(head.weight), dsum, resid=denc, ld_resid=denc.stride(0))
        denc = dsum
        C.wgrad(dctc_c, S["d"]["enc"], C.G(head.weight))
        head_params = [head.weight]
    # by tile rounds (the default release schedule): the decoder's weight gradients (the 96 long cross K/V tiles and
    # 672 short ones) are not a launch of their own but join the first encoder group's — one ~2-round launch instead
    # of a 313-K-step one plus a 249-K-step one (modelled with kernels.xcd_plan) and one segment boundary fewer;
    # their all-reduce then starts five encoder layers later, still overlapping the rest of the backward
    carry = ready is not None and own and RELEASE_LAYERS == 0
    if own:
        if not carry:
            _release(C, ready, list(model.decoder.parameters()))
    dfeats = encoder_bwd(C, model.encoder, S["e"], denc, gate_feats=True, ready=ready if own else None,
                         carry=list(model.decoder.parameters()) if carry else None, with_norm_out=head_params)
    Bk.frontend_bwd(C, S["f"], dfeats, model.input_layer[0], model.input_layer[2])
    if own:
        C.flush_wgrad()


def _dlogits_padded(C, dlogits, rows, V, Vp):
    g = torch.zeros(rows, Vp, dtype=C.cd, device=dlogits.device)
    g[:, :V].copy_(dlogits.reshape(rows, V))
    return g


# ------------------------------------------------------------------------------------------- Functions

class _TransformerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, C, spectrum, text, mask, enc_spec, *params):
        logits, S = model_forward(C, model, spectrum, text, mask, enc_spec=enc_spec)
        ctx.model, ctx.C, ctx.S = model, C, S
        B, L = text.shape
        V = model.decoder._classifier.V
        ctx.shape = (B, L, V, logits.shape[1])
        out = logits.view(B, L, -1)
        return out[:, :, :V] if V != logits.shape[1] else out

    @staticmethod
    def backward(ctx, dlogits):
        B, L, V, Vp = ctx.shape
        C = ctx.C
        model_backward(C, ctx.model, ctx.S, _dlogits_padded(C, dlogits, B * L, V, Vp))
        ctx.S = None
        return (None,) * (6 + len(_params(ctx.model)))


def transformer(model, spectrum, text, mask, input_lengths=None):
    """input_lengths (valid encoder frames per utterance) mask the padded frames where the model has mask_padding."""
    C = make_ctx(model, model.decoder.p)
    enc_spec = None
    lens = pad_lengths(model, input_lengths)
    if lens is not None:
        from .model import subsampled
        _, enc_spec = key_spec(lens, spectrum.shape[0], subsampled(spectrum.shape[-1]), C.store.device)
    return _TransformerFn.apply(model, C, spectrum, text, mask, enc_spec, *_params(model))


class _FrontEndFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fe, C, spectrum, *params):
        feats, S = Bk.frontend_fwd(C, spectrum, fe[0], fe[2])
        ctx.fe, ctx.C, ctx.S = fe, C, S
        B, F, T, F1, T1, F2, T2 = S["dims"]
        return feats.view(B, T2, F2, 64).permute(0, 3, 2, 1)

    @staticmethod
    def backward(ctx, g):
        C, S = ctx.C, ctx.S
        _prepare_grads(C)
        buf = g.permute(0, 3, 2, 1).to(C.cd).contiguous()
        B, F, T, F1, T1, F2, T2 = S["dims"]
        dy2 = buf.view(B * T2, F2 * 64)
        K.ewise(K.EW_RELU_GRAD, dy2, dy2, b=S["feats"])   # the conv2 ReLU gate (model.py:170), in place
        Bk.frontend_bwd(C, S, dy2, ctx.fe[0], ctx.fe[2])
        return (None,) * (3 + len(_params(ctx.fe)))


def frontend(fe, spectrum):
    C = make_ctx(fe, 0.0)
    return _FrontEndFn.apply(fe, C, spectrum, *_params(fe))


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, C, x, input_lengths, *params):
        feats, B, T = encoder_input(C, x)
        y, S = encoder_fwd(C, enc, feats, B, T, key_spec(input_lengths, B, T, feats.device)[1])
        ctx.enc, ctx.C, ctx.S, ctx.xshape = enc, C, S, (B, T, x.shape[1], x.shape[2])
        return y.view(B, T, -1)

    @staticmethod
    def backward(ctx, g):
        C, S = ctx.C, ctx.S
        _prepare_grads(C)
        B, T, Cc, F2 = ctx.xshape
        own = C.defer_wgrad()
        dfeats = encoder_bwd(C, ctx.enc, S, g.reshape(B * T, -1).contiguous(), gate_feats=False)
        if own:
            C.flush_wgrad()
        dx = dfeats.view(B, T, F2, Cc).permute(0, 3, 2, 1)
        return (None, None, dx, None) + (None,) * len(_params(ctx.enc))


def encoder(enc, x, input_lengths=None):
    C = make_ctx(enc, enc.p)
    return _EncoderFn.apply(enc, C, x, input_lengths, *_params(enc))


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dec, C, text, mask, enc_x, enc_lengths, *params):
        B, Te, d = enc_x.shape
        enc_c = enc_x.reshape(B * Te, d).to(C.cd).contiguous()
        L = text.shape[1]
        xspec = key_spec(enc_lengths, B, Te, enc_c.device)[1]
        logits, S = decoder_fwd(C, dec, text, mask, enc_c, B, L, Te, xspec=xspec)
        ctx.dec, ctx.C, ctx.S = dec, C, S
        V = dec._classifier.V
        ctx.shape = (B, L, V, logits.shape[1], Te, d)
        out = logits.view(B, L, -1)
        return out[:, :, :V] if V != logits.shape[1] else out

    @staticmethod
    def backward(ctx, dlogits):
        B, L, V, Vp, Te, d = ctx.shape
        C = ctx.C
        _prepare_grads(C)
        own = C.defer_wgrad()
        denc = decoder_bwd(C, ctx.dec, ctx.S, _dlogits_padded(C, dlogits, B * L, V, Vp))
        if own:
            C.flush_wgrad()
        return (None, None, None, None, denc.view(B, Te, d), None) + (None,) * len(_params(ctx.dec))


def decoder(dec, x, mask, enc_x, enc_lengths=None):
    C = make_ctx(dec, dec.p)
    return _DecoderFn.apply(dec, C, x, mask, enc_x, enc_lengths, *_params(dec))


@torch.no_grad()
def decoder_evaluate(dec, x, enc_x, enc_lengths=None):
    """Decoder.evaluate (model.py:125-151) with its quirks: causal-only mask, NO final LayerNorm before the
    classifier, no break on EOS (every sample runs seq_len steps), returns the LAST sample's token row and the list
    of logits snapshots `prob[:, :-1].squeeze()` (one per EOS hit or final step, samples in order).

    Eval mode: the whole batch decodes together with per-layer K/V caches (one position per step: causality makes
    the reference's full-prefix recomputation redundant), the cross-attention K/V of all layers projected once, and
    the next tokens chosen on the GPU (asrx_greedy_argmax) — no host round trip until the end.  Train mode with
    dropout (model.py:137 applies self._dropout, and every layer's dropouts are live): the reference's
    per-sample prefix recomputation, whose fresh masks a cache cannot reproduce.

    enc_lengths (valid rows of each encoder output): the cross-attention masks the padded rows."""
    if dec.training and dec.p > 0:
        return _decoder_evaluate_recompute(dec, x, enc_x, enc_lengths)
    return _decoder_evaluate_cached(dec, x, enc_x, enc_lengths)


def _decoder_evaluate_recompute(dec, x, enc_x, enc_lengths=None):
    C = make_ctx(dec, dec.p)
    B, Te, d = enc_x.shape
    xspec = key_spec(enc_lengths, B, Te, enc_x.device)[1]
    V = dec._classifier.V
    probs = []
    decoder_input = None
    for s in range(x.shape[0]):
        decoder_input = x[s].unsqueeze(0).to(enc_x.device)
        e = enc_x[s].reshape(Te, d).to(C.cd).contiguous()
        for i in range(1, dec._seq_len + 1):
            L = decoder_input.shape[1]
            spec = MaskSpec(1, True)
            xs = None if xspec is None else MaskSpec.keys(xspec.kvalid[s:s + 1])
            logits, _ = decoder_fwd(C, dec, decoder_input, None, e, 1, L, Te, final_norm=False, spec=spec, xspec=xs)
            prob = logits[:, :V].view(1, L, V)
            next_word = prob.argmax(dim=-1)[:, -1].unsqueeze(1)
            decoder_input = torch.cat([decoder_input, next_word.to(decoder_input.dtype)], dim=-1)
            if next_word.item() == dec._eos_token_id or i == dec._seq_len:
                probs.append(prob[:, :-1].squeeze())
    return decoder_input, probs


def _mha_params(m):
    """(weight, bias, rows) of an MHA's q, k | v and out projections; in self-attention the first two are row
    blocks of the fused q | k | v weight."""
    out = m._out_linear
    d = out.weight.shape[0]
    if m.cross:
        qkv = [(m.wq, m.bq, slice(None)), (m.wkv, m.bkv, slice(None))]
    else:
        qkv = [(m.wqkv, m.bqkv, slice(0, d)), (m.wqkv, m.bqkv, slice(d, None))]
    return qkv + [(out.weight, out.bias, slice(None))]


def _mha_fwd_w(C, m):
    """(Wq, bq, Wkv, bkv, Wo, bo) of Bk.attn_core_fwd with separate q and k | v projections."""
    return sum(((C.W(p)[r], b.data[r]) for p, b, r in _mha_params(m)), ())


def _decode_position(C, dec, cur, pe, t, kvs, kvx, B, W, Te, xspec=None):
    """One decoder position for B samples x W hypotheses (rows b*W + w): the embedding of `cur` at position t through
    every layer (pe = the positional table), returning the fp32 stream [B*W, d].  kvs [n][B*W][P][2d] are the
    self-attention K/V caches, which gain position t; kvx [B*Te][n*2d] holds every layer's cross-attention K/V per
    SAMPLE: the W hypotheses of a sample share it, so cross-attention runs as batch = B with W queries each (W = 1:
    greedy decoding).  xspec: MaskSpec.keys over each sample's Te encoder rows, for the cross-attention."""
    d, H = dec.emb_dim, dec.num_heads
    dh = d // H
    R = B * W
    none = MaskSpec()
    cross = xspec or none
    xs = torch.empty(R, d, dtype=torch.float32, device=cur.device)
    K.embed_fwd(cur, dec._embedding.weight.data, pe[t:t + 1], xs, 1)
    for l, layer in enumerate(dec._layers):
        mha, cr = layer._mask_attention, layer._cross_attention
        # masked self-attention: the new position's K/V join the cache, its query attends to positions 0..t
        h, _, _ = Bk.ln_fwd(C, xs, layer._norm1)
        x1, _ = Bk.attn_core_fwd(C, _mha_fwd_w(C, mha), h, R, H, dh, 1, t + 1, none, xk=h, kv=kvs[l],
                                 kv_dst=kvs[l][:, t], resid=xs)
        # cross-attention over the encoder output (no mask, model.py:71, unless the batch is padded: xspec)
        h2, _, _ = Bk.ln_fwd(C, x1, layer._norm2)
        w = (C.W(cr.wq), cr.bq.data, None, None, C.W(cr._out_linear.weight), cr._out_linear.bias.data)
        x2, _ = Bk.attn_core_fwd(C, w, h2, B, H, dh, W, Te, cross, kv=kvx[:, l * 2 * d:], resid=x1)
        xs, _ = Bk.ffn_fwd(C, x2, layer._norm3, layer._feedforward)
    return xs


def _decoder_evaluate_cached(dec, x, enc_x, enc_lengths=None):
    C = make_ctx(dec, 0.0)
    C.train, C.p = False, 0.0
    dev = enc_x.device
    B, Te, d = enc_x.shape
    xspec = key_spec(enc_lengths, B, Te, dev)[1]
    n, H, steps = len(dec._layers), dec.num_heads, dec._seq_len
    dh = d // H
    cls = dec._classifier
    V, Vp = cls.V, cls.Vp
    L0 = x.shape[1]
    P = L0 - 1 + steps                      # positions processed (the last input has L0 + steps - 1 tokens)
    pe = dec._pe.pe[0]
    if P > pe.shape[0]:
        raise ValueError(f"decoder length {P} exceeds the PE table ({pe.shape[0]}) as in layers.py:73")
    if B == 0 or steps == 0:
        return x[-1:].to(dev) if B else x.to(dev), []
    enc_c = torch.empty(B * Te, d, dtype=C.cd, device=dev)
    K.cast(enc_x.reshape(B * Te, d).contiguous(), enc_c)
    Wkv, bkv, _, _ = _kv_block(C, dec)
    kvx = torch.empty(B * Te, n * 2 * d, dtype=C.cd, device=dev)      # every layer's cross-attention K/V
    K.linear(enc_c, Wkv, kvx, bias=bkv)
    kvs = torch.empty(n, B, P, 2 * d, dtype=C.cd, device=dev)          # self-attention K/V caches
    logits = torch.empty(B, P, Vp, dtype=torch.float32, device=dev)
    tokens = torch.empty(B, L0 + steps, dtype=torch.int64, device=dev)
    tokens[:, :L0] = x.to(device=dev, dtype=torch.int64)
    cur = tokens[:, 0].contiguous()
    for t in range(P):
        xs = _decode_position(C, dec, cur, pe, t, kvs, kvx, B, 1, Te, xspec)
        hc = torch.empty(B, d, dtype=C.cd, device=dev)       # no final LayerNorm in evaluate (model.py:142)
        K.cast(xs, hc)
        lg = logits[:, t]
        K.gemm(hc, C.W(cls.weight), lg, B, Vp, d, lda=d, ldb=d, ldc=P * Vp)
        if t + 1 >= L0:
            K.greedy_argmax(lg, V, tokens[:, t + 1], cur)
        else:
            cur = tokens[:, t + 1].contiguous()
    tok = tokens.cpu()
    eos = dec._eos_token_id
    probs = []
    for s in range(B):
        for i in range(1, steps + 1):
            Li = L0 + i - 1                                  # input length at step i
            if int(tok[s, Li]) == eos or i == steps:
                probs.append(logits[s:s + 1, :Li - 1, :V].squeeze())
    return tokens[B - 1:B].to(x.dtype), probs


class BeamResult(NamedTuple):
    """Decoder.beam_search / Transformer.beam_search: per sample the `nbest` best hypotheses, best first.
    tokens (B, nbest, L0 + steps) int64: prompt, generated tokens, EOS after a hypothesis's end (steps = max_len
    unless polling stopped the loop early); lengths (B, nbest) int64: generated tokens, the EOS included; scores
    (B, nbest) fp32: summed log-probabilities (-inf: fewer than nbest hypotheses exist)."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    scores: torch.Tensor


def beam_backtrack(parents, toks):
    """Follow the parent links of a beam history back from the last step.  parents / toks: [steps][B][W] integer
    arrays (the slot a step's hypothesis extends, the token it adds).  Returns [B][W][steps]: the token sequence of
    every final slot."""
    parents, toks = torch.as_tensor(parents), torch.as_tensor(toks)
    steps, B, W = toks.shape
    out = torch.empty(B, W, steps, dtype=torch.int64)
    slot = torch.arange(W).expand(B, W)
    for s in range(steps - 1, -1, -1):
        out[:, :, s] = toks[s].gather(1, slot)
        slot = parents[s].gather(1, slot).long()
    return out


def beam_rank(scores, lengths, length_penalty):
    """Order of each sample's W hypotheses: descending score / len**length_penalty, ties by slot, dead (-inf or
    NaN) hypotheses last.  scores fp32 [B][W], lengths [B][W]; returns int64 [B][W] slot numbers."""
    key = scores.double()
    if length_penalty != 0.0:
        key = key / lengths.clamp(min=1).double() ** float(length_penalty)
    key = torch.where(torch.isfinite(scores), key, torch.full_like(key, float("-inf")))
    return torch.sort(key, dim=1, descending=True, stable=True).indices


def check_lm(lm, lm_weight, token_bonus, V=None):
    """The LM arguments of the decoders, checked before any device work: (lm_weight, token_bonus) as floats, the weight
    0.0 where no LM takes part (lm=None or lm_weight == 0: the decoders then issue exactly the launches they issue
    without these arguments, and token_bonus is not applied).  V: the classifier's vocabulary, which the LM's must
    equal."""
    beta, bonus = float(lm_weight), float(token_bonus)
    if beta != beta or beta < 0.0 or math.isinf(beta):
        raise ValueError(f"lm_weight {lm_weight} must be a finite number >= 0")
    if not math.isfinite(bonus):
        raise ValueError(f"token_bonus {token_bonus} must be finite")
    if lm is None or beta == 0.0:
        return 0.0, 0.0
    if V is not None and lm.vocab_size != V:
        raise ValueError(f"the LM's vocabulary ({lm.vocab_size}) is not the classifier's ({V})")
    return beta, bonus


@torch.no_grad()
def decoder_beam_search(dec, x, enc_x, beam=4, max_len=None, length_penalty=0.0, final_norm=True, nbest=1, poll=8,
                        ctc=None, ctc_weight=0.0, lm=None, lm_weight=0.0, token_bonus=0.0, enc_lengths=None):
    """Beam-search decoding on the KV-cached decoder (the reference has none: Decoder.evaluate, model.py:125-151, is
    greedy).  x (B, L0 >= 1) is the prompt, prefilled with teacher forcing; `max_len` new tokens (default seq_len)
    are then chosen with `beam` hypotheses per sample, each step keeping the `beam` best continuations by summed
    log-probability (ties: lower parent slot, then lower token id); a hypothesis that emitted EOS is frozen.  The
    hypotheses are finally ranked by score / len**length_penalty (len counts the generated tokens, EOS included).

    final_norm=True (default) applies the decoder's last LayerNorm before the classifier, as Decoder.forward does
    (model.py:122) and as models are therefore trained; final_norm=False reproduces the logits of `evaluate`, which
    skips it (model.py:142).

    Everything per step runs on the device (asrx_beam_step picks the slots, asrx_gather_rows reorders the K/V
    caches into their second buffer); the host reads nothing until the end, except every `poll` steps (0 = never)
    the count of live hypotheses, to stop once all have finished.  Eval only: dropout is off.

    ctc_weight = lam in (0, 1] decodes jointly with a CTC head (Watanabe et al. 2017): a hypothesis is ranked by
    (1 - lam) * log p_att + lam * log p_ctc, the second term the CTC prefix probability of its generated labels, and
    `scores` are these joint scores.  ctc = (logits, T, blank, input_lengths): the head's fp32 logits [B*T, >= V] of
    the utterances, their frame count, the blank id and optional int32 frame counts per sample.  Every selecting step
    then scores the whole vocabulary (asrx_ctc_prefix_score), selects (asrx_beam_step_joint) and advances the
    survivors' CTC states (asrx_ctc_prefix_advance), all on the device.  The prompt must be one token (the CTC
    prefix is the generated labels only).  ctc_weight = 0 (default) is the attention-only search, launch for launch.

    lm (an asrx.NgramLM on the device) with lm_weight = beta > 0 adds shallow fusion: every generated token, the EOS
    included, also earns beta * log p_lm(token | BOS, the tokens before it) + token_bonus, so a finished hypothesis
    scores (1 - lam) * log p_att + lam * log p_ctc + beta * log p_lm + token_bonus * len.  Two more launches per step:
    asrx_ngram_score writes the `extra` matrix of asrx_beam_step_joint (with lam > 0 it folds lam * the CTC scores in),
    asrx_ngram_advance moves the survivors' LM contexts.  The prompt must be one token, the LM's sentence start.
    lm=None or lm_weight = 0 (default) issues exactly the launches described above.

    enc_lengths (valid rows of each encoder output): every cross-attention masks the padded rows (one more launch in
    front, asrx_length_mask).  None (default) issues exactly the launches described above."""
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"ctc_weight {ctc_weight} outside [0, 1]")
    beta, bonus = check_lm(lm, lm_weight, token_bonus, dec._classifier.V)
    if beta > 0.0 and x.dim() == 2 and x.shape[1] != 1:
        raise ValueError(f"lm_weight > 0 takes a one-token prompt, got L0 = {x.shape[1]}")
    if lam > 0.0:
        if ctc is None:
            raise RuntimeError("asrx: ctc_weight > 0 needs the CTC head's logits (a model built with ctc=True)")
        if x.dim() == 2 and x.shape[1] != 1:
            raise ValueError(f"ctc_weight > 0 takes a one-token prompt, got L0 = {x.shape[1]}")
    C = make_ctx(dec, 0.0)
    C.train, C.p = False, 0.0
    dev = enc_x.device
    B, Te, d = enc_x.shape
    n = len(dec._layers)
    W = int(beam)
    steps = dec._seq_len if max_len is None else int(max_len)
    nbest, poll = int(nbest), int(poll)
    if not 1 <= W <= 16:
        raise ValueError(f"beam must be in 1..16, got {beam}")
    if not 1 <= nbest <= W:
        raise ValueError(f"nbest must be in 1..beam, got {nbest}")
    if x.dim() != 2 or x.shape[0] != B or x.shape[1] < 1:
        raise ValueError(f"prompt must be (B, L0 >= 1) with B = {B}, got {tuple(x.shape)}")
    if steps < 0 or poll < 0:
        raise ValueError("max_len and poll must be >= 0")
    cls = dec._classifier
    V, Vp = cls.V, cls.Vp
    eos = int(dec._eos_token_id)
    L0 = x.shape[1]
    P = L0 - 1 + steps
    pe = dec._pe.pe[0]
    if P > pe.shape[0]:
        raise ValueError(f"decoder length {P} exceeds the PE table ({pe.shape[0]}) as in layers.py:73")
    prompt = x.to(device="cpu", dtype=torch.int64)
    if B == 0 or steps == 0:
        return BeamResult(prompt[:, None, :].expand(B, nbest, L0).contiguous(),
                          torch.zeros(B, nbest, dtype=torch.int64), torch.zeros(B, nbest, dtype=torch.float32))
    R = B * W
    xspec = key_spec(enc_lengths, B, Te, dev)[1]
    enc_c = torch.empty(B * Te, d, dtype=C.cd, device=dev)
    K.cast(enc_x.reshape(B * Te, d).contiguous(), enc_c)
    Wkv, bkv, _, _ = _kv_block(C, dec)
    kvx = torch.empty(B * Te, n * 2 * d, dtype=C.cd, device=dev)       # cross-attention K/V: per sample, not per beam
    K.linear(enc_c, Wkv, kvx, bias=bkv)
    kvs = torch.empty(n, R, P, 2 * d, dtype=C.cd, device=dev)           # self-attention K/V caches and, for W > 1,
    kvs_alt = torch.empty_like(kvs) if W > 1 else None                  # the buffer each reorder gathers into
    xr = prompt.to(dev).repeat_interleave(W, dim=0)                     # (R, L0): every beam starts on the prompt
    score0 = torch.full((B, W), float("-inf"), dtype=torch.float32)
    score0[:, 0] = 0.0                                                  # one live root: the others can only lose
    state = (score0.reshape(R).to(dev), torch.zeros(R, dtype=torch.uint8, device=dev),
             torch.zeros(R, dtype=torch.int32, device=dev))
    other = tuple(torch.empty_like(a) for a in state)
    tok_h = torch.empty(steps, R, dtype=torch.int64, device=dev)
    par_h = torch.empty(steps, R, dtype=torch.int32, device=dev)
    src_row = torch.empty(R, dtype=torch.int32, device=dev)
    n_live = torch.zeros(steps, dtype=torch.int32, device=dev)          # one zeroed word per step
    cur = xr[:, 0].contiguous()
    done = steps
    prefix = None
    if lam > 0.0:
        ctc_logits, ctc_T, ctc_blank, ctc_lengths = ctc
        if ctc_lengths is not None:
            ctc_lengths = ctc_lengths.to(device=dev, dtype=torch.int32).contiguous()
        prefix = K.CtcPrefix(ctc_logits, B, W, int(ctc_T), V, ctc_blank, ctc_lengths)
        delta = torch.empty(R, Vp, dtype=torch.float32, device=dev)
    ngram = None
    if beta > 0.0:
        ngram = K.NgramState(lm, B, W)
        extra = torch.empty(R, Vp, dtype=torch.float32, device=dev)
    for t in range(P):
        xs = _decode_position(C, dec, cur, pe, t, kvs, kvx, B, W, Te, xspec)
        s = t - (L0 - 1)
        if s < 0:
            cur = xr[:, t + 1].contiguous()
            continue
        if final_norm:
            hc, _, _ = Bk.ln_fwd(C, xs, dec._norm_layer)
        else:
            hc = torch.empty(R, d, dtype=C.cd, device=dev)
            K.cast(xs, hc)
        lg = torch.empty(R, Vp, dtype=torch.float32, device=dev)
        K.gemm(hc, C.W(cls.weight), lg, R, Vp, d, lda=d, ldb=d, ldc=Vp)
        if prefix is None and ngram is None:
            K.beam_step(lg, V, B, W, eos, state, other, tok_h[s], par_h[s], src_row, cur=cur, n_live=n_live[s:s + 1])
        elif ngram is None:
            prefix.score(eos, delta)
            K.beam_step_joint(lg, V, B, W, eos, delta, 1.0 - lam, lam, state, other, tok_h[s], par_h[s], src_row,
                              cur=cur, n_live=n_live[s:s + 1])
            prefix.advance(eos, par_h[s], tok_h[s], state[1])
        else:       # extra = lam * ctc + beta * lm + bonus in one launch, selected with extra_weight = 1
            if prefix is not None:
                prefix.score(eos, delta)
                ngram.score(extra, delta, lam, beta, bonus)
            else:
                ngram.score(extra, None, 0.0, beta, bonus)
            K.beam_step_joint(lg, V, B, W, eos, extra, 1.0 - lam, 1.0, state, other, tok_h[s], par_h[s], src_row,
                              cur=cur, n_live=n_live[s:s + 1])
            if prefix is not None:
                prefix.advance(eos, par_h[s], tok_h[s], state[1])
            ngram.advance(eos, par_h[s], tok_h[s], state[1])
        state, other = other, state
        if poll and (s + 1) % poll == 0 and s + 1 < steps and int(n_live[s]) == 0:
            done = s + 1
            break
        if W > 1 and s + 1 < steps:      # (one beam: the parent is always slot 0, the cache stays in place)
            K.gather_rows(kvs, kvs_alt, src_row, n, R, (t + 1) * 2 * d, P * 2 * d, R * P * 2 * d)
            kvs, kvs_alt = kvs_alt, kvs
    score, _, length = (a.cpu().view(B, W) for a in state)
    seqs = beam_backtrack(par_h[:done].cpu().view(done, B, W), tok_h[:done].cpu().view(done, B, W))
    order = beam_rank(score, length, length_penalty)[:, :nbest]
    best = seqs.gather(1, order[:, :, None].expand(-1, -1, done))
    tokens = torch.cat([prompt[:, None, :].expand(B, nbest, L0), best], dim=2)
    return BeamResult(tokens, length.long().gather(1, order), score.gather(1, order))


def transformer_beam_search(model, spectrum, text=None, ctc_weight=0.0, input_lengths=None, **kw):
    """Transformer.beam_search: front end and encoder as in `evaluate` (model.py:201-206), then
    decoder_beam_search.  text=None starts every sample on a BOS column (id 1).  ctc_weight > 0: joint
    CTC/attention decoding, the one encoder output also feeding the model's CTC head (input_lengths: optional valid
    encoder frames per sample; on a model with mask_padding they also mask the encoder's self-attention and the
    cross-attention, with or without the CTC term)."""
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"ctc_weight {ctc_weight} outside [0, 1]")
    if lam > 0.0 and getattr(model, "ctc_head", None) is None:
        raise RuntimeError("asrx: ctc_weight > 0 needs a model with a CTC head (Transformer(..., ctc=True))")
    if lam > 0.0 and text is not None and text.dim() == 2 and text.shape[1] != 1:
        raise ValueError(f"ctc_weight > 0 takes a one-token prompt, got L0 = {text.shape[1]}")
    beta, _ = check_lm(kw.get("lm"), kw.get("lm_weight", 0.0), kw.get("token_bonus", 0.0), model.decoder._classifier.V)
    if beta > 0.0 and text is not None and text.dim() == 2 and text.shape[1] != 1:
        raise ValueError(f"lm_weight > 0 takes a one-token prompt, got L0 = {text.shape[1]}")
    lens = pad_lengths(model, input_lengths)
    with torch.no_grad():
        enc = _encode(model, spectrum, lens)
    if text is None:
        text = torch.ones(spectrum.shape[0], 1, dtype=torch.int64)
    if lens is not None:
        kw["enc_lengths"] = lens
    if lam == 0.0:
        return decoder_beam_search(model.decoder, text, enc, **kw)
    logits, B, T = _ctc_logits_of(model, enc)
    return decoder_beam_search(model.decoder, text, enc, ctc=(logits, T, model.ctc_blank, input_lengths),
                               ctc_weight=lam, **kw)


def _encode(model, spectrum, lens=None):
    """Front end and encoder as in `evaluate` (model.py:201-203); lens: the lengths to mask with (pad_lengths)."""
    feats = model.input_layer(spectrum)
    return model.encoder(feats) if lens is None else model.encoder(feats, input_lengths=lens)


@torch.no_grad()
def transformer_evaluate(model, spectrum, text, input_lengths=None):
    """Transformer.evaluate (model.py:201-206); input_lengths as in transformer()."""
    lens = pad_lengths(model, input_lengths)
    enc = _encode(model, spectrum, lens)
    return model.decoder.evaluate(text, enc) if lens is None else model.decoder.evaluate(text, enc, enc_lengths=lens)


@torch.no_grad()
def transformer_ctc_logits(model, spectrum, input_lengths=None):
    """Front end and encoder as in `evaluate`, then the CTC head: (fp32 logits [B*T', Vp], B, T').  input_lengths: as in
    transformer() (mask_padding models: the encoder masks the padded frames)."""
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("asrx: the model has no CTC head (build it with Transformer(..., ctc=True))")
    return _ctc_logits_of(model, _encode(model, spectrum, pad_lengths(model, input_lengths)))


@torch.no_grad()
def _ctc_logits_of(model, enc):
    """The CTC head on an encoder output (B, T', d): (fp32 logits [B*T', Vp], B, T')."""
    B, T, d = enc.shape
    C = make_ctx(model, 0.0)
    return ctc_head_fwd(C, model, enc.reshape(B * T, d).to(C.cd).contiguous()), B, T


@torch.no_grad()
def transformer_ctc_greedy(model, spectrum, input_lengths=None):
    logits, B, T = transformer_ctc_logits(model, spectrum, input_lengths)
    if input_lengths is not None:
        input_lengths = input_lengths.to(device=logits.device, dtype=torch.int32).contiguous()
    return K.ctc_greedy(logits, model.ctc_head.V, T, model.ctc_blank, input_lengths)


@torch.no_grad()
def transformer_align(model, spectrum, text, mask=None, input_lengths=None, *, bos_token_id=1):
    """Transformer.align: front end, encoder and CTC head, the transcript's CTC targets as the Trainer builds them
    (asrx_ctc_targets: `text` (B, n) where mask >= 1, without BOS / EOS / PAD), then asrx_ctc_align."""
    logits, B, T = transformer_ctc_logits(model, spectrum, input_lengths)
    dev = logits.device
    dec = model.decoder
    drop = [int(bos_token_id), int(dec._eos_token_id)]
    if dec.pad_token_id is not None:
        drop.append(int(dec.pad_token_id))
    text = text.to(device=dev, dtype=torch.int64)
    if text.dim() != 2 or text.shape[0] != B:
        raise ValueError(f"text {tuple(text.shape)} does not hold one row for each of the {B} spectrograms")
    if mask is None:
        mask = torch.ones_like(text) if dec.pad_token_id is None else text != int(dec.pad_token_id)
    targets, lengths = K.ctc_targets(text if text.stride(1) == 1 else text.contiguous(),
                                     mask.to(device=dev, dtype=torch.float32).contiguous(), drop, model.ctc_blank)
    if input_lengths is not None:
        input_lengths = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
    # (a row longer than the kernel's 255 labels has no alignment there: its score is -inf)
    return K.ctc_align(logits, model.ctc_head.V, T, targets, lengths, input_lengths,
                       max_target_len=min(targets.shape[1], 255), blank=model.ctc_blank)


# ------------------------------------------------------------------------------------------- two-pass decoding

class RescoreResult(BeamResult):
    """A BeamResult (tokens, lengths, scores: the same three fields, so it unpacks and indexes alike) that also
    carries the two terms of the combined score: att_scores and ctc_scores, fp32 (B, nbest), and, where the order is
    a minimum-Bayes-risk one (rescore(mbr_scale=...), asrx.mbr_rerank), `risks`: each hypothesis's expected edit
    distance under the n-best posterior, fp32 (B, nbest), else None.  `lm_scores`: each hypothesis's log p_lm where a
    language model took part in the ranking (rescore(lm=...)), fp32 (B, nbest), else None; ctc_scores stays pure."""

    def __new__(cls, tokens, lengths, scores, att_scores=None, ctc_scores=None, risks=None, lm_scores=None):
        self = super().__new__(cls, tokens, lengths, scores)
        self.att_scores, self.ctc_scores, self.risks, self.lm_scores = att_scores, ctc_scores, risks, lm_scores
        return self


BOS_ID = 1          # the start token of a decode without a prompt (transformer_beam_search's text=None)
IGNORE_ID = -1      # target id of the positions asrx_seq_logprob leaves out


def _rescore_labels(dec, max_len):
    """max_labels of a two-pass decode: the decoder row holds BOS and the labels, its targets the labels and EOS."""
    L = min(dec._seq_len if max_len is None else int(max_len), 255)
    if L < 2:
        raise ValueError(f"two-pass decoding needs a decoder length >= 2, got {L}")
    if L > dec._pe.pe[0].shape[0]:
        raise ValueError(f"decoder length {L} exceeds the PE table ({dec._pe.pe[0].shape[0]}) as in layers.py:73")
    return L, L - 1


def _check_beam(beam, nbest):
    W, nbest = int(beam), int(nbest)
    if not 1 <= W <= 16:
        raise ValueError(f"beam must be in 1..16, got {beam}")
    if not 1 <= nbest <= W:
        raise ValueError(f"nbest must be in 1..beam, got {nbest}")
    return W, nbest


def _first_pass(ctc, B, V, W, max_labels, dev):
    """ctc = (logits, T, blank, input_lengths[, V]): the head's vocabulary is the fifth entry where the caller has the
    head (the Transformer entries pass it); without it the decoder's V is taken, which a shared vocabulary makes the
    same."""
    logits, T, blank, lengths = ctc[:4]
    V = int(ctc[4]) if len(ctc) > 4 else V
    if not 0 <= int(blank) < V <= logits.shape[1]:
        raise ValueError(f"CTC vocabulary {V} / blank {blank} do not fit logits of {logits.shape[1]} columns")
    if lengths is not None:
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
    if logits.shape[0] != B * int(T):
        raise ValueError(f"CTC logits have {logits.shape[0]} rows, expected B * T = {B * int(T)}")
    return K.ctc_prefix_beam(logits, V, int(T), int(blank), W, max_labels, lengths)


def _words(*ts):
    """One int32 device vector of the given int32 / fp32 / int64 tensors (a single host copy then reads them all)."""
    return torch.cat([t.contiguous().view(torch.int32).reshape(-1) for t in ts])


def _split(flat, *shapes_dtypes):
    out, o = [], 0
    for shape, dt in shapes_dtypes:
        n = 1
        for s in shape:
            n *= s
        n *= 2 if dt == torch.int64 else 1
        out.append(flat[o:o + n].view(dt).reshape(shape))
        o += n
    return out


@torch.no_grad()
def decoder_ctc_beam_search(dec, ctc, B, beam=8, nbest=1, max_len=None):
    """The first pass alone (asrx_ctc_prefix_beam): per sample the `nbest` best of `beam` CTC prefix-beam hypotheses.
    ctc = (logits, T, blank, input_lengths[, V of the head]) as in decoder_beam_search.  BeamResult: tokens (B, nbest, max_labels)
    int64 labels padded with the blank id, lengths (B, nbest) label counts, scores (B, nbest) fp32 log p_ctc (-inf:
    fewer hypotheses exist).  One host copy at the end."""
    W, nbest = _check_beam(beam, nbest)
    _, max_labels = _rescore_labels(dec, max_len)
    dev = ctc[0].device
    tok, lens, score, _ = _first_pass(ctc, B, dec._classifier.V, W, max_labels, dev)
    flat = _words(tok, lens, score).cpu()
    tok, lens, score = _split(flat, ((B, W, max_labels), torch.int64), ((B, W), torch.int32), ((B, W), torch.float32))
    return BeamResult(tok[:, :nbest].clone(), lens[:, :nbest].long(), score[:, :nbest].clone())


@torch.no_grad()
def decoder_rescore(dec, enc_x, ctc, beam=8, ctc_weight=0.5, nbest=1, final_norm=True, max_len=None, mbr_scale=None,
                    lm=None, lm_weight=0.0, token_bonus=0.0, enc_lengths=None):
    """Two-pass decoding ("attention rescoring"): asrx_ctc_prefix_beam yields `beam` complete hypotheses per sample
    from the CTC head's logits alone; ONE teacher-forced decoder forward over all B * beam of them (rows BOS, labels;
    targets labels, EOS; cross-attention grouped per sample, nothing expanded) gives each log p_att, and they are
    ranked by log p_att + ctc_weight * log p_ctc.  ctc = (logits, T, blank, input_lengths[, V of the head]);
    at most min(max_len or seq_len, 255) - 1 labels.  Everything runs on the device in a fixed launch sequence with
    one host copy at the end.  Returns a RescoreResult filled as beam_search fills a BeamResult: tokens (B, nbest,
    1 + L) = BOS, labels, EOS..., lengths = labels + 1 (0: no such hypothesis), scores = the combined score, plus
    att_scores and ctc_scores.  Eval only: dropout is off.

    mbr_scale = a number >= 0: the final order is the minimum-Bayes-risk one instead.  The first pass's labels, still
    on the device, go through asrx_edit_distance (all beam x beam pairs per sample) and asrx_mbr_rank with the
    posterior softmax(mbr_scale * combined score): two more launches before the same single host copy, and `risks`
    is filled.  None (default) issues exactly the launches above.

    lm (an asrx.NgramLM on the device) with lm_weight = beta > 0: the rank is log p_att + ctc_weight * log p_ctc +
    beta * log p_lm + token_bonus * len, the LM over the labels and the EOS after its sentence start.  One more launch
    (asrx_ngram_seq_logprob, which folds the CTC term in; asrx_rescore_rank then adds the two sums), and `lm_scores`
    is filled.  lm=None or lm_weight = 0 (default) issues exactly the launches above.

    enc_lengths (valid rows of each encoder output): the second pass's cross-attention masks the padded rows, one row
    of key validity per sample for its `beam` hypotheses.  None (default): the launches above."""
    lam = float(ctc_weight)
    if lam != lam or lam < 0.0:
        raise ValueError(f"ctc_weight {ctc_weight} must be >= 0")
    beta, bonus = check_lm(lm, lm_weight, token_bonus, dec._classifier.V)
    if mbr_scale is not None:
        mbr_scale = float(mbr_scale)
        if mbr_scale != mbr_scale or mbr_scale < 0.0:
            raise ValueError(f"mbr_scale {mbr_scale} must be >= 0")
    if ctc is None:
        raise RuntimeError("asrx: rescoring needs the CTC head's logits (a model built with ctc=True)")
    W, nbest = _check_beam(beam, nbest)
    L, max_labels = _rescore_labels(dec, max_len)
    C = make_ctx(dec, 0.0)
    C.train, C.p = False, 0.0
    dev = enc_x.device
    B, Te, d = enc_x.shape
    cls = dec._classifier
    eos = int(dec._eos_token_id)
    pad = int(dec.pad_token_id if dec.pad_token_id is not None else 0)
    if B == 0:
        z = torch.zeros(0, nbest, dtype=torch.float32)
        return RescoreResult(torch.zeros(0, nbest, 1 + L, dtype=torch.int64), torch.zeros(0, nbest, dtype=torch.int64),
                             z, z.clone(), z.clone(), None if mbr_scale is None else z.clone(),
                             z.clone() if beta > 0.0 else None)
    R = B * W
    tok, lens, cscore, n_hyp = _first_pass(ctc, B, cls.V, W, max_labels, dev)
    dec_in, dec_tgt, mask = K.hyp_tokens(tok, lens, n_hyp, B, W, L, BOS_ID, eos, pad, IGNORE_ID)
    enc_c = torch.empty(B * Te, d, dtype=C.cd, device=dev)
    K.cast(enc_x.reshape(B * Te, d).contiguous(), enc_c)
    logits, _ = decoder_fwd(C, dec, dec_in, mask, enc_c, R, L, Te, final_norm=final_norm, group=W,
                            xspec=key_spec(enc_lengths, B, Te, dev)[1])
    att = K.seq_logprob(logits, cls.V, dec_tgt, IGNORE_ID, n_hyp, W)
    if beta > 0.0:
        lm_s, rest = K.ngram_seq_logprob(lm, dec_tgt, IGNORE_ID, n_hyp, W, cscore, lam, beta, bonus)
        score, order = K.rescore_rank(att, rest, B, W, 1.0, 1.0)
    else:
        score, order = K.rescore_rank(att, cscore, B, W, 1.0, lam)
    f32, i32 = torch.float32, torch.int32
    tail = []                                   # optional [B, W] fp32 vectors behind the six fixed ones
    if mbr_scale is not None:
        dist, _ = K.edit_distance(tok, None, lens, None, (), None, "cross", W, n_hyp, counts=False)
        risk, order = K.mbr_rank(dist, score, B, W, mbr_scale, n_hyp)
        tail.append(risk)
    if beta > 0.0:
        tail.append(lm_s)
    flat = _words(dec_tgt, lens, order, score, att, cscore, *tail).cpu()
    tail = list(flat[flat.numel() - len(tail) * B * W:].view(f32).reshape(len(tail), B, W))
    lm_s = tail.pop() if beta > 0.0 else None
    risk = tail.pop() if mbr_scale is not None else None
    tgt, lens, order, score, att, cscore = _split(flat, ((B, W, L), torch.int64), ((B, W), i32), ((B, W), i32),
                                                  ((B, W), f32), ((B, W), f32), ((B, W), f32))
    order = order[:, :nbest].long()
    live = torch.isfinite(score.gather(1, order))
    rows = tgt.gather(1, order[:, :, None].expand(-1, -1, L))
    rows = torch.where(rows == IGNORE_ID, torch.full_like(rows, eos), rows)
    tokens = torch.cat([torch.full((B, nbest, 1), BOS_ID, dtype=torch.int64), rows], dim=2)
    lengths = torch.where(live, lens.gather(1, order).long() + 1, torch.zeros(B, nbest, dtype=torch.int64))
    return RescoreResult(tokens, lengths, score.gather(1, order), att.gather(1, order), cscore.gather(1, order),
                         None if risk is None else risk.gather(1, order),
                         None if lm_s is None else lm_s.gather(1, order))


def transformer_ctc_beam_search(model, spectrum, beam=8, input_lengths=None, nbest=1, max_len=None):
    """Transformer.ctc_beam_search: front end, encoder, CTC head and the first pass only."""
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("asrx: CTC beam search needs a model with a CTC head (Transformer(..., ctc=True))")
    _check_beam(beam, nbest)
    logits, B, T = transformer_ctc_logits(model, spectrum, input_lengths)
    ctc = (logits, T, model.ctc_blank, input_lengths, model.ctc_head.V)
    return decoder_ctc_beam_search(model.decoder, ctc, B, beam, nbest, max_len)


def transformer_rescore(model, spectrum, beam=8, ctc_weight=0.5, input_lengths=None, nbest=1, final_norm=True,
                        max_len=None, mbr_scale=None, lm=None, lm_weight=0.0, token_bonus=0.0):
    """Transformer.rescore: front end and encoder as in `evaluate`, the CTC head on the one encoder output, then
    decoder_rescore."""
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("asrx: rescoring needs a model with a CTC head (Transformer(..., ctc=True))")
    lam = float(ctc_weight)
    if lam != lam or lam < 0.0:
        raise ValueError(f"ctc_weight {ctc_weight} must be >= 0")
    _check_beam(beam, nbest)
    check_lm(lm, lm_weight, token_bonus, model.decoder._classifier.V)
    lens = pad_lengths(model, input_lengths)
    with torch.no_grad():
        enc = _encode(model, spectrum, lens)
    logits, B, T = _ctc_logits_of(model, enc)
    return decoder_rescore(model.decoder, enc, (logits, T, model.ctc_blank, input_lengths, model.ctc_head.V), beam,
                           lam, nbest, final_norm, max_len, mbr_scale, lm, lm_weight, token_bonus, enc_lengths=lens)


# ------------------------------------------------------------------------------------------- sub-modules

def _cd_input(C, x):
    return x.reshape(-1, x.shape[-1]).to(C.cd).contiguous()


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ln, C, x, *params):
        x2 = x.reshape(-1, x.shape[-1]).float().contiguous()
        y, mean, rstd = Bk.ln_fwd(C, x2, ln, out_dtype=torch.float32)
        ctx.ln, ctx.C, ctx.S, ctx.shape = ln, C, (x2, mean, rstd), x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        C = ctx.C
        _prepare_grads(C)
        x2, mean, rstd = ctx.S
        dx = Bk.ln_bwd(C, x2, g.reshape(x2.shape).float().contiguous(), ctx.ln, mean, rstd)
        return (None, None, dx.view(ctx.shape)) + (None,) * len(_params(ctx.ln))


def layernorm(ln, x):
    C = make_ctx(ln, 0.0)
    return _LayerNormFn.apply(ln, C, x, *_params(ln))


class _MHAFn(torch.autograd.Function):
    """Standalone MHA: y = Drop(W_o . attn(x W_q, kv W_k, kv W_v) + b_o) — no LayerNorm, no residual."""

    @staticmethod
    def forward(ctx, m, C, x, enc_x, attention_mask, *params):
        B, Lq, d = x.shape
        Lk = Lq if enc_x is None else enc_x.shape[1]
        H = m.num_heads
        xc = _cd_input(C, x)
        kc = xc if enc_x is None else _cd_input(C, enc_x)
        spec = MaskSpec.from_attention_mask(attention_mask.to(xc.device) if attention_mask is not None else None,
                                            B, Lq, Lk)
        y, S = Bk.attn_core_fwd(C, _mha_fwd_w(C, m), xc, B, H, d // H, Lq, Lk, spec, xk=kc)
        ctx.m, ctx.C, ctx.S = m, C, S
        ctx.io = (enc_x is None, x.dtype, (x if enc_x is None else enc_x).dtype, Lk)
        return y.view(B, Lq, d).to(x.dtype) if x.dtype != torch.float32 else y.view(B, Lq, d)

    @staticmethod
    def backward(ctx, g):
        C, S, m = ctx.C, ctx.S, ctx.m
        _prepare_grads(C)
        B, Lq, d = g.shape
        self_attn, xdtype, kdtype, Lk = ctx.io
        # dropout bwd of the output (same RNG stream as the forward epilogue)
        dy_c = Bk.drop_bwd_c(C, g.reshape(B * Lq, d).contiguous(), S["sd"])
        w = [(C.W(p)[r], C.G(p)[r], C.G(b)[r]) for p, b, r in _mha_params(m)]
        dx, dk_in, _ = Bk.attn_core_bwd(C, S, w, dy_c, C.wgrad, torch.float32, sum_dk=self_attn)
        dx = Bk.as_dtype(dx.view(B, Lq, d), xdtype)
        dk = None if self_attn else Bk.as_dtype(dk_in.view(B, Lk, d), kdtype)
        return (None, None, dx, dk, None) + (None,) * len(_params(m))


def mha(m, x, enc_x=None, attention_mask=None):
    C = make_ctx(m, m.p)
    return _MHAFn.apply(m, C, x, enc_x, attention_mask, *_params(m))


class _FFNFn(torch.autograd.Function):
    """Standalone FeedForward (layers.py:53-58), no residual."""

    @staticmethod
    def forward(ctx, ff, C, x, *params):
        xc = _cd_input(C, x)
        y, f, _ = Bk.ffn_core_fwd(C, Bk.ffn_w_fwd(C, ff), xc)
        ctx.ff, ctx.C, ctx.S = ff, C, (xc, f, x.shape, x.dtype)
        return y.view(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        C, ff = ctx.C, ctx.ff
        _prepare_grads(C)
        xc, f, shape, xdt = ctx.S
        g_c = g.reshape(xc.shape[0], -1).float().contiguous().to(C.cd)
        dx, _ = Bk.ffn_core_bwd(C, Bk.ffn_w_bwd(C, ff), xc, f, None, g_c, C.wgrad, torch.float32)
        return (None, None, dx.view(shape).to(xdt)) + (None,) * len(_params(ff))


def feed_forward(ff, x):
    C = make_ctx(ff, ff.p)
    return _FFNFn.apply(ff, C, x, *_params(ff))


class _EncLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, C, x, *params):
        B, T, d = x.shape
        x32 = x.reshape(B * T, d).float().contiguous()
        y, S = Bk.enc_layer_fwd(C, x32, layer, B, T, layer.num_heads)
        ctx.layer, ctx.C, ctx.S, ctx.xdt = layer, C, S, x.dtype
        return y.view(B, T, d).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        C = ctx.C
        _prepare_grads(C)
        B, T, d = g.shape
        g32 = g.reshape(B * T, d).float().contiguous()
        dx = Bk.enc_layer_bwd(C, ctx.S, g32, g32.to(C.cd), None)
        return (None, None, dx.view(B, T, d).to(ctx.xdt)) + (None,) * len(_params(ctx.layer))


def encoder_layer(layer, x):
    C = make_ctx(layer, layer.p)
    return _EncLayerFn.apply(layer, C, x, *_params(layer))


class _DecLayerFn(torch.autograd.Function):
    """Standalone DecoderLayer(x, mask, enc_x): `mask` is the attention mask as the reference passes it to
    the layer (bool/uint8 broadcastable to (B, L, L), >0 = masked), cross-attention K/V from enc_x."""

    @staticmethod
    def forward(ctx, layer, C, x, mask, enc_x, *params):
        B, L, d = x.shape
        Te = enc_x.shape[1]
        x32 = x.reshape(B * L, d).float().contiguous()
        enc_c = _cd_input(C, enc_x)
        ca = layer._cross_attention
        kv = torch.empty(B * Te, 2 * d, dtype=C.cd, device=x32.device)
        K.linear(enc_c, C.W(ca.wkv), kv, bias=ca.bkv.data)
        spec = MaskSpec.from_attention_mask(mask.to(x32.device) if mask is not None else None, B, L, L)
        y, S = Bk.dec_layer_fwd(C, x32, layer, B, L, layer.num_heads, spec, kv, 2 * d, Te)
        ctx.layer, ctx.C, ctx.S, ctx.extra = layer, C, S, (enc_c, kv, x.dtype, enc_x.dtype, Te)
        return y.view(B, L, d).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        C, layer = ctx.C, ctx.layer
        _prepare_grads(C)
        enc_c, kv, xdt, edt, Te = ctx.extra
        B, L, d = g.shape
        g32 = g.reshape(B * L, d).float().contiguous()
        dkv = torch.empty(B * Te, 2 * d, dtype=C.cd, device=g32.device)
        dx = Bk.dec_layer_bwd(C, ctx.S, g32, g32.to(C.cd), dkv, None)
        ca = layer._cross_attention
        denc = torch.empty(B * Te, d, dtype=torch.float32, device=g32.device)
        K.linear_dgrad(dkv, C.W(ca.wkv), denc)
        K.linear_wgrad(dkv, enc_c, C.G(ca.wkv), bias_grad=C.G(ca.bkv))
        return (None, None, dx.view(B, L, d).to(xdt), None, denc.view(B, Te, d).to(edt)) + \
            (None,) * len(_params(layer))


def decoder_layer(layer, x, mask, enc_x):
    C = make_ctx(layer, layer.p)
    return _DecLayerFn.apply(layer, C, x, mask, enc_x, *_params(layer))
