"""Drop-in replacement for modules/Transformer/new/model.py — the reference's second, post-LN model family
(Encoder / Decoder / their layers / Transformer with the batch-dict forward and the greedy evaluate).  Same
constructor arguments, forward signatures and state_dict schema (tests/test_host_cpu.py checks it against the
reference); compute on libasrx.so through asrx.new.ops.

Behaviour is that of the variant run with its own new/layers.py and new/masking.py (as shipped it imports the main
modules and raises).  Masks are built in their structured form — key validity by length or by the EOS
padding token, causality — instead of the reference's expanded (B, L, L) tensors, which the attention kernels would
re-read per score.  The softmax of a row whose keys are ALL masked is NaN in the reference (no nan_to_num in
new/layers.py:29) and 0 here; no such row occurs in the variant's use (every query sees BOS / a frame of length >= 1).
The VGG front-end (new/model.py:163-174) is built for state_dict compatibility and, as in the reference, unused.
"""
import math

import torch
from torch import nn

from .. import blocks as Bk
from .. import kernels as K
from ..layers import LayerNorm, _Lin
from . import ops as O
from .layers import MHA, FeedForward, TrainablePositionalEncoding


def _cfg(m, p):
    root = getattr(m, "_asrx_root", None)
    root = root() if root is not None else m
    cd = torch.bfloat16 if getattr(root, "precision", "fp32") == "bf16" else torch.float32
    dev = next(m.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("asrx.new: the model must live on the GPU (no CPU fallback)")
    return O.Cfg(cd, p, m.training, dev)


def _mha_args(m, cross):
    hd = m.num_heads * m.emb_dim
    if cross:
        return m.wqkv[:hd], m.bqkv[:hd], m.wqkv[hd:], m.bqkv[hd:], m.out.weight, m.out.bias
    return m.wqkv, m.bqkv, None, None, m.out.weight, m.out.bias


def _spec_from(attention_mask, B, Lq, Lk, device):
    if attention_mask is None or isinstance(attention_mask, K.MaskSpec):
        return attention_mask if attention_mask is not None else K.MaskSpec()
    return K.MaskSpec.from_attention_mask(attention_mask.to(device), B, Lq, Lk)


def mha_forward(m, x, enc_x=None, attention_mask=None, cfg=None):
    """MHA.forward (new/layers.py:44-46); attention_mask: a dense mask (> 0 = masked) or a kernels.MaskSpec."""
    cfg = cfg or _cfg(m, m.p)
    B, Lq, _ = x.shape
    Lk = enc_x.shape[1] if enc_x is not None else Lq
    spec = _spec_from(attention_mask, B, Lq, Lk, x.device)
    return O.MHAResFn.apply(x.float(), None if enc_x is None else enc_x.float(), spec, m, cfg,
                            *_mha_args(m, enc_x is not None))


def ffn_forward(ff, x, cfg=None):
    cfg = cfg or _cfg(ff, ff.p)
    return O.FFNResFn.apply(x.float(), cfg, ff.squeeze.weight, ff.squeeze.bias, ff.unsqueeze.weight,
                            ff.unsqueeze.bias)


def _post_ln(ln, x, rows_mask):
    """LN(x) * non_pad_mask (new/model.py:24-25): rows_mask fp32 [B*L] (or None)."""
    B, L, d = x.shape
    y = O.LNFn.apply(x.reshape(B * L, d), ln.weight, ln.bias, "scale" if rows_mask is not None else None, rows_mask)
    return y.view(B, L, d)


def _rows(non_pad_mask, B, L, device):
    """non_pad_mask (B, L, 1) / (B, L) of 0/1 -> fp32 [B*L] (a contiguous view; no copy when already so)."""
    if non_pad_mask is None:
        return None
    return non_pad_mask.reshape(B * L).to(device=device, dtype=torch.float32).contiguous()


class EncoderLayer(nn.Module):
    """new/model.py:9-29: x = norm1(MHA(x, mask)) * npm; x = norm2(FF(x)) * npm (post-LN, residuals inside)."""

    def __init__(self, emb_dim, num_heads, ff_dim, dropout):
        super().__init__()
        self.emb_dim, self.num_heads, self.ff_dim, self.dropout = emb_dim, num_heads, ff_dim, dropout
        self.attention = MHA(num_heads, emb_dim, dropout)
        self.norm1 = LayerNorm(emb_dim)
        self.ff = FeedForward(emb_dim, ff_dim, dropout)
        self.norm2 = LayerNorm(emb_dim)

    def forward(self, x, attention_mask, non_pad_mask, cfg=None):
        cfg = cfg or _cfg(self, self.dropout)
        B, T, _ = x.shape
        rows = _rows(non_pad_mask, B, T, x.device)
        x = _post_ln(self.norm1, mha_forward(self.attention, x, None, attention_mask, cfg), rows)
        return _post_ln(self.norm2, ffn_forward(self.ff, x, cfg), rows)


class Encoder(nn.Module):
    """new/model.py:32-64: (B, C, F, T) -> (B, T, C*F) -> norm_in(lin_in(x)) + pe -> layers, with the frames past
    each length masked as keys and zeroed after every norm."""

    def __init__(self, seq_len, emb_dim, num_layers, num_heads, ff_dim, dropout=0.1):
        super().__init__()
        self.seq_len, self.emb_dim, self.num_layers = seq_len, emb_dim, num_layers
        self.num_heads, self.ff_dim, self.dropout = num_heads, ff_dim, dropout
        self.lin_in = _Lin(emb_dim, emb_dim)
        self.norm_in = LayerNorm(emb_dim)
        self.pe = TrainablePositionalEncoding(self.seq_len, self.emb_dim)
        self.layers = nn.ModuleList([EncoderLayer(emb_dim, num_heads, ff_dim, dropout) for _ in range(num_layers)])

    def forward(self, x, lens, cfg=None):
        B, C, Fm, T = x.shape
        d = self.emb_dim
        if T > self.pe.pe.shape[1]:
            # the reference's `x + self.pe[:, :T]` fails to broadcast there (new/layers.py:79-80)
            raise ValueError(f"asrx.new.Encoder: {T} frames exceed the positional table's {self.pe.pe.shape[1]}")
        cfg = cfg or _cfg(self, self.dropout)
        xt = torch.empty(B, T, C * Fm, dtype=torch.float32, device=x.device)
        K.transpose_last2(x.reshape(B, C * Fm, T).float().contiguous(), xt)
        valid = torch.arange(T, device=x.device).unsqueeze(0) < lens.to(x.device).reshape(-1, 1)   # mask glue
        rows = valid.reshape(-1).float()
        spec = O.valid_spec(valid)
        h = O.LinearFn.apply(xt.view(B * T, C * Fm), self.lin_in.weight, self.lin_in.bias, cfg)
        h = O.LNFn.apply(h, self.norm_in.weight, self.norm_in.bias, "add", self.pe.pe[0, :T].contiguous())
        h = h.view(B, T, d)
        for layer in self.layers:
            h = layer(h, spec, rows, cfg)
        return h


class DecoderLayer(nn.Module):
    """new/model.py:67-91: masked self-attention, cross-attention (encoder key mask), FF — each post-LN * npm."""

    def __init__(self, emb_dim, num_heads, ff_dim, dropout):
        super().__init__()
        self.emb_dim, self.num_heads, self.ff_dim, self.dropout = emb_dim, num_heads, ff_dim, dropout
        self.mask_attention = MHA(num_heads, emb_dim, dropout)
        self.norm1 = LayerNorm(emb_dim)
        self.attention = MHA(num_heads, emb_dim, dropout)
        self.norm2 = LayerNorm(emb_dim)
        self.ff = FeedForward(emb_dim, ff_dim, dropout)
        self.norm3 = LayerNorm(emb_dim)

    def forward(self, x, attention_mask, enc_x, enc_mask, non_pad_mask, cfg=None):
        cfg = cfg or _cfg(self, self.dropout)
        B, L, _ = x.shape
        rows = _rows(non_pad_mask, B, L, x.device)
        x = _post_ln(self.norm1, mha_forward(self.mask_attention, x, None, attention_mask, cfg), rows)
        x = _post_ln(self.norm2, mha_forward(self.attention, x, enc_x, enc_mask, cfg), rows)
        return _post_ln(self.norm3, ffn_forward(self.ff, x, cfg), rows)


class Decoder(nn.Module):
    """new/model.py:94-142: EOS is the padding token of the decoder rows (:117-118); forward(x, enc_x, enc_lens) ->
    logits (B, L, V); evaluate(enc_x, device) -> (tokens (B, seq_len + 1) int32, last logits, eoses)."""

    def __init__(self, vocab_size, seq_len, emb_dim, num_layers, num_heads, ff_dim, eos_token, bos_token, dropout=0.1,
                 padding_idx=0):
        super().__init__()
        self.seq_len, self.emb_dim, self.num_layers = seq_len, emb_dim, num_layers
        self.num_heads, self.ff_dim, self.vocab_size = num_heads, ff_dim, vocab_size
        self.padding_idx, self.eos_token, self.bos_token = padding_idx, eos_token, bos_token
        self.p = float(dropout)
        self.emb = nn.Embedding(vocab_size, emb_dim, padding_idx=padding_idx)
        self.pe = TrainablePositionalEncoding(self.seq_len, self.emb_dim)
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([DecoderLayer(emb_dim, num_heads, ff_dim, dropout) for _ in range(num_layers)])
        self.classifier = _Lin(emb_dim, vocab_size, bias=False)

    def _check_len(self, L):
        if L > self.pe.pe.shape[1]:
            # embed_fwd reads pe[t] for every t < L: past the table is past its allocation (the reference's broadcast
            # of pe[:, :L] raises, new/layers.py:79-80)
            raise ValueError(f"asrx.new.Decoder: {L} tokens exceed the positional table's {self.pe.pe.shape[1]}")

    def _run(self, x, enc_x, self_spec, enc_spec, rows, cfg):
        B, L = x.shape
        d = self.emb_dim
        self._check_len(L)
        h = O.EmbedFn.apply(self.emb.weight, x, self.pe.pe[0, :L].contiguous(), L, self.padding_idx, cfg)
        h = h.view(B, L, d)
        enc_x = enc_x.float()
        for layer in self.layers:
            h = layer(h, self_spec, enc_x, enc_spec, rows, cfg)
        return O.LinearFn.apply(h.reshape(B * L, d), self.classifier.weight, None, cfg).view(B, L, self.vocab_size)

    def forward(self, x, enc_x, enc_lens, cfg=None):
        B, L = x.shape
        self._check_len(L)
        cfg = cfg or _cfg(self, self.p)
        dev = enc_x.device
        x = x.to(dev)
        valid = x.ne(self.eos_token)                                                           # mask glue
        Te = enc_x.shape[1]
        enc_valid = torch.arange(Te, device=dev).unsqueeze(0) < enc_lens.to(dev).reshape(-1, 1)
        return self._run(x, enc_x, O.valid_spec(valid, causal=True), O.valid_spec(enc_valid),
                         valid.reshape(-1).float(), cfg)

    def evaluate(self, enc_x, device, cache=True):
        """new/model.py:125-142: greedy from BOS for seq_len steps (causal mask only, no cross mask, all rows kept);
        the argmax of each step on the device, the EOS steps resolved once at the end.  cache (default, round 6): the
        KV-cached decode of _evaluate_cached; False — or dropout active (training mode), whose masks are drawn per
        full-prefix pass — recomputes the full prefix every step as the reference does."""
        cfg = _cfg(self, self.p)
        if cache and cfg.p == 0.0:
            return self._evaluate_cached(enc_x, device, cfg)
        B = enc_x.shape[0]
        dev = enc_x.device
        dec_in = torch.full((B, 1), self.bos_token, dtype=torch.int64, device=dev)
        causal = O.valid_spec(None, causal=True)
        prob, nexts = None, []
        for _ in range(self.seq_len):
            L = dec_in.shape[1]
            prob = self._run(dec_in, enc_x, causal, K.MaskSpec(), None, cfg)
            nxt = torch.empty(B, 1, dtype=torch.int64, device=dev)
            last = prob[:, -1].contiguous()
            K.greedy_argmax(last, self.vocab_size, nxt[:, 0])
            nexts.append(nxt)
            dec_in = torch.cat([dec_in, nxt], dim=1)
        steps = torch.cat(nexts, dim=1).cpu()                 # one host synchronisation
        eoses = torch.full((B,), self.seq_len - 1)
        for i in range(self.seq_len):
            eoses[steps[:, i] == self.eos_token] = i
        return dec_in.to(torch.int32).to(device), prob, eoses


    def _evaluate_cached(self, enc_x, device, cfg):
        """The reference's greedy loop (new/model.py:125-142) recomputes every prefix position at every step; with
        the causal self-attention the logits of position t do not depend on later tokens, so only the new position
        runs through the layers: its self-attention K / V join per-layer caches [B, seq_len, 2 h d], and every layer's
        cross-attention K / V of the encoder output are projected once.  The logits of position t are written when t
        is processed; after the last step they are the reference's final-step logits (all seq_len positions)."""
        cd = cfg.cd
        B, Te, d = enc_x.shape
        dev = enc_x.device
        S, H, n, V = self.seq_len, self.num_heads, self.num_layers, self.vocab_size
        hd = H * d
        self._check_len(S)
        C, none = cfg.ctx, K.MaskSpec()
        enc_c = O._cd(enc_x.reshape(B * Te, d).float().contiguous(), cd)

        def ln(x, norm):          # the post-LN of new/model.py:80-89 (non_pad_mask is all ones in evaluate)
            y = torch.empty_like(x)
            K.layernorm_fwd(x, norm.weight.detach(), norm.bias.detach(), y)
            return y

        lw = []   # per layer: the cast weights of the three sublayers, the cross K / V of the encoder output
        for layer in self.layers:
            sa, ca, ff = layer.mask_attention, layer.attention, layer.ff
            wq = O._w(ca.wqkv, cd)
            kvx = torch.empty(B * Te, 2 * hd, dtype=cd, device=dev)
            K.linear(enc_c, wq[hd:], kvx, bias=ca.bqkv[hd:].detach())
            wqkv, bqkv = O._w(sa.wqkv, cd), sa.bqkv.detach()
            lw.append(((wqkv[:hd], bqkv[:hd], wqkv[hd:], bqkv[hd:], O._w(sa.out.weight, cd), sa.out.bias.detach()),
                       (wq[:hd], ca.bqkv[:hd].detach(), None, None, O._w(ca.out.weight, cd), ca.out.bias.detach()),
                       (O._w(ff.squeeze.weight, cd), ff.squeeze.bias.detach(),
                        O._w(ff.unsqueeze.weight, cd), ff.unsqueeze.bias.detach()), kvx))
        wcls = O._w(self.classifier.weight, cd)
        caches = torch.empty(n, B, S, 2 * hd, dtype=cd, device=dev)
        logits = torch.empty(B, S, V, dtype=torch.float32, device=dev)
        tokens = torch.empty(B, S + 1, dtype=torch.int64, device=dev)
        tokens[:, 0] = self.bos_token
        cur = tokens[:, 0].contiguous()
        pe = self.pe.pe[0]
        for t in range(S):
            x = torch.empty(B, d, dtype=torch.float32, device=dev)
            K.embed_fwd(cur, self.emb.weight.detach(), pe[t:t + 1].contiguous(), x, 1)   # (eval: no dropout)
            for layer, cache, (w_self, w_cross, w_ff, kvx) in zip(self.layers, caches, lw):
                # masked self-attention: the new position's K / V into the cache, its query over positions 0..t
                xc = O._cd(x, cd)
                y, _ = Bk.attn_core_fwd(C, w_self, xc, B, H, d, 1, t + 1, none, xk=xc, kv=cache, kv_dst=cache[:, t],
                                        resid=x)
                x1 = ln(y, layer.norm1)
                # cross-attention over the encoder output (no mask in evaluate, new/model.py:136)
                y2, _ = Bk.attn_core_fwd(C, w_cross, O._cd(x1, cd), B, H, d, 1, Te, none, kv=kvx, resid=x1)
                x2 = ln(y2, layer.norm2)
                # feed-forward with its residual
                y3, _, _ = Bk.ffn_core_fwd(C, w_ff, O._cd(x2, cd), resid=x2)
                x = ln(y3, layer.norm3)
            lg = logits[:, t]
            K.gemm(O._cd(x, cd), wcls, lg, B, V, d, lda=d, ldb=d, ldc=S * V)
            K.greedy_argmax(lg, V, tokens[:, t + 1], cur)
        steps = tokens[:, 1:].cpu()                           # one host synchronisation
        eoses = torch.full((B,), S - 1)
        for i in range(S):
            eoses[steps[:, i] == self.eos_token] = i
        return tokens.to(torch.int32).to(device), logits, eoses


class Transformer(nn.Module):
    """new/model.py:145-209.  forward(batch) with batch = {'spectre' (B, 1, n_mels, T), 'spectrogram_len' (B,),
    'encoded_text' (B, dec_seq_len)} -> logits (B, L, V); evaluate(batch) -> (tokens, last logits, eoses).
    precision: "fp32" (the reference's) or "bf16" (GEMM operands bf16, fp32 accumulation and residual stream)."""

    def __init__(self, vocab_size, n_mels, enc_seq_len, dec_seq_len, hidden_dim, enc_num_layers, dec_num_layers,
                 num_heads, ff_dim, device, dropout=0.1, sr=16000, n_fft=1024, padding_idx=4, eos_token=2, bos_token=1,
                 *, precision="fp32"):
        super().__init__()
        self.n_mels = n_mels
        self.enc_seq_len = math.ceil(enc_seq_len * sr / n_fft * 2)
        self.vgg = nn.Sequential(
            nn.Conv2d(1, hidden_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(hidden_dim, hidden_dim, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2),
            nn.Conv2d(hidden_dim, hidden_dim * 2, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(hidden_dim * 2, hidden_dim * 2, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2))
        self.seq_len, self.vocab_size, self.emb_dim = dec_seq_len, vocab_size, n_mels
        self.vgg_seq_out = self.enc_seq_len
        self.eos_token, self.bos_token = eos_token, bos_token
        self.encoder = Encoder(seq_len=self.vgg_seq_out, emb_dim=self.emb_dim, num_layers=enc_num_layers,
                               num_heads=num_heads, ff_dim=ff_dim, dropout=dropout)
        self.decoder = Decoder(vocab_size=vocab_size, seq_len=self.seq_len, emb_dim=self.emb_dim,
                               num_layers=dec_num_layers, num_heads=num_heads, ff_dim=ff_dim, eos_token=eos_token,
                               bos_token=bos_token, dropout=dropout, padding_idx=padding_idx)
        self.device = device
        self.precision = precision
        import weakref
        ref = weakref.ref(self)
        for mod in self.modules():
            if mod is not self:
                mod.__dict__["_asrx_root"] = ref

    def forward(self, batch):
        cfg = _cfg(self, self.decoder.p)
        enc_x = self.encoder(batch["spectre"], batch["spectrogram_len"], cfg)
        return self.decoder(batch["encoded_text"], enc_x, batch["spectrogram_len"], cfg)

    def evaluate(self, batch):
        enc_x = self.encoder(batch["spectre"], batch["spectrogram_len"])
        return self.decoder.evaluate(enc_x, self.device)
