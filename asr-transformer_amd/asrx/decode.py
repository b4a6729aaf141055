"""Decoding drivers (inference, no autograd) of the Decoder and the Transformer: greedy `evaluate`, beam search with CTC
and n-gram LM fusion, CTC-only decoding and alignment, two-pass rescoring.  One engine runs every KV-cached decode
(CachedDecoder), one rule fuses a beam step's score sources (fusion_rule), one function checks the arguments
(check_args).  The programs run here (decoder_fwd, the CTC head) are asrx.functions'."""
import math
from typing import NamedTuple

import torch

from . import blocks as Bk
from . import kernels as K
from .functions import _i32_on, _kv_block, _mha_fwd_w, ctc_head_fwd, decoder_fwd, key_spec, make_ctx, pad_lengths
from .kernels import MaskSpec


# ------------------------------------------------------------------------------------------- results and arguments

class BeamResult(NamedTuple):
    """Decoder.beam_search / Transformer.beam_search: per sample the `nbest` best hypotheses, best first.
    tokens (B, nbest, L0 + steps) int64: prompt, generated tokens, EOS after a hypothesis's end (steps = max_len
    unless polling stopped the loop early); lengths (B, nbest) int64: generated tokens, the EOS included; scores
    (B, nbest) fp32: summed log-probabilities (-inf: fewer than nbest hypotheses exist)."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    scores: torch.Tensor


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


class CtcInput(NamedTuple):
    """The decoders' `ctc=` argument; a plain tuple of the first four or of all five is taken too.  V: the head's
    vocabulary where the caller has the head; None: the decoder's V, which a shared vocabulary makes the same."""
    logits: torch.Tensor                    # the CTC head's fp32 logits [B*T, >= V] of the utterances
    T: int                                  # their frame count
    blank: int
    input_lengths: torch.Tensor = None      # int32 frame counts per sample
    V: int = None


BOS_ID = 1          # the start token of a decode without a prompt (transformer_beam_search's text=None)
IGNORE_ID = -1      # target id of the positions asrx_seq_logprob leaves out
NO_LOGITS = "asrx: ctc_weight > 0 needs the CTC head's logits (a model built with ctc=True)"
NO_HEAD = "asrx: ctc_weight > 0 needs a model with a CTC head (Transformer(..., ctc=True))"


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


def check_mbr_scale(scale):
    scale = float(scale)
    if scale != scale or scale < 0.0:
        raise ValueError(f"mbr_scale {scale} must be >= 0")
    return scale


def _check_beam(beam, nbest):
    W, nbest = int(beam), int(nbest)
    if not 1 <= W <= 16:
        raise ValueError(f"beam must be in 1..16, got {beam}")
    if not 1 <= nbest <= W:
        raise ValueError(f"nbest must be in 1..beam, got {nbest}")
    return W, nbest


def check_args(V, ctc_weight, no_ctc, lm=None, lm_weight=0.0, token_bonus=0.0, beam=4, nbest=1, mbr_scale=None,
               prompt=None, rescore=False, **_):
    """The arguments of a beam search or (rescore=True: no prompt, the CTC input always needed, any ctc_weight >= 0) of
    a two-pass decode, judged on the host: (lam, beta, bonus, W, nbest, mbr_scale).  The Transformer entries call it
    before the encoder runs, the Decoder entries call it again.  prompt: the token rows (None: the BOS column);
    no_ctc: None where the CTC term has its input, else the text of the RuntimeError that says what is missing."""
    lam = float(ctc_weight)
    if rescore and (lam != lam or lam < 0.0):
        raise ValueError(f"ctc_weight {ctc_weight} must be >= 0")
    if not rescore and not 0.0 <= lam <= 1.0:
        raise ValueError(f"ctc_weight {ctc_weight} outside [0, 1]")
    beta, bonus = check_lm(lm, lm_weight, token_bonus, V)
    if mbr_scale is not None:
        mbr_scale = check_mbr_scale(mbr_scale)
    many = prompt is not None and prompt.dim() == 2 and prompt.shape[1] != 1
    if beta > 0.0 and many:
        raise ValueError(f"lm_weight > 0 takes a one-token prompt, got L0 = {prompt.shape[1]}")
    if (rescore or lam > 0.0) and no_ctc is not None:
        raise RuntimeError(no_ctc)
    if lam > 0.0 and many:
        raise ValueError(f"ctc_weight > 0 takes a one-token prompt, got L0 = {prompt.shape[1]}")
    return (lam, beta, bonus) + _check_beam(beam, nbest) + (mbr_scale,)


# ------------------------------------------------------------------------------------------- the cached decoder

class CachedDecoder:
    """The KV-cached decoder of B samples x W hypotheses (rows b*W + w) over P positions, eval only: what the greedy
    `evaluate` and the beam search share, set up for a prompt of L0 tokens and `steps` new ones (P = L0 - 1 + steps).
    kvs [n][B*W][P][2d] are the self-attention K/V caches, which gain position t in `position` (kvs_alt, W > 1 only:
    the buffer `reorder` gathers into); kvx [B*Te][n*2d] holds every layer's cross-attention K/V per SAMPLE: the W
    hypotheses of a sample share it, so cross-attention runs as batch = B with W queries each (W = 1: greedy
    decoding).  xspec: MaskSpec.keys over each sample's Te encoder rows, for the cross-attention, or None."""

    def __init__(self, dec, enc_x, W, L0, steps, enc_lengths=None):
        C = self.C = make_ctx(dec, 0.0)
        C.train, C.p = False, 0.0
        B, Te, d = enc_x.shape
        P = L0 - 1 + steps                      # positions processed (the last input has L0 + steps - 1 tokens)
        self.dec, self.B, self.W, self.P, self.Te, self.d, self.pe = dec, B, W, P, Te, d, dec._pe.pe[0]
        if P > self.pe.shape[0]:
            raise ValueError(f"decoder length {P} exceeds the PE table ({self.pe.shape[0]}) as in layers.py:73")
        self.live = B > 0 and steps > 0
        if not self.live:                       # nothing to decode: the caller returns its empty result
            return
        dev, n = enc_x.device, len(dec._layers)
        self.xspec = key_spec(enc_lengths, B, Te, dev)[1]
        enc_c = torch.empty(B * Te, d, dtype=C.cd, device=dev)
        K.cast(enc_x.reshape(B * Te, d).contiguous(), enc_c)
        Wkv, bkv, _, _ = _kv_block(C, dec)
        self.kvx = torch.empty(B * Te, n * 2 * d, dtype=C.cd, device=dev)
        K.linear(enc_c, Wkv, self.kvx, bias=bkv)
        self.kvs = torch.empty(n, B * W, P, 2 * d, dtype=C.cd, device=dev)
        self.kvs_alt = torch.empty_like(self.kvs) if W > 1 else None

    def position(self, cur, t):
        """The embedding of the tokens `cur` [B*W] at position t through every layer: the fp32 stream [B*W, d]."""
        C, dec, B, W, d, kvs, kvx = self.C, self.dec, self.B, self.W, self.d, self.kvs, self.kvx
        H = dec.num_heads
        dh = d // H
        R = B * W
        none = MaskSpec()
        cross = self.xspec or none
        xs = torch.empty(R, d, dtype=torch.float32, device=cur.device)
        K.embed_fwd(cur, dec._embedding.weight.data, self.pe[t:t + 1], xs, 1)
        for l, layer in enumerate(dec._layers):
            mha, cr = layer._mask_attention, layer._cross_attention
            # masked self-attention: the new position's K/V join the cache, its query attends to positions 0..t
            h, _, _ = Bk.ln_fwd(C, xs, layer._norm1)
            x1, _ = Bk.attn_core_fwd(C, _mha_fwd_w(C, mha), h, R, H, dh, 1, t + 1, none, xk=h, kv=kvs[l],
                                     kv_dst=kvs[l][:, t], resid=xs)
            # cross-attention over the encoder output (no mask, model.py:71, unless the batch is padded: xspec)
            h2, _, _ = Bk.ln_fwd(C, x1, layer._norm2)
            w = (C.W(cr.wq), cr.bq.data, None, None, C.W(cr._out_linear.weight), cr._out_linear.bias.data)
            x2, _ = Bk.attn_core_fwd(C, w, h2, B, H, dh, W, self.Te, cross, kv=kvx[:, l * 2 * d:], resid=x1)
            xs, _ = Bk.ffn_fwd(C, x2, layer._norm3, layer._feedforward)
        return xs

    def logits(self, xs, out, ldc, final_norm):
        """out (the caller's fp32 rows, stride ldc) <- the classifier on xs behind the last LayerNorm, or a cast."""
        C, dec, d, R = self.C, self.dec, self.d, xs.shape[0]
        if final_norm:
            hc, _, _ = Bk.ln_fwd(C, xs, dec._norm_layer)
        else:
            hc = torch.empty(R, d, dtype=C.cd, device=xs.device)
            K.cast(xs, hc)
        K.gemm(hc, C.W(dec._classifier.weight), out, R, dec._classifier.Vp, d, lda=d, ldb=d, ldc=ldc)

    def reorder(self, src_row, t):
        """Row r of the caches <- row src_row[r], positions 0..t (asrx_gather_rows into the second buffer)."""
        n, R, P, d = len(self.dec._layers), self.B * self.W, self.P, self.d
        K.gather_rows(self.kvs, self.kvs_alt, src_row, n, R, (t + 1) * 2 * d, P * 2 * d, R * P * 2 * d)
        self.kvs, self.kvs_alt = self.kvs_alt, self.kvs


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


def _decoder_evaluate_cached(dec, x, enc_x, enc_lengths=None):
    dev = enc_x.device
    B, steps, L0 = enc_x.shape[0], dec._seq_len, x.shape[1]
    eng = CachedDecoder(dec, enc_x, 1, L0, steps, enc_lengths)
    if not eng.live:                        # B == 0 or steps == 0
        return x[-1:].to(dev) if B else x.to(dev), []
    V, Vp = dec._classifier.V, dec._classifier.Vp
    logits = torch.empty(B, eng.P, Vp, dtype=torch.float32, device=dev)
    tokens = torch.empty(B, L0 + steps, dtype=torch.int64, device=dev)
    tokens[:, :L0] = x.to(device=dev, dtype=torch.int64)
    cur = tokens[:, 0].contiguous()
    for t in range(eng.P):
        lg = logits[:, t]
        eng.logits(eng.position(cur, t), lg, eng.P * Vp, final_norm=False)   # no final LayerNorm in evaluate
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


# ------------------------------------------------------------------------------------------- beam search

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


def fusion_rule(lam, beta, bonus, eos, prefix=None, ngram=None, delta=None, extra=None):
    """What a selecting beam step does with a CTC prefix scorer (prefix, weight lam) and / or an n-gram LM (ngram, weight
    beta, per-token bonus) beside the decoder: (scores, select, joint, sources).  scores: the (method, arguments) calls
    that fill the extra score matrix; select: K.beam_step, or K.beam_step_joint with joint = (extra matrix, att_weight,
    extra_weight); sources: whose advance(eos, parent, tok, fin_prev) follows the selection, CTC first.  CTC alone:
    delta unscaled, weights (1 - lam, lam).  With an LM: extra = lam * delta + beta * lm + bonus in asrx_ngram_score's
    one launch (no CTC: lam is 0, no delta), weights (1 - lam, 1).  The bit-exact tests pin this arithmetic."""
    scores = [] if prefix is None else [(prefix.score, (eos, delta))]
    joint = () if prefix is None else (delta, 1.0 - lam, lam)
    if ngram is not None:
        scores.append((ngram.score, (extra, None if prefix is None else delta, lam, beta, bonus)))
        joint = (extra, 1.0 - lam, 1.0)
    return scores, K.beam_step_joint if joint else K.beam_step, joint, [x for x in (prefix, ngram) if x is not None]


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
    V, Vp = dec._classifier.V, dec._classifier.Vp
    lam, beta, bonus, W, nbest, _ = check_args(V, ctc_weight, NO_LOGITS if ctc is None else None, lm, lm_weight,
                                               token_bonus, beam, nbest, prompt=x)
    B, dev = enc_x.shape[0], enc_x.device
    steps = dec._seq_len if max_len is None else int(max_len)
    poll = int(poll)
    if x.dim() != 2 or x.shape[0] != B or x.shape[1] < 1:
        raise ValueError(f"prompt must be (B, L0 >= 1) with B = {B}, got {tuple(x.shape)}")
    if steps < 0 or poll < 0:
        raise ValueError("max_len and poll must be >= 0")
    eos = int(dec._eos_token_id)
    L0 = x.shape[1]
    eng = CachedDecoder(dec, enc_x, W, L0, steps, enc_lengths)     # (cross-attention K/V: per sample, not per beam)
    prompt = x.to(device="cpu", dtype=torch.int64)
    if not eng.live:                                                # B == 0 or steps == 0
        return BeamResult(prompt[:, None, :].expand(B, nbest, L0).contiguous(),
                          torch.zeros(B, nbest, dtype=torch.int64), torch.zeros(B, nbest, dtype=torch.float32))
    R = B * W
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
    prefix = ngram = delta = extra = None
    if lam > 0.0:
        ctc = CtcInput(*ctc)
        prefix = K.CtcPrefix(ctc.logits, B, W, int(ctc.T), V, ctc.blank, _i32_on(dev, ctc.input_lengths))
        delta = torch.empty(R, Vp, dtype=torch.float32, device=dev)
    if beta > 0.0:
        ngram = K.NgramState(lm, B, W)
        extra = torch.empty(R, Vp, dtype=torch.float32, device=dev)
    scores, select, joint, sources = fusion_rule(lam, beta, bonus, eos, prefix, ngram, delta, extra)
    for t in range(eng.P):
        xs = eng.position(cur, t)
        s = t - (L0 - 1)
        if s < 0:
            cur = xr[:, t + 1].contiguous()
            continue
        lg = torch.empty(R, Vp, dtype=torch.float32, device=dev)
        eng.logits(xs, lg, Vp, final_norm)
        for fill, args in scores:
            fill(*args)
        select(lg, V, B, W, eos, *joint, state, other, tok_h[s], par_h[s], src_row, cur=cur, n_live=n_live[s:s + 1])
        for source in sources:
            source.advance(eos, par_h[s], tok_h[s], state[1])
        state, other = other, state
        if poll and (s + 1) % poll == 0 and s + 1 < steps and int(n_live[s]) == 0:
            done = s + 1
            break
        if W > 1 and s + 1 < steps:      # (one beam: the parent is always slot 0, the cache stays in place)
            eng.reorder(src_row, t)
    score, _, length = (a.cpu().view(B, W) for a in state)
    seqs = beam_backtrack(par_h[:done].cpu().view(done, B, W), tok_h[:done].cpu().view(done, B, W))
    order = beam_rank(score, length, length_penalty)[:, :nbest]
    best = seqs.gather(1, order[:, :, None].expand(-1, -1, done))
    tokens = torch.cat([prompt[:, None, :].expand(B, nbest, L0), best], dim=2)
    return BeamResult(tokens, length.long().gather(1, order), score.gather(1, order))


def _encode(model, spectrum, lens=None):
    """Front end and encoder as in `evaluate` (model.py:201-203); lens: the lengths to mask with (pad_lengths)."""
    feats = model.input_layer(spectrum)
    return model.encoder(feats) if lens is None else model.encoder(feats, input_lengths=lens)


def transformer_beam_search(model, spectrum, text=None, ctc_weight=0.0, input_lengths=None, **kw):
    """Transformer.beam_search: front end and encoder as in `evaluate` (model.py:201-206), then
    decoder_beam_search.  text=None starts every sample on a BOS column (id 1).  ctc_weight > 0: joint
    CTC/attention decoding, the one encoder output also feeding the model's CTC head (input_lengths: optional valid
    encoder frames per sample; on a model with mask_padding they also mask the encoder's self-attention and the
    cross-attention, with or without the CTC term)."""
    lam = check_args(model.decoder._classifier.V, ctc_weight, NO_HEAD if getattr(model, "ctc_head", None) is None
                     else None, prompt=text, **kw)[0]
    lens = pad_lengths(model, input_lengths)
    with torch.no_grad():
        enc = _encode(model, spectrum, lens)
    if text is None:
        text = torch.full((spectrum.shape[0], 1), BOS_ID, dtype=torch.int64)
    if lens is not None:
        kw["enc_lengths"] = lens
    if lam > 0.0:
        logits, B, T = _ctc_logits_of(model, enc)
        kw.update(ctc=CtcInput(logits, T, model.ctc_blank, input_lengths), ctc_weight=lam)
    return decoder_beam_search(model.decoder, text, enc, **kw)


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
    return K.ctc_greedy(logits, model.ctc_head.V, T, model.ctc_blank, _i32_on(logits.device, input_lengths))


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
    # The Trainer's width rule (a text row holds BOS and EOS): up to 257 columns take asrx_ctc_align (255 labels),
    # wider rows asrx_ctc_align_long (4095).  A row with more labels than that has no alignment: its score is -inf.
    use_long, max_l = K.ctc_path(targets.shape[1], framing=2)
    return K.ctc_align(logits, model.ctc_head.V, T, targets, lengths, _i32_on(dev, input_lengths),
                       max_target_len=max_l, blank=model.ctc_blank, long=use_long)


# ------------------------------------------------------------------------------------------- two-pass decoding

def _rescore_labels(dec, max_len):
    """max_labels of a two-pass decode: the decoder row holds BOS and the labels, its targets the labels and EOS."""
    L = min(dec._seq_len if max_len is None else int(max_len), 255)
    if L < 2:
        raise ValueError(f"two-pass decoding needs a decoder length >= 2, got {L}")
    if L > dec._pe.pe[0].shape[0]:
        raise ValueError(f"decoder length {L} exceeds the PE table ({dec._pe.pe[0].shape[0]}) as in layers.py:73")
    return L, L - 1


def _first_pass(ctc, B, V, W, max_labels, dev):
    """ctc: a CtcInput; without its V the decoder's V is taken."""
    logits, T, blank = ctc.logits, int(ctc.T), int(ctc.blank)
    V = V if ctc.V is None else int(ctc.V)
    if not 0 <= blank < V <= logits.shape[1]:
        raise ValueError(f"CTC vocabulary {V} / blank {ctc.blank} do not fit logits of {logits.shape[1]} columns")
    if logits.shape[0] != B * T:
        raise ValueError(f"CTC logits have {logits.shape[0]} rows, expected B * T = {B * T}")
    return K.ctc_prefix_beam(logits, V, T, blank, W, max_labels, _i32_on(dev, ctc.input_lengths))


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
    ctc = CtcInput(*ctc)
    tok, lens, score, _ = _first_pass(ctc, B, dec._classifier.V, W, max_labels, ctc.logits.device)
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
    cls = dec._classifier
    no_ctc = "asrx: rescoring needs the CTC head's logits (a model built with ctc=True)" if ctc is None else None
    lam, beta, bonus, W, nbest, mbr_scale = check_args(cls.V, ctc_weight, no_ctc, lm, lm_weight, token_bonus, beam,
                                                       nbest, mbr_scale, rescore=True)
    L, max_labels = _rescore_labels(dec, max_len)
    C = make_ctx(dec, 0.0)
    C.train, C.p = False, 0.0
    dev = enc_x.device
    B, Te, d = enc_x.shape
    eos = int(dec._eos_token_id)
    pad = int(dec.pad_token_id if dec.pad_token_id is not None else 0)
    if B == 0:
        z = torch.zeros(0, nbest, dtype=torch.float32)
        return RescoreResult(torch.zeros(0, nbest, 1 + L, dtype=torch.int64), torch.zeros(0, nbest, dtype=torch.int64),
                             z, z.clone(), z.clone(), None if mbr_scale is None else z.clone(),
                             z.clone() if beta > 0.0 else None)
    R = B * W
    tok, lens, cscore, n_hyp = _first_pass(CtcInput(*ctc), B, cls.V, W, max_labels, dev)
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
    ctc = CtcInput(logits, T, model.ctc_blank, input_lengths, model.ctc_head.V)
    return decoder_ctc_beam_search(model.decoder, ctc, B, beam, nbest, max_len)


def transformer_rescore(model, spectrum, beam=8, ctc_weight=0.5, input_lengths=None, nbest=1, final_norm=True,
                        max_len=None, mbr_scale=None, lm=None, lm_weight=0.0, token_bonus=0.0):
    """Transformer.rescore: front end and encoder as in `evaluate`, the CTC head on the one encoder output, then
    decoder_rescore."""
    no_head = "asrx: rescoring needs a model with a CTC head (Transformer(..., ctc=True))"
    check_args(model.decoder._classifier.V, ctc_weight, no_head if getattr(model, "ctc_head", None) is None else None,
               lm, lm_weight, token_bonus, beam, nbest, mbr_scale, rescore=True)
    lens = pad_lengths(model, input_lengths)
    with torch.no_grad():
        enc = _encode(model, spectrum, lens)
    logits, B, T = _ctc_logits_of(model, enc)
    ctc = CtcInput(logits, T, model.ctc_blank, input_lengths, model.ctc_head.V)
    return decoder_rescore(model.decoder, enc, ctc, beam, ctc_weight, nbest, final_norm, max_len, mbr_scale, lm,
                           lm_weight, token_bonus, enc_lengths=lens)
