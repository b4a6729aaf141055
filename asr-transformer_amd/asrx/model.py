"""Drop-in replacements for modules/Transformer/model.py: EncoderLayer, Encoder, DecoderLayer, Decoder,
Transformer — same constructor signatures (model.py:9-16, 28-39, 55-63, 78-102, 154-191), same forward /
evaluate signatures, same state_dict keys.  Whole stacks run as explicit native kernel programs
(asrx.blocks) behind one autograd node each; parameters live in one flat buffer (asrx.params).

Extra keyword-only knobs (not in the reference): precision ("bf16" training path | "fp32" parity path),
attention ("fused" LDS-tiled kernel | "unfused" materialised scores + row softmax), ctc / ctc_blank (Transformer
only: a CTC head on the encoder output, one extra state_dict key `ctc_head.weight`), mask_padding (Transformer only:
the entry points that take `input_lengths` also mask the padded frames in the encoder's self-attention and in the
cross-attention; a plain attribute, no state_dict key).
"""
import math
import weakref

import torch
from torch import nn

from .layers import MHA, FeedForward, LayerNorm, TrainablePositionalEncoding, _Lin


def _adopt(root):
    """Point every submodule at `root`, whose flat parameter store they share (weakref: no module cycle)."""
    for m in root.modules():
        if m is not root:
            m.__dict__["_asrx_root"] = weakref.ref(root)


def subsampled(n):
    """model.py:172 / the conv arithmetic of model.py:168-171."""
    return ((n - 3) // 2 + 1 - 3) // 2 + 1


class _LinIn(_Lin):
    """Encoder._lin_in (model.py:32).  Stored with its input columns permuted from the reference's channel-major
    feature order (c*F''+f, model.py:43-45) to (f*64+c): the conv2 GEMM then writes the encoder input directly
    and the reference's transpose+contiguous copy disappears.  state_dict hooks un/permute."""

    def __init__(self, fin, fout, n_freq):
        super().__init__(fin, fout)
        self.n_freq = n_freq      # F''
        self.n_ch = fin // n_freq  # 64

    def _to_ref(self, w):          # phys (d, F*64 + c) -> ref (d, c*F + f)
        d = w.shape[0]
        return w.reshape(d, self.n_freq, self.n_ch).permute(0, 2, 1).reshape(d, -1)

    def _from_ref(self, w):
        d = w.shape[0]
        return w.reshape(d, self.n_ch, self.n_freq).permute(0, 2, 1).reshape(d, -1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        w = self.weight if keep_vars else self.weight.detach()
        destination[prefix + "weight"] = self._to_ref(w).contiguous()
        destination[prefix + "bias"] = self.bias if keep_vars else self.bias.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        sd = dict(state_dict)
        if prefix + "weight" in sd:
            sd[prefix + "weight"] = self._from_ref(sd[prefix + "weight"])
        super()._load_from_state_dict(sd, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class _Classifier(nn.Module):
    """Decoder._classifier = Linear(d, V, bias=False) (model.py:102).  Rows padded to a multiple of 64 (V=250
    -> 256) so the logits/dlogits rows are 16-byte aligned GEMM operands; padding rows stay zero."""

    def __init__(self, d, V):
        super().__init__()
        self.V = V
        self.Vp = (V + 63) // 64 * 64
        a = 1.0 / math.sqrt(d)
        w = torch.zeros(self.Vp, d)
        w[:V].uniform_(-a, a)
        self.weight = nn.Parameter(w)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        w = self.weight if keep_vars else self.weight.detach()
        destination[prefix + "weight"] = w[:self.V] if keep_vars else w[:self.V].clone()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        key = prefix + "weight"
        if key not in state_dict:
            missing_keys.append(key)
            return
        with torch.no_grad():
            self.weight.zero_()
            self.weight[:self.V].copy_(state_dict[key])


class _Embedding(nn.Module):
    """nn.Embedding(V, d, padding_idx) container (model.py:94): key `weight`; the padding row is zero at init
    and never receives gradient."""

    def __init__(self, V, d, padding_idx):
        super().__init__()
        self.padding_idx = padding_idx
        w = torch.randn(V, d)
        if padding_idx is not None:
            w[padding_idx] = 0
        self.weight = nn.Parameter(w)


class FrontEnd(nn.Sequential):
    """Transformer.input_layer (model.py:168-171) with the reference's child indices (0: conv, 1: relu,
    2: conv, 3: relu).  conv2's weight is kept channels-last (cout, kh, kw, cin) in memory, which is the
    [64][576] operand of the im2col GEMM.  forward returns the reference's logical (B, 64, F'', T'') tensor as
    a permuted view of the (B, T'', F'', 64) buffer the encoder consumes."""

    def __init__(self):
        super().__init__(nn.Conv2d(1, 64, 3, stride=2), nn.ReLU(), nn.Conv2d(64, 64, 3, stride=2), nn.ReLU())
        self[2].weight._asrx_phys = ((64, 3, 3, 64), (0, 3, 1, 2))
        with torch.no_grad():
            self[2].weight.data = self[2].weight.data.contiguous(memory_format=torch.channels_last)

    def forward(self, spectrum):
        from .functions import frontend
        return frontend(self, spectrum)


class EncoderLayer(nn.Module):
    """model.py:9-25"""

    def __init__(self, emb_dim, num_heads, ff_dim, dropout):
        super().__init__()
        self.num_heads, self.p = num_heads, float(dropout)
        self._norm_in = LayerNorm(emb_dim)          # unused by the reference forward (model.py:12)
        self._attention = MHA(num_heads, emb_dim, dropout)
        self._norm1 = LayerNorm(emb_dim)
        self._feedforward = FeedForward(emb_dim, ff_dim, dropout)
        self._norm2 = LayerNorm(emb_dim)
        _adopt(self)

    def forward(self, x):
        from .functions import encoder_layer
        return encoder_layer(self, x)


class Encoder(nn.Module):
    """model.py:28-52"""

    def __init__(self, seq_len, emb_dim, input_dim, num_layers, num_heads, ff_dim, dropout=0.1, n_freq=None):
        super().__init__()
        self.emb_dim, self.num_heads, self.p = emb_dim, num_heads, float(dropout)
        n_freq = n_freq if n_freq is not None else input_dim // 64
        self._lin_in = _LinIn(input_dim, emb_dim, n_freq)
        self._norm_out = LayerNorm(emb_dim)
        self._pe = TrainablePositionalEncoding(seq_len, emb_dim)
        self._layers = nn.ModuleList([EncoderLayer(emb_dim, num_heads, ff_dim, dropout) for _ in range(num_layers)])
        _adopt(self)

    def forward(self, x, input_lengths=None):
        """input_lengths (B,): the valid rows (encoder frames) of each utterance; every layer's self-attention then
        masks the keys behind them.  The padding must be finite; the valid rows of the output are a
        function of the valid frames only, the padded rows are finite but unspecified.  None: no mask (model.py:21)."""
        from .functions import encoder
        return encoder(self, x, input_lengths)


class DecoderLayer(nn.Module):
    """model.py:55-75"""

    def __init__(self, emb_dim, num_heads, ff_dim, dropout):
        super().__init__()
        self.num_heads, self.p = num_heads, float(dropout)
        self._mask_attention = MHA(num_heads, emb_dim, dropout)
        self._norm1 = LayerNorm(emb_dim)
        self._cross_attention = MHA(num_heads, emb_dim, dropout, cross=True)
        self._norm2 = LayerNorm(emb_dim)
        self._feedforward = FeedForward(emb_dim, ff_dim, dropout)
        self._norm3 = LayerNorm(emb_dim)
        _adopt(self)

    def forward(self, x, mask, enc_x):
        from .functions import decoder_layer
        return decoder_layer(self, x, mask, enc_x)


class Decoder(nn.Module):
    """model.py:78-151"""

    def __init__(self, vocab_size, seq_len, emb_dim, num_layers, num_heads, ff_dim, eos_token_id, dropout=0.1,
                 pad_token_id=0):
        super().__init__()
        self._seq_len = seq_len
        self._eos_token_id = eos_token_id
        self.pad_token_id = pad_token_id
        self.vocab_size, self.emb_dim, self.num_heads, self.p = vocab_size, emb_dim, num_heads, float(dropout)
        self._embedding = _Embedding(vocab_size, emb_dim, pad_token_id)
        self._pe = TrainablePositionalEncoding(seq_len, emb_dim)
        self._dropout = nn.Dropout(dropout)
        self._layers = nn.ModuleList([DecoderLayer(emb_dim, num_heads, ff_dim, dropout) for _ in range(num_layers)])
        self._norm_layer = LayerNorm(emb_dim)
        self._classifier = _Classifier(emb_dim, vocab_size)
        _adopt(self)

    def forward(self, x, mask, enc_x, enc_lengths=None):
        """enc_lengths (B,): the valid rows of each encoder output; every layer's cross-attention then masks the rows
        behind them (an utterance with no valid row gets a zero cross-attention).  None: no mask
        (model.py:71)."""
        from .functions import decoder
        return decoder(self, x, mask, enc_x, enc_lengths)

    def evaluate(self, x, enc_x, enc_lengths=None):
        """enc_lengths: as in forward."""
        from .decode import decoder_evaluate
        return decoder_evaluate(self, x, enc_x, enc_lengths)

    def beam_search(self, x, enc_x, beam=4, max_len=None, length_penalty=0.0, final_norm=True, nbest=1, poll=8,
                    ctc=None, ctc_weight=0.0, lm=None, lm_weight=0.0, token_bonus=0.0, enc_lengths=None):
        """Beam-search decoding (no reference counterpart; see decode.decoder_beam_search) -> BeamResult.
        lm / lm_weight / token_bonus: shallow fusion with an asrx.NgramLM on the device.  enc_lengths: as in forward."""
        from .decode import decoder_beam_search
        return decoder_beam_search(self, x, enc_x, beam, max_len, length_penalty, final_norm, nbest, poll, ctc,
                                   ctc_weight, lm, lm_weight, token_bonus, enc_lengths)

    def rescore(self, enc_x, ctc, beam=8, ctc_weight=0.5, nbest=1, final_norm=True, max_len=None, mbr_scale=None,
                lm=None, lm_weight=0.0, token_bonus=0.0, enc_lengths=None):
        """Two-pass decoding from an encoder output and its CTC logits, ctc = (logits, T, blank, input_lengths) as in
        beam_search (no reference counterpart; see decode.decoder_rescore) -> RescoreResult.  mbr_scale: a number
        orders the hypotheses by minimum Bayes risk under softmax(mbr_scale * score) and fills `risks`.  lm (an
        asrx.NgramLM on the device) with lm_weight > 0 adds lm_weight * log p_lm + token_bonus * len to the rank and
        fills `lm_scores`.  enc_lengths: as in forward, for the second pass's cross-attention."""
        from .decode import decoder_rescore
        return decoder_rescore(self, enc_x, ctc, beam, ctc_weight, nbest, final_norm, max_len, mbr_scale, lm,
                               lm_weight, token_bonus, enc_lengths)


class Transformer(nn.Module):
    """model.py:154-206.  forward(spectrum (B,1,F,T), text (B,L) int, mask (B,L)) -> logits (B,L,V).

    mask_padding=True (keyword-only, default False; a plain attribute that may be set after loading): every entry
    point that takes `input_lengths` — valid ENCODER frames per utterance, asrx.subsampled(spectrogram frames) —
    also masks the keys behind them in the encoder's self-attention and in the decoder's cross-attention (DESIGN.md
    §18).  The contract: the padding must be finite (a masked NaN value row still poisons 0 * NaN); the valid rows of
    every output are then a function of the valid frames only, whatever the utterance is batched with; padded encoder
    rows are finite but unspecified; an utterance shorter than 7 spectrogram frames (0 encoder frames) gives finite
    outputs with a zero cross-attention, and no gradient.  With the flag off, or without input_lengths, every call
    runs launch for launch as it did before the flag existed (no key mask: model.py:21,71)."""

    def __init__(self, vocab_size, input_dim, embedding_dim, decoder_seq_len, encoder_seq_len, encoder_num_layers,
                 decoder_num_layers, num_heads, ff_dim, dropout=0.1, pad_token_id=4, eos_token_id=2, *,
                 precision="bf16", attention="fused", ctc=False, ctc_blank=None, mask_padding=False):
        super().__init__()
        self.input_layer = FrontEnd()
        n_freq = subsampled(input_dim)
        fdim = n_freq * 64
        self.input_encoding = _Lin(fdim, embedding_dim)   # built but unused by the reference (model.py:173)
        self.encoder = Encoder(seq_len=encoder_seq_len, input_dim=fdim, emb_dim=embedding_dim,
                               num_layers=encoder_num_layers, num_heads=num_heads, ff_dim=ff_dim, dropout=dropout,
                               n_freq=n_freq)
        self.decoder = Decoder(vocab_size=vocab_size, seq_len=decoder_seq_len, emb_dim=embedding_dim,
                               num_layers=decoder_num_layers, num_heads=num_heads, ff_dim=ff_dim,
                               eos_token_id=eos_token_id, dropout=dropout, pad_token_id=pad_token_id)
        self.precision = precision
        self.attention = attention
        self.mask_padding = bool(mask_padding)
        # ctc=True: a bias-free linear head on the encoder output (after Encoder._norm_out) for the hybrid
        # CTC/attention objective (asrx.train.Trainer(ctc_weight=...)) and decoder-free best-path decoding.  Registered
        # last, so every other parameter keeps its key, its initial values under a given seed and its place in the
        # flat store; ctc=False builds exactly the reference's module tree.
        self.ctc_blank = int(pad_token_id if ctc_blank is None else ctc_blank)
        if ctc:
            if not 0 <= self.ctc_blank < vocab_size:
                raise ValueError(f"ctc_blank {self.ctc_blank} outside the vocabulary [0, {vocab_size})")
            self.ctc_head = _Classifier(embedding_dim, vocab_size)
        _adopt(self)

    def forward(self, spectrum, text, mask, input_lengths=None):
        """input_lengths (B,): valid encoder frames per utterance; used where mask_padding is set (see the class)."""
        from .functions import transformer
        return transformer(self, spectrum, text, mask, input_lengths)

    def evaluate(self, spectrum, text, input_lengths=None):
        """input_lengths: as in forward."""
        from .decode import transformer_evaluate
        return transformer_evaluate(self, spectrum, text, input_lengths)

    def beam_search(self, spectrum, text=None, ctc_weight=0.0, input_lengths=None, **kw):
        """Front end, encoder, then Decoder.beam_search(text, enc, **kw); text=None is a BOS column (id 1).
        ctc_weight in (0, 1] (ctc=True models): joint CTC/attention decoding, hypotheses ranked by
        (1 - ctc_weight) * log p_att + ctc_weight * log p_ctc; input_lengths: valid encoder frames per sample (with
        mask_padding they also mask the padded frames in the encoder and the cross-attention, at any ctc_weight).
        lm=, lm_weight=, token_bonus= (an asrx.NgramLM on the device): shallow fusion, every generated token also
        earns lm_weight * log p_lm + token_bonus; lm=None or lm_weight=0 is the search without an LM."""
        from .decode import transformer_beam_search
        return transformer_beam_search(self, spectrum, text, ctc_weight, input_lengths, **kw)

    def ctc_logits(self, spectrum, input_lengths=None):
        """Front end, encoder and the CTC head (ctc=True models), no grad: fp32 logits (B, T', V).  input_lengths: as
        in forward (the rows behind them are then unspecified)."""
        from .decode import transformer_ctc_logits
        logits, B, T = transformer_ctc_logits(self, spectrum, input_lengths)
        return logits.view(B, T, -1)[:, :, :self.ctc_head.V]

    def ctc_greedy(self, spectrum, input_lengths=None):
        """CTC best-path transcript without the decoder: per frame the arg-max of ctc_logits, repeats collapsed,
        blanks removed, on the device.  input_lengths: (B,) valid encoder frames (None: all T').  Returns (tokens
        (B, T') int64 left-packed and padded with the blank id, lengths (B,) int32), both on the device."""
        from .decode import transformer_ctc_greedy
        return transformer_ctc_greedy(self, spectrum, input_lengths)

    def align(self, spectrum, text, mask=None, input_lengths=None):
        """Forced alignment without the decoder (ctc=True models): the best CTC path through the T' encoder frames
        that collapses to the transcript, on the device (asrx_ctc_align; asrx_ctc_align_long for n > 257, up to 4095
        labels).  text: (B, n) token ids, of which the
        positions with mask >= 1 (None: text != pad) that are not BOS / EOS / PAD are the labels, as in training;
        input_lengths: (B,) valid encoder frames (None: all T').  Returns a CtcAlignment, all on the device:
        frame_pos (B, T') int32 label position per frame (-1: blank), frame_logp (B, T') fp32, start / end (B, Lmax)
        int32 frames [start, end) of each label (asrx.frame_span maps them to spectrogram frames), conf (B, Lmax) fp32
        per-label confidence, score (B,) fp32 log-probability of the path (-inf: the transcript cannot be aligned, for
        instance more labels than frames), and targets (B, n) int64 / target_lengths (B,) int32, which map a position
        back to its token id."""
        from .decode import transformer_align
        return transformer_align(self, spectrum, text, mask, input_lengths)

    def ctc_beam_search(self, spectrum, beam=8, input_lengths=None, nbest=1):
        """CTC prefix beam search without the decoder (ctc=True models): front end, encoder, head, then the whole
        search in one launch (asrx_ctc_prefix_beam).  Returns a BeamResult: tokens (B, nbest, max_labels) int64 labels
        padded with the blank id, lengths (B, nbest) label counts, scores (B, nbest) fp32 log p_ctc, best first;
        max_labels = min(decoder seq_len, 255) - 1."""
        from .decode import transformer_ctc_beam_search
        return transformer_ctc_beam_search(self, spectrum, beam, input_lengths, nbest)

    def rescore(self, spectrum, beam=8, ctc_weight=0.5, input_lengths=None, nbest=1, final_norm=True, max_len=None,
                mbr_scale=None, lm=None, lm_weight=0.0, token_bonus=0.0):
        """Two-pass decoding (ctc=True models): ctc_beam_search's `beam` hypotheses, one teacher-forced decoder forward
        over all of them, ranked by log p_att + ctc_weight * log p_ctc.  Returns a RescoreResult: a BeamResult
        filled as beam_search fills it (tokens BOS, labels, EOS...; lengths count the EOS; scores combined) with
        att_scores and ctc_scores besides.  input_lengths: valid encoder frames per sample: the first pass's CTC
        frames, and with mask_padding also the keys of the encoder's self-attention and of the second pass's
        cross-attention.
        mbr_scale = a number >= 0: the order is the minimum-Bayes-risk one under softmax(mbr_scale * score) over the
        `beam` hypotheses (asrx_edit_distance + asrx_mbr_rank on the device) and `risks` is filled; None: as before.
        lm (an asrx.NgramLM on the device) with lm_weight > 0 adds lm_weight * log p_lm + token_bonus * len to the rank
        (asrx_ngram_seq_logprob) and fills `lm_scores`."""
        from .decode import transformer_rescore
        return transformer_rescore(self, spectrum, beam, ctc_weight, input_lengths, nbest, final_norm, max_len,
                                   mbr_scale, lm, lm_weight, token_bonus)

    def token_drop_ids(self, bos_token_id=1):
        """The ids that are no labels: (BOS, EOS, PAD) and the CTC blank where it is another id.  As `drop` they
        reduce a transcript row, a beam-search row and a CTC row alike to their labels (asrx.ErrorRate,
        asrx.edit_distance, asrx.mbr_rerank)."""
        ids = [int(bos_token_id), int(self.decoder._eos_token_id)]
        if self.decoder.pad_token_id is not None:
            ids.append(int(self.decoder.pad_token_id))
        if getattr(self, "ctc_head", None) is not None:
            ids.append(self.ctc_blank)
        return tuple(dict.fromkeys(ids))
