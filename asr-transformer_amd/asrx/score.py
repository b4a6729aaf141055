"""Scoring decoded tokens on the device: edit distance and token error rates (asrx_edit_distance), the n-best oracle
error rate, and minimum-Bayes-risk selection from an n-best list (asrx_mbr_rank).  DESIGN.md section 13.

Every decoder's output layout is read by one rule: a row's sequence is its first `length` entries, cut before the
first `stop` id, without the `drop` ids.  `text` rows (BOS, labels, EOS, PAD...), BeamResult.tokens (prompt, tokens, EOS
fill) and CTC results (labels, blank fill) all reduce to their labels with drop = Transformer.token_drop_ids()."""
import math
from typing import NamedTuple

import torch

from . import kernels as K
from .decode import BeamResult, RescoreResult, check_mbr_scale


class EditCounts(NamedTuple):
    """edit_distance: int32 device tensors of one shape ((N,) "pairs", (B, W) "group", (B, W, W) "cross").  dist =
    sub + dele + ins; -1 marks a pair with an absent slot, -2 a sequence of more than 4095 tokens (255 where no row
    has more than 255 columns; the counts are -1 there).  dele: reference tokens without a hypothesis counterpart; ins:
    the converse; ref_len: reference tokens."""
    dist: torch.Tensor
    sub: torch.Tensor
    dele: torch.Tensor
    ins: torch.Tensor
    ref_len: torch.Tensor


class MbrResult(BeamResult):
    """A BeamResult re-ordered by mbr_rerank, with `risks` fp32 (B, nbest): the expected edit distance of each
    hypothesis under the n-best posterior (+inf: no such hypothesis)."""

    def __new__(cls, tokens, lengths, scores, risks=None):
        self = super().__new__(cls, tokens, lengths, scores)
        self.risks = risks
        return self


def _device(*ts):
    for t in ts:
        if t is not None and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _rows(t, dev):
    t = t.to(device=dev, dtype=torch.int64)
    return t if t.stride(-1) == 1 else t.contiguous()


def _i32(t, dev):
    return None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)


@torch.no_grad()
def edit_distance(hyp, ref=None, hyp_lengths=None, ref_lengths=None, *, drop=(), stop=None, mode="pairs",
                  n_hyp=None):
    """Levenshtein alignment of token rows on the device (one asrx_edit_distance launch, or asrx_edit_distance_long
    where a side has more than 255 columns: the same integers; no synchronisation).

    mode "pairs": hyp (N, cols) against ref (N, cols'), row by row.  "group": hyp (B, W, cols), each of a sample's W
    hypotheses against its one reference, ref (B, cols').  "cross": hyp (B, W, cols), all W x W pairs within each
    sample (W <= 16; ref unused): the matrix an MBR selection needs.  Lengths are optional int tensors per row (None:
    the whole row); drop (at most four ids) and stop describe the rows (module docstring); n_hyp (B,) marks the
    slots j >= n_hyp[b] of "group" / "cross" as absent.  The alignment minimises (edits, substitutions)
    lexicographically, so it does not depend on any backtrace order.  Returns EditCounts."""
    if mode not in K.ED_MODES:
        raise ValueError(f"mode {mode!r} is none of {sorted(K.ED_MODES)}")
    if len(drop) > 4:
        raise ValueError(f"at most four drop ids, got {len(drop)}")
    if mode == "pairs":
        if hyp.dim() != 2 or ref is None or ref.dim() != 2 or ref.shape[0] != hyp.shape[0]:
            raise ValueError("pairs mode takes hyp (N, cols) and ref (N, cols')")
        W, shape = 1, (hyp.shape[0],)
    else:
        if hyp.dim() != 3:
            raise ValueError(f"{mode} mode takes hyp (B, W, cols), got {tuple(hyp.shape)}")
        B, W, cols = hyp.shape
        if mode == "cross" and not 1 <= W <= 16:
            raise ValueError(f"cross mode takes 1..16 hypotheses per sample, got {W}")
        if mode == "group" and (ref is None or ref.dim() != 2 or ref.shape[0] != B):
            raise ValueError(f"group mode takes ref (B, cols') with B = {B}")
        shape = (B, W) if mode == "group" else (B, W, W)
    if hyp.numel() == 0 or (mode != "cross" and ref.shape[1] == 0):
        raise ValueError("edit_distance needs at least one row and one column")
    dev = _device(hyp, ref)
    hyp = _rows(hyp, dev).reshape(-1, hyp.shape[-1])
    ref = None if mode == "cross" else _rows(ref, dev)
    use_long, _ = K.edit_path(hyp.shape[1], 0 if ref is None else ref.shape[1])
    dist, cnt = K.edit_distance(hyp, ref, _i32(hyp_lengths, dev), None if ref is None else _i32(ref_lengths, dev),
                                drop, stop, mode, W, None if mode == "pairs" else _i32(n_hyp, dev), long=use_long)
    return EditCounts(dist.view(shape), *(cnt[:, k].view(shape) for k in range(4)))


def reduce_counts(records, max_tokens=255):
    """The arithmetic of ErrorRate.compute on host data: records = [(dist [B, W], counts [B, W, 4]), ...] integer
    tensors as asrx_edit_distance writes them in GROUP mode (slot 0 the 1-best).  max_tokens: the bound the records
    were scored with (one int, or one per record), named where a dist of -2 is met."""
    tot = dict(edits=0, sub=0, dele=0, ins=0, ref=0, samples=0, wrong=0, oracle=0)
    nbest = False
    base = 0
    for u, (dist, counts) in enumerate(records):
        dist, counts = torch.as_tensor(dist).long(), torch.as_tensor(counts).long()
        B, W = dist.shape
        nbest = nbest or W > 1
        long = (dist == -2).nonzero()
        if len(long):
            b, w = (int(x) for x in long[0])
            bound = max_tokens[u] if isinstance(max_tokens, (list, tuple)) else max_tokens
            raise ValueError(f"sample {base + b} (row {b} of update {u}, hypothesis {w}): a sequence of more than "
                             f"{bound} tokens cannot be scored")
        none = (dist[:, 0] < 0).nonzero()
        if len(none):
            b = int(none[0])
            raise ValueError(f"sample {base + b} (row {b} of update {u}) has no hypothesis")
        best = dist[:, 0]
        tot["edits"] += int(best.sum())
        tot["sub"] += int(counts[:, 0, 0].sum())
        tot["dele"] += int(counts[:, 0, 1].sum())
        tot["ins"] += int(counts[:, 0, 2].sum())
        tot["ref"] += int(counts[:, 0, 3].sum())
        tot["samples"] += B
        tot["wrong"] += int((best > 0).sum())
        live = torch.where(dist >= 0, dist, torch.full_like(dist, 1 << 30))
        tot["oracle"] += int(live.min(dim=1).values.sum())
        base += B
    n = tot["ref"]

    def rate(x, d):
        return x / d if d > 0 else math.nan

    out = {"ter": rate(tot["edits"], n), "sub": rate(tot["sub"], n), "del": rate(tot["dele"], n),
           "ins": rate(tot["ins"], n), "ser": rate(tot["wrong"], tot["samples"]),
           "n_edits": tot["edits"], "n_sub": tot["sub"], "n_del": tot["dele"], "n_ins": tot["ins"], "n_ref": n,
           "n_samples": tot["samples"], "n_wrong": tot["wrong"]}
    if nbest:
        out["oracle_ter"] = rate(tot["oracle"], n)
        out["n_oracle_edits"] = tot["oracle"]
    return out


class ErrorRate:
    """Token error rate of decoded batches against their transcripts, accumulated on the device.

        er = asrx.ErrorRate(model.token_drop_ids())
        er.update_result(model.rescore(spectrum, beam=8, nbest=8), text)     # any decoder's result
        er.compute()     # {"ter", "sub", "del", "ins", "ser", "oracle_ter", "n_edits", ...}

    update / update_result launch one kernel each and synchronise nothing; compute() makes one host copy."""

    def __init__(self, drop, stop=None):
        self.drop = tuple(int(d) for d in drop)
        if len(self.drop) > 4:
            raise ValueError(f"at most four drop ids, got {len(self.drop)}")
        self.stop = None if stop is None else int(stop)
        self._records = []
        self._bounds = []     # per update: the token bound it was scored with (255, or 4095 for wide rows)

    def reset(self):
        self._records = []
        self._bounds = []

    @torch.no_grad()
    def update(self, hyp, ref, hyp_lengths=None, ref_lengths=None, n_hyp=None):
        """hyp: (B, cols) 1-best rows or (B, nbest, cols) n-best rows, best first; ref (B, cols') transcripts;
        lengths per row or None; n_hyp (B,): hypotheses that exist per sample (None: all)."""
        if hyp.dim() == 2:
            hyp = hyp[:, None, :]
        if hyp.dim() != 3 or ref.dim() != 2 or ref.shape[0] != hyp.shape[0]:
            raise ValueError(f"hyp {tuple(hyp.shape)} / ref {tuple(ref.shape)}: expected (B, [nbest,] cols) and "
                             f"(B, cols')")
        dev = _device(hyp, ref)
        B, W, cols = hyp.shape
        hyp = _rows(hyp, dev).reshape(B * W, cols)
        use_long, bound = K.edit_path(cols, ref.shape[1])
        dist, cnt = K.edit_distance(hyp, _rows(ref, dev), _i32(hyp_lengths, dev), _i32(ref_lengths, dev), self.drop,
                                    self.stop, "group", W, _i32(n_hyp, dev), long=use_long)
        self._records.append((dist, cnt, B, W))
        self._bounds.append(bound)

    def update_result(self, result, text):
        """result: a BeamResult / RescoreResult of any decoder (slots with a non-finite score are absent; they come
        last in every decoder's order), or ctc_greedy's (tokens, lengths) pair; text (B, n) transcripts."""
        if hasattr(result, "scores"):
            dev = _device(result.tokens, text)
            n_hyp = torch.isfinite(result.scores.to(dev)).sum(dim=1)
            return self.update(result.tokens, text, None, None, n_hyp)
        tokens, lengths = result
        return self.update(tokens, text, lengths)

    def compute(self):
        """One host copy of everything accumulated, then reduce_counts."""
        if not self._records:
            return reduce_counts([])
        flat = torch.cat([t.reshape(-1) for d, c, _, _ in self._records for t in (d, c)]).cpu()
        host, o = [], 0
        for _, _, B, W in self._records:
            host.append((flat[o:o + B * W].view(B, W), flat[o + B * W:o + 5 * B * W].view(B, W, 4)))
            o += 5 * B * W
        return reduce_counts(host, max_tokens=list(self._bounds))


@torch.no_grad()
def mbr_rerank(result, scale=1.0, drop=(), stop=None):
    """Minimum-Bayes-risk re-ordering of an n-best result (BeamResult or RescoreResult, tokens (B, W <= 16, cols)):
    each sample's hypotheses sorted by their expected edit distance to the others under the posterior
    softmax(scale * scores) (ties and the order of absent hypotheses: by slot).  scale = 0 ranks by the plain mean
    distance (the medoid first).  drop / stop describe the token rows as in edit_distance.  One CROSS-mode
    asrx_edit_distance launch, one asrx_mbr_rank launch, one host copy.  Returns the same fields re-ordered plus
    `risks` (B, W): a RescoreResult for a RescoreResult, else an MbrResult."""
    scale = check_mbr_scale(scale)
    tokens, lengths, scores = result.tokens, result.lengths, result.scores
    if tokens.dim() != 3 or not 1 <= tokens.shape[1] <= 16 or tokens.shape[0] == 0 or tokens.shape[2] == 0:
        raise ValueError(f"mbr_rerank takes tokens (B > 0, 1..16, cols > 0), got {tuple(tokens.shape)}")
    dev = _device(tokens, scores)
    B, W, cols = tokens.shape
    sc = scores.to(device=dev, dtype=torch.float32).contiguous()
    n_hyp = torch.isfinite(sc).sum(dim=1).to(torch.int32)
    dist, _ = K.edit_distance(_rows(tokens, dev).reshape(B * W, cols), None, None, None, drop, stop, "cross", W, n_hyp,
                              counts=False, long=K.edit_path(cols)[0])
    risk, order = K.mbr_rank(dist, sc.reshape(-1), B, W, scale, n_hyp)
    flat = torch.cat([risk.view(torch.int32).reshape(-1), order.reshape(-1)]).cpu()
    risk = flat[:B * W].view(torch.float32).view(B, W)
    order = flat[B * W:].view(B, W).long()

    def pick(t):
        t = t.cpu()
        return t.gather(1, order if t.dim() == 2 else order[:, :, None].expand(-1, -1, t.shape[2]))

    out = (pick(tokens), pick(lengths), pick(scores))
    if isinstance(result, RescoreResult):
        lm_scores = getattr(result, "lm_scores", None)
        return RescoreResult(*out, pick(result.att_scores), pick(result.ctc_scores), risk.gather(1, order),
                             None if lm_scores is None else pick(lm_scores))
    return MbrResult(*out, risk.gather(1, order))
