"""Torch references for the beam-search tests (CPU, fp64): one selection step as asrx_beam_step defines it, and a
whole beam search over the oracle decoder with full-prefix recomputation (no cache, no kernels).

Ordering rule: candidates by descending score, ties by ascending flat index w*V + v (a stable descending sort of
the flattened W x V candidates); a finished beam offers only (w, eos) at its own score; NaN reads as -inf."""
import itertools

import torch
import torch.nn.functional as F

from oracle.ref_model import _ln, decoder_layer, pe_table

INF = float("inf")


def select(cand, exists, W):
    """cand [W*V] fp64 scores, exists [W*V] bool.  Returns (flat indices of the W best, their scores, gap): gap is
    the smallest difference between consecutive candidates among the W + 1 best.  Two -inf neighbours are an exact
    tie in every precision (settled by the index rule), so they do not count towards the gap."""
    idx = torch.nonzero(exists).flatten()
    vals = torch.nan_to_num(cand[idx], nan=-INF, posinf=INF, neginf=-INF)
    order = torch.sort(vals, descending=True, stable=True)
    assert idx.numel() >= W
    top = order.values[:W + 1]
    gap = INF
    for a, b in zip(top[:-1].tolist(), top[1:].tolist()):
        if not (a == -INF and b == -INF):
            gap = min(gap, a - b)
    return idx[order.indices[:W]], order.values[:W], gap


def beam_step(logits, score, fin, length, eos, V):
    """One step for B samples.  logits [B, W, >=V] (columns past V ignored), score / fin / length [B, W].
    Returns dict(score, tok, parent, src_row, fin, len, n_live, gap), computed in fp64."""
    B, W = score.shape
    lp = torch.log_softmax(logits[:, :, :V].double(), dim=-1)
    out = dict(score=torch.empty(B, W, dtype=torch.float64), tok=torch.empty(B, W, dtype=torch.int64),
               parent=torch.empty(B, W, dtype=torch.int64), src_row=torch.empty(B, W, dtype=torch.int64),
               fin=torch.empty(B, W, dtype=torch.bool), len=torch.empty(B, W, dtype=torch.int64))
    gap = INF
    for b in range(B):
        cand = score[b].double()[:, None] + lp[b]
        exists = torch.ones(W, V, dtype=torch.bool)
        for w in range(W):
            if fin[b, w]:
                exists[w] = False
                exists[w, eos] = True
                cand[w, eos] = score[b, w].double()
        flat, vals, g = select(cand.flatten(), exists.flatten(), W)
        gap = min(gap, g)
        parent, tok = flat // V, flat % V
        pfin = fin[b].bool()[parent]
        out["score"][b], out["tok"][b], out["parent"][b] = vals, tok, parent
        out["src_row"][b] = b * W + parent
        out["fin"][b] = pfin | (tok == eos)
        out["len"][b] = length[b].long()[parent] + (~pfin).long()
    out["n_live"] = int((~out["fin"]).sum())
    out["gap"] = gap
    return out


def decoder_logits(P, cfg, rows, enc, final_norm):
    """Last-position logits [R, V] (fp64) of the oracle decoder on token rows [R, L] with a causal mask, the
    optional final LayerNorm (Decoder.forward applies it, Decoder.evaluate does not) and the classifier."""
    L = rows.shape[1]
    pe = pe_table(cfg.dec_len, cfg.d_model).double()
    causal = torch.triu(torch.ones((L, L), dtype=torch.uint8), diagonal=1)
    h = F.embedding(rows, P["decoder._embedding.weight"], padding_idx=cfg.pad_id) + pe[:L].unsqueeze(0)
    for l in range(cfg.n_dec):
        h = decoder_layer(P, f"decoder._layers.{l}", h, causal, enc, cfg, False)
    if final_norm:
        h = _ln(P, "decoder._norm_layer", h)
    return F.linear(h, P["decoder._classifier.weight"])[:, -1]


def beam_search(P, cfg, enc, prompt, W, eos, max_len, final_norm=True, length_penalty=0.0):
    """Reference beam search.  P: oracle parameters (any float dtype; run in fp64), enc [B, Te, d], prompt [B, L0].
    Returns dict(tokens [B, W, L0 + max_len], lengths [B, W], scores [B, W] fp64, gap, finished): hypotheses ranked
    best first (score / len**length_penalty, dead ones last), gap = the smallest margin any selection had,
    finished = the number of final hypotheses that ended on EOS."""
    P = {k: v.double() for k, v in P.items()}
    enc = enc.double()
    B, L0 = prompt.shape
    V = cfg.vocab_size
    tokens = torch.empty(B, W, L0 + max_len, dtype=torch.int64)
    lengths = torch.empty(B, W, dtype=torch.int64)
    scores = torch.empty(B, W, dtype=torch.float64)
    gap, finished = INF, 0
    for b in range(B):
        rows = prompt[b].long().unsqueeze(0).repeat(W, 1)
        score = torch.full((1, W), -INF, dtype=torch.float64)
        score[0, 0] = 0.0
        fin = torch.zeros(1, W, dtype=torch.bool)
        length = torch.zeros(1, W, dtype=torch.int64)
        for _ in range(max_len):
            lg = decoder_logits(P, cfg, rows, enc[b:b + 1].expand(W, -1, -1), final_norm)
            r = beam_step(lg.unsqueeze(0), score, fin, length, eos, V)
            gap = min(gap, r["gap"])
            rows = torch.cat([rows[r["parent"][0]], r["tok"][0].unsqueeze(1)], dim=1)
            score, fin, length = r["score"], r["fin"], r["len"]
        key = score[0].clone()
        if length_penalty != 0.0:
            key = key / length[0].clamp(min=1).double() ** length_penalty
        key[~torch.isfinite(score[0])] = -INF
        order = torch.sort(key, descending=True, stable=True).indices
        tokens[b], lengths[b], scores[b] = rows[order], length[0][order], score[0][order]
        finished += int(fin.sum())
    return dict(tokens=tokens, lengths=lengths, scores=scores, gap=gap, finished=finished)


def sequence_score(P, cfg, enc_b, row, L0, eos, final_norm=True):
    """Summed log-probability (fp64) the oracle decoder gives the generated part row[L0:] of one token row, up to
    and including the first EOS."""
    P = {k: v.double() for k, v in P.items()}
    total = 0.0
    for i in range(L0, row.numel()):
        lg = decoder_logits(P, cfg, row[:i].long().unsqueeze(0), enc_b.double().unsqueeze(0), final_norm)
        total += float(torch.log_softmax(lg[0, :cfg.vocab_size], dim=-1)[int(row[i])])
        if int(row[i]) == eos:
            break
    return total


def brute_force_best(P, cfg, enc_b, prompt_row, steps, eos, final_norm=True):
    """Exhaustive search over all V**steps continuations of one prompt under the finished rule (after EOS only
    EOS, at no cost): the best (token row, score), the first of equal ones in lexicographic order."""
    P = {k: v.double() for k, v in P.items()}
    V = cfg.vocab_size
    best, best_score = None, -INF
    for seq in itertools.product(range(V), repeat=steps):
        row = prompt_row.long().clone()
        score, done, ok = 0.0, False, True
        for tok in seq:
            if done:
                if tok != eos:
                    ok = False
                    break
            else:
                lg = decoder_logits(P, cfg, row.unsqueeze(0), enc_b.double().unsqueeze(0), final_norm)
                score += float(torch.log_softmax(lg[0, :V], dim=-1)[tok])
                done = tok == eos
            row = torch.cat([row, torch.tensor([tok])])
        if ok and score > best_score:
            best, best_score = row, score
    return best, best_score
