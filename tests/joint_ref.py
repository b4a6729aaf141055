"""Torch references for joint CTC/attention beam search (CPU; fp64, or fp32 to measure the formulas' own
single-precision error, from which the kernel tolerances derive).

CTC prefix scoring, 0-based frames, y_t = softmax(ctc_logits[t]), T_b valid frames.  For a prefix g (the generated
labels), gn_t(g) / gb_t(g) = the probability of all paths over frames 0..t that collapse to g and end in a non-blank /
in the blank; at t = -1 gb = 1 for the empty prefix and everything else is 0.  For h = g.c, c != blank:
    phi_t   = gb_{t-1}(g) + (c != last(g) ? gn_{t-1}(g) : 0)
    psi(h)  = sum_t phi_t y_t(c)                                   the prefix probability of h
    gn_t(h) = (gn_{t-1}(h) + phi_t) y_t(c)
    gb_t(h) = (gb_{t-1}(h) + gn_{t-1}(h)) y_t(blank)
    p(g ends) = gn_{T_b-1}(g) + gb_{T_b-1}(g)
The step score of a continuation is delta(g, c) = log psi(g.c) - log psi(g) (log psi(empty) = 0), for c = EOS
log p(g ends) - log psi(g), for c = blank -inf; summed along a finished hypothesis it telescopes to log p_ctc.

A PrefixState holds R = B*W slots in natural-log units: nb [R, T] = log(gn_t + gb_t), b [R, T] = log gb_t (-inf at
t >= T_b), logpsi [R], last [R] (-1: the empty prefix), which are exactly the two variants of phi the scorer needs."""
import itertools
import math
from typing import NamedTuple

import torch

from tests import beam_ref

INF = float("inf")


class PrefixState(NamedTuple):
    nb: torch.Tensor
    b: torch.Tensor
    logpsi: torch.Tensor
    last: torch.Tensor


def log_probs(logits, dtype=torch.float64):
    """logits [B, T, >= V] -> log softmax over the given columns, in dtype."""
    return torch.log_softmax(logits.to(dtype), dim=-1)


def frame_counts(B, T, input_lengths=None):
    if input_lengths is None:
        return [T] * B
    return [max(0, min(T, int(n))) for n in input_lengths]


def root_state(lp, frames, W, blank):
    """The empty prefix in every slot: gn = 0, gb_t = prod_{u <= t} y_u(blank)."""
    B, T, _ = lp.shape
    nb = torch.full((B * W, T), -INF, dtype=lp.dtype)
    for b in range(B):
        nb[b * W:(b + 1) * W, :frames[b]] = torch.cumsum(lp[b, :frames[b], blank], 0)
    return PrefixState(nb, nb.clone(), torch.zeros(B * W, dtype=lp.dtype), torch.full((B * W,), -1, dtype=torch.int64))


def _phi(st, r, Tb):
    """(phi with gn, phi without) of slot r over t < Tb: the state one frame earlier, the t = -1 values in front."""
    first = torch.tensor([0.0 if int(st.last[r]) < 0 else -INF], dtype=st.nb.dtype)
    if Tb == 0:
        return first[:0], first[:0]
    return torch.cat([first, st.nb[r, :Tb - 1]]), torch.cat([first, st.b[r, :Tb - 1]])


def end_score(frames, st, W):
    """[R]: log p(g ends) - log psi(g), the step score of EOS (-inf for a slot whose psi is 0)."""
    out = torch.full_like(st.logpsi, -INF)
    for r in range(st.logpsi.numel()):
        Tb = frames[r // W]
        if st.logpsi[r] != -INF:
            out[r] = st.nb[r, Tb - 1] - st.logpsi[r] if Tb > 0 else (0.0 if int(st.last[r]) < 0 else -INF)
    return out


def prefix_score(lp, frames, st, W, blank, eos):
    """delta [R, V]: the step score of every continuation of every slot (eos < 0: no EOS column, every column but
    the blank's is a label)."""
    B, T, V = lp.shape
    out = torch.full((B * W, V), -INF, dtype=lp.dtype)
    ends = end_score(frames, st, W)
    for r in range(B * W):
        b = r // W
        Tb = frames[b]
        base = st.logpsi[r]
        if base == -INF:
            continue
        last = int(st.last[r])
        if Tb > 0:
            pn, pb = _phi(st, r, Tb)
            x = pn[:, None] + lp[b, :Tb]
            if last >= 0:
                x[:, last] = pb + lp[b, :Tb, last]
            out[r] = torch.logsumexp(x, dim=0) - base
        if eos >= 0:
            out[r, eos] = ends[r]
        out[r, blank] = -INF
    return out


def prefix_advance(lp, frames, st, W, parent, tok, fin_prev, blank, eos):
    """The state after a selection: slot j of sample b extends slot parent[j] by tok[j]; a finished parent or an
    EOS copies the parent's state."""
    B, T, V = lp.shape
    R = B * W
    src = torch.tensor([(j // W) * W + int(parent[j]) for j in range(R)])
    nb, bb = st.nb[src].clone(), st.b[src].clone()
    logpsi, last = st.logpsi[src].clone(), st.last[src].clone()
    chain = [j for j in range(R) if not bool(fin_prev[src[j]]) and int(tok[j]) != eos]
    if not chain:
        return PrefixState(nb, bb, logpsi, last)
    Tmax = max(frames[j // W] for j in chain)
    n = len(chain)
    phi = torch.full((n, max(Tmax, 1)), -INF, dtype=lp.dtype)
    yc = torch.zeros(n, max(Tmax, 1), dtype=lp.dtype)
    yb = torch.zeros(n, max(Tmax, 1), dtype=lp.dtype)
    live = torch.zeros(n, max(Tmax, 1), dtype=torch.bool)
    for i, j in enumerate(chain):
        b, Tb, c = j // W, frames[j // W], int(tok[j])
        pn, pb = _phi(st, int(src[j]), Tb)
        phi[i, :Tb] = pb if c == int(st.last[src[j]]) else pn
        yc[i, :Tb] = lp[b, :Tb, c]
        yb[i, :Tb] = lp[b, :Tb, blank]
        live[i, :Tb] = True
    gn = torch.full((n,), -INF, dtype=lp.dtype)
    gb = torch.full((n,), -INF, dtype=lp.dtype)
    o_nb = torch.full((n, T), -INF, dtype=lp.dtype)
    o_b = torch.full((n, T), -INF, dtype=lp.dtype)
    for t in range(Tmax):
        nn = torch.logaddexp(gn, phi[:, t]) + yc[:, t]
        nbk = torch.logaddexp(gb, gn) + yb[:, t]
        gn, gb = nn, nbk
        o_nb[:, t] = torch.where(live[:, t], torch.logaddexp(gn, gb), o_nb[:, t])
        o_b[:, t] = torch.where(live[:, t], gb, o_b[:, t])
    psi = torch.logsumexp(torch.where(live, phi + yc, torch.full_like(phi, -INF)), dim=1)
    for i, j in enumerate(chain):
        nb[j], bb[j], logpsi[j], last[j] = o_nb[i], o_b[i], psi[i], int(tok[j])
    return PrefixState(nb, bb, logpsi, last)


def sequence_ctc_score(lp_b, Tb, labels, blank, eos):
    """log p_ctc of one label sequence as the scorer sees it: the sum of delta along the sequence plus the EOS term
    (one sample, lp_b [T, V]).  -inf for a sequence no alignment of T_b frames can produce."""
    lp = lp_b.unsqueeze(0)
    st = root_state(lp, [Tb], 1, blank)
    total = 0.0
    zero = torch.zeros(1, dtype=torch.uint8)
    for c in labels:
        total = total + float(prefix_score(lp, [Tb], st, 1, blank, eos)[0, c])
        st = prefix_advance(lp, [Tb], st, 1, torch.zeros(1, dtype=torch.int64), torch.tensor([c]), zero, blank, eos)
    return total + float(prefix_score(lp, [Tb], st, 1, blank, eos)[0, eos])


def brute_force_prefix(lp_b, blank):
    """By enumeration of all V**T paths (one sample, lp_b [T, V] fp64): {labels: (psi, p_end)} for every label
    sequence that some path produces as a prefix; psi(g) = the probability that the collapsed path STARTS with g
    (psi(empty) = 1), p_end(g) = that it EQUALS g."""
    T, V = lp_b.shape
    psi, end = {}, {}
    for path in itertools.product(range(V), repeat=T):
        p = math.exp(sum(float(lp_b[t, s]) for t, s in enumerate(path)))
        out, prev = [], None
        for s in path:
            if s != prev and s != blank:
                out.append(s)
            prev = s
        end[tuple(out)] = end.get(tuple(out), 0.0) + p
        for k in range(len(out) + 1):
            psi[tuple(out[:k])] = psi.get(tuple(out[:k]), 0.0) + p
    return psi, end


def joint_step(logits, extra, att_weight, extra_weight, score, fin, length, eos, V):
    """beam_ref.beam_step with the second term: a live beam's candidate is score + att_weight * log_softmax(logits)
    + extra_weight * extra (fp64; a NaN candidate, e.g. 0 * -inf, reads as -inf).  logits [B, W, >= V],
    extra [B, W, >= V], score / fin / length [B, W]."""
    B, W = score.shape
    lp = torch.log_softmax(logits[:, :, :V].double(), dim=-1)
    ex = extra[:, :, :V].double()
    out = dict(score=torch.empty(B, W, dtype=torch.float64), tok=torch.empty(B, W, dtype=torch.int64),
               parent=torch.empty(B, W, dtype=torch.int64), src_row=torch.empty(B, W, dtype=torch.int64),
               fin=torch.empty(B, W, dtype=torch.bool), len=torch.empty(B, W, dtype=torch.int64))
    gap = INF
    for b in range(B):
        cand = score[b].double()[:, None] + att_weight * lp[b] + extra_weight * ex[b]
        exists = torch.ones(W, V, dtype=torch.bool)
        for w in range(W):
            if fin[b, w]:
                exists[w] = False
                exists[w, eos] = True
                cand[w, eos] = score[b, w].double()
        flat, vals, g = beam_ref.select(cand.flatten(), exists.flatten(), W)
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


def joint_search(step_logits, lp, frames, W, eos, blank, lam, steps):
    """Joint beam search over any source of attention logits: step_logits(rows [B, W, s] generated tokens) ->
    [B, W, V].  Returns dict(tokens [B, W, steps] in slot order, score, fin, len [B, W], gap, history): history =
    per step (parent [B*W], tok [B*W], the flags before the step [B*W], the step's delta [B*W, V])."""
    B, T, V = lp.shape
    st = root_state(lp, frames, W, blank)
    score = torch.full((B, W), -INF, dtype=torch.float64)
    score[:, 0] = 0.0
    fin = torch.zeros(B, W, dtype=torch.bool)
    length = torch.zeros(B, W, dtype=torch.int64)
    rows = torch.zeros(B, W, 0, dtype=torch.int64)
    gap = INF
    history = []
    for _ in range(steps):
        delta = prefix_score(lp, frames, st, W, blank, eos).view(B, W, V)
        r = joint_step(step_logits(rows), delta, 1.0 - lam, lam, score, fin, length, eos, V)
        gap = min(gap, r["gap"])
        history.append((r["parent"].flatten(), r["tok"].flatten(), fin.flatten().clone(), delta.view(B * W, V)))
        st = prefix_advance(lp, frames, st, W, r["parent"].flatten(), r["tok"].flatten(), fin.flatten(), blank, eos)
        rows = torch.cat([rows.gather(1, r["parent"][:, :, None].expand(-1, -1, rows.shape[2])),
                          r["tok"][:, :, None]], dim=2)
        score, fin, length = r["score"], r["fin"], r["len"]
    return dict(tokens=rows, score=score, fin=fin, len=length, gap=gap, history=history)


def joint_beam_search(P, cfg, enc, prompt, W, eos, max_len, ctc_weight, blank, input_lengths=None, final_norm=True,
                      length_penalty=0.0):
    """Reference joint CTC/attention beam search over the oracle decoder and the CTC head enc @ ctc_head.weight^T
    (P["ctc_head.weight"], [>= V, d]; fp64 throughout).  enc [B, Te, d], prompt [B, 1].  Returns what
    beam_ref.beam_search returns: tokens [B, W, 1 + max_len], lengths, scores (the joint scores), gap, finished,
    hypotheses ranked best first."""
    P = {k: v.double() for k, v in P.items()}
    enc = enc.double()
    B, Te, _ = enc.shape
    V = cfg.vocab_size
    assert prompt.shape == (B, 1)
    lp = log_probs(torch.nn.functional.linear(enc, P["ctc_head.weight"][:V]))
    frames = frame_counts(B, Te, input_lengths)
    tokens = torch.empty(B, W, 1 + max_len, dtype=torch.int64)
    lengths = torch.empty(B, W, dtype=torch.int64)
    scores = torch.empty(B, W, dtype=torch.float64)
    gap, finished = INF, 0
    for b in range(B):
        def step_logits(rows, b=b):
            full = torch.cat([prompt[b].long().view(1, 1).expand(W, 1), rows[0]], dim=1)
            return beam_ref.decoder_logits(P, cfg, full, enc[b:b + 1].expand(W, -1, -1), final_norm).unsqueeze(0)
        r = joint_search(step_logits, lp[b:b + 1], frames[b:b + 1], W, eos, blank, ctc_weight, max_len)
        gap = min(gap, r["gap"])
        key = r["score"][0].clone()
        if length_penalty != 0.0:
            key = key / r["len"][0].clamp(min=1).double() ** length_penalty
        key[~torch.isfinite(r["score"][0])] = -INF
        order = torch.sort(key, descending=True, stable=True).indices
        tokens[b] = torch.cat([prompt[b].long().view(1, 1).expand(W, 1), r["tokens"][0]], dim=1)[order]
        lengths[b], scores[b] = r["len"][0][order], r["score"][0][order]
        finished += int(r["fin"].sum())
    return dict(tokens=tokens, lengths=lengths, scores=scores, gap=gap, finished=finished)
