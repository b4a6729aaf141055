"""Reference CTC prefix beam search (CPU, numpy; fp64, or fp32 to measure the recursion's own single-precision error,
from which the kernel tolerances derive) for asrx_ctc_prefix_beam, and the references of the rescoring kernels.

The beam is an ordered list of prefixes (tuples of labels) keyed by a dictionary; a prefix g carries (pb, pnb), the
log-probability of the paths over the frames so far that collapse to g and end in the blank / in a non-blank, and
tot = logaddexp(pb, pnb).  At frame t with y = log_softmax(logits[t]) the candidate matrix is [W][V]:
    column blank of row w     the stay: pb' = tot(w) + y(blank), pnb' = pnb(w) + y(last(w)) (-inf for the root)
    column c != blank         the extension g.c: pnb' = (c == last(w) ? pb(w) : tot(w)) + y(c), pb' = -inf; a prefix
                              that already has max_labels labels offers -inf
    merge                     if g.c is itself in the beam (row w'), the extension's mass is added to the stay of w',
                              pnb'(w') = logaddexp(pnb'(w'), ext), stay term first then the single possible parent's,
                              and candidate (w, c) becomes -inf
    selection                 the W best by logaddexp(pb', pnb') under (score descending, flat index w*V + c
                              ascending), NaN read as -inf, -inf never selected; the new beam is in selection order
Every frame's scores are renormalised by the frame's best score; the offsets accumulate in a Python float (a double)."""
import numpy as np
import torch

INF = float("inf")


def log_softmax(x):
    mx = x.max(axis=-1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(axis=-1, keepdims=True, dtype=x.dtype)))


def prefix_beam(logits, W, blank, max_labels, frames=None, dtype=np.float64, identity="labels"):
    """logits [T, >= V] of one utterance (any float array; the first V = logits.shape[1] columns are all read, so
    slice before the call).  Returns dict(prefixes: list of label tuples in final rank order, scores: float64
    [n] natural-log totals, renorm: the same without the accumulated offset (dtype), boundary: the smallest gap
    between the W-th and the (W+1)-th candidate over all frames, final: the smallest gap between neighbours of the
    final ranking, merges: how many extensions were merged into a stay, recreated: how many times a prefix that had
    been pruned came back into the beam while one of its children had stayed there: the case in which a prefix must
    be recognised by its labels, not by when it was made).

    identity="node" is NOT the algorithm: it models a search that knows a prefix by the node made when it was first
    selected (a child points to its parent's node), which loses the merge once a pruned parent comes back under a
    new node.  The tests use it to show that their re-creation cases tell the two apart."""
    x = np.asarray(logits).astype(dtype)
    T, V = x.shape
    Tb = T if frames is None else max(0, min(T, int(frames)))
    y = log_softmax(x) if T else x
    ninf = dtype(-INF)
    beam, pb, pnb = [()], np.array([0.0], dtype), np.array([ninf], dtype)
    off, boundary, merges, recreated = 0.0, INF, 0, 0
    ever = {()}
    node, par, made = [0], [-1], 1          # identity="node": each slot's node, its parent's, the next fresh id
    with np.errstate(invalid="ignore"):
        for t in range(Tb):
            n = len(beam)
            if n == 0:
                break
            index = {g: w for w, g in enumerate(beam)}
            tot = np.logaddexp(pb, pnb)
            yt = y[t]
            cand = tot[:, None] + yt[None, :]
            spnb = np.full(n, ninf, dtype)
            for w, g in enumerate(beam):
                if g:
                    cand[w, g[-1]] = pb[w] + yt[g[-1]]
                    spnb[w] = pnb[w] + yt[g[-1]]
                if len(g) >= max_labels:
                    cand[w, :] = ninf
            spb = tot + yt[blank]
            nodes = {v: w for w, v in enumerate(node)}
            for w1, g in enumerate(beam):      # stay term first, then the one parent that may be in the beam
                if g and (g[:-1] in index if identity == "labels" else par[w1] in nodes):
                    w0 = index[g[:-1]] if identity == "labels" else nodes[par[w1]]
                    spnb[w1] = np.logaddexp(spnb[w1], cand[w0, g[-1]])
                    cand[w0, g[-1]] = ninf
                    merges += 1
            spb = np.where(np.isnan(spb), ninf, spb)
            spnb = np.where(np.isnan(spnb), ninf, spnb)
            cand[:, blank] = np.logaddexp(spb, spnb)
            flat = np.where(np.isnan(cand), ninf, cand).reshape(-1)
            order = np.lexsort((np.arange(flat.size), -flat))[:W + 1]
            order = [int(i) for i in order if flat[i] > -INF]
            if len(order) > W:
                boundary = min(boundary, float(flat[order[W - 1]]) - float(flat[order[W]]))
                order = order[:W]
            if not order:
                beam, pb, pnb = [], pb[:0], pnb[:0]
                break
            m = flat[order[0]]
            off += float(m)
            nb, npb, npnb, nnode, npar = [], [], [], [], []
            for i in order:
                w, c = divmod(i, V)
                if c == blank:
                    nb.append(beam[w]); npb.append(spb[w] - m); npnb.append(spnb[w] - m)
                    nnode.append(node[w]); npar.append(par[w])
                else:
                    nb.append(beam[w] + (c,)); npb.append(ninf); npnb.append(flat[i] - m)
                    nnode.append(made); npar.append(node[w])
                    made += 1
            node, par = nnode, npar
            fresh = [g for g in nb if g in ever and g not in index]
            recreated += sum(1 for g in fresh if any(len(q) == len(g) + 1 and q[:-1] == g for q in nb))
            ever.update(nb)
            beam, pb, pnb = nb, np.array(npb, dtype), np.array(npnb, dtype)
    tot = np.logaddexp(pb, pnb) if len(beam) else np.zeros(0, dtype)
    final = min([float(tot[i]) - float(tot[i + 1]) for i in range(len(beam) - 1)], default=INF)
    return dict(prefixes=beam, scores=off + tot.astype(np.float64), renorm=tot, boundary=boundary, final=final,
                merges=merges, recreated=recreated)


def batch(logits, V, W, blank, max_labels, lengths=None, dtype=np.float64):
    """prefix_beam per sample of logits [B, T, ld] (torch or numpy): list of its results."""
    x = logits.numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    return [prefix_beam(x[b, :, :V], W, blank, max_labels, None if lengths is None else lengths[b], dtype)
            for b in range(x.shape[0])]


def bounds(ref64, ref32):
    """(selection bound, score bound function) of one case from the fp64 and fp32 runs of the reference, the rule of
    DESIGN sections 9 and 10: 4 x the fp32 recursion's own error, floored at 1e-5 * max(1, |value|).  The kernel
    selects and ranks on the RENORMALISED scores (magnitude O(10)), so the margins are held against the bound of
    those; the scores that leave carry the accumulated offset and are held against the bound at their own magnitude.
    The fp32 run must have kept the fp64 run's hypotheses (the margins guarantee it)."""
    e_sel = e_out = 0.0
    big = 1.0
    for a, b in zip(ref64, ref32):
        assert a["prefixes"] == b["prefixes"], "fp32 and fp64 reference runs disagree on the hypotheses"
        if len(a["prefixes"]):
            e_sel = max(e_sel, float(np.abs(a["renorm"].astype(np.float64) - b["renorm"].astype(np.float64)).max()))
            e_out = max(e_out, float(np.abs(a["scores"] - b["scores"]).max()))
            big = max(big, float(np.abs(a["renorm"]).max()))
    sel = max(4 * e_sel, 1e-5 * big)
    return sel, (lambda v: max(4 * e_out, 1e-5 * max(1.0, abs(v))))


def enumerate_paths(logits, blank):
    """{label tuple: probability} by summing all V**T frame paths of logits [T, V] (fp64)."""
    import itertools
    y = log_softmax(np.asarray(logits, np.float64))
    T, V = y.shape
    out = {}
    for path in itertools.product(range(V), repeat=T):
        g, prev = [], -1
        for c in path:
            if c != prev and c != blank:
                g.append(c)
            prev = c
        out[tuple(g)] = out.get(tuple(g), 0.0) + float(np.exp(sum(y[t, c] for t, c in enumerate(path))))
    return out


# ------------------------------------------------------------------------------------------------ second pass

def hyp_tokens(prefixes, n_slots, L, bos, eos, pad, ignore):
    """asrx_hyp_tokens for one sample: the rows of its live prefixes, then dead slots."""
    dec_in = torch.full((n_slots, L), pad, dtype=torch.int64)
    dec_tgt = torch.full((n_slots, L), ignore, dtype=torch.int64)
    mask = torch.zeros(n_slots, L)
    for j, g in enumerate(prefixes):
        g = list(g)[:L - 1]
        n = len(g)
        dec_in[j, 0] = bos
        dec_in[j, 1:n + 1] = torch.tensor(g, dtype=torch.int64)
        dec_tgt[j, :n] = torch.tensor(g, dtype=torch.int64)
        dec_tgt[j, n] = eos
        mask[j, :n + 1] = 1
    return dec_in, dec_tgt, mask


def seq_logprob(logits, tgt, ignore):
    """logits [N, L, V] -> fp64 [N]: the summed log-softmax at the targets that are not `ignore`."""
    lp = torch.log_softmax(logits.double(), dim=-1)
    keep = tgt != ignore
    g = lp.gather(2, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    return torch.where(keep, g, torch.zeros_like(g)).sum(dim=1)


def rank(scores):
    """Slots of fp [B, W] scores best first: descending, ties by slot, NaN read as -inf."""
    key = torch.where(torch.isnan(scores), torch.full_like(scores, -INF), scores)
    return torch.sort(key, dim=1, descending=True, stable=True).indices
