"""References for the n-gram LM tests (CPU, fp64).

The LM reference is the textbook recursion over the n-gram DICTIONARY {token tuple: (logp, backoff)}:
    p(w | h) = the entry of h + (w,) if there is one, else backoff(h) + p(w | h[1:])      (log domain)
with backoff(h) = 0 for a context that is no entry and p(w | ()) = the unigram entry or `oov`.  It never sees the
trie, the node numbers or the per-order lookups of asrx.lm / csrc/ngram.hip.

lm_beam_search is the LM-fused beam search, composed from joint_ref.joint_step, joint_ref.prefix_score /
prefix_advance and beam_ref.decoder_logits: a live candidate scores
    score + (1 - lam) * log p_att + lam * delta_ctc + beta * log p_lm + bonus."""
import torch

from tests import beam_ref, joint_ref

INF = float("inf")


def logprob(ngrams, order, history, w, oov=-INF):
    """log p(w | the last order - 1 tokens of history), fp64."""
    h = tuple(int(t) for t in history)
    h = h[len(h) - min(len(h), order - 1):]
    return _rec(ngrams, h, int(w), oov)


def _rec(ngrams, h, w, oov):
    g = h + (w,)
    if g in ngrams:
        return float(ngrams[g][0])
    if not h:
        return oov
    bo = ngrams[h][1] if h in ngrams else 0.0
    return (0.0 if bo is None else float(bo)) + _rec(ngrams, h[1:], w, oov)


def partials(ngrams, order, history, w, oov=-INF):
    """The running sums of the same evaluation, the explicit entry first and the back-off weights added from the
    shortest context to the longest (the order the kernels add them in): what an fp32 evaluation rounds."""
    h = tuple(int(t) for t in history)
    h = h[len(h) - min(len(h), order - 1):]
    bos = []
    while True:
        g = h + (int(w),)
        if g in ngrams:
            acc = float(ngrams[g][0])
            break
        if not h:
            acc = oov
            break
        bo = ngrams[h][1] if h in ngrams else 0.0
        bos.append(0.0 if bo is None else float(bo))
        h = h[1:]
    out = [acc]
    for b in reversed(bos):
        acc += b
        out.append(acc)
    return out


def row(ngrams, order, history, V, oov=-INF):
    """fp64 [V]: log p(v | history) for every v."""
    return torch.tensor([logprob(ngrams, order, history, v, oov) for v in range(V)], dtype=torch.float64)


def sequence_logprob(ngrams, order, tokens, bos, V, ignore=None, oov=-INF):
    """(sum of log p(token | bos, earlier tokens), scored positions) of one row; positions equal to `ignore` or
    outside [0, V) are skipped and do not enter the history.  bos None or < 0: no sentence start."""
    hist = [] if bos is None or bos < 0 else [int(bos)]
    total, n = 0.0, 0
    for t in tokens:
        t = int(t)
        if t == ignore or not 0 <= t < V:
            continue
        total += logprob(ngrams, order, hist, t, oov)
        hist.append(t)
        n += 1
    return total, n


def brute_force_order3(ngrams, V, oov=-INF):
    """Every p(w | a b), p(w | a), p(w) of an order-3 table straight from the definition of a back-off model, written
    out case by case instead of recursively: {(history tuple, w): logp}."""
    def e(g):
        return ngrams[g][0] if g in ngrams else None

    def bo(h):
        b = ngrams[h][1] if h in ngrams else 0.0
        return 0.0 if b is None else b

    out = {}
    for w in range(V):
        uni = e((w,)) if e((w,)) is not None else oov
        out[((), w)] = uni
        for a in range(V):
            bi = e((a, w)) if e((a, w)) is not None else bo((a,)) + uni
            out[((a,), w)] = bi
            for z in range(V):
                tri = e((z, a, w))
                out[((z, a), w)] = tri if tri is not None else bo((z, a)) + bi
    return out


def random_table(V, order, seed, density=0.3, max_children=None, drop_suffix=True, max_contexts=150):
    """A random prefix-closed table {tuple: (logp, backoff)} with logp in [-12, 0] and backoff in [-3, 0]: every
    unigram, then per order a random subset of the extensions of (at most max_contexts, evenly spread, of) the previous
    order's n-grams, so the size stays linear in V and in the order.  It is NOT suffix-closed (drop_suffix removes the
    bigram (b, c) of one trigram (a, b, c) where that leaves no orphan)."""
    g = torch.Generator().manual_seed(seed)

    def lp():       # (fp32 arithmetic: every value is exactly representable in the kernels' table)
        return float(-12.0 * torch.rand((), generator=g))

    def bo():
        return float(-3.0 * torch.rand((), generator=g))

    grams = {(v,): (lp(), bo() if order > 1 else 0.0) for v in range(V)}
    level = list(grams)
    for n in range(2, order + 1):
        nxt = []
        for h in level[::max(1, len(level) // max_contexts)]:
            k = int(torch.randint(0, max(2, int(density * min(V, 40))), (), generator=g))
            if max_children is not None:
                k = min(k, max_children)
            if k == 0:
                continue
            for w in sorted(set(torch.randint(0, V, (k,), generator=g).tolist())):
                grams[h + (w,)] = (lp(), bo() if n < order else 0.0)
                nxt.append(h + (w,))
        level = nxt
    if drop_suffix and order >= 3:
        for t in [t for t in grams if len(t) == 3]:
            s = t[1:]
            if s in grams and s != t[:2] and not any(len(u) > 2 and u[:2] == s for u in grams):
                del grams[s]
                break
    return grams


def lm_beam_search(P, cfg, enc, prompt, W, eos, max_len, ngrams, order, bos, lm_weight, bonus=0.0, ctc_weight=0.0,
                   blank=None, final_norm=True):
    """Reference LM-fused (joint) beam search over the oracle decoder, fp64.  enc [B, Te, d], prompt [B, 1].  Returns
    dict(tokens [B, W, 1 + max_len], lengths, scores, gap, finished), hypotheses ranked best first."""
    P = {k: v.double() for k, v in P.items()}
    enc = enc.double()
    B, Te, _ = enc.shape
    V = cfg.vocab_size
    lam, beta = float(ctc_weight), float(lm_weight)
    assert prompt.shape == (B, 1)
    lp = joint_ref.log_probs(torch.nn.functional.linear(enc, P["ctc_head.weight"][:V])) if lam > 0.0 else None
    tokens = torch.empty(B, W, 1 + max_len, dtype=torch.int64)
    lengths = torch.empty(B, W, dtype=torch.int64)
    scores = torch.empty(B, W, dtype=torch.float64)
    gap, finished = INF, 0
    for b in range(B):
        score = torch.full((1, W), -INF, dtype=torch.float64)
        score[0, 0] = 0.0
        fin = torch.zeros(1, W, dtype=torch.bool)
        length = torch.zeros(1, W, dtype=torch.int64)
        rows = torch.zeros(1, W, 0, dtype=torch.int64)
        st = joint_ref.root_state(lp[b:b + 1], [Te], W, blank) if lam > 0.0 else None
        for _ in range(max_len):
            full = torch.cat([prompt[b].long().view(1, 1).expand(W, 1), rows[0]], dim=1)
            logits = beam_ref.decoder_logits(P, cfg, full, enc[b:b + 1].expand(W, -1, -1), final_norm).unsqueeze(0)
            extra = torch.stack([row(ngrams, order, [bos] + rows[0, w].tolist(), V) for w in range(W)]) * beta + bonus
            if lam > 0.0:
                extra = extra + lam * joint_ref.prefix_score(lp[b:b + 1], [Te], st, W, blank, eos)
            r = joint_ref.joint_step(logits, extra.unsqueeze(0), 1.0 - lam, 1.0, score, fin, length, eos, V)
            gap = min(gap, r["gap"])
            if lam > 0.0:
                st = joint_ref.prefix_advance(lp[b:b + 1], [Te], st, W, r["parent"].flatten(), r["tok"].flatten(),
                                              fin.flatten(), blank, eos)
            rows = torch.cat([rows.gather(1, r["parent"][:, :, None].expand(-1, -1, rows.shape[2])),
                              r["tok"][:, :, None]], dim=2)
            score, fin, length = r["score"], r["fin"], r["len"]
        order_ = torch.sort(torch.where(torch.isfinite(score[0]), score[0], torch.full_like(score[0], -INF)),
                            descending=True, stable=True).indices
        tokens[b] = torch.cat([prompt[b].long().view(1, 1).expand(W, 1), rows[0]], dim=1)[order_]
        lengths[b], scores[b] = length[0][order_], score[0][order_]
        finished += int(fin.sum())
    return dict(tokens=tokens, lengths=lengths, scores=scores, gap=gap, finished=finished)
