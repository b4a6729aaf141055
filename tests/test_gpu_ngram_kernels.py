"""asrx_ngram_score, asrx_ngram_advance and asrx_ngram_seq_logprob on the GPU against tests/ngram_ref.py, the fp64
recursion over the n-gram dictionary (it shares nothing with the trie).

Tolerance of a score (derived, not measured).  The table's values are fp32 numbers (logp in [-12, 0], backoff in
[-3, 0]) and the weights are dyadic, so the inputs are exact and only the kernel's own roundings count: at most
order - 1 additions of back-off weights, one fused multiply-add for lm_weight * lm + bonus, one for the base term.
Each rounds by at most 2^-24 of its result, so the error of an element is below (order + 1) * 2^-24 * max |partial
sum|; the tests hold every element to (order + 3) * 2^-24 * max |partial sum| of that element, and require the -inf
positions to be identical.

Tolerance of a sequence score.  lm_out is a sequential fp32 sum of the per-position terms: each term carries the
error above (its own order - 1 additions), each addition of the running sum rounds by 2^-24 of the partial sum, so
|error| <= 2^-24 * (order * sum_i max|partials of term i| + sum_i |S_i|) with S_i the running sums (`order` instead of
order - 1 covers the second-order terms); `out` adds two fused multiply-adds on top.  Along a path of L = 7 tokens
with order >= 3 the terms are bit-identical to the score kernel's columns (one device function), the sum has L - 1 = 6
<= order + 3 roundings, and the check uses the score bound itself: (order + 3) * 2^-24 * max |partial sum|."""
import functools
import math

import pytest
import torch

from tests import ngram_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
U = 2.0 ** -24
R = 6
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lds_limit():
    from asrx.kernels import NGRAM_LDS_V
    return NGRAM_LDS_V


def feature_table(V, order, seed):
    """ngram_ref.random_table plus the shapes the kernels must get right.  With A = 1, Z = 0, O = V - 1 (4 for V = 5):
      (A, w) for w = 0, V - 1 and, for V > 300, 298 more tokens: more children than a workgroup has threads, the first
          and the last column among them;
      Z has no children at all; O has exactly one, (O, 0);
      (2, 3, 4) exists (order >= 3) and (3, 4) does not: a context present at order 3 whose suffix is absent at
          order 2; (2, 3, 4, 0) (order >= 4) can then only be found through the order-3 context;
      the unigrams of V - 1 and of 2 are -inf.
    Returns (dictionary, histories of the R slots)."""
    g = ngram_ref.random_table(V, order, seed, drop_suffix=False)
    A, Z, O = 1, 0, (V - 1 if V > 5 else 4)
    val = iter((-12.0 * torch.rand(400, generator=torch.Generator().manual_seed(seed + 1))).tolist())   # fp32 values
    for k in [k for k in g if len(k) > 1 and (k[0] in (Z, O) or k[:2] == (3, 4))]:
        del g[k]
    if order >= 2:
        many = {0, V - 1}
        if V > 300:
            many |= set(torch.randperm(V, generator=torch.Generator().manual_seed(seed))[:298].tolist())
        for w in sorted(many):
            g.setdefault((A, w), (next(val), 0.0 if order == 2 else -0.5))
        g[(O, 0)] = (-1.25, 0.0 if order == 2 else -0.75)
        g.setdefault((2, 3), (-2.5, 0.0 if order == 2 else -1.5))
    if order >= 3:
        g.setdefault((2, 3, 4), (-0.625, 0.0 if order == 3 else -2.25))
        assert (3, 4) not in g
    if order >= 4:
        g.setdefault((2, 3, 4, 0), (-0.375, 0.0))
    g[(V - 1,)] = (-INF, g[(V - 1,)][1])
    g[(2 % V,)] = (-INF, g[(2 % V,)][1])
    deep = max((k for k in g if len(k) <= max(order - 1, 1)), key=lambda k: (len(k), k))
    hists = [(), (A,), (Z,), (O,), deep, (2, 3, 4)]
    return g, hists


@functools.lru_cache(maxsize=None)
def score_case(V, order):
    """(lm on the device, ctx int32 [R, max(order - 1, 1)], lm fp64 [R, V], max |partial| of the chain fp64 [R, V])."""
    import asrx
    g, hists = feature_table(V, order, 7 * V + order)
    lm = asrx.NgramLM(g, order, V, bos_id=None)
    if V > 300 and order >= 2:
        fc = lm.first_child.tolist()
        assert fc[1 + 1 + 1] - fc[1 + 1] > 256                    # the children of (A,)
        assert fc[1 + 0 + 1] == fc[1 + 0]                         # Z: none
    ctx = torch.full((R, max(order - 1, 1)), -1, dtype=torch.int32)
    want = torch.empty(R, V, dtype=torch.float64)
    big = torch.empty(R, V, dtype=torch.float64)
    for r, h in enumerate(hists):
        c = lm.context(h)
        if order > 1:
            ctx[r, :order - 1] = torch.tensor(c, dtype=torch.int32)
        for v in range(V):
            parts = ngram_ref.partials(g, order, h, v)
            want[r, v] = parts[-1]
            big[r, v] = max((abs(p) for p in parts if p != -INF), default=0.0)
    if order >= 4:
        assert ctx[5, 1] == -1 and ctx[5, 2] >= 0                 # the order-3 context without its order-2 suffix
    if order >= 2:
        assert bool((ctx[0] == -1).all())
    return lm.to(dev), ctx, want, big


def _state(lm, ctx):
    from asrx.kernels import NgramState
    st = NgramState(lm, R, 1)
    st.cur.copy_(ctx.to(dev))
    return st


def _check(got, want, bound, what):
    got = got.double().cpu()
    assert not bool(torch.isnan(got).any()), what
    assert torch.equal(got == -INF, want == -INF), f"{what}: the -inf positions differ"
    assert not bool((got == INF).any())
    fin = want != -INF
    err = (got[fin] - want[fin]).abs()
    room = err / bound[fin].clamp(min=1e-300)
    print(f"{what}: worst error {float(err.max()) if err.numel() else 0.0:.3e}, "
          f"worst error / bound {float(room.max()) if room.numel() else 0.0:.3f}")
    assert bool((err <= bound[fin]).all()), what


V_CASES = [5, 97, 5400, "lds", "lds+1"]


@pytest.mark.parametrize("order", [1, 2, 3, 6])
@pytest.mark.parametrize("Vc", V_CASES)
def test_ngram_score_matches_reference(Vc, order):
    V = {"lds": _lds_limit(), "lds+1": _lds_limit() + 1}.get(Vc, Vc)
    lm, ctx, want, big = score_case(V, order)
    st = _state(lm, ctx)
    ld = V + 3
    lw, bw, bonus = 0.5, 0.375, 0.25
    # without base
    out = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=dev)
    st.score(out, None, 0.0, lw, bonus)
    ref = lw * want + bonus
    bound = (order + 3) * U * torch.maximum(big, ref.abs().nan_to_num(0, 0, 0))
    _check(out[:, :V], ref, bound, f"V {V} order {order} lm only")
    assert bool((out[:, V:] == SENTINEL).all())
    again = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=dev)
    st.score(again, None, 0.0, lw, bonus)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # lm_weight = 1, bonus = 0: the table's own sums
    plain = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=dev)
    st.score(plain)
    _check(plain[:, :V], want, (order + 3) * U * big, f"V {V} order {order} plain")
    # with base, -inf columns in it
    gen = torch.Generator().manual_seed(V + order)
    base = (8.0 * torch.rand(R, V + 5, generator=gen) - 10.0)
    base[:, 1 % V] = -INF
    base[2, :] = -INF
    base[3, V - 1] = -INF
    based = base[:, :V].double()
    out2 = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=dev)
    st.score(out2, base.to(dev), bw, lw, bonus)
    ref2 = bw * based + ref
    bound2 = (order + 3) * U * torch.maximum(torch.maximum(big, ref.abs().nan_to_num(0, 0, 0)),
                                             ref2.abs().nan_to_num(0, 0, 0))
    _check(out2[:, :V], ref2, bound2, f"V {V} order {order} with base")
    assert bool((out2[:, V:] == SENTINEL).all())
    # a zero weight drops the base term: no 0 * -inf
    out3 = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=dev)
    st.score(out3, base.to(dev), 0.0, lw, bonus)
    assert torch.equal(out3.view(torch.int32), out.view(torch.int32))


def test_ngram_score_reads_bad_context_entries_as_absent():
    """A ctx entry outside [0, n_nodes) reads as -1 (so does any negative one)."""
    V, order = 97, 3
    lm, ctx, want, big = score_case(V, order)
    bad = ctx.clone()
    bad[0] = torch.tensor([lm.n_nodes, -7], dtype=torch.int32)
    bad[2, 1] = 2 ** 31 - 1
    ref = torch.full((R, V), SENTINEL, dtype=torch.float32, device=dev)
    _state(lm, ctx).score(ref)
    got = torch.full((R, V), SENTINEL, dtype=torch.float32, device=dev)
    _state(lm, bad).score(got)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_ngram_kernels_survive_a_malformed_table():
    """The host never inspects the table, so the kernels clamp: child ranges that point outside the table or run
    backwards, token values outside [0, V).  Every output stays inside its row, the sentinels stand, the unigram
    level (which needs nothing but logp) is intact wherever no malformed child list overwrote it."""
    import asrx
    from asrx.kernels import NgramState, ngram_seq_logprob
    V, order = 23, 3
    g = ngram_ref.random_table(V, order, 3)
    lm = asrx.NgramLM(g, order, V, bos_id=1)
    fc, tok = lm.first_child.clone(), lm.token.clone()
    fc[1 + 5] = -40                        # the children of token 5: [-40, ...)
    fc[1 + 6 + 1] = lm.n_nodes + 1000      # the children of token 6: [..., far past the end)
    fc[1 + 8], fc[1 + 9] = fc[1 + 9].item(), fc[1 + 8].item()    # a range that runs backwards
    tok[V + 1:V + 1 + 12] = torch.tensor([V, V + 100, -1, -2 ** 31, 2 ** 31 - 1, V] * 2, dtype=torch.int32)
    lm.first_child, lm.token = fc, tok
    lm.to(dev)
    st = NgramState(lm, R, 1)
    st.cur.copy_(torch.tensor([[1 + 5, -1], [1 + 6, -1], [1 + 8, V + 3], [1 + 9, lm.n_nodes - 1], [1 + 0, V + 1],
                               [1 + 7, V + 2]], dtype=torch.int32).to(dev))
    out = torch.full((R + 2, V + 4), SENTINEL, dtype=torch.float32, device=dev)
    st.score(out[1:R + 1])
    assert bool((out[0] == SENTINEL).all()) and bool((out[R + 1] == SENTINEL).all())
    assert bool((out[:, V:] == SENTINEL).all())
    assert not bool(torch.isnan(out).any()) and bool((out[1:R + 1, :V] <= 0).all())
    parent = torch.zeros(R, dtype=torch.int32, device=dev)
    toks = torch.tensor([3, 4, 5, 6, V + 1, -1], dtype=torch.int64, device=dev)
    st.advance(2, parent, toks, torch.zeros(R, dtype=torch.uint8, device=dev))
    new = st.cur.cpu()
    assert bool(((new >= -1) & (new < lm.n_nodes)).all())
    tgt = torch.randint(0, V, (R, 9), generator=torch.Generator().manual_seed(0)).to(dev)
    lm_s, comb = ngram_seq_logprob(lm, tgt, -1)
    assert not bool(torch.isnan(lm_s).any()) and bool((lm_s <= 0).all())


# ------------------------------------------------------------------------------------------------ advance

@pytest.mark.parametrize("order", [1, 2, 4, 6])
def test_ngram_advance_follows_the_histories(order):
    """Six chained steps over B = 2 x W = 3 slots: permuted parents, finished parents and EOS (the parent's state is
    copied), tokens without a child and tokens outside the vocabulary (-1 from that order on).  After every step the
    state equals the host lookups of each slot's history, and a node is present exactly where the dictionary has the
    k-gram."""
    import asrx
    from asrx.kernels import NgramState
    B, W, V, eos, bos = 2, 3, 13, 2, 1
    g = ngram_ref.random_table(V, order, 11 + order, density=0.5)
    lm = asrx.NgramLM(g, order, V, bos_id=bos)
    host = [[bos] for _ in range(B * W)]
    fin = torch.zeros(B * W, dtype=torch.uint8)
    lm.to(dev)
    st = NgramState(lm, B, W)
    gen = torch.Generator().manual_seed(order)
    exist = [k for k in g if len(k) >= 2]
    hits = misses = copies = 0
    for step in range(6):
        parent = torch.randint(0, W, (B * W,), generator=gen).to(torch.int32)
        tok = torch.randint(0, V, (B * W,), generator=gen)
        for j in range(B * W):                      # steer half of the slots along n-grams that exist
            h = host[(j // W) * W + int(parent[j])]
            nxt = [k[-1] for k in exist if len(h) >= len(k) - 1 and tuple(h[len(h) - len(k) + 1:]) == k[:-1]]
            if nxt and j % 2 == 0:
                tok[j] = nxt[int(torch.randint(0, len(nxt), (1,), generator=gen))]
        if step == 2:
            tok[1], tok[4] = eos, V + 4
        if step == 3:
            tok[0] = -5
        before = st.cur.clone()
        st.advance(eos, parent.to(dev), tok.to(dev), fin.to(dev))
        again = NgramState(lm, B, W)
        again.cur.copy_(before)
        again.advance(eos, parent.to(dev), tok.to(dev), fin.to(dev))
        assert torch.equal(st.cur[:, :order - 1], again.cur[:, :order - 1])     # (order 1: there is no state)
        new_host, new_fin = [], fin.clone()
        for j in range(B * W):
            ps = (j // W) * W + int(parent[j])
            if fin[ps] or int(tok[j]) == eos:
                new_host.append(list(host[ps]))
                copies += 1
            else:
                new_host.append(host[ps] + [int(tok[j])])
            new_fin[j] = fin[ps] | (int(tok[j]) == eos)
        host, fin = new_host, new_fin
        got = st.cur.cpu()
        for j in range(B * W):
            if order == 1:
                continue
            want = lm.context(host[j])
            assert got[j, :order - 1].tolist() == want, (step, j, host[j], got[j].tolist(), want)
            for k in range(1, order):
                tail = tuple(host[j][len(host[j]) - k:]) if k <= len(host[j]) else None
                present = tail is not None and all(0 <= t < V for t in tail) and (k == 1 or tail in g)
                assert (want[k - 1] >= 0) == present
                hits += present and k > 1
                misses += (not present) and k > 1
    if order >= 4:
        assert hits >= 5 and misses >= 5 and copies >= 1, (hits, misses, copies)


# ------------------------------------------------------------------------------------------------ sequences

@pytest.mark.parametrize("order", [1, 3, 6])
@pytest.mark.parametrize("L", [1, 7, 255])
def test_ngram_seq_logprob_matches_reference(L, order):
    import asrx
    from asrx.kernels import ngram_seq_logprob
    B, W, V, bos, ignore = 2, 3, 37, 1, -1
    N = B * W
    g = ngram_ref.random_table(V, order, 5 + order, density=0.5)
    lm = asrx.NgramLM(g, order, V, bos_id=bos).to(dev)
    gen = torch.Generator().manual_seed(L + order)
    tgt = torch.randint(0, V, (N, L + 2), generator=gen)
    tgt[torch.rand(N, L + 2, generator=gen) < 0.15] = ignore
    tgt[torch.rand(N, L + 2, generator=gen) < 0.05] = V + 5
    for n in range(N):                              # steer the rows along n-grams that exist, as text would
        for i in range(1, L):
            if int(tgt[n, i - 1]) in range(V) and i % 3:
                nxt = [k[-1] for k in g if len(k) == 2 and k[0] == int(tgt[n, i - 1])]
                if nxt:
                    tgt[n, i] = nxt[i % len(nxt)]
    tgt[0, :] = torch.where(tgt[0] == ignore, tgt[0], tgt[0].clamp(0, V - 1))
    n_hyp = torch.tensor([3, 2], dtype=torch.int32)
    add = (-20.0 * torch.rand(N, generator=gen)).float()
    scale, lw, bonus = 0.5, 0.375, 0.25
    view = tgt.to(dev)[:, :L]                       # row stride L + 2
    lm_s, out = ngram_seq_logprob(lm, view, ignore, n_hyp.to(dev), W, add.to(dev), scale, lw, bonus)
    lm_2, out_2 = ngram_seq_logprob(lm, view, ignore, n_hyp.to(dev), W, add.to(dev), scale, lw, bonus)
    assert torch.equal(lm_s.view(torch.int32), lm_2.view(torch.int32))
    assert torch.equal(out.view(torch.int32), out_2.view(torch.int32))
    lm_s, out = lm_s.double().cpu(), out.double().cpu()
    worst = 0.0
    for n in range(N):
        if n % W >= int(n_hyp[n // W]):
            assert float(lm_s[n]) == -INF and float(out[n]) == -INF
            continue
        hist, total, cnt, e_terms, e_sum = [bos], 0.0, 0, 0.0, 0.0
        for t in tgt[n, :L].tolist():
            if t == ignore or not 0 <= t < V:
                continue
            parts = ngram_ref.partials(g, order, hist, t)
            assert parts[-1] != -INF
            e_terms += max(abs(p) for p in parts)
            total += parts[-1]
            e_sum += abs(total)
            hist.append(t)
            cnt += 1
        assert total == pytest.approx(ngram_ref.sequence_logprob(g, order, tgt[n, :L].tolist(), bos, V, ignore)[0])
        bound = U * (order * e_terms + e_sum)
        err = abs(float(lm_s[n]) - total)
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (n, float(lm_s[n]), total, bound)
        want = scale * float(add[n]) + lw * total + bonus * cnt
        b_out = lw * bound + 3 * U * max(abs(want), abs(lw * total + bonus * cnt))
        assert abs(float(out[n]) - want) <= b_out, (n, float(out[n]), want, b_out)
    print(f"L {L} order {order}: worst error / bound {worst:.3f}")
    # without add, n_hyp and weights: out is lm_out; a zero scale drops an add term of -inf
    lm_3, out_3 = ngram_seq_logprob(lm, view, ignore)
    assert torch.equal(lm_3.view(torch.int32), out_3.view(torch.int32))
    live = torch.tensor([n % W < int(n_hyp[n // W]) for n in range(N)])
    assert torch.equal(lm_3.cpu()[live].double(), lm_s[live])
    lm_4, out_4 = ngram_seq_logprob(lm, view, ignore, add=torch.full((N,), -INF, device=dev), add_scale=0.0)
    assert torch.equal(out_4.view(torch.int32), lm_3.view(torch.int32))


@pytest.mark.parametrize("order", [3, 6])
def test_score_columns_along_a_path_sum_to_the_sequence_score(order):
    """Seven tokens from the sentence start: score, pick the path's column, advance.  The terms are the sequence
    kernel's own (one device function computes both), so only its L - 1 = 6 <= order + 3 additions separate the two:
    (order + 3) * 2^-24 * max |partial sum|."""
    import asrx
    from asrx.kernels import NgramState, ngram_seq_logprob
    V, bos, eos, L = 37, 1, 2, 7
    g = ngram_ref.random_table(V, order, 5 + order, density=0.5)
    lm = asrx.NgramLM(g, order, V, bos_id=bos).to(dev)
    paths = []
    for n in range(R):                              # half of each path follows n-grams that exist
        h, row = [bos], []
        for i in range(L):
            nxt = [k[-1] for k in g if len(k) >= 2 and len(h) >= len(k) - 1 and tuple(h[len(h) - len(k) + 1:]) == k[:-1]
                   and k[-1] != eos]
            t = nxt[(n + i) % len(nxt)] if nxt and (n + i) % 2 else 3 + (5 * n + 7 * i) % (V - 3)
            row.append(t)
            h.append(t)
        paths.append(row)
    tgt = torch.tensor(paths, dtype=torch.int64, device=dev)
    st = NgramState(lm, R, 1)
    cols = torch.empty(R, L, dtype=torch.float32, device=dev)
    out = torch.empty(R, V, dtype=torch.float32, device=dev)
    zero = torch.zeros(R, dtype=torch.uint8, device=dev)
    parent = torch.zeros(R, dtype=torch.int32, device=dev)
    for i in range(L):
        st.score(out)
        cols[:, i] = out.gather(1, tgt[:, i:i + 1])[:, 0]
        st.advance(eos, parent, tgt[:, i].contiguous(), zero)
    lm_s, _ = ngram_seq_logprob(lm, tgt, -1)
    cols, lm_s = cols.double().cpu(), lm_s.double().cpu()
    for n in range(R):
        run = torch.cumsum(cols[n], 0)
        bound = (order + 3) * U * float(run.abs().max())
        assert math.isfinite(float(lm_s[n]))
        assert abs(float(lm_s[n]) - float(run[-1])) <= bound, (n, float(lm_s[n]), float(run[-1]), bound)
        want = ngram_ref.sequence_logprob(g, order, paths[n], bos, V)[0]
        assert abs(float(run[-1]) - want) <= L * (order + 3) * U * float(run.abs().max())
