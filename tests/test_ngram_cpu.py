"""N-gram LM shallow fusion, host side (no GPU): the reference recursion (tests/ngram_ref.py) against a case-by-case
enumeration, asrx.NgramLM's trie, host scorer, ARPA reader / writer and estimator against that reference, the
argument validation of the three entry points, and the Python argument errors."""
import math

import pytest
import torch

from tests import ngram_ref

INF = float("inf")
ERR_ARG, ERR_UNSUPPORTED = -1, -3
P0 = 0x10000   # never dereferenced: validation returns before any launch
LN10 = math.log(10.0)


def _table_v4():
    """V = 4, order 3, not suffix-closed: the trigram (0, 1, 2) stands without the bigram (1, 2)."""
    g = {(v,): (-1.0 - 0.25 * v, -0.5 - 0.125 * v) for v in range(4)}
    g[(3,)] = (-INF, -0.25)
    g.update({(0, 1): (-0.75, -0.375), (0, 3): (-2.0, None), (2, 2): (-1.5, -1.0), (3, 0): (-0.5, 0.0),
              (0, 1, 2): (-0.125, 0.0), (0, 1, 0): (-3.0, 0.0), (2, 2, 2): (-0.0625, 0.0), (3, 0, 1): (-1.25, 0.0)})
    return g


# ------------------------------------------------------------------------------------------------ reference

def test_reference_matches_brute_force_enumeration():
    g = _table_v4()
    want = ngram_ref.brute_force_order3(g, 4)
    assert len(want) == 4 + 16 + 64
    for (h, w), v in want.items():
        got = ngram_ref.logprob(g, 3, h, w)
        assert got == v or abs(got - v) <= 1e-15, (h, w, got, v)
        assert ngram_ref.partials(g, 3, h, w)[-1] == pytest.approx(got, abs=1e-15) or got == -INF
    # a longer history uses its last two tokens only; an order-1 view ignores it altogether
    assert ngram_ref.logprob(g, 3, (3, 2, 0, 1), 2) == want[((0, 1), 2)]
    assert ngram_ref.logprob({k: v for k, v in g.items() if len(k) == 1}, 1, (0, 1), 2) == want[((), 2)]
    total, n = ngram_ref.sequence_logprob(g, 3, [1, -1, 2, 9, 0], 0, 4, ignore=-1)
    assert n == 3 and total == pytest.approx(want[((0,), 1)] + want[((0, 1), 2)] + want[((1, 2), 0)], abs=1e-15)


# ------------------------------------------------------------------------------------------------ builder, scorer

def _check_layout(lm):
    fc, tok = lm.first_child.tolist(), lm.token.tolist()
    V = lm.vocab_size
    assert len(fc) == lm.n_nodes + 1 and len(tok) == lm.n_nodes and fc[0] == 1 and fc[1] == V + 1
    assert tok[1:V + 1] == list(range(V))                       # dense unigrams: token v is node 1 + v
    assert fc[-1] == lm.n_nodes and all(a <= b for a, b in zip(fc, fc[1:]))   # contiguous, in node order
    for i in range(lm.n_nodes):
        kids = tok[fc[i]:fc[i + 1]]
        assert kids == sorted(set(kids)), (i, kids)             # ascending, no repeats
        assert all(c > i for c in range(fc[i], fc[i + 1]))      # breadth-first: children after their parent


@pytest.mark.parametrize("V,order,seed", [(4, 3, 0), (7, 1, 1), (9, 2, 2), (11, 4, 3), (6, 6, 4)])
def test_builder_invariants_and_host_scorer(V, order, seed):
    import asrx
    g = _table_v4() if seed == 0 else ngram_ref.random_table(V, order, seed)
    lm = asrx.NgramLM(g, order, V)
    _check_layout(lm)
    assert lm.n_nodes == 1 + V + sum(1 for k in g if len(k) > 1)
    assert lm.logp.dtype == torch.float32 and lm.first_child.dtype == torch.int32
    gen = torch.Generator().manual_seed(seed)
    hists = [()] + [tuple(torch.randint(0, V, (n,), generator=gen).tolist()) for n in (1, 2, 3, 5, 7) for _ in range(12)]
    hists += [k[:-1] for k in g][:60]                           # contexts that do exist
    for h in hists:
        for w in range(V):
            got, want = lm.logprob(h, w), ngram_ref.logprob(g, order, h, w)
            assert got == want or abs(got - want) <= 1e-12, (h, w, got, want)
        ctx = lm.context(h)
        assert len(ctx) == order - 1
        for k, nd in enumerate(ctx, 1):
            present = k <= len(h) and (k == 1 or tuple(h[len(h) - k:]) in g)
            assert (nd >= 0) == present, (h, k, nd)


def test_constructor_rejects_bad_tables():
    import asrx
    ok = {(0,): (-1.0, -0.5), (1,): (-1.0, 0.0), (0, 1): (-0.5, 0.0)}
    asrx.NgramLM(ok, 2, 3)
    with pytest.raises(ValueError):
        asrx.NgramLM({(0,): (-1.0, 0.0), (1, 0): (-1.0, 0.0)}, 2, 3)           # prefix (1,) is no entry
    with pytest.raises(ValueError):
        asrx.NgramLM({**ok, (0, 1, 1): (-1.0, 0.0)}, 2, 3)                    # longer than the order
    with pytest.raises(ValueError):
        asrx.NgramLM({**ok, (0, 3): (-1.0, 0.0)}, 2, 3)                       # token outside the vocabulary
    with pytest.raises(ValueError):
        asrx.NgramLM(ok, 7, 3)
    with pytest.raises(ValueError):
        asrx.NgramLM(ok, 2, 3, bos_id=3)
    with pytest.raises(ValueError):
        asrx.NgramLM({(0,): (float("nan"), 0.0)}, 1, 3)


# ------------------------------------------------------------------------------------------------ ARPA

ARPA = """\
some toolkit's banner line

\\data\\
ngram 1=6
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.30103
-1.0\t</s>
-2.0\t<unk>
-0.5\t5\t-0.25
-0.75\t6\t-0.125
-1.5\tword

\\2-grams:
-0.25\t<s> 5\t-0.5
-0.125 5 6
-0.375\t6 </s>
-0.0625\t5 word

\\3-grams:
-0.03125\t<s> 5 6
-0.015625\t5 word 6

\\end\\
"""


def test_arpa_parsing():
    import asrx
    lm = asrx.NgramLM.from_arpa(ARPA, 10, bos_id=1, eos_id=2)
    assert lm.order == 3 and lm.vocab_size == 10 and lm.bos_id == 1 and lm.eos_id == 2
    assert lm.dropped == 3                                       # "word", "5 word", "5 word 6"
    assert lm.oov_logp == pytest.approx(-2.0 * LN10, abs=1e-15)  # <unk> sets the default of the ids not covered
    g = lm.ngrams
    assert set(g) == {(1,), (2,), (5,), (6,), (1, 5), (5, 6), (6, 2), (1, 5, 6)}
    assert g[(5,)] == (pytest.approx(-0.5 * LN10), pytest.approx(-0.25 * LN10))       # log10 -> ln
    assert g[(2,)] == (pytest.approx(-1.0 * LN10), 0.0)                                # a missing back-off is 0
    assert g[(1, 5)] == (pytest.approx(-0.25 * LN10), pytest.approx(-0.5 * LN10))      # <s> is bos_id
    assert g[(5, 6)][1] == 0.0 and g[(1, 5, 6)][0] == pytest.approx(-0.03125 * LN10)
    assert lm.logprob((1, 5), 6) == pytest.approx(-0.03125 * LN10)
    assert lm.logprob((1,), 6) == pytest.approx((-0.30103 - 0.75) * LN10)              # backed off through <s>
    assert lm.logprob((), 7) == pytest.approx(-2.0 * LN10)                             # an id the file lacks
    _check_layout(lm)
    # a word map: everything token_id cannot map is dropped, an explicit oov stays the default without <unk>
    words = {"5": 3, "6": 4, "word": 8}
    lm2 = asrx.NgramLM.from_arpa(ARPA, 10, token_id=words.__getitem__, bos_id=0, eos_id=9)
    assert lm2.dropped == 0 and (3, 8, 4) in lm2.ngrams and (0, 3) in lm2.ngrams and (4, 9) in lm2.ngrams


def test_arpa_rejects_inconsistent_files():
    import asrx
    with pytest.raises(ValueError):                              # the bigram "7 6" without a unigram "7"
        asrx.NgramLM.from_arpa(ARPA.replace("-0.125 5 6", "-0.125 7 6"), 10)
    with pytest.raises(ValueError):                              # a count that disagrees with the header
        asrx.NgramLM.from_arpa(ARPA.replace("ngram 2=4", "ngram 2=5"), 10)
    with pytest.raises(ValueError):
        asrx.NgramLM.from_arpa(ARPA.replace("-0.375\t6 </s>\n", ""), 10)
    with pytest.raises(ValueError):                              # cut off before \end\
        asrx.NgramLM.from_arpa(ARPA.replace("\\end\\", ""), 10)
    with pytest.raises(ValueError):
        asrx.NgramLM.from_arpa(ARPA.replace("\\3-grams:", "\\4-grams:"), 10)


@pytest.mark.parametrize("oov", [-INF, -7.5])
def test_write_arpa_round_trip(tmp_path, oov):
    import asrx
    g = ngram_ref.random_table(12, 3, 5)
    g[(7,)] = (-INF, g[(7,)][1])
    lm = asrx.NgramLM(g, 3, 12, bos_id=1, oov_logp=oov, eos_id=2)
    path = tmp_path / "lm.arpa"
    lm.write_arpa(path)
    back = asrx.NgramLM.from_arpa(str(path), 12, bos_id=1, eos_id=2)
    assert back.dropped == 0 and back.order == 3 and set(back.ngrams) == set(lm.ngrams)
    assert back.oov_logp == oov or abs(back.oov_logp - oov) <= 1e-12
    for k, (lp, bo) in lm.ngrams.items():
        blp, bbo = back.ngrams[k]
        assert (blp == lp or abs(blp - lp) <= 1e-12) and abs(bbo - bo) <= 1e-12, k
    assert torch.equal(back.first_child, lm.first_child) and torch.equal(back.token, lm.token)
    assert float((back.logp - lm.logp).nan_to_num(0, 0, 0).abs().max()) <= 1e-6
    assert torch.equal(torch.isinf(back.logp), torch.isinf(lm.logp))
    with open(path) as f:                                        # and a file object reads like the path
        assert set(asrx.NgramLM.from_arpa(f, 12, bos_id=1, eos_id=2).ngrams) == set(lm.ngrams)


# ------------------------------------------------------------------------------------------------ estimator

def _corpus(seed, n=40, lo=5, hi=60):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        L = int(torch.randint(2, 8, (1,), generator=g))
        out.append(torch.randint(lo, hi, (L,), generator=g).tolist())
    return out


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_estimator_is_exactly_normalised(order):
    """sum_v p(v | h) = 1 to 1e-12 for contexts that were seen, that were never seen, and that are partly seen, with
    the reference recursion on the estimator's dictionary AND with the trie's own scorer."""
    import asrx
    V, bos, eos, pad = 64, 1, 2, 4
    corpus = _corpus(0)
    lm = asrx.NgramLM.estimate(corpus, order, V, bos_id=bos, eos_id=eos, exclude=(pad,), discount=0.75)
    assert lm.order == order and lm.logp[1 + pad] == -INF and lm.eos_id == eos
    _check_layout(lm)
    gen = torch.Generator().manual_seed(order)
    hists = [(), (bos,)]
    for s in corpus[:10]:
        row = [bos] + s
        hists += [tuple(row[:i]) for i in range(1, len(row) + 1)]                       # seen contexts
    hists += [tuple(torch.randint(0, V, (n,), generator=gen).tolist()) for n in (1, 2, 3, 4) for _ in range(10)]
    hists += [tuple(s[:2]) + (63,) for s in corpus[:5]] + [(63,) + tuple(s[:2]) for s in corpus[:5]]
    worst = 0.0
    for h in hists:
        for f in (lambda v: ngram_ref.logprob(lm.ngrams, order, h, v), lambda v: lm.logprob(h, v)):
            total = math.fsum(math.exp(f(v)) for v in range(V))
            worst = max(worst, abs(total - 1.0))
            assert abs(total - 1.0) <= 1e-12, (h, total)
    print(f"order {order}: worst |sum - 1| = {worst:.2e} over {len(hists)} contexts")
    # the explicit entry is the interpolated probability: p(w | h) = (c(h, w) - D) / c(h) + backoff(h) * p(w | h[1:])
    if order == 2:
        w = corpus[0][0]
        c_hw = sum(1 for q in corpus if q[0] == w)
        types = len({q[0] for q in corpus})
        want = (c_hw - 0.75) / len(corpus) + 0.75 * types / len(corpus) * math.exp(lm.logprob((), w))
        assert math.exp(lm.logprob((bos,), w)) == pytest.approx(want, rel=1e-12)
        assert lm.ngrams[(bos,)][1] == pytest.approx(math.log(0.75 * types / len(corpus)), rel=1e-12)


def test_estimator_argument_errors():
    import asrx
    with pytest.raises(ValueError):
        asrx.NgramLM.estimate([[5, 4]], 2, 10, exclude=(4,))          # an excluded id in the corpus
    with pytest.raises(ValueError):
        asrx.NgramLM.estimate([[5, 11]], 2, 10)
    with pytest.raises(ValueError):
        asrx.NgramLM.estimate([[5]], 2, 10, discount=1.0)
    with pytest.raises(ValueError):
        asrx.NgramLM.estimate([], 2, 10)


# ------------------------------------------------------------------------------------------------ C-ABI

TABLE = dict(first_child=P0, token=P0 + 0x1000, logp=P0 + 0x2000, backoff=P0 + 0x3000, n_nodes=40, order=3, V=10)


def _score_args(**kw):
    a = dict(TABLE, ctx=P0 + 0x4000, R=6, base=P0 + 0x10000, ld_base=16, base_weight=0.3, lm_weight=0.5, bonus=0.25,
             out=P0 + 0x20000, ld_out=16, stream=None)
    a.update(kw)
    return list(a.values())


def _advance_args(**kw):
    a = dict(TABLE, B=2, W=4, eos=2, parent=P0 + 0x4000, tok=P0 + 0x5000, fin_prev=P0 + 0x6000, ctx_in=P0 + 0x10000,
             ctx_out=P0 + 0x20000, stream=None)
    a.update(kw)
    return list(a.values())


def _seq_args(**kw):
    a = dict(TABLE, tgt=P0 + 0x4000, ld_tgt=7, N=8, L=7, ignore=-1, bos=1, n_hyp=P0 + 0x5000, W=4, add=P0 + 0x6000,
             add_scale=0.5, lm_weight=0.5, bonus=0.0, lm_out=P0 + 0x7000, out=P0 + 0x8000, stream=None)
    a.update(kw)
    return list(a.values())


BAD_TABLE = [dict(first_child=None), dict(token=None), dict(logp=None), dict(backoff=None), dict(order=0),
             dict(order=7), dict(V=0), dict(V=-2), dict(n_nodes=10), dict(n_nodes=0)]
NAN = float("nan")


def test_abi_version_and_symbols():
    import asrx
    from asrx._lib import SIGNATURES
    from asrx.kernels import NGRAM_LDS_V
    lib = asrx.native()
    assert lib.asrx_version() >= 10
    for name, args in (("asrx_ngram_score", _score_args()), ("asrx_ngram_advance", _advance_args()),
                       ("asrx_ngram_seq_logprob", _seq_args())):
        assert getattr(lib, name) is not None and len(SIGNATURES[name]) == len(args)
    assert lib.asrx_ngram_score(*_score_args(R=0)) == 0
    assert lib.asrx_ngram_advance(*_advance_args(B=0)) == 0
    assert lib.asrx_ngram_seq_logprob(*_seq_args(N=0)) == 0
    assert lib.asrx_ngram_advance(*_advance_args(order=1, n_nodes=11)) == 0      # a unigram model has no state
    assert NGRAM_LDS_V == 8192 and asrx.NgramLM is not None
    # sizes the kernels do not take are refused as unsupported, also before any device access
    assert lib.asrx_ngram_score(*_score_args(V=(1 << 20) + 1, n_nodes=(1 << 21), ld_out=1 << 21,
                                             ld_base=1 << 21)) == ERR_UNSUPPORTED
    assert lib.asrx_ngram_seq_logprob(*_seq_args(L=4097, ld_tgt=4097)) == ERR_UNSUPPORTED


@pytest.mark.parametrize("bad", BAD_TABLE + [dict(ctx=None), dict(out=None), dict(R=-1), dict(ld_out=9),
                                             dict(ld_base=9), dict(base_weight=NAN), dict(lm_weight=NAN),
                                             dict(bonus=NAN), dict(lm_weight=INF), dict(base_weight=-INF),
                                             dict(bonus=INF), dict(out=P0 + 0x10000), dict(out=P0 + 0x10000 + 8),
                                             dict(base=P0 + 0x20000 + 64 * 5)])
def test_ngram_score_rejects_bad_arguments_without_gpu(bad):
    """Besides the ranges: out must not overlap base, a non-finite weight is refused."""
    import asrx
    assert asrx.native().asrx_ngram_score(*_score_args(**bad)) == ERR_ARG


def test_ngram_score_takes_no_base_and_any_padding():
    """base may be null (ld_base is then not looked at); R = 0 is checked like any other call."""
    import asrx
    lib = asrx.native()
    assert lib.asrx_ngram_score(*_score_args(R=0, base=None, ld_base=0)) == 0
    assert lib.asrx_ngram_score(*_score_args(R=0, ld_out=9)) == ERR_ARG


@pytest.mark.parametrize("bad", BAD_TABLE + [dict(B=-1), dict(W=0), dict(eos=-1), dict(eos=10), dict(parent=None),
                                             dict(tok=None), dict(fin_prev=None), dict(ctx_in=None),
                                             dict(ctx_out=None), dict(ctx_out=P0 + 0x10000),
                                             dict(ctx_out=P0 + 0x10000 + 4 * 15), dict(ctx_in=P0 + 0x20000 + 4)])
def test_ngram_advance_rejects_bad_arguments_without_gpu(bad):
    """Besides the ranges: the output set must not overlap the input set (the caller ping-pongs)."""
    import asrx
    assert asrx.native().asrx_ngram_advance(*_advance_args(**bad)) == ERR_ARG


@pytest.mark.parametrize("bad", BAD_TABLE + [dict(tgt=None), dict(lm_out=None), dict(out=None), dict(N=-1), dict(L=0),
                                             dict(ld_tgt=6), dict(bos=-2), dict(bos=10), dict(W=0), dict(W=3),
                                             dict(add_scale=NAN), dict(lm_weight=NAN), dict(bonus=NAN),
                                             dict(lm_weight=INF)])
def test_ngram_seq_logprob_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_ngram_seq_logprob(*_seq_args(**bad)) == ERR_ARG


# ------------------------------------------------------------------------------------------------ Python arguments

def _model(ctc=True, V=30):
    import asrx
    return asrx.Transformer(V, 8, 16, 8, 16, 1, 1, 2, 32, dropout=0.0, precision="fp32", ctc=ctc)


def _lm(V=30):
    import asrx
    return asrx.NgramLM.estimate([[5, 6, 7], [6, 7, 8]], 3, V, exclude=(4,))


def test_decoder_argument_errors():
    """Raised before anything touches a device (the LM itself is still on the host here): a negative, NaN or infinite
    lm_weight, a non-finite token_bonus, an LM over another vocabulary, a prompt of more than one token."""
    spectrum = torch.zeros(2, 1, 8, 20)
    m, lm = _model(), _lm()
    for kw in (dict(lm_weight=-0.1), dict(lm_weight=NAN), dict(lm_weight=INF), dict(lm_weight=0.5, token_bonus=NAN),
               dict(lm_weight=0.5, token_bonus=INF)):
        with pytest.raises(ValueError):
            m.beam_search(spectrum, lm=lm, **kw)
        with pytest.raises(ValueError):
            m.rescore(spectrum, lm=lm, **kw)
    with pytest.raises(ValueError):
        m.beam_search(spectrum, lm=_lm(31), lm_weight=0.5)
    with pytest.raises(ValueError):
        m.rescore(spectrum, lm=_lm(31), lm_weight=0.5)
    with pytest.raises(ValueError):
        m.beam_search(spectrum, torch.ones(2, 3, dtype=torch.int64), lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError):
        _model(False).beam_search(spectrum, lm=lm, lm_weight=-1.0)      # (checked even where no LM takes part)
    dec = m.decoder
    enc = torch.zeros(2, 4, 16)
    one = torch.ones(2, 1, dtype=torch.int64)
    with pytest.raises(ValueError):
        dec.beam_search(one, enc, lm=lm, lm_weight=-2.0)
    with pytest.raises(ValueError):
        dec.beam_search(one, enc, lm=_lm(29), lm_weight=0.5)
    with pytest.raises(ValueError):
        dec.beam_search(torch.ones(2, 2, dtype=torch.int64), enc, lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError):
        dec.rescore(enc, (enc, 4, 0, None), lm=lm, lm_weight=NAN)
    with pytest.raises(ValueError):
        dec.rescore(enc, (enc, 4, 0, None), lm=_lm(29), lm_weight=0.5)


def test_rescore_result_keeps_its_positional_fields():
    import asrx
    z = torch.zeros(1, 1)
    r = asrx.RescoreResult(z, z, z, z + 1, z + 2, z + 3)
    assert r.lm_scores is None and float(r.risks) == 3.0 and len(r) == 3
    assert float(asrx.RescoreResult(z, z, z, lm_scores=z + 4).lm_scores) == 4.0
