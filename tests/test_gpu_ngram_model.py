"""N-gram LM shallow fusion end to end: Transformer.beam_search(..., lm=, lm_weight=, token_bonus=) and
Transformer.rescore(..., lm=...) on the GPU against fp64 references on the CPU: tests/ngram_ref.lm_beam_search (the
oracle decoder with full-prefix recomputation, joint_ref's CTC prefix scorer, the dictionary recursion for the LM) and,
for rescoring, tests/ctc_beam_ref.py's first pass with each hypothesis scored on its own.

Model and data: the c1 setup of test_gpu_joint_model.py (copied, not imported): fp32, det_params(cfg, 3) with the
classifier times 4, that CTC head, EOS 22, 8 new tokens, 3 samples.  The LM is NgramLM.estimate (order 3, D = 0.75,
BOS 1, the pad id excluded) on 40 sequences drawn from torch.Generator().manual_seed(0): each L = randint(2, 8), then L
tokens randint(5, 60).

Reference margins on the CPU (the smallest gap between the W-th and the (W + 1)-th candidate of any selection):
    ctc_weight 0    lm_weight 0.5  beam 1:  7.5e-1
    ctc_weight 0    lm_weight 0.5  beam 4:  6.8e-3
    ctc_weight 0.3  lm_weight 0.5  beam 4:  5.0e-3
    ctc_weight 0.3  lm_weight 0.3  beam 4:  2.3e-2
and the LM changes the best hypothesis of all 3 samples in each.  Seed 1 for the corpus leaves a margin below 1e-3:
keep seed 0 or check again on the CPU."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ref_model import CONFIGS, _ln, decoder_layer, det_params, encoder as oracle_encoder, front_end, pe_table
from tests import beam_ref, ctc_beam_ref, joint_ref, ngram_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
EOS, BOS, MAX_LEN, NSAMPLES, ORDER = 22, 1, 8, 3, 3
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def setup():
    """(cfg, P with ctc_head.weight, spectrum [3, 1, 80, 100], oracle encoder output fp64 [3, 24, 128])."""
    cfg = CONFIGS["c1"]["cfg"]
    P = det_params(cfg, 3)
    P["decoder._classifier.weight"] = P["decoder._classifier.weight"] * 4
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_c1.npz")
    s = torch.from_numpy(np.load(golden)["spectrum"])[:NSAMPLES]
    Pd = {k: v.double() for k, v in P.items()}
    enc = oracle_encoder(Pd, front_end(Pd, s.double()), cfg, False)
    head = 0.15 * torch.randn(cfg.vocab_size, cfg.d_model, generator=torch.Generator().manual_seed(5))
    mean = enc.mean(dim=(0, 1)).float()
    head[cfg.pad_id] = 9.0 * mean / float(mean @ mean)
    P["ctc_head.weight"] = head
    return cfg, P, s, enc


@functools.lru_cache(maxsize=None)
def model():
    import asrx
    cfg, P, s, enc = setup()
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, precision="fp32", ctc=True)
    sd = m.state_dict()
    sd.update(P)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.decoder._eos_token_id = EOS
    assert m.ctc_blank == cfg.pad_id
    return m


def corpus(seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(40):
        L = int(torch.randint(2, 8, (1,), generator=g))
        out.append(torch.randint(5, 60, (L,), generator=g).tolist())
    return out


@functools.lru_cache(maxsize=None)
def language_model(device=None):
    import asrx
    cfg = setup()[0]
    lm = asrx.NgramLM.estimate(corpus(), ORDER, cfg.vocab_size, bos_id=BOS, eos_id=EOS, exclude=(cfg.pad_id,),
                               discount=0.75)
    return lm if device is None else lm.to(device)


@functools.lru_cache(maxsize=None)
def reference(lam, beta, W):
    cfg, P, s, enc = setup()
    prompt = torch.ones(NSAMPLES, 1, dtype=torch.int64)
    return ngram_ref.lm_beam_search(P, cfg, enc, prompt, W, EOS, MAX_LEN, language_model().ngrams, ORDER, BOS, beta,
                                    0.0, lam, cfg.pad_id)


@functools.lru_cache(maxsize=None)
def reference_without_lm(lam, W):
    cfg, P, s, enc = setup()
    prompt = torch.ones(NSAMPLES, 1, dtype=torch.int64)
    if lam == 0.0:
        return beam_ref.beam_search(P, cfg, enc, prompt, W, EOS, MAX_LEN)
    return joint_ref.joint_beam_search(P, cfg, enc, prompt, W, EOS, MAX_LEN, lam, cfg.pad_id)


def parts_of(row, n, b, lam):
    """(log p_att, log p_ctc, log p_lm) of the finished hypothesis row[1 : 1 + n] of sample b, each computed on its own
    in fp64: the oracle decoder position by position, the CTC prefix scorer along the labels, the LM recursion."""
    cfg, P, s, enc = setup()
    labels = row[1:n].tolist()
    att = beam_ref.sequence_score(P, cfg, enc[b], row, 1, EOS)
    ctc = 0.0
    if lam > 0.0:
        lp = joint_ref.log_probs(F.linear(enc[b:b + 1], P["ctc_head.weight"].double()[:cfg.vocab_size]))[0]
        ctc = joint_ref.sequence_ctc_score(lp, enc.shape[1], labels, cfg.pad_id, EOS)
    lm, cnt = ngram_ref.sequence_logprob(language_model().ngrams, ORDER, labels + [EOS], BOS, cfg.vocab_size)
    assert cnt == n
    return att, ctc, lm


def check_identity(r, lam, beta, bonus):
    """Every finished hypothesis: score = (1 - lam) * att + lam * ctc + beta * lm + bonus * len, within 1e-4."""
    checked = 0
    for b in range(r.tokens.shape[0]):
        for w in range(r.tokens.shape[1]):
            row, n = r.tokens[b, w].cpu(), int(r.lengths[b, w])
            if n == 0 or int(row[n]) != EOS:
                continue
            att, ctc, lm = parts_of(row, n, b, lam)
            want = (1.0 - lam) * att + lam * ctc + beta * lm + bonus * n
            assert abs(float(r.scores[b, w]) - want) <= 1e-4, (b, w, float(r.scores[b, w]), want, (att, ctc, lm, n))
            checked += 1
    return checked


@pytest.mark.parametrize("lam,beta,W", [(0.0, 0.5, 1), (0.0, 0.5, 4), (0.3, 0.5, 4), (0.3, 0.3, 4)])
def test_lm_beam_search_matches_oracle(lam, beta, W):
    """Every hypothesis of every sample: token rows and lengths exactly, scores within 1e-4 (the project's model-level
    bound).  Conditions on the reference: its smallest selection margin is at least 1e-3, and the LM changes the best
    hypothesis of every sample."""
    cfg, P, s, enc = setup()
    ref, plain = reference(lam, beta, W), reference_without_lm(lam, W)
    print(f"lam {lam} beta {beta} W {W}: reference margin {ref['gap']:.3e}, finished {ref['finished']}")
    assert ref["gap"] >= 1e-3
    for b in range(NSAMPLES):
        assert not torch.equal(ref["tokens"][b, 0], plain["tokens"][b, 0]), b
    lm = language_model(dev)
    r = model().beam_search(s.to(dev), ctc_weight=lam, beam=W, max_len=MAX_LEN, nbest=W, poll=0, lm=lm, lm_weight=beta)
    assert r.tokens.shape == (NSAMPLES, W, 1 + MAX_LEN) and r.scores.dtype == torch.float32
    assert torch.equal(r.tokens.cpu(), ref["tokens"])
    assert torch.equal(r.lengths.cpu().long(), ref["lengths"])
    err = float((r.scores.cpu().double() - ref["scores"]).abs().max())
    print(f"lam {lam} beta {beta} W {W}: score error {err:.3e}")
    assert err <= 1e-4
    r0 = model().beam_search(s.to(dev), ctc_weight=lam, beam=W, max_len=MAX_LEN, nbest=W, poll=0)
    for b in range(NSAMPLES):
        assert not torch.equal(r.tokens[b, 0], r0.tokens[b, 0]), b
    assert check_identity(r, lam, beta, 0.0) >= NSAMPLES


def test_token_bonus_enters_once_per_generated_token():
    """token_bonus = 0.5 with and without the CTC term, polling on: the four-term identity on the decoder's own
    hypotheses (no search reference is needed for it)."""
    cfg, P, s, enc = setup()
    lm = language_model(dev)
    for lam in (0.0, 0.3):
        r = model().beam_search(s.to(dev), ctc_weight=lam, beam=4, max_len=MAX_LEN, nbest=4, lm=lm, lm_weight=0.5,
                                token_bonus=0.5, poll=1)
        assert check_identity(r, lam, 0.5, 0.5) >= NSAMPLES


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("lam", [0.0, 0.3])
def test_no_lm_and_zero_weight_are_the_search_without_the_arguments(lam):
    cfg, P, s, enc = setup()
    kw = dict(ctc_weight=lam, beam=4, max_len=MAX_LEN, nbest=4, poll=0)
    a = model().beam_search(s.to(dev), **kw)
    for extra in (dict(lm=None, lm_weight=0.5, token_bonus=0.5), dict(lm=language_model(dev), lm_weight=0.0),
                  dict(lm=language_model(dev), lm_weight=0.0, token_bonus=1.0)):
        b = model().beam_search(s.to(dev), **kw, **extra)
        for u, v in zip(a, b):
            assert torch.equal(_bits(u), _bits(v)), extra
    ra = model().rescore(s.to(dev), beam=8, nbest=8)
    for extra in (dict(lm=None, lm_weight=0.5), dict(lm=language_model(dev), lm_weight=0.0, token_bonus=1.0)):
        rb = model().rescore(s.to(dev), beam=8, nbest=8, **extra)
        for u, v in zip(ra, rb):
            assert torch.equal(_bits(u), _bits(v)), extra
        assert torch.equal(_bits(ra.att_scores), _bits(rb.att_scores)) and rb.lm_scores is None
        assert torch.equal(_bits(ra.ctc_scores), _bits(rb.ctc_scores))


# ------------------------------------------------------------------------------------------------ rescoring

def att_logprob(Pd, cfg, labels, enc_b):
    """log p_att(labels, EOS | BOS) of the oracle decoder on the unpadded row, fp64."""
    row = torch.tensor([[BOS] + list(labels)], dtype=torch.int64)
    L = row.shape[1]
    pe = pe_table(cfg.dec_len, cfg.d_model).double()
    causal = torch.triu(torch.ones((L, L), dtype=torch.uint8), diagonal=1)
    h = F.embedding(row, Pd["decoder._embedding.weight"]) + pe[:L].unsqueeze(0)
    for l in range(cfg.n_dec):
        h = decoder_layer(Pd, f"decoder._layers.{l}", h, causal, enc_b, cfg, False)
    h = _ln(Pd, "decoder._norm_layer", h)
    lp = torch.log_softmax(F.linear(h, Pd["decoder._classifier.weight"]), dim=-1)[0]
    return float(sum(lp[i, t] for i, t in enumerate(list(labels) + [EOS])))


@functools.lru_cache(maxsize=None)
def rescore_reference(W, lam, beta, bonus):
    """Per sample (prefixes in final order, combined, att, ctc, lm scores fp64 in that order, the smallest gap of the
    final ranking), and the first pass's smallest selection margin."""
    cfg, P, s, enc = setup()
    V = cfg.vocab_size
    Pd = {k: v.double() for k, v in P.items()}
    logits = F.linear(enc, P["ctc_head.weight"].double()[:V])
    grams = language_model().ngrams
    out, boundary = [], INF
    for b, r in enumerate(ctc_beam_ref.batch(logits, V, W, cfg.pad_id, min(cfg.dec_len, 255) - 1)):
        boundary = min(boundary, r["boundary"])
        att = torch.tensor([att_logprob(Pd, cfg, g, enc[b:b + 1]) for g in r["prefixes"]], dtype=torch.float64)
        ctc = torch.from_numpy(r["scores"]).double()
        lm = torch.tensor([ngram_ref.sequence_logprob(grams, ORDER, list(g) + [EOS], BOS, V)[0] for g in r["prefixes"]],
                          dtype=torch.float64)
        n = torch.tensor([len(g) + 1 for g in r["prefixes"]], dtype=torch.float64)
        comb = att + lam * ctc + beta * lm + bonus * n
        order = ctc_beam_ref.rank(comb[None])[0]
        ranked = comb[order]
        gap = float((ranked[:-1] - ranked[1:]).min()) if len(ranked) > 1 else INF
        out.append(([r["prefixes"][int(i)] for i in order], ranked, att[order], ctc[order], lm[order], gap))
    return out, boundary


@pytest.mark.parametrize("lam,beta,bonus", [(0.5, 0.5, 0.0), (0.0, 0.5, 0.25)])
def test_rescore_with_lm_matches_reference_pipeline(lam, beta, bonus):
    """beam 8: lm_scores, att_scores, ctc_scores and the combined scores within 1e-4 of the reference, hypothesis by
    hypothesis; the order equal wherever the reference's ranking margin is at least 1e-3, which must cover every
    sample."""
    cfg, P, s, enc = setup()
    W = 8
    ref, boundary = rescore_reference(W, lam, beta, bonus)
    print(f"lam {lam} beta {beta} bonus {bonus}: first-pass margin {boundary:.3e}, "
          f"ranking margins {[f'{x[5]:.3e}' for x in ref]}")
    assert boundary >= 1e-3 and all(x[5] >= 1e-3 for x in ref)
    r = model().rescore(s.to(dev), beam=W, ctc_weight=lam, nbest=W, lm=language_model(dev), lm_weight=beta,
                        token_bonus=bonus)
    L = min(cfg.dec_len, 255)
    assert r.tokens.shape == (NSAMPLES, W, 1 + L) and r.lm_scores.shape == (NSAMPLES, W)
    worst = 0.0
    for b, (prefixes, comb, att, ctc, lm, gap) in enumerate(ref):
        for j in range(W):
            if j >= len(prefixes):
                assert int(r.lengths[b, j]) == 0 and float(r.scores[b, j]) == -INF
                continue
            g = list(prefixes[j])
            assert int(r.lengths[b, j]) == len(g) + 1
            assert r.tokens[b, j].tolist() == [BOS] + g + [EOS] * (L - len(g)), (b, j, r.tokens[b, j].tolist(), g)
            for got, want in ((r.scores, comb), (r.att_scores, att), (r.ctc_scores, ctc), (r.lm_scores, lm)):
                err = abs(float(got[b, j]) - float(want[j]))
                worst = max(worst, err)
                assert err <= 1e-4, (b, j, float(got[b, j]), float(want[j]))
    print(f"worst score error {worst:.3e}")
    plain = model().rescore(s.to(dev), beam=W, ctc_weight=lam, nbest=W)
    assert plain.lm_scores is None and not torch.equal(plain.scores, r.scores)


def test_rescore_with_lm_and_mbr():
    """The MBR path is unchanged on top: the same hypotheses, `risks` and `lm_scores` both filled, and
    asrx.mbr_rerank carries lm_scores along."""
    import asrx
    cfg, P, s, enc = setup()
    lm = language_model(dev)
    a = model().rescore(s.to(dev), beam=8, nbest=8, lm=lm, lm_weight=0.5)
    b = model().rescore(s.to(dev), beam=8, nbest=8, lm=lm, lm_weight=0.5, mbr_scale=1.0)
    assert b.risks is not None and b.lm_scores is not None and b.risks.shape == b.lm_scores.shape
    c = asrx.mbr_rerank(a, 1.0, drop=model().token_drop_ids())
    assert c.lm_scores is not None and c.risks is not None
    for other in (b, c):                    # the same hypotheses in another order, each with its own LM score
        for i in range(NSAMPLES):
            rows_a = {tuple(t.tolist()): float(x) for t, x, n in zip(a.tokens[i], a.lm_scores[i], a.lengths[i]) if n > 0}
            rows_o = {tuple(t.tolist()): float(x) for t, x, n in zip(other.tokens[i], other.lm_scores[i],
                                                                     other.lengths[i]) if n > 0}
            assert rows_a == rows_o
