"""Two-pass decoding end to end: Transformer.ctc_beam_search and Transformer.rescore on the GPU against a reference
pipeline in fp64 on the CPU: the oracle front end and encoder, the CTC head as enc @ W^T, tests/ctc_beam_ref.py, then
the oracle decoder run PER HYPOTHESIS, unpadded (row BOS, labels; causal mask only), its log-probabilities of
labels, EOS summed, and the hypotheses ranked by log p_att + lam * log p_ctc.

Model and data are those of test_gpu_joint_model.py (c1, ctc=True, fp32, the 4x classifier and a head biased to the
blank), so hypotheses are short and the margins wide: every selection margin of the reference's first pass and every
gap of its final rankings must exceed 1e-3, ten times the 1e-4 bound of the model-level tests."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle.ref_model import _ln, decoder_layer, pe_table
from tests import ctc_beam_ref as R
from tests import test_gpu_joint_model as J

pytestmark = pytest.mark.gpu
dev = "cuda"
EOS, NSAMPLES, BOS = J.EOS, J.NSAMPLES, 1
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def model():
    return J.build()


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
    tgt = list(labels) + [EOS]
    return float(sum(lp[i, t] for i, t in enumerate(tgt)))


@functools.lru_cache(maxsize=None)
def first_pass(W):
    cfg, P, s, enc = J.setup()
    V = cfg.vocab_size
    logits = F.linear(enc, P["ctc_head.weight"].double()[:V])
    return R.batch(logits, V, W, cfg.pad_id, min(cfg.dec_len, 255) - 1)


@functools.lru_cache(maxsize=None)
def reference(W, lam):
    """Per sample: (prefixes in final order, combined, att, ctc scores fp64 in that order), and the smallest margin."""
    cfg, P, s, enc = J.setup()
    Pd = {k: v.double() for k, v in P.items()}
    out, gap = [], INF
    for b, r in enumerate(first_pass(W)):
        gap = min(gap, r["boundary"])
        att = torch.tensor([att_logprob(Pd, cfg, g, enc[b:b + 1]) for g in r["prefixes"]], dtype=torch.float64)
        ctc = torch.from_numpy(r["scores"]).double()
        comb = att + lam * ctc
        order = R.rank(comb[None])[0]
        ranked = comb[order]
        if len(ranked) > 1:
            gap = min(gap, float((ranked[:-1] - ranked[1:]).min()))
        out.append(([r["prefixes"][int(i)] for i in order], ranked, att[order], ctc[order]))
    return out, gap


@pytest.mark.parametrize("W,lam", [(1, 0.5), (4, 0.5), (8, 0.0)])
def test_rescore_matches_reference_pipeline(W, lam):
    """All W hypotheses of every sample and their order exactly; attention, CTC and combined scores within 1e-4."""
    cfg, P, s, enc = J.setup()
    ref, gap = reference(W, lam)
    print(f"W {W} lam {lam}: reference margin {gap:.3e}")
    assert gap >= 1e-3
    r = model().rescore(s.to(dev), beam=W, ctc_weight=lam, nbest=W)
    L = min(cfg.dec_len, 255)
    assert r.tokens.shape == (NSAMPLES, W, 1 + L) and r.scores.dtype == torch.float32
    worst = 0.0
    for b, (prefixes, comb, att, ctc) in enumerate(ref):
        for j in range(W):
            if j >= len(prefixes):
                assert int(r.lengths[b, j]) == 0 and float(r.scores[b, j]) == -INF
                continue
            g = list(prefixes[j])
            assert int(r.lengths[b, j]) == len(g) + 1
            assert r.tokens[b, j].tolist() == [BOS] + g + [EOS] * (L - len(g)), (b, j, r.tokens[b, j].tolist(), g)
            for got, want in ((r.scores, comb), (r.att_scores, att), (r.ctc_scores, ctc)):
                err = abs(float(got[b, j]) - float(want[j]))
                worst = max(worst, err)
                assert err <= 1e-4, (b, j, float(got[b, j]), float(want[j]))
    print(f"W {W} lam {lam}: worst score error {worst:.3e}")


@pytest.mark.parametrize("W", [1, 4, 8])
def test_ctc_beam_search_alone_matches_the_first_pass(W):
    cfg, P, s, enc = J.setup()
    ref = first_pass(W)
    assert min(r["boundary"] for r in ref) >= 1e-3 and min(r["final"] for r in ref) >= 1e-3
    r = model().ctc_beam_search(s.to(dev), beam=W, nbest=W)
    ml = min(cfg.dec_len, 255) - 1
    assert r.tokens.shape == (NSAMPLES, W, ml)
    for b, rb in enumerate(ref):
        for j, g in enumerate(rb["prefixes"]):
            g = list(g)
            assert int(r.lengths[b, j]) == len(g)
            assert r.tokens[b, j].tolist() == g + [cfg.pad_id] * (ml - len(g))
            assert abs(float(r.scores[b, j]) - float(rb["scores"][j])) <= 1e-4
        assert bool((r.scores[b, len(rb["prefixes"]):] == -INF).all())
    il = torch.tensor([enc.shape[1], 10, 0])
    part = model().ctc_beam_search(s.to(dev), beam=W, nbest=W, input_lengths=il)
    assert torch.equal(part.tokens[0], r.tokens[0]) and torch.equal(part.scores[0], r.scores[0])
    assert int(part.lengths[2, 0]) == 0 and float(part.scores[2, 0]) == 0.0
    assert bool((part.scores[2, 1:] == -INF).all())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_existing_decodes_keep_their_bits_around_the_new_path():
    """beam_search(ctc_weight=0.3) and evaluate give the same bits before and after the two-pass decode ran, and
    decoder_fwd called as before returns the logits of a call with the grouping argument at its default."""
    from asrx import functions as Fn
    cfg, P, s, enc = J.setup()
    m = model()
    text = torch.ones(NSAMPLES, 1, dtype=torch.int64)
    kw = dict(ctc_weight=0.3, beam=4, max_len=J.MAX_LEN, nbest=4, poll=0)
    b0 = m.beam_search(s.to(dev), **kw)
    e0 = m.evaluate(s.to(dev), text)
    m.rescore(s.to(dev), beam=4)
    m.ctc_beam_search(s.to(dev), beam=4)
    b1 = m.beam_search(s.to(dev), **kw)
    e1 = m.evaluate(s.to(dev), text)
    for u, v in zip(b0, b1):
        assert torch.equal(_bits(u), _bits(v))
    assert torch.equal(e0[0], e1[0]) and len(e0[1]) == len(e1[1])
    for u, v in zip(e0[1], e1[1]):
        assert torch.equal(_bits(u.contiguous()), _bits(v.contiguous()))
    with torch.no_grad():
        C = Fn.make_ctx(m.decoder, 0.0)
        C.train, C.p = False, 0.0
        B, Te, d = enc.shape
        enc_c = enc.float().reshape(B * Te, d).to(dev)
        rows = torch.randint(0, cfg.vocab_size, (B, 6), generator=torch.Generator().manual_seed(1))
        mask = torch.ones(B, 6)
        mask[1, 4:] = 0
        old, _ = Fn.decoder_fwd(C, m.decoder, rows, mask, enc_c, B, 6, Te)
        new, _ = Fn.decoder_fwd(C, m.decoder, rows, mask, enc_c, B, 6, Te, group=1)
        assert torch.equal(_bits(old), _bits(new))
        # grouped: W copies of a sample's row over ONE encoder output give that row's logits
        W = 3
        rep = rows.repeat_interleave(W, dim=0)
        grp, _ = Fn.decoder_fwd(C, m.decoder, rep, mask.repeat_interleave(W, dim=0), enc_c, B * W, 6, Te, group=W)
        V = cfg.vocab_size
        a = old.view(B, 6, -1)[:, :, :V].cpu()
        g = grp.view(B, W, 6, -1)[:, :, :, :V].cpu()
        valid = mask.bool()
        for w in range(W):
            assert float((g[:, w][valid] - a[valid]).abs().max()) <= 1e-4


def test_rescore_bf16_smoke():
    """bf16: it runs, the scores are finite and ranked, and its best hypothesis lies among the fp32 run's W."""
    cfg, P, s, enc = J.setup()
    W = 4
    r32 = model().rescore(s.to(dev), beam=W, nbest=W)
    r = J.build("bf16").rescore(s.to(dev), beam=W, nbest=W)
    assert r.tokens.shape == r32.tokens.shape
    live = r.lengths > 0
    assert bool(live[:, 0].all()) and bool(torch.isfinite(r.scores[live]).all())
    assert bool(torch.isfinite(r.att_scores[live]).all()) and bool(torch.isfinite(r.ctc_scores[live]).all())
    assert bool((r.scores[:, :-1] >= r.scores[:, 1:]).all())
    for b in range(NSAMPLES):
        best = r.tokens[b, 0].tolist()
        assert any(best == r32.tokens[b, j].tolist() for j in range(W) if int(r32.lengths[b, j]) > 0), (b, best)
