"""Joint CTC/attention beam search end to end: Transformer.beam_search(spectrum, ctc_weight=lam) on the GPU against
tests/joint_ref.joint_beam_search (the oracle front end, encoder and decoder with full-prefix recomputation, the CTC
head as enc @ W^T, fp64 on the CPU), and against torch's CTC likelihood as an independent check of the CTC term.

Model: c1, ctc=True, fp32, det_params(cfg, 3) with test_gpu_beam_model.py's 4x classifier; the head is random rows of
scale 0.15 plus a blank row along the mean encoder output (logit about +9), so that the head emits mostly blank as a
trained one does and short hypotheses end with a competitive score."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.ref_model import CONFIGS, det_params, encoder as oracle_encoder, front_end
from tests import ctc_ref, joint_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
EOS, MAX_LEN, NSAMPLES = 22, 8, 3
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


def build(precision="fp32"):
    import asrx
    cfg, P, s, enc = setup()
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, precision=precision, ctc=True)
    sd = m.state_dict()
    sd.update(P)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.decoder._eos_token_id = EOS
    assert m.ctc_blank == cfg.pad_id
    return m


@functools.lru_cache(maxsize=None)
def model():
    return build()


@functools.lru_cache(maxsize=None)
def reference(lam, W):
    cfg, P, s, enc = setup()
    prompt = torch.ones(NSAMPLES, 1, dtype=torch.int64)
    return joint_ref.joint_beam_search(P, cfg, enc, prompt, W, EOS, MAX_LEN, lam, cfg.pad_id)


@pytest.mark.parametrize("lam,W", [(0.3, 1), (0.3, 4), (1.0, 4)])
def test_joint_beam_search_matches_oracle(lam, W):
    """Every hypothesis of every sample: token rows and lengths exactly, joint scores within 1e-4 (the bound of the
    attention-only model test).  The reference's smallest selection margin must exceed 1e-3, far above the fp32
    path's error.  For lam = 1 the score of every finished hypothesis is also -nll of torch's fp64 CTC on the head's
    logits for its labels, and some hypothesis must have finished."""
    cfg, P, s, enc = setup()
    ref = reference(lam, W)
    print(f"reference margin {ref['gap']:.3e}, finished hypotheses {ref['finished']}")
    assert ref["gap"] >= 1e-3
    r = model().beam_search(s.to(dev), ctc_weight=lam, beam=W, max_len=MAX_LEN, nbest=W, poll=0)
    assert r.tokens.shape == (NSAMPLES, W, 1 + MAX_LEN) and r.scores.dtype == torch.float32
    assert torch.equal(r.tokens.cpu(), ref["tokens"])
    assert torch.equal(r.lengths.cpu().long(), ref["lengths"])
    err = float((r.scores.cpu().double() - ref["scores"]).abs().max())
    print(f"lam {lam} W {W}: joint score error {err:.3e}")
    assert err <= 1e-4
    if lam == 1.0:
        assert ref["finished"] >= 1
        logits = torch.nn.functional.linear(enc, P["ctc_head.weight"].double())
        checked = 0
        for b in range(NSAMPLES):
            for w in range(W):
                row = r.tokens[b, w, 1:].cpu()
                n = int(r.lengths[b, w])
                if n == 0 or int(row[n - 1]) != EOS:
                    continue
                labels = row[:n - 1]
                tg = torch.full((1, MAX_LEN), cfg.pad_id, dtype=torch.int64)
                tg[0, :n - 1] = labels
                nll, _ = ctc_ref.ctc_reference(logits[b:b + 1], tg, None, torch.tensor([n - 1]), cfg.pad_id)
                assert abs(float(r.scores[b, w]) + float(nll[0])) <= 1e-4, (b, w, float(r.scores[b, w]), float(nll[0]))
                checked += 1
        assert checked >= 1


def test_zero_ctc_weight_is_the_attention_only_search_bit_for_bit():
    cfg, P, s, enc = setup()
    kw = dict(beam=4, max_len=MAX_LEN, nbest=4, poll=0)
    a = model().beam_search(s.to(dev), **kw)
    b = model().beam_search(s.to(dev), ctc_weight=0.0, **kw)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths)
    assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    c = model().beam_search(s.to(dev), ctc_weight=0.3, **kw)           # (and the CTC term does change the search)
    assert not torch.equal(a.scores, c.scores)


def test_joint_beam_search_with_input_lengths_and_polling():
    """Frame counts below T' change the CTC term of those samples only; polling changes nothing here."""
    cfg, P, s, enc = setup()
    kw = dict(ctc_weight=0.3, beam=4, max_len=MAX_LEN, nbest=4)
    full = model().beam_search(s.to(dev), poll=0, **kw)
    il = torch.tensor([enc.shape[1], 10, enc.shape[1]])
    part = model().beam_search(s.to(dev), input_lengths=il, poll=1, **kw)
    assert all(torch.equal(u[[0, 2]], v[[0, 2]]) for u, v in zip(full, part))
    assert not torch.equal(full.scores[1], part.scores[1])
    prompt = torch.ones(NSAMPLES, 1, dtype=torch.int64)
    ref = joint_ref.joint_beam_search(P, cfg, enc, prompt, 4, EOS, MAX_LEN, 0.3, cfg.pad_id, input_lengths=il)
    assert ref["gap"] >= 1e-3
    assert torch.equal(part.tokens.cpu(), ref["tokens"]) and torch.equal(part.lengths.cpu().long(), ref["lengths"])
    assert float((part.scores.cpu().double() - ref["scores"]).abs().max()) <= 1e-4


def test_joint_beam_search_bf16():
    """bf16: finite scores in ranking order and valid shapes (parity is bounded by the decoder's bf16 error, as in
    the attention-only bf16 test)."""
    cfg, P, s, enc = setup()
    r = build("bf16").beam_search(s.to(dev), ctc_weight=0.3, beam=4, max_len=MAX_LEN, nbest=4, poll=0)
    assert r.tokens.shape == (NSAMPLES, 4, 1 + MAX_LEN) and r.lengths.shape == (NSAMPLES, 4)
    assert bool(torch.isfinite(r.scores).all()) and bool((r.scores[:, :-1] >= r.scores[:, 1:]).all())
    assert bool((r.tokens[:, :, 0] == 1).all()) and int(r.tokens.min()) >= 0 and int(r.tokens.max()) < cfg.vocab_size
    assert int(r.lengths.min()) >= 1 and int(r.lengths.max()) <= MAX_LEN
