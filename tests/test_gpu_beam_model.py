"""Beam-search decoding end to end: Decoder.beam_search / Transformer.beam_search on the GPU against the reference
beam search over the oracle decoder (tests/beam_ref.py: full-prefix recomputation in fp64 on the CPU), its ties to
the greedy `evaluate`, and the early stop."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.ref_model import CONFIGS, det_params, encoder as oracle_encoder, front_end
from tests import beam_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
EOS, MAX_LEN = 22, 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build(P, cfg, precision="fp32"):
    import asrx
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, precision=precision)
    sd = m.state_dict()
    sd.update(P)
    m.load_state_dict(sd)
    return m.to(dev).eval()


@functools.lru_cache(maxsize=None)
def parity_setup():
    """c1 with det_params(cfg, 3) and a 4x classifier (sharper distributions: wider margins, EOS hits), a random
    encoder output for three samples."""
    cfg = CONFIGS["c1"]["cfg"]
    P = det_params(cfg, 3)
    P["decoder._classifier.weight"] = P["decoder._classifier.weight"] * 4
    enc = torch.randn(3, 24, 128, generator=torch.Generator().manual_seed(7))
    return cfg, P, enc, torch.ones(3, 1, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def parity_reference(W, final_norm):
    cfg, P, enc, prompt = parity_setup()
    return beam_ref.beam_search(P, cfg, enc, prompt, W, EOS, MAX_LEN, final_norm=final_norm)


@functools.lru_cache(maxsize=None)
def parity_model():
    cfg, P, enc, prompt = parity_setup()
    m = build(P, cfg)
    m.decoder._eos_token_id = EOS
    return m


@pytest.mark.parametrize("final_norm,W", [(True, 3), (True, 4), (True, 8), (False, 3), (False, 4)])
def test_beam_search_matches_oracle_beam(final_norm, W):
    """fp32, prompt [1], 8 new tokens, every hypothesis of every sample: token rows and lengths exactly, scores
    within 1e-4.  The reference's smallest selection margin (recomputed here; 2.3e-3 or more with the final
    LayerNorm, 6.9e-3 without) must exceed 1e-3, far above the fp32 path's error, and some hypothesis must have
    finished early so that the frozen-beam rule was in play."""
    cfg, P, enc, prompt = parity_setup()
    ref = parity_reference(W, final_norm)
    print(f"reference margin {ref['gap']:.3e}, finished hypotheses {ref['finished']}")
    assert ref["gap"] >= 1e-3
    assert ref["finished"] >= 1 and int(ref["lengths"].min()) < MAX_LEN
    r = parity_model().decoder.beam_search(prompt.to(dev), enc.to(dev), beam=W, max_len=MAX_LEN, length_penalty=0.0,
                                           final_norm=final_norm, nbest=W, poll=0)
    assert r.tokens.shape == (3, W, 1 + MAX_LEN) and r.tokens.dtype == torch.int64
    assert r.lengths.shape == (3, W) and r.scores.shape == (3, W) and r.scores.dtype == torch.float32
    assert torch.equal(r.tokens.cpu(), ref["tokens"])
    assert torch.equal(r.lengths.cpu().long(), ref["lengths"])
    err = float((r.scores.cpu().double() - ref["scores"]).abs().max())
    print(f"score error {err:.3e}")
    assert err <= 1e-4


def test_beam_search_nbest_and_length_penalty():
    """nbest keeps the head of the ranking; a length penalty reorders the same hypotheses by score / len**p."""
    cfg, P, enc, prompt = parity_setup()
    dec = parity_model().decoder
    kw = dict(beam=4, max_len=MAX_LEN, poll=0)
    full = dec.beam_search(prompt.to(dev), enc.to(dev), nbest=4, **kw)
    one = dec.beam_search(prompt.to(dev), enc.to(dev), **kw)
    assert one.tokens.shape == (3, 1, 1 + MAX_LEN)
    assert torch.equal(one.tokens, full.tokens[:, :1]) and torch.equal(one.scores, full.scores[:, :1])
    pen = dec.beam_search(prompt.to(dev), enc.to(dev), nbest=4, length_penalty=1.0, **kw)
    ref = beam_ref.beam_search(P, cfg, enc, prompt, 4, EOS, MAX_LEN, length_penalty=1.0)
    assert torch.equal(pen.tokens.cpu(), ref["tokens"]) and torch.equal(pen.lengths.cpu().long(), ref["lengths"])
    key = pen.scores.double() / pen.lengths.double()
    assert bool((key[:, :-1] >= key[:, 1:]).all())
    with pytest.raises(ValueError):
        dec.beam_search(prompt.to(dev), enc.to(dev), beam=17)
    with pytest.raises(ValueError):
        dec.beam_search(prompt.to(dev), enc.to(dev), beam=2, nbest=3)
    with pytest.raises(ValueError):
        dec.beam_search(prompt.to(dev), enc.to(dev), beam=2, max_len=cfg.dec_len + 1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("prefix", [1, 3])
def test_beam_one_without_final_norm_is_greedy_evaluate(precision, prefix):
    """beam = 1, final_norm = False, no length penalty: the last sample's tokens are those of the cached greedy
    decode (`evaluate`) up to and including its first generated EOS, and EOS from there on."""
    from asrx.decode import _decoder_evaluate_cached
    cfg = CONFIGS["c1"]["cfg"]
    m = build(det_params(cfg, 3), cfg, precision)
    g = torch.Generator().manual_seed(5)
    B, Te, d = 3, 24, cfg.d_model
    enc = (torch.randn(B, Te, d, generator=g)).to(dev)
    x = torch.randint(5, cfg.vocab_size, (B, prefix), generator=g, dtype=torch.int64)
    x[:, 0] = 1
    x = x.to(torch.int32).to(dev)
    dec = m.decoder
    dec._eos_token_id = eos = int(torch.randint(5, cfg.vocab_size, (1,), generator=g))
    dec._seq_len = min(dec._seq_len, dec._pe.pe.shape[1] - prefix + 1)
    with torch.no_grad():
        row, _ = _decoder_evaluate_cached(dec, x, enc)
    r = dec.beam_search(x, enc, beam=1, final_norm=False, length_penalty=0.0, poll=0)
    row = row.cpu().long()[0]
    assert r.tokens.shape == (B, 1, prefix + dec._seq_len) and row.shape == (prefix + dec._seq_len,)
    expect = row.clone()
    hits = (row[prefix:] == eos).nonzero().flatten()
    n = int(hits[0]) + 1 if hits.numel() else dec._seq_len
    expect[prefix + n:] = eos
    assert torch.equal(r.tokens[B - 1, 0].cpu(), expect)
    assert int(r.lengths[B - 1, 0]) == n
    assert torch.equal(r.tokens[:, 0, :prefix].cpu(), x.cpu().long())


def test_poll_stops_early_with_the_same_result():
    """With a zero classifier every continuation ties, the index rule picks token 0 first, and with EOS = 0 one
    more hypothesis finishes per step: all W = 3 are done after three steps.  poll = 1 then stops there (shorter
    token rows), poll = 0 runs all 8 steps; hypotheses, lengths and scores are the same.  On the parity model,
    where hypotheses stay alive, polling changes nothing at all."""
    cfg, P, enc, prompt = parity_setup()
    Pz = dict(P)
    Pz["decoder._classifier.weight"] = torch.zeros_like(P["decoder._classifier.weight"])
    m = build(Pz, cfg)
    m.decoder._eos_token_id = 0
    kw = dict(beam=3, max_len=MAX_LEN, nbest=3)
    r0 = m.decoder.beam_search(prompt.to(dev), enc.to(dev), poll=0, **kw)
    r1 = m.decoder.beam_search(prompt.to(dev), enc.to(dev), poll=1, **kw)
    assert r0.tokens.shape == (3, 3, 1 + MAX_LEN)
    assert r1.tokens.shape == (3, 3, 1 + 3)
    assert torch.equal(r1.tokens, r0.tokens[:, :, :4]) and bool((r0.tokens[:, :, 4:] == 0).all())
    assert torch.equal(r1.lengths, r0.lengths) and torch.equal(r1.scores, r0.scores)
    assert r1.lengths[0].tolist() == [1, 2, 3]
    logv = float(np.log(cfg.vocab_size))
    assert torch.allclose(r1.scores[0].double(), torch.tensor([-logv, -2 * logv, -3 * logv], dtype=torch.float64),
                          atol=1e-5)
    dec = parity_model().decoder
    a = dec.beam_search(prompt.to(dev), enc.to(dev), beam=4, max_len=MAX_LEN, nbest=4, poll=0)
    b = dec.beam_search(prompt.to(dev), enc.to(dev), beam=4, max_len=MAX_LEN, nbest=4, poll=1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_transformer_beam_search_front_door(golden_dir):
    """Transformer.beam_search(spectrum) on the c1 golden spectrum from a BOS column: shapes, scores in ranking
    order, and the best score equal (1e-4) to what the oracle model gives the same token row."""
    g = np.load(os.path.join(golden_dir, "model_c1.npz"))
    cfg = CONFIGS["c1"]["cfg"]
    P = det_params(cfg, 0)
    m = build(P, cfg)
    s = torch.from_numpy(g["spectrum"])
    B = s.shape[0]
    r = m.beam_search(s.to(dev), beam=4, nbest=4)
    assert type(r).__name__ == "BeamResult"
    import asrx
    assert isinstance(r, asrx.BeamResult)
    assert r.tokens.shape == (B, 4, 1 + cfg.dec_len) and r.lengths.shape == (B, 4) and r.scores.shape == (B, 4)
    assert bool((r.tokens[:, :, 0] == 1).all())
    assert bool((r.scores[:, :-1] >= r.scores[:, 1:]).all()) and bool(torch.isfinite(r.scores).all())
    assert int(r.lengths.min()) >= 1 and int(r.lengths.max()) <= cfg.dec_len
    Pd = {k: v.double() for k, v in P.items()}
    enc = oracle_encoder(Pd, front_end(Pd, s.double()), cfg, False)
    for b in range(B):
        row = r.tokens[b, 0].cpu()
        want = beam_ref.sequence_score(P, cfg, enc[b], row, 1, cfg.eos_id, True)
        assert abs(float(r.scores[b, 0]) - want) <= 1e-4, (b, float(r.scores[b, 0]), want)
        n = int(r.lengths[b, 0])
        assert bool((row[1 + n:] == cfg.eos_id).all())
