"""Model-level parity of the drop-in asrx modules against the reference's golden vectors and the oracle.

Tolerances: fp32 path <= 1e-3 relative (max-norm) on logits — we hold it to 1e-4;
bf16 path at the bench model dims (c3, c5): within BF16_FACTOR = 1.5x the error of the reference's own bf16 path
(the oracle under torch's bf16 autocast) against the fp32 oracle, in the max norm, with >= 98% argmax agreement;
small golden configs: <= 1.5e-2 relative with >= 98% argmax agreement."""
import os

import numpy as np
import pytest
import torch

from oracle.ref_model import CONFIGS, det_params, forward as oracle_forward, synthetic_batch
from tests.bf16_check import check_bf16_forward

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def build(name, precision="fp32", dropout=None, attention="fused", seed=0):
    import asrx
    cfg = CONFIGS[name]["cfg"]
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout if dropout is None else dropout,
                         precision=precision, attention=attention)
    sd = m.state_dict()
    sd.update(det_params(cfg, seed))
    m.load_state_dict(sd)
    return m.to(dev), cfg


def golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"model_{name}.npz"))


@pytest.mark.parametrize("name", ["micro", "c1"])
def test_forward_fp32_golden(golden_dir, name):
    g = golden(golden_dir, name)
    m, cfg = build(name, "fp32")
    m.eval()
    s, t, k = (torch.from_numpy(g[x]) for x in ("spectrum", "text", "mask"))
    with torch.no_grad():
        logits = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev))
    assert relerr(logits, g["logits"]) < 1e-4


@pytest.mark.parametrize("attention", ["fused", "unfused"])
@pytest.mark.parametrize("name", ["micro", "c1"])
def test_forward_bf16_golden(golden_dir, name, attention):
    g = golden(golden_dir, name)
    m, cfg = build(name, "bf16", attention=attention)
    m.eval()
    s, t, k = (torch.from_numpy(g[x]) for x in ("spectrum", "text", "mask"))
    with torch.no_grad():
        logits = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev))
    ref = torch.from_numpy(g["logits"])
    assert relerr(logits, ref) < 1.5e-2
    agree = float((logits.cpu().argmax(-1) == ref.argmax(-1)).double().mean())
    assert agree >= 0.98


def test_forward_c2_fp32_vs_oracle():
    """c2 (d=256, h=4, 6+6 layers, B=32, T=512) fp32 forward vs the oracle on the host."""
    m, cfg = build("c2", "fp32")
    m.eval()
    spec = CONFIGS["c2"]
    s, t, k = synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=1234)
    P = det_params(cfg, 0)
    with torch.no_grad():
        ref = oracle_forward(P, s, t[:, :-1], k[:, :-1], cfg, False)
        logits = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev))
    assert relerr(logits, ref) < 1e-3


def test_forward_c3_bf16_vs_oracle():
    """Paper config (d=512, h=8, 12+12) at T=1000 with a 2-utterance batch, bf16 fused path, bounded by the
    reference's own bf16-autocast error."""
    m, cfg = build("c3", "bf16")
    m.eval()
    s, t, k = synthetic_batch(cfg, 2, 1000, 65, seed=1234)
    P = det_params(cfg, 0)
    with torch.no_grad():
        logits = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)).cpu()
    check_bf16_forward(logits, P, s, t[:, :-1], k[:, :-1], cfg, "c3 B=2")


def test_forward_c5_long_utterance_bf16_vs_oracle():
    """c5 long-utterance stress geometry at the bench's decoder length: T = 4000 frames -> T' = 999 encoder
    positions (O(T'^2) attention on the streamed LDS K/V path since T' > 256), L = 256 text positions (the
    256-key causal decoder self-attention and the 256-query x 999-key cross-attention), two utterances, bf16 fused
    path vs the oracle on the host, bounded by the reference's own bf16-autocast error."""
    m, cfg = build("c5", "bf16")
    m.eval()
    s, t, k = synthetic_batch(cfg, 2, 4000, 257, seed=4321)
    assert int(k[:, :-1].sum(-1).max()) > 128 and int(k[:, :-1].sum(-1).min()) < 256   # long and padded rows
    P = det_params(cfg, 0)
    with torch.no_grad():
        logits = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)).cpu()
    check_bf16_forward(logits, P, s, t[:, :-1], k[:, :-1], cfg, "c5 B=2 L=256")


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_train_grads_micro(golden_dir, precision, tol):
    g = golden(golden_dir, "micro")
    m, cfg = build("micro", precision, dropout=0.0)
    m.train()
    s, t, k = (torch.from_numpy(g[x]).to(dev) for x in ("spectrum", "text", "mask"))
    logits = m(s, t[:, :-1], k[:, :-1])
    loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2), t[:, 1:])
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < tol * abs(float(g["loss"]))
    named = dict(m.named_parameters())
    sd_grads = {}
    # map reference-key gradients through the state_dict hooks: load grads as "weights" into a twin module
    import asrx
    twin = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=0.0)
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.grad.cpu() if p1.grad is not None else torch.zeros_like(p2))
    gsd = twin.state_dict()
    gmax = max(float(np.abs(g["grad/" + k]).max()) for k in g["grad_names"])
    for key in g["grad_names"]:
        ref = g["grad/" + key]
        if float(np.abs(ref).max()) < 1e-6 * gmax:
            # mathematically zero gradient (e.g. the K bias: softmax is shift-invariant along keys) — the
            # reference holds fp32 rounding noise there; require an absolute match at the global scale
            assert float((gsd[key].double() - torch.from_numpy(ref).double()).abs().max()) < tol * 1e-2 * gmax, key
            continue
        assert relerr(gsd[key], ref) < tol, key


def test_train_grads_c1_norms(golden_dir):
    g = golden(golden_dir, "c1")
    m, cfg = build("c1", "fp32", dropout=0.0)
    m.train()
    s, t, k = (torch.from_numpy(g[x]).to(dev) for x in ("spectrum", "text", "mask"))
    logits = m(s, t[:, :-1], k[:, :-1])
    loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2), t[:, 1:])
    loss.backward()
    import asrx
    twin = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=0.0)
    with torch.no_grad():
        for p1, p2 in zip(m.parameters(), twin.parameters()):
            p2.copy_(p1.grad.cpu())
    gsd = twin.state_dict()
    for key, n in zip(g["grad_names"], g["grad_norms"]):
        assert abs(float(gsd[key].norm()) - n) <= 1e-3 * n + 1e-6, key
    for key in g["nograd_names"]:
        assert float(gsd[key].abs().max()) == 0.0, key


def test_greedy_decode_c1(golden_dir):
    g = golden(golden_dir, "c1")
    m, cfg = build("c1", "fp32")
    m.eval()
    s = torch.from_numpy(g["spectrum"]).to(dev)
    bos = torch.full((s.shape[0], 1), 1, dtype=torch.int32, device=dev)
    row, probs = m.evaluate(s, bos)
    np.testing.assert_array_equal(row.cpu().numpy(), g["greedy_row"])
    assert len(probs) == int(g["greedy_nprobs"])
    assert relerr(probs[-1], g["greedy_last_probs"]) < 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("prefix", [1, 3])
def test_greedy_decode_cache_equals_recompute(precision, prefix):
    """The KV-cached batched decode (eval) returns what the reference's per-sample full-prefix recomputation
    returns (model.py:125-151, restated as decode._decoder_evaluate_recompute): the same last-sample token row,
    the same number of EOS/final-step logits snapshots, each of the same shape and value; also with a multi-token
    prompt (prefill through the cache)."""
    from asrx.decode import _decoder_evaluate_cached, _decoder_evaluate_recompute
    m, cfg = build("c1", precision, seed=3)
    m.eval()
    g = torch.Generator().manual_seed(5)
    B, Te, d = 3, 24, cfg.d_model
    enc = (torch.randn(B, Te, d, generator=g)).to(dev)
    x = torch.randint(5, cfg.vocab_size, (B, prefix), generator=g, dtype=torch.int64)
    x[:, 0] = 1
    x = x.to(torch.int32).to(dev)
    dec = m.decoder
    dec._eos_token_id = int(torch.randint(5, cfg.vocab_size, (1,), generator=g))   # EOS hits do occur
    # the last input holds prefix + seq_len - 1 tokens; the PE table (layers.py:73) bounds it, as in the reference
    dec._seq_len = min(dec._seq_len, dec._pe.pe.shape[1] - prefix + 1)
    with torch.no_grad():
        row_c, probs_c = _decoder_evaluate_cached(dec, x, enc)
        row_r, probs_r = _decoder_evaluate_recompute(dec, x, enc)
    assert row_c.dtype == row_r.dtype and row_c.shape == row_r.shape
    assert torch.equal(row_c.cpu(), row_r.cpu())
    assert len(probs_c) == len(probs_r)
    tol = 1e-5 if precision == "fp32" else 2e-2
    for a, b in zip(probs_c, probs_r):
        assert a.shape == b.shape
        if a.numel():
            assert relerr(a, b) < tol


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_submodules_golden(golden_dir, precision, tol):
    """Standalone drop-in MHA / FeedForward / LayerNorm / EncoderLayer / DecoderLayer (micro config)."""
    g = np.load(os.path.join(golden_dir, "ops_micro.npz"))
    m, cfg = build("micro", precision)
    m.eval()
    x, enc = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["enc"]).to(dev)
    dmask = torch.from_numpy(g["dmask"]).bool().to(dev)
    el, dl = m.encoder._layers[0], m.decoder._layers[0]
    with torch.no_grad():
        assert relerr(el._attention(x), g["mha_self"]) < tol
        assert relerr(dl._mask_attention(x, attention_mask=dmask), g["mha_masked"]) < tol
        assert relerr(dl._cross_attention(x, enc_x=enc), g["mha_cross"]) < tol
        assert relerr(el._feedforward(x), g["ffn"]) < tol
        assert relerr(el._norm1(x), g["ln"]) < tol
        assert relerr(el(x), g["enc_layer"]) < tol
        assert relerr(dl(x, dmask, enc), g["dec_layer"]) < tol


def test_submodule_grads_fp32():
    """Backward of the standalone modules vs the oracle's autograd (fp32, dropout 0)."""
    from oracle.ref_model import decoder_layer as o_dec_layer, multi_head
    m, cfg = build("micro", "fp32", dropout=0.0)
    m.train()
    P = {k: v.clone().requires_grad_(True) for k, v in det_params(cfg).items()}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 9, cfg.d_model, generator=g)
    enc = torch.randn(2, 13, cfg.d_model, generator=g)
    mask = torch.triu(torch.ones(9, 9, dtype=torch.bool), 1)
    # decoder layer
    xr, er = x.clone().requires_grad_(True), enc.clone().requires_grad_(True)
    yr = o_dec_layer(P, "decoder._layers.0", xr, mask, er, cfg, False)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd, ed = x.to(dev).requires_grad_(True), enc.to(dev).requires_grad_(True)
    yd = m.decoder._layers[0](xd, mask.to(dev), ed)
    yd.backward(gy.to(dev))
    assert relerr(yd.detach(), yr.detach()) < 1e-4
    assert relerr(xd.grad, xr.grad) < 1e-3
    assert relerr(ed.grad, er.grad) < 1e-3
    # MHA standalone (self-attention)
    m.zero_grad()
    xr2 = x.clone().requires_grad_(True)
    yr2 = multi_head(P, "encoder._layers.0._attention", xr2, None, None, cfg, False)
    yr2.backward(gy)
    xd2 = x.to(dev).requires_grad_(True)
    yd2 = m.encoder._layers[0]._attention(xd2)
    yd2.backward(gy.to(dev))
    assert relerr(xd2.grad, xr2.grad) < 1e-3


@pytest.mark.parametrize("cfgname", ["micro", "c2"])
def test_trainer_fresh_grads_match_zeroed(cfgname):
    """Trainer steps leave the Linear-weight gradients unzeroed and write them with beta = 0 (FreshGrads): the
    gradients must equal, bit for bit, those of a step that zeroes the whole buffer first (dropout 0, no
    optimizer step in between)."""
    from asrx.train import Trainer
    m, cfg = build(cfgname, "bf16", dropout=0.0)
    m.train()
    spec = CONFIGS[cfgname]
    s, t, k = synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=11)
    s, t, k = s.to(dev), t.to(dev), k.to(dev)
    tr = Trainer(m)
    assert tr._wonly
    tr.store.grad.fill_(float("nan"))        # stale garbage in the unzeroed regions must never leak through
    tr.forward_backward(s, t, k)              # first step: binds grads, zeroes everything
    tr.store.grad.fill_(float("nan"))
    tr.forward_backward(s, t, k)              # fresh mode
    g_fresh = tr.store.grad.clone()
    assert torch.isfinite(g_fresh).all()
    tr._wonly = []
    tr.store.grad.fill_(float("nan"))
    tr.forward_backward(s, t, k)              # whole-buffer zero
    assert torch.equal(g_fresh, tr.store.grad)


@pytest.mark.parametrize("every", [1, 0])
def test_trainer_release_path_fresh_grads(every, monkeypatch):
    """Multi-GPU backward structure on one GPU: an injected all-reduce (doubling every range it is handed)
    receives decoder / upper-encoder ranges mid-backward and the rest at finish(); with unzeroed weight
    gradients (FreshGrads) every range must already hold its final gradient when handed over.  every: fixed
    one-layer release groups, or 0 = the default by tile rounds (at c2's size: everything at finish, so the
    decoder's carried gradients are handed over there)."""
    from asrx import functions
    from asrx.train import Trainer
    monkeypatch.setattr(functions, "RELEASE_LAYERS", every)
    m, cfg = build("c2", "bf16", dropout=0.0)
    m.train()
    spec = CONFIGS["c2"]
    s, t, k = synthetic_batch(cfg, 8, spec["frames"], spec["text_len"] + 1, seed=5)
    s, t, k = s.to(dev), t.to(dev), k.to(dev)
    ref = Trainer(m)
    ref._wonly = []
    ref.forward_backward(s, t, k)
    g_ref = ref.store.grad.clone()
    seen = []

    def fake(view):
        seen.append(view.numel())
        view.mul_(2.0)

    tr = Trainer(m, allreduce_fn=fake)
    assert tr.reducer.active and tr._wonly
    tr.forward_backward(s, t, k)              # binds / zeroes
    tr.reducer.finish()
    tr.store.grad.fill_(float("nan"))
    seen.clear()
    tr.forward_backward(s, t, k)              # fresh mode, ranges released mid-backward
    tr.reducer.finish()
    torch.cuda.synchronize()
    assert len(seen) > 1 or every == 0
    assert sum(seen) == tr.store.grad.numel()
    assert torch.equal(tr.store.grad, 2.0 * g_ref)


def test_bf16_training_reduces_loss():
    """A few bf16 AdamW steps (dropout 0.1) on one c1 batch drive the loss down."""
    import asrx
    m, cfg = build("c1", "bf16")
    m.train()
    spec = CONFIGS["c1"]
    s, t, k = synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=7)
    s, t, k = s.to(dev), t.to(dev), k.to(dev)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        logits = m(s, t[:, :-1], k[:, :-1])
        loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2), t[:, 1:])
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.7 * losses[0], losses


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_forward_equals_eager(precision):
    """asrx.infer.GraphedForward: replayed forwards equal the eager forward bit for bit, for new inputs of the
    captured shape, and a new shape captures a new graph."""
    from asrx.infer import GraphedForward
    m, cfg = build("c1", precision, seed=2)
    m.eval()
    fwd = GraphedForward(m)
    for seed, B in ((1, 2), (2, 2), (3, 3)):
        s, t, k = synthetic_batch(cfg, B, CONFIGS["c1"]["frames"], CONFIGS["c1"]["text_len"] + 1, seed=seed)
        s, t, k = s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)
        with torch.no_grad():
            ref = m(s, t, k).clone()
        got = fwd(s, t, k)
        assert torch.equal(got, ref)
    assert len(fwd._graphs) == 2
