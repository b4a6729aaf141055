"""Parity of the post-LN model family (asrx.new, the drop-in for modules/Transformer/new/) against the reference's own
outputs (tests/golden/new_model.npz, made by tests/golden/make_golden_new.py from the variant run with its own
layers / masking) and against the pinned oracle (oracle/ref_model_new.py).

Tolerances: fp32 path — logits and encoder output <= 1e-4 relative (max norm), loss <= 1e-5 relative, every
parameter gradient <= 1e-3 relative, greedy evaluate tokens / EOS steps exact; bf16 path — logits within 1.5x the
error of the oracle under torch's bf16 autocast (the reference's own bf16 path) against fp32."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_model_new as N
from tests.golden_io import load_golden

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def build(name, precision="fp32", dropout=None, seed=0):
    import asrx.new
    c = N.NEW_CONFIGS[name]
    m = asrx.new.Transformer(c.vocab_size, c.n_mels, c.enc_seq_len, c.dec_seq_len, c.hidden_dim, c.n_enc, c.n_dec,
                             c.n_heads, c.ff_dim, dev, dropout=c.dropout if dropout is None else dropout, sr=c.sr,
                             n_fft=c.n_fft, padding_idx=c.pad_id, eos_token=c.eos_id, bos_token=c.bos_id,
                             precision=precision)
    sd = m.state_dict()
    sd.update(N.det_params(c, seed))
    m.load_state_dict(sd)
    return m.to(dev), c


def golden_batch(golden_dir, name):
    g = load_golden(golden_dir, "new_model.npz")
    p = name + "/"
    batch = {"spectre": torch.from_numpy(g[p + "spectre"]).to(dev),
             "spectrogram_len": torch.from_numpy(g[p + "lens"]).to(dev),
             "encoded_text": torch.from_numpy(g[p + "text"]).to(dev)}
    return g, p, batch


def targets(text, eos):
    t = torch.full_like(text, eos)
    t[:, :-1] = text[:, 1:]
    return t


@pytest.mark.parametrize("name", ["new_micro", "new_small"])
def test_new_forward_grads_fp32_golden(golden_dir, name):
    """fp32: eval logits and encoder output, the dropout-0 training loss and every parameter gradient (the unused
    VGG front-end none) against the reference's own values."""
    g, p, batch = golden_batch(golden_dir, name)
    m, c = build(name)
    m.eval()
    with torch.no_grad():
        logits = m(batch)
        enc = m.encoder(batch["spectre"], batch["spectrogram_len"])
    assert relerr(logits, g[p + "logits"]) < 1e-4
    assert relerr(enc, g[p + "enc"]) < 1e-4
    m.train()
    m.zero_grad()
    lg = m(batch)
    loss = torch.nn.functional.cross_entropy(lg.transpose(1, 2), targets(batch["encoded_text"], c.eos_id))
    loss.backward()
    assert abs(float(loss) - float(g[p + "loss"])) < 1e-5 * abs(float(g[p + "loss"]))
    named = {}
    for k, prm in m.named_parameters():
        named[k] = prm
    # gradients under the reference keys: load them as weights into a twin (the state_dict hooks split the fused
    # q / k / v storage back into per-head keys)
    twin, _ = build(name)
    with torch.no_grad():
        for (k1, p1), (k2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert k1 == k2
            p2.copy_(p1.grad if p1.grad is not None else torch.zeros_like(p2))
    gsd = twin.state_dict()
    # a gradient that is zero in exact arithmetic (the key bias: softmax is shift-invariant along the keys) holds
    # only rounding noise in either implementation (~1e-11): its error is measured against the largest gradient
    gmax = max(float(np.abs(g[p + "grad/" + k]).max()) for k in g[p + "grad_names"])
    for k in g[p + "grad_names"]:
        want = g[p + "grad/" + k]
        den = max(float(np.abs(want).max()), 1e-4 * gmax)
        err = float((gsd[k].double().cpu() - torch.from_numpy(want).double()).abs().max()) / den
        assert err < 1e-3, (k, err)
    for k in g[p + "nograd_names"]:
        assert named[k].grad is None or float(named[k].grad.abs().max()) == 0.0, k


@pytest.mark.parametrize("name", ["new_micro", "new_small"])
def test_new_evaluate_fp32_golden(golden_dir, name):
    """Greedy evaluate (new/model.py:125-142): token rows, EOS steps exact, last-step logits."""
    g, p, batch = golden_batch(golden_dir, name)
    m, c = build(name)
    m.eval()
    with torch.no_grad():
        toks, last, eoses = m.evaluate(batch)
    np.testing.assert_array_equal(toks.cpu().numpy(), g[p + "eval_tokens"])
    np.testing.assert_array_equal(eoses.numpy(), g[p + "eval_eoses"])
    assert toks.dtype == torch.int32
    assert relerr(last, g[p + "eval_last"]) < 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_new_evaluate_kv_cache_equals_full_prefix_recompute(precision):
    """The KV-cached greedy decode (Decoder._evaluate_cached, the default) against the reference's full-prefix
    recompute of every step (evaluate(..., cache=False), new/model.py:125-142) on the same weights: token rows and
    EOS steps exact, the final step's logits (every position) within fp32 rounding; bf16: the logits of every
    position whose inputs are identical in both paths within 2e-2, more than one position per row on average
    (synthetic_batch seed 11)."""
    m, c = build("new_small", precision)
    m.eval()
    s, lens, text = N.synthetic_batch(c, 5, seed=11)
    with torch.no_grad():
        enc = m.encoder(s.to(dev), lens.to(dev))
        t0, l0, e0 = m.decoder.evaluate(enc, dev, cache=False)
        t1, l1, e1 = m.decoder.evaluate(enc, dev)
    assert l0.shape == l1.shape and t0.shape == t1.shape and t1.dtype == torch.int32
    if precision == "bf16":
        # (bf16: the two paths run GEMMs of different row counts, whose fp32 sums may round an activation
        #  differently; a near-tie can then flip a token and every later position with it — per row, the positions
        #  up to and including the first step whose tokens differ are computed from identical inputs and compared)
        s0, s1 = t0[:, 1:].cpu(), t1[:, 1:].cpu()
        rows, steps = s0.shape
        same_inputs = torch.zeros(rows, steps, dtype=torch.bool)
        for r in range(rows):
            flips = (s0[r] != s1[r]).nonzero()
            same_inputs[r, :int(flips[0]) + 1 if flips.numel() else steps] = True
        assert relerr(l1.cpu()[same_inputs], l0.cpu()[same_inputs]) < 2e-2
        assert int(t1.min()) >= 0 and int(t1.max()) < c.vocab_size
        compared = int(same_inputs.sum())
        assert compared > rows, f"{compared} positions compared over {rows} rows: none past position 0"
        return
    assert torch.equal(t0.cpu(), t1.cpu())
    assert torch.equal(e0, e1)
    assert relerr(l1, l0.cpu()) < 1e-5


def test_new_forward_bf16_vs_oracle_autocast_bound():
    """bf16 operands (fp32 accumulation and residual stream): logits within 1.5x the error of the oracle under
    torch's bf16 autocast against the fp32 oracle."""
    m, c = build("new_small", "bf16")
    m.eval()
    s, lens, text = N.synthetic_batch(c, 4, seed=7)
    batch = {"spectre": s.to(dev), "spectrogram_len": lens.to(dev), "encoded_text": text.to(dev)}
    with torch.no_grad():
        logits = m(batch).cpu()
    P = N.det_params(c, 0)
    with torch.no_grad():
        ref = N.forward(P, s, lens, text, c, False)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref16 = N.forward(P, s, lens, text, c, False).float()
    e, e16 = relerr(logits, ref), relerr(ref16, ref)
    print(f"\nnew_small bf16: logits rel err {e:.3e} (autocast path {e16:.3e})")
    assert e <= 1.5 * e16, (e, e16)


def test_new_layers_standalone_dense_masks():
    """The drop-in EncoderLayer / DecoderLayer called as the reference calls them — dense boolean masks, a
    (B, L, 1) non_pad_mask — against the oracle's layer functions (fp32)."""
    m, c = build("new_micro")
    m.eval()
    P = N.det_params(c, 0)
    g = torch.Generator().manual_seed(3)
    B, T, L, d = 2, c.enc_len, c.dec_seq_len, c.n_mels
    x = torch.randn(B, T, d, generator=g)
    lens = torch.tensor([T, T - 7])
    npm = N.valid_rows(lens, T)
    mask = npm.lt(1).unsqueeze(1).expand(-1, T, -1)
    with torch.no_grad():
        y = m.encoder.layers[0](x.to(dev), mask.to(dev), npm.unsqueeze(-1).to(dev))
    k = "encoder.layers.0"
    want = N._ln(P, k + ".norm1", N.mha(P, k + ".attention", x, None, mask, c, False)) * npm.unsqueeze(-1)
    want = N._ln(P, k + ".norm2", N.ffn(P, k + ".ff", want, c, False)) * npm.unsqueeze(-1)
    assert relerr(y, want) < 1e-4
    xd = torch.randn(B, L, d, generator=g)
    text = torch.tensor([[1, 9, 8, 2, 2, 2, 2, 2], [1, 7, 6, 5, 11, 12, 13, 2]])
    npm_d = text.ne(c.eos_id).float().unsqueeze(-1)
    causal = torch.triu(torch.ones((L, L), dtype=torch.uint8), diagonal=1).unsqueeze(0).expand(B, -1, -1)
    amask = (causal + text.eq(c.eos_id).unsqueeze(1).expand(-1, L, -1)).gt(0)
    emask = npm.lt(1).unsqueeze(1).expand(-1, L, -1)
    with torch.no_grad():
        yd = m.decoder.layers[1](xd.to(dev), amask.to(dev), x.to(dev), emask.to(dev), npm_d.to(dev))
    want_d = N.decoder_layer(P, "decoder.layers.1", xd, amask, x, emask, npm_d, c, False)
    assert relerr(yd, want_d) < 1e-4


def test_new_training_steps_reduce_loss():
    """Dropout 0.1, bf16: a few AdamW steps on one batch drive the loss down (finite gradients throughout)."""
    m, c = build("new_small", "bf16", dropout=0.1)
    m.train()
    s, lens, text = N.synthetic_batch(c, 4, seed=9)
    batch = {"spectre": s.to(dev), "spectrogram_len": lens.to(dev), "encoded_text": text.to(dev)}
    tgt = targets(batch["encoded_text"], c.eos_id)
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(m(batch).transpose(1, 2), tgt)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.8 * losses[0], losses


def test_new_wide_fp32_forward_and_grads_vs_oracle():
    """The variant beyond the fixtures' toy widths: d_model 256 (4 full-width heads of 256, ff 1024), 4+4 layers,
    125 encoder frames, 32 text positions — fp32 logits (<= 1e-4) and every parameter gradient of the dropout-0
    training loss (<= 1e-3, the key-bias rule) against the oracle (oracle/ref_model_new.py, pinned to the
    reference's fixtures at the toy sizes) run in fp64."""
    import asrx.new
    c = N.NewConfig(vocab_size=250, n_mels=256, enc_seq_len=4, dec_seq_len=32, hidden_dim=8, n_enc=4, n_dec=4,
                    n_heads=4, ff_dim=1024)
    m = asrx.new.Transformer(c.vocab_size, c.n_mels, c.enc_seq_len, c.dec_seq_len, c.hidden_dim, c.n_enc, c.n_dec,
                             c.n_heads, c.ff_dim, dev, dropout=0.0, sr=c.sr, n_fft=c.n_fft, padding_idx=c.pad_id,
                             eos_token=c.eos_id, bos_token=c.bos_id)
    sd = m.state_dict()
    sd.update(N.det_params(c, 0))
    m.load_state_dict(sd)
    m = m.to(dev).train()
    s, lens, text = N.synthetic_batch(c, 4, seed=21)
    batch = {"spectre": s.to(dev), "spectrogram_len": lens.to(dev), "encoded_text": text.to(dev)}
    logits = m(batch)
    tgt = targets(text, c.eos_id)
    loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2), tgt.to(dev))
    loss.backward()
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    P = {k: v.double().requires_grad_(True) for k, v in N.det_params(c, 0).items()}
    ref = N.forward(P, s.double(), lens, text, c, True)
    ref_loss = torch.nn.functional.cross_entropy(ref.transpose(1, 2), tgt)
    ref_loss.backward()
    e = relerr(logits.detach(), ref.detach())
    ref_loss = ref_loss.detach()
    print(f"\nnew d256 4+4 fp32: logits rel err {e:.2e}, loss {float(loss.detach()):.6f} vs {float(ref_loss):.6f}")
    assert e < 1e-4, e
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-5 * abs(float(ref_loss))
    twin = asrx.new.Transformer(c.vocab_size, c.n_mels, c.enc_seq_len, c.dec_seq_len, c.hidden_dim, c.n_enc, c.n_dec,
                                c.n_heads, c.ff_dim, dev, dropout=0.0, sr=c.sr, n_fft=c.n_fft, padding_idx=c.pad_id,
                                eos_token=c.eos_id, bos_token=c.bos_id).to(dev)
    with torch.no_grad():
        for (k1, p1), (k2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert k1 == k2
            p2.copy_(p1.grad if p1.grad is not None else torch.zeros_like(p2))
    gsd = twin.state_dict()
    names = [k for k, v in P.items() if v.grad is not None]
    gmax = max(float(P[k].grad.abs().max()) for k in names)
    worst = 0.0
    for k in names:
        want = P[k].grad
        den = max(float(want.abs().max()), 1e-4 * gmax)
        err = float((gsd[k].double().cpu() - want).abs().max()) / den
        worst = max(worst, err)
        assert err < 1e-3, (k, err)
    print(f"{len(names)} gradients, worst {worst:.2e}")
