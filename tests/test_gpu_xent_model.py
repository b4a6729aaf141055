"""Label-smoothed cross-entropy at model level, on micro configurations with vocabularies 250 (Vp 256) and 1500
(Vp 1536, beyond the old kernel's 1024): Trainer(label_smoothing=eps) against the oracle under
F.cross_entropy(label_smoothing=eps), eager against captured steps, the hybrid CTC objective, predictions and
statistics, the untouched default step, and asrx.CrossEntropyLoss in the reference-style loops of both families.

Tolerances: test_gpu_model.py's for the same comparison at eps = 0 (test_train_grads_micro: loss and every gradient
1e-3 relative at fp32, a mathematically zero gradient 1e-5 of the largest; loss 5e-2 at bf16); captured against eager
steps bit for bit, as test_gpu_graph.py; the module against torch 1e-5 on the loss and 1e-2 on the gradient."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from oracle.ref_model import CONFIGS, OracleConfig, det_params, forward as oracle_forward, synthetic_batch

pytestmark = pytest.mark.gpu
dev = "cuda"
CASES = [(250, 0.1), (1500, 0.0), (1500, 0.1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def config(vocab):
    cfg = dataclasses.replace(CONFIGS["micro"]["cfg"], vocab_size=vocab)
    assert isinstance(cfg, OracleConfig)
    return cfg


def build(cfg, precision, ctc=False):
    import asrx
    torch.manual_seed(11)            # the CTC head's initial values (every other parameter is overwritten below)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision=precision, ctc=ctc)
    sd = m.state_dict()
    sd.update(det_params(cfg, 0))
    m.load_state_dict(sd)
    return m.to(dev).train()


def batch(cfg, seed=2024, n=None):
    spec = CONFIGS["micro"]
    return synthetic_batch(cfg, n or spec["batch"], spec["frames"], spec["text_len"] + 1, seed=seed)


_ORACLE = {}


def oracle(cfg, eps):
    """Loss and gradients of the oracle model under F.cross_entropy(label_smoothing=eps), once per case."""
    key = (cfg.vocab_size, eps)
    if key not in _ORACLE:
        P = {k: v.clone().requires_grad_(True) for k, v in det_params(cfg, 0).items()}
        s, t, k = batch(cfg)
        logits = oracle_forward(P, s, t[:, :-1], k[:, :-1], cfg, False)
        loss = F.cross_entropy(logits.transpose(1, 2), t[:, 1:], label_smoothing=eps)
        loss.backward()
        _ORACLE[key] = (float(loss.detach()), {k: (v.grad.detach().clone() if v.grad is not None else None)
                                               for k, v in P.items()}, logits.detach())
    return _ORACLE[key]


def grads_by_ref_key(m, cfg):
    """Gradients under the reference state_dict keys: a twin's save hooks undo the packing."""
    import asrx
    twin = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=0.0)
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.grad.cpu() if p1.grad is not None else torch.zeros_like(p2))
    return twin.state_dict()


def record_calls(monkeypatch):
    from asrx import kernels as K
    calls = []
    real = K.call
    monkeypatch.setattr(K, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("vocab,eps", CASES)
def test_trainer_loss_and_gradients_vs_oracle_fp32(vocab, eps, monkeypatch):
    from asrx.train import Trainer
    cfg = config(vocab)
    m = build(cfg, "fp32")
    s, t, k = (x.to(dev) for x in batch(cfg))
    tr = Trainer(m, label_smoothing=eps, preds=True, graph=False)
    calls = record_calls(monkeypatch)
    tr.forward_backward(s, t, k)
    loss = float(tr.forward_backward(s, t, k))
    ref_loss, ref, ref_logits = oracle(cfg, eps)
    print(f"\nV {vocab} eps {eps}: loss {loss:.6f} oracle {ref_loss:.6f}")
    assert abs(loss - ref_loss) < 1e-3 * abs(ref_loss)
    # the new entry point, with fp32 gradients for the fp32 model (no cast of dlogits behind it)
    ce = [a for name, a in calls if name.startswith("asrx_cross_entropy")]
    assert [name for name, _ in calls if name.startswith("asrx_cross_entropy")] == ["asrx_cross_entropy_ls"] * 2
    from asrx._lib import F32
    assert ce[0][10] == F32 and abs(ce[0][6] - eps) < 1e-7 and ce[0][2] == vocab and ce[0][3] == (vocab + 63) // 64 * 64
    gsd = grads_by_ref_key(m, cfg)
    gmax = max(float(v.abs().max()) for v in ref.values() if v is not None)
    for key, want in ref.items():
        if want is None:
            assert float(gsd[key].abs().max()) == 0.0, key
        elif float(want.abs().max()) < 1e-6 * gmax:       # mathematically zero (test_gpu_model.py's rule)
            assert float((gsd[key].double() - want.double()).abs().max()) < 1e-3 * 1e-2 * gmax, key
        else:
            assert relerr(gsd[key], want) < 1e-3, key
    # predictions are the logits' argmax, the statistics those of the predictions
    B, L = t.shape[0], t.shape[1] - 1
    with torch.no_grad():
        logits = m(s, t[:, :-1], k[:, :-1])
    assert torch.equal(tr.last_preds.view(B, L), logits.argmax(-1))
    tgt = t[:, 1:].reshape(-1)
    stats = tr.last_stats
    assert stats.is_cuda and stats.shape == (2,) and stats.dtype == torch.float32
    acc = torch.tensor(float((tr.last_preds == tgt).sum()) / tgt.numel(), dtype=torch.float32)
    assert float(stats[1]) == float(acc)
    nll = F.cross_entropy(ref_logits.transpose(1, 2).double(), t[:, 1:].cpu())
    assert abs(float(stats[0]) - float(nll)) < 1e-3 * float(nll)


@pytest.mark.parametrize("vocab,eps", CASES)
def test_trainer_bf16_eager_and_captured_steps(vocab, eps):
    """bf16: the loss within test_gpu_model.py's bf16 bound of the oracle's; 6 steps of a graph-mode trainer (its eager
    warm-up steps, the capture, replays; eps is a launch constant of the captured rows launch) give the losses,
    parameters, predictions and statistics of 6 eager ones."""
    from asrx.train import Trainer
    cfg = config(vocab)
    data = [tuple(x.to(dev) for x in batch(cfg, seed=100 + i)) for i in range(6)]
    first = tuple(x.to(dev) for x in batch(cfg))
    loss = float(Trainer(build(cfg, "bf16"), label_smoothing=eps, graph=False).forward_backward(*first))
    ref_loss = oracle(cfg, eps)[0]
    print(f"\nV {vocab} eps {eps} bf16: loss {loss:.6f} oracle {ref_loss:.6f}")
    assert abs(loss - ref_loss) < 5e-2 * abs(ref_loss)
    runs = []
    for graph in (False, True):
        m = build(cfg, "bf16")
        tr = Trainer(m, lr=1e-3, graph=graph, label_smoothing=eps, preds=True)
        losses, stats, preds = [], [], []
        for b in data:
            losses.append(float(tr.step(*b)))
            stats.append(tr.last_stats.tolist())
            preds.append(tr.last_preds.clone())
        torch.cuda.synchronize()
        assert (tr._cap is not None) == graph
        runs.append((tr.store.flat.clone(), losses, stats, preds))
    assert runs[0][1] == runs[1][1]
    assert runs[0][2] == runs[1][2]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(set(runs[0][1])) == 6


def test_hybrid_ctc_objective_is_the_weighted_sum():
    """ctc_weight 0.3, eps 0.1, fp32: the step's loss is 0.7 * CE_ls + 0.3 * CTC with CE_ls the smoothed
    cross-entropy of the model's logits (torch) and CTC torch's F.ctc_loss on the model's CTC head, each computed on
    its own.  Bound 1e-4 relative: both terms are fp32 sums of a few hundred terms (~1e-6), and torch's log-softmax
    and CTC recursion round differently from the kernels' at that level."""
    from asrx import kernels as K
    from asrx.train import Trainer
    cfg = config(1500)
    m = build(cfg, "fp32", ctc=True)
    s, t, k = (x.to(dev) for x in batch(cfg))
    tr = Trainer(m, ctc_weight=0.3, label_smoothing=0.1, graph=False)
    loss = float(tr.forward_backward(s, t, k))
    assert tr.last_stats is not None
    with torch.no_grad():
        logits = m(s, t[:, :-1], k[:, :-1])
        ce = float(F.cross_entropy(logits.transpose(1, 2).double(), t[:, 1:], label_smoothing=0.1))
        cl = m.ctc_logits(s).double()
        tg, tl = K.ctc_targets(t, k, tr._ctc_drop, m.ctc_blank)
        il = torch.full((t.shape[0],), cl.shape[1], dtype=torch.long)
        ctc = float(F.ctc_loss(F.log_softmax(cl, -1).transpose(0, 1).cpu(), tg.cpu(), il, tl.cpu().long(),
                               blank=m.ctc_blank, reduction="mean", zero_infinity=True))
    want = 0.7 * ce + 0.3 * ctc
    print(f"\nhybrid loss {loss:.6f} = 0.7 * {ce:.6f} + 0.3 * {ctc:.6f} = {want:.6f}")
    assert ctc > 0 and abs(loss - want) < 1e-4 * abs(want)
    # and the smoothing reaches the decoder through the (1 - w) factor on CE alone: w = 0 gives CE_ls itself
    plain = float(Trainer(m, label_smoothing=0.1, graph=False).forward_backward(s, t, k))
    assert abs(plain - ce) < 1e-4 * abs(ce)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_step_keeps_the_old_entry_point(precision, monkeypatch):
    """Trainer(label_smoothing=0) on a V = 250 model: asrx_cross_entropy, never the new entry; no statistics."""
    from asrx.train import Trainer
    cfg = config(250)
    m = build(cfg, precision)
    s, t, k = (x.to(dev) for x in batch(cfg))
    calls = record_calls(monkeypatch)
    for tr in (Trainer(m, graph=False), Trainer(m, label_smoothing=0.0, graph=False, preds=True)):
        del calls[:]
        tr.step(s, t, k)
        tr.step(s, t, k)
        names = [name for name, _ in calls if "cross_entropy" in name or "xent" in name]
        assert names == ["asrx_cross_entropy"] * 2
        assert tr.last_stats is None
    with pytest.raises(ValueError):
        Trainer(m, label_smoothing=1.0)
    with pytest.raises(ValueError):
        Trainer(m, label_smoothing=-0.1)


@pytest.mark.parametrize("vocab", [250, 1500])
@pytest.mark.parametrize("ignore_index,eps", [(-100, 0.1), (4, 0.1), (-100, 0.0)])
def test_module_on_views_copies_and_rows(vocab, ignore_index, eps, monkeypatch):
    """asrx.CrossEntropyLoss on the reference-style transposed view of the model's (B, L, Vp)[:, :, :V] output (read in
    place: ld = Vp), on a contiguous (N, V, L) copy (ld = V) and on its (rows, V) view: one loss, one gradient,
    torch's."""
    import asrx
    cfg = config(vocab)
    m = build(cfg, "fp32")
    s, t, k = (x.to(dev) for x in batch(cfg))
    with torch.no_grad():
        out = m(s, t[:, :-1], k[:, :-1])                      # (B, L, V), a view of the padded buffer
    B, L, V = out.shape
    Vp = (V + 63) // 64 * 64
    assert out.stride() == (L * Vp, Vp, 1)
    tgt = t[:, 1:]
    assert int((tgt == 4).sum()) > 0
    ce = asrx.CrossEntropyLoss(ignore_index=ignore_index, label_smoothing=eps)
    ref = torch.nn.CrossEntropyLoss(ignore_index=ignore_index, label_smoothing=eps)
    xr = out.detach().double().requires_grad_(True)
    want = ref(xr.transpose(1, 2), tgt)
    want.backward()
    calls = record_calls(monkeypatch)
    got = []
    for form in ("view", "copy", "rows"):
        x = out.detach().requires_grad_(True)
        if form == "view":
            loss = ce(x.transpose(1, 2), tgt)
        elif form == "copy":
            loss = ce(x.transpose(1, 2).contiguous(), tgt)
        else:
            loss = ce(x.reshape(B * L, V), tgt.reshape(-1))
        (3.0 * loss).backward()
        got.append((float(loss.detach()), x.grad.clone() / 3.0, ce.last_stats.tolist()))
    lds = [a[3] for name, a in calls if name == "asrx_cross_entropy_ls"]
    assert lds == [Vp, V, Vp]
    for lo, g, st in got:
        assert abs(lo - float(want)) < 1e-5 * abs(float(want))
        assert relerr(g, xr.grad) < 1e-2
        assert abs(lo - got[0][0]) <= 1e-6 * abs(lo) and st[1] == got[0][2][1]
        assert abs(st[0] - got[0][2][0]) <= 1e-6 * abs(st[0])
        assert relerr(g, got[0][1]) < 1e-6                    # (the scalar and the 16-B path round alike)
    nll = torch.nn.functional.cross_entropy(xr.detach().transpose(1, 2), tgt, ignore_index=ignore_index)
    assert abs(got[0][2][0] - float(nll)) < 1e-5 * float(nll)
    # under no_grad there is no gradient and nothing to save
    with torch.no_grad():
        assert abs(float(ce(out.transpose(1, 2), tgt)) - float(want)) < 1e-5 * abs(float(want))


def test_reference_style_train_epoch_of_both_families():
    """train_epoch of asrx (vocabulary 1500) and of asrx.new, with asrx.CrossEntropyLoss(label_smoothing=0.1) where
    the recipes pass nn.CrossEntropyLoss: the same epoch loss as with torch's module, from the same initial weights."""
    import asrx
    import asrx.new
    from asrx.train import eval_epoch, train_epoch
    from oracle import ref_model_new as N
    cfg = config(1500)
    data = []
    for i in range(2):
        s, t, k = batch(cfg, seed=300 + i)
        data.append({"spectrum": s, "text": t, "mask": k})
    losses = []
    for lf in (torch.nn.CrossEntropyLoss(label_smoothing=0.1), asrx.CrossEntropyLoss(label_smoothing=0.1)):
        m = build(cfg, "fp32")
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        val, _ = eval_epoch(m, data, cfg.eos_id, 1, lf, dev)      # (before training: the same weights for both)
        metrics, _, _ = train_epoch(m, data, lf, opt, dev)
        losses.append((metrics["Train Loss"], val["Val Loss"]))
    print(f"\nasrx train/val loss: torch {losses[0]}, asrx {losses[1]}")
    assert abs(losses[0][0] - losses[1][0]) < 1e-4 * losses[0][0]
    assert abs(losses[0][1] - losses[1][1]) < 1e-4 * losses[0][1]

    class Tok:
        eos_token_id = 2

        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join(str(int(t)) for t in row if not (skip_special_tokens and int(t) < 5)) for row in ids]

    c = N.NEW_CONFIGS["new_micro"]
    tok = Tok()
    spectre, lens, text = N.synthetic_batch(c, 4, seed=10)
    true = torch.full_like(text, c.eos_id)
    true[:, :-1] = text[:, 1:]
    loader = [{"spectre": spectre, "spectrogram_len": lens, "encoded_text": text, "text_len": lens,
               "true_text": true, "text": tok.batch_decode(true)}]
    losses = []
    for lf in (torch.nn.CrossEntropyLoss(label_smoothing=0.1), asrx.CrossEntropyLoss(label_smoothing=0.1)):
        torch.manual_seed(5)
        m = asrx.new.Transformer(c.vocab_size, c.n_mels, c.enc_seq_len, c.dec_seq_len, c.hidden_dim, c.n_enc, c.n_dec,
                                 c.n_heads, c.ff_dim, "cuda", dropout=0.0, sr=c.sr, n_fft=c.n_fft,
                                 padding_idx=c.pad_id, eos_token=c.eos_id, bos_token=c.bos_id).cuda()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
        before = [p.detach().clone() for p in m.parameters()]
        vm, _ = asrx.new.eval_epoch(m, loader, tok, lf, "cuda")
        metrics, _ = asrx.new.train_epoch(m, loader, tok, lf, opt, sched, "cuda")
        assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
        losses.append((metrics["Train Loss"], vm["Val Loss"]))
    print(f"asrx.new train/val loss: torch {losses[0]}, asrx {losses[1]}")
    assert abs(losses[0][0] - losses[1][0]) < 1e-4 * losses[0][0]
    assert abs(losses[0][1] - losses[1][1]) < 1e-4 * abs(losses[0][1])
    assert lf.last_stats is not None and lf.last_stats.shape == (2,)
