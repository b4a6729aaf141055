"""The hybrid CTC/attention objective at model level (c1 dimensions unless stated): Trainer(ctc_weight=w) against the
oracle's autograd of (1 - w) * CE + w * F.ctc_loss(log_softmax(enc @ W_head^T)), the cross-entropy share of the
gradient, the captured and the fused-AdamW step with CTC on, the untouched default path, and best-path decoding.

Tolerances are test_gpu_train_parity.py's (GRAD_TOL / MAX_TOL per tensor through its check_grads, loss 1e-2
relative): imported, not restated."""
import pytest
import torch
import torch.nn.functional as F

from oracle.ref_model import CONFIGS, det_params, forward as oracle_forward, synthetic_batch
from tests import ctc_ref
from tests.test_gpu_train_parity import GRAD_TOL, MAX_TOL, check_grads, frorel, relerr

pytestmark = pytest.mark.gpu
dev = "cuda"
W_CTC = 0.3
BOS = 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build(name, precision, ctc, dropout=0.0, head_seed=11):
    import asrx
    cfg = CONFIGS[name]["cfg"]
    torch.manual_seed(head_seed)     # the head's initial values (every other parameter is overwritten below)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=dropout, precision=precision, ctc=ctc)
    sd = m.state_dict()
    sd.update(det_params(cfg, 0))
    m.load_state_dict(sd)
    return m.to(dev).train(), cfg


def batch(name, n=None, seed=2024):
    spec = CONFIGS[name]
    return synthetic_batch(spec["cfg"], n or spec["batch"], spec["frames"], spec["text_len"] + 1, seed=seed)


def grads_by_ref_key(m, cfg):
    """Gradients under the reference state_dict keys (+ ctc_head.weight): a twin's save hooks undo the packing."""
    import asrx
    twin = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=0.0, ctc=hasattr(m, "ctc_head"))
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.grad.cpu() if p1.grad is not None else torch.zeros_like(p2))
    return twin.state_dict()


def steady_grads(m, s, t, k, **kw):
    """Two forward_backward calls without an optimizer step (the second is the steady-state path)."""
    from asrx.train import Trainer
    tr = Trainer(m, **kw)
    tr.store.grad.fill_(float("nan"))
    tr.forward_backward(s.to(dev), t.to(dev), k.to(dev))
    tr.store.grad.fill_(float("nan"))
    loss = tr.forward_backward(s.to(dev), t.to(dev), k.to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(tr.store.grad).all()
    return float(loss), tr


def oracle_joint(cfg, head_w, s, t, k, w):
    """Loss and gradients of (1 - w) * CE + w * CTC_mean by the oracle's autograd (fp32, host)."""
    P = {kk: v.clone().requires_grad_(True) for kk, v in det_params(cfg, 0).items()}
    P["ctc_head.weight"] = head_w.detach().cpu().float().clone().requires_grad_(True)
    logits, enc = oracle_forward(P, s, t[:, :-1], k[:, :-1], cfg, False, return_encoder=True)
    ce = F.cross_entropy(logits.transpose(1, 2), t[:, 1:])
    tg, tl = ctc_ref.targets_loop(t, k, (BOS, cfg.eos_id, cfg.pad_id), cfg.pad_id)
    lp = F.log_softmax(F.linear(enc, P["ctc_head.weight"]), dim=-1).transpose(0, 1)
    il = torch.full((t.shape[0],), enc.shape[1], dtype=torch.long)
    per = F.ctc_loss(lp, tg, il, tl.long(), blank=cfg.pad_id, reduction="none")
    assert torch.isfinite(per).all(), "the batch must be feasible at T'"      # the condition on the inputs
    ctc = F.ctc_loss(lp, tg, il, tl.long(), blank=cfg.pad_id, reduction="mean", zero_infinity=True)
    loss = (1 - w) * ce + w * ctc
    loss.backward()
    return float(loss.detach()), float(ce.detach()), float(ctc.detach()), {kk: (v.grad.detach().clone() if v.grad is not None else None)
                                                for kk, v in P.items()}


def test_joint_loss_and_gradients_vs_oracle_fp32():
    m, cfg = build("c1", "fp32", ctc=True)
    s, t, k = batch("c1")
    assert (s.shape[-1] - 3) // 2 + 1 >= 3 and m.ctc_blank == cfg.pad_id
    loss, tr = steady_grads(m, s, t, k, ctc_weight=W_CTC)
    ref_loss, ce, ctc, ref = oracle_joint(cfg, m.ctc_head.weight[:cfg.vocab_size], s, t, k, W_CTC)
    print(f"\njoint loss {loss:.6f} oracle {ref_loss:.6f} (CE {ce:.4f}, CTC {ctc:.4f})")
    assert abs(loss - ref_loss) < 1e-2 * abs(ref_loss)
    gsd = grads_by_ref_key(m, cfg)
    names = [kk for kk, v in ref.items() if v is not None]
    assert "ctc_head.weight" in names
    check_grads(gsd, ref, names, "c1 fp32 joint")
    for kk, v in ref.items():
        if v is None:
            assert float(gsd[kk].abs().max()) == 0.0, kk
    # the padded rows of the head take no gradient
    V = cfg.vocab_size
    assert float(m.ctc_head.weight.grad[V:].abs().max()) == 0.0


def test_decoder_gradients_are_the_cross_entropy_share():
    """The decoder sees the CTC term only through the factor on CE: its gradients under ctc_weight w are (1 - w)
    times the ctc_weight = 0 run's."""
    m, cfg = build("c1", "fp32", ctc=True)
    s, t, k = batch("c1")
    _, tr = steady_grads(m, s, t, k, ctc_weight=0.0)
    g0 = {n: p.grad.detach().clone() for n, p in m.decoder.named_parameters()}
    enc0 = m.encoder._norm_out.weight.grad.detach().clone()
    assert float(m.ctc_head.weight.grad.abs().max()) == 0.0
    _, tr = steady_grads(m, s, t, k, ctc_weight=W_CTC)
    gmax = max(float(g.abs().max()) for g in g0.values())
    for n, p in m.decoder.named_parameters():
        want = g0[n] * (1 - W_CTC)
        if float(want.abs().max()) < 1e-6 * gmax:
            assert float((p.grad - want).abs().max()) < GRAD_TOL * 1e-2 * gmax, n
            continue
        assert frorel(p.grad, want) < GRAD_TOL and relerr(p.grad, want) < MAX_TOL, n
    # ... while the encoder also carries the head's data gradient
    assert frorel(m.encoder._norm_out.weight.grad, enc0 * (1 - W_CTC)) > 1e-3
    assert float(m.ctc_head.weight.grad.abs().max()) > 0.0


def _run_steps(name, n_batch, steps, graph, fused, monkeypatch, ctc_weight=W_CTC, wd=0.01):
    import asrx.train as T
    monkeypatch.setattr(T, "FUSED_ADAM", fused)
    m, cfg = build(name, "bf16", ctc=True)
    data = [tuple(x.to(dev) for x in batch(name, n_batch, seed=300 + i)) for i in range(steps)]
    tr = T.Trainer(m, lr=2e-3, weight_decay=wd, graph=graph, ctc_weight=ctc_weight)
    losses = [float(tr.step(*b)) for b in data]
    torch.cuda.synchronize()
    return tr, m, losses


def test_graph_replay_equals_eager_with_ctc(monkeypatch):
    """6 steps over changing batches, bf16, dropout 0: the captured step (CTC launches included: one chain, no new
    input buffer) equals the eager step bit for bit."""
    e, me, l0 = _run_steps("c1", None, 6, False, True, monkeypatch)
    g, mg, l1 = _run_steps("c1", None, 6, True, True, monkeypatch)
    assert e._cap is None and g._cap is not None
    assert len(g._cap[0].graphs) == 1
    assert l0 == l1
    assert torch.equal(e.store.flat, g.store.flat) and torch.equal(e.m, g.m) and torch.equal(e.v, g.v)
    assert not torch.equal(me.ctc_head.weight, build("c1", "bf16", ctc=True)[0].ctc_head.weight)   # the head trains


def test_fused_adam_equals_separate_adam_with_ctc(monkeypatch):
    """c3 dimensions at B = 2 (the grouped ws launch, as test_gpu_fused_adam.py): with the head's weight gradient in
    the grouped launch, fused and separate AdamW agree bit for bit, and the head's range is covered."""
    ref, _, l0 = _run_steps("c3", 2, 4, False, False, monkeypatch)
    tr, m, l1 = _run_steps("c3", 2, 4, False, True, monkeypatch)
    assert tr._cover and ref._cover is None
    assert tr.store.offset(m.ctc_head.weight) in {o for o, _ in tr._cover}
    assert l0 == l1
    for a, b in ((ref.store.flat, tr.store.flat), (ref.m, tr.m), (ref.v, tr.v), (ref.store.shadow, tr.store.shadow)):
        assert torch.equal(a, b)


def test_release_schedule_carries_the_head(monkeypatch):
    """Multi-GPU structure on one GPU (as test_gpu_graph.py's release test): an injected all-reduce that doubles
    each range it is handed.  With CTC on, every gradient — the head's, released with Encoder._norm_out, included —
    is reduced exactly once (twice the plain gradient), and the step captured in segments equals the eager one bit
    for bit."""
    from asrx import functions
    import asrx.train as T
    monkeypatch.setattr(functions, "RELEASE_LAYERS", 1)
    m, cfg = build("c1", "bf16", ctc=True)
    b = tuple(x.to(dev) for x in batch("c1", seed=41))
    plain = T.Trainer(m, lr=0.0, graph=False, ctc_weight=W_CTC)
    for _ in range(2):
        plain.step(*b)
    torch.cuda.synchronize()
    want = plain.store.grad.clone() * 2.0
    o, k = plain.store.offset(m.ctc_head.weight), m.ctc_head.weight.numel()
    assert float(want[o:o + k].abs().max()) > 0.0
    got = []
    for graph in (False, True):
        seen = []

        def fake(view):
            seen.append(view.numel())
            view.mul_(2.0)
        tr = T.Trainer(m, lr=0.0, allreduce_fn=fake, graph=graph, ctc_weight=W_CTC)
        for _ in range(4):
            seen.clear()
            tr.step(*b)
        torch.cuda.synchronize()
        assert (tr._cap is not None) == graph and len(seen) > 1
        if graph:
            assert len(tr._cap[0].graphs) > 1
        got.append(tr.store.grad.clone())
    assert torch.equal(got[0], got[1])
    # against the plain step the weight gradients are issued in other groups: fp32 rounding at most, per range
    for a, n in ((0, want.numel()), (o, k)):
        assert frorel(got[0][a:a + n], want[a:a + n]) < 1e-6, (a, n)


@pytest.mark.parametrize("graph", [False, True])
def test_default_path_is_untouched(graph, monkeypatch):
    """ctc=False, and ctc=True under ctc_weight = 0, after Trainer steps (weight decay on): loss, gradients,
    parameters and moments of the shared parameters are bit-identical; the head keeps its values and its m / v ranges
    stay zero (no gradient, no AdamW, no decay: the frozen mechanism)."""
    import asrx.train as T
    runs = []
    for ctc in (False, True):
        m, cfg = build("c1", "bf16", ctc=ctc)
        head0 = m.ctc_head.weight.detach().clone() if ctc else None
        data = [tuple(x.to(dev) for x in batch("c1", seed=500 + i)) for i in range(4)]
        tr = T.Trainer(m, lr=2e-3, weight_decay=0.01, graph=graph)
        losses = [float(tr.step(*b)) for b in data]
        torch.cuda.synchronize()
        assert (tr._cap is not None) == graph
        runs.append((m, tr, losses, head0))
    (m0, t0, l0, _), (m1, t1, l1, head0) = runs
    assert l0 == l1
    n = t0.store.flat.numel()
    assert t1.store.flat.numel() > n
    for a, b in ((t0.store.flat, t1.store.flat), (t0.store.grad, t1.store.grad), (t0.m, t1.m), (t0.v, t1.v)):
        assert torch.equal(a, b[:n])
    p0 = dict(m0.named_parameters())
    for name, p in m1.named_parameters():
        if name != "ctc_head.weight":
            assert torch.equal(p, p0[name]) and torch.equal(p.grad, p0[name].grad), name
    o, k = t1.store.offset(m1.ctc_head.weight), m1.ctc_head.weight.numel()
    assert o >= n
    assert torch.equal(m1.ctc_head.weight, head0)
    assert float(t1.m[o:o + k].abs().max()) == 0.0 and float(t1.v[o:o + k].abs().max()) == 0.0
    assert float(t1.store.grad[o:o + k].abs().max()) == 0.0


def test_ctc_greedy_equals_the_python_collapse():
    m, cfg = build("c1", "bf16", ctc=True)
    m.eval()
    s, t, k = batch("c1")
    logits = m.ctc_logits(s.to(dev))
    B, Tp, V = logits.shape
    assert (B, Tp, V) == (s.shape[0], 24, cfg.vocab_size) and logits.dtype == torch.float32
    tok, n = m.ctc_greedy(s.to(dev))
    assert tok.is_cuda and n.is_cuda and tok.dtype == torch.int64 and n.dtype == torch.int32
    want_tok, want_n = ctc_ref.greedy_loop(logits.cpu(), m.ctc_blank)
    assert torch.equal(tok.cpu(), want_tok) and torch.equal(n.cpu(), want_n)
    il = torch.tensor([24, 10, 0, 17])
    tok, n = m.ctc_greedy(s.to(dev), il.to(dev))
    want_tok, want_n = ctc_ref.greedy_loop(logits.cpu(), m.ctc_blank, il)
    assert torch.equal(tok.cpu(), want_tok) and torch.equal(n.cpu(), want_n)
    m0, _ = build("c1", "bf16", ctc=False)
    with pytest.raises(RuntimeError, match="ctc=True"):
        m0.ctc_logits(s.to(dev))
