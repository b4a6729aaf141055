"""Transcripts beyond 255 labels through the public interface: asrx.CTCLoss, Transformer.align, the Trainer's hybrid
objective and asrx.ErrorRate take the `_long` entries where a width asks for them, and only there.

The model is a micro hybrid Transformer (1 + 1 layers, d 64) with decoder_seq_len 320 and encoder_seq_len 340 on 1350
spectrogram frames, so T' = 336 encoder frames carry transcripts of about 300 labels.  References: torch's CPU fp64
ctc_loss (tests/ctc_ref.py) under the rule of tests/test_gpu_ctc_kernels.py; tests/ctc_align_ref.py under its `bound`;
the host Levenshtein recursion of tests/test_gpu_edit_long_kernels.py; for the Trainer the project's loss tolerance of
1e-2 relative (tests/test_gpu_ctc_model.py) and bit equality between the eager and the captured step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_align_ref as R
from tests import ctc_ref
from tests.test_gpu_edit_long_kernels import long_align

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
V, F_IN, D, DEC, ENC, T_IN = 250, 80, 64, 320, 340, 1350
BOS, EOS, PAD = 1, 2, 4
W_CTC = 0.3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build(precision, seed=5):
    import asrx
    torch.manual_seed(seed)
    m = asrx.Transformer(V, F_IN, D, DEC, ENC, 1, 1, 4, 256, dropout=0.0, pad_token_id=PAD, eos_token_id=EOS,
                         precision=precision, ctc=True)
    return m.to(dev)


def transcript(n, seed):
    """n labels in [5, V) without adjacent repeats: they align in n frames."""
    g = torch.Generator().manual_seed(seed)
    out = []
    while len(out) < n:
        c = int(torch.randint(5, V, (1,), generator=g))
        if not out or c != out[-1]:
            out.append(c)
    return out


def text_batch(lens, width, seed):
    """(spectrum (B, 1, F, T), text (B, width) = BOS, labels, EOS, PAD ..., mask)."""
    g = torch.Generator().manual_seed(seed)
    spectrum = torch.randn(len(lens), 1, F_IN, T_IN, generator=g)
    text = torch.full((len(lens), width), PAD, dtype=torch.int64)
    for b, n in enumerate(lens):
        row = [BOS] + transcript(n, 10 * seed + b) + [EOS]
        text[b, :len(row)] = torch.tensor(row)
    return spectrum, text, (text != PAD).float()


def test_ctc_loss_module_with_300_columns():
    """Fails without the long entry: asrx.CTCLoss raises ValueError above 255 columns."""
    import asrx
    B, T, Vc, Lmax = 2, 700, 30, 300
    g = torch.Generator().manual_seed(1)
    tl = torch.tensor([300, 120], dtype=torch.int32)
    tg = torch.randint(1, Vc, (B, Lmax), generator=g)
    logits = torch.randn(B, T, Vc, generator=g)
    nll64, g64 = ctc_ref.ctc_reference(logits, tg, None, tl, 0, torch.float64)
    nll32, g32 = ctc_ref.ctc_reference(logits, tg, None, tl, 0, torch.float32)
    assert torch.isfinite(nll64).all()
    x = logits.to(dev).requires_grad_(True)
    loss = asrx.CTCLoss(blank=0, reduction="mean")(x, tg.to(dev), None, tl.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    w = ctc_ref.sample_weights(tl, B, "mean")
    want = float((nll64 * w).sum())
    rel = max(4 * float(((nll32.double() - nll64).abs() / nll64.abs()).max()), 1e-6)
    print(f"CTCLoss L300: loss {float(loss):.6f} reference {want:.6f} relative bound {rel:.2e}")
    assert abs(float(loss) - want) <= rel * abs(want) + 2e-7 * abs(want)
    wg, wg32 = g64 * w.view(-1, 1, 1), g32.double() * w.view(-1, 1, 1)
    tol = max(4 * float((wg32 - wg).abs().max()), 1e-6)
    err = float((x.grad.cpu().double() - wg).abs().max())
    print(f"CTCLoss L300: gradient error {err:.3g} bound {tol:.3g}")
    assert err <= tol


def test_align_a_300_label_transcript():
    """Fails without the long entry: the 300-label row scores -inf.  The path is valid and its fp64 score lies within
    `bound` of the reference optimum on the model's own CTC logits."""
    m = build("fp32")
    with torch.no_grad():
        m.ctc_head.weight.mul_(4.0)      # spread the frame posteriors
    m.eval()
    spectrum, text, _ = text_batch([300, 40], 302, seed=3)
    logits = m.ctc_logits(spectrum.to(dev)).float().cpu()
    Tp = logits.shape[1]
    assert Tp == 336 and text.shape[1] > 257
    a = m.align(spectrum.to(dev), text.to(dev))
    torch.cuda.synchronize()
    assert a.start.shape == (2, 302) and a.frame_pos.shape == (2, Tp)
    for b, n in enumerate((300, 40)):
        tr = text[b, 1:1 + n].tolist()
        assert int(a.target_lengths[b]) == n and a.targets[b, :n].tolist() == tr
        x = logits[b].numpy()
        r = R.viterbi(x, tr, m.ctc_blank, Tp, 302)
        r32 = R.viterbi(x, tr, m.ctc_blank, Tp, 302, dtype=np.float32)
        assert r["feasible"]
        err = abs(r["score"] - r32["score"])
        bound = R.bound(err, r["score"])
        pos = a.frame_pos[b].cpu().numpy()
        assert float(a.score[b]) > -INF
        assert R.path_is_valid(pos, tr, Tp)
        total, flp = R.rescore(x, tr, m.ctc_blank, pos, Tp)
        print(f"align sample {b}: L {n}, score {float(a.score[b]):.4f}, path in fp64 {total:.4f}, optimum "
              f"{r['score']:.4f}, bound {bound:.2e}")
        assert r["score"] - bound <= total <= r["score"] + 1e-9
        assert abs(float(a.score[b]) - total) <= bound
        ws, we, _ = R.spans_of(pos, flp, n, 302)
        assert a.start[b].tolist() == ws.tolist() and a.end[b].tolist() == we.tolist()


def _torch_joint(m, s, t, k, drop_long=False):
    """(1 - w) CE + w CTC_mean with torch (fp64, host) from the model's own decoder and CTC logits."""
    with torch.no_grad():
        dec = m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)).double().cpu()
        enc = m.ctc_logits(s.to(dev)).double().cpu()
    ce = F.cross_entropy(dec.transpose(1, 2), t[:, 1:])
    tg, tl = ctc_ref.targets_loop(t, k, (BOS, EOS, PAD), PAD)
    il = torch.full((t.shape[0],), enc.shape[1], dtype=torch.long)
    per = F.ctc_loss(F.log_softmax(enc, -1).transpose(0, 1), tg, il, tl.long(), blank=PAD, reduction="none")
    assert torch.isfinite(per).all()          # the condition on the inputs
    per = per / tl.clamp_min(1)
    if drop_long:
        per = torch.where(tl > 255, torch.zeros_like(per), per)
    return float((1 - W_CTC) * ce + W_CTC * per.mean())


def test_trainer_at_text_width_301_keeps_the_long_rows():
    """Fails without the long entry: the CTC term of the 299-label row is dropped by zero_infinity."""
    from asrx.train import Trainer
    m = build("fp32").train()
    s, t, k = text_batch([299, 150], 301, seed=7)
    tr = Trainer(m, ctc_weight=W_CTC, bos_token_id=BOS, graph=False)
    loss = float(tr.forward_backward(s.to(dev), t.to(dev), k.to(dev)))
    torch.cuda.synchronize()
    want, without = _torch_joint(m, s, t, k), _torch_joint(m, s, t, k, drop_long=True)
    print(f"trainer width 301: loss {loss:.6f}, torch {want:.6f}, without the long row's CTC term {without:.6f}")
    assert abs(want - without) > 5e-2 * abs(want)          # the inputs tell the two apart
    assert abs(loss - want) <= 1e-2 * abs(want)
    assert torch.isfinite(tr.store.grad).all() and float(m.ctc_head.weight.grad.abs().max()) > 0.0


def _run_steps(graph, steps=5):
    from asrx.train import Trainer
    m = build("bf16").train()
    data = [tuple(x.to(dev) for x in text_batch([299, 150], 301, seed=20 + i)) for i in range(steps)]
    tr = Trainer(m, lr=2e-3, weight_decay=0.01, graph=graph, ctc_weight=W_CTC, bos_token_id=BOS)
    losses = [float(tr.step(*b)) for b in data]
    torch.cuda.synchronize()
    return tr, losses


def test_trainer_graph_replay_equals_eager_at_width_301():
    """bf16, dropout 0, changing batches: the captured step, asrx_ctc_loss_long's four launches included, equals the
    eager step bit for bit (the comparison of tests/test_gpu_ctc_model.py)."""
    e, l0 = _run_steps(False)
    g, l1 = _run_steps(True)
    assert e._cap is None and g._cap is not None
    assert l0 == l1 and all(np.isfinite(l0))
    assert torch.equal(e.store.flat, g.store.flat) and torch.equal(e.m, g.m) and torch.equal(e.v, g.v)


@pytest.mark.parametrize("width,long", [(257, False), (258, True)])
def test_trainer_dispatch_by_text_width(width, long, monkeypatch):
    """Width 257 (BOS, 255 labels, EOS) is the step of before: asrx_ctc_loss and no `_long` entry.  258 takes
    asrx_ctc_loss_long and no asrx_ctc_loss.  Counted by wrapping the binding's call."""
    from asrx import _lib, kernels as K
    from asrx.train import Trainer
    names = []

    def counting(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(K, "call", counting)
    m = build("bf16").train()
    s, t, k = text_batch([width - 2, 100], width, seed=9)
    tr = Trainer(m, ctc_weight=W_CTC, bos_token_id=BOS, graph=False)
    loss = float(tr.forward_backward(s.to(dev), t.to(dev), k.to(dev)))
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    assert names.count("asrx_ctc_loss_long") == (1 if long else 0)
    assert names.count("asrx_ctc_loss") == (0 if long else 1)
    assert sum(n.endswith("_long") for n in names) == (1 if long else 0)


def test_error_rate_with_300_token_rows():
    """Fails without the long entry: ErrorRate.compute raises ValueError above 255 tokens."""
    import asrx
    rng = np.random.default_rng(8)
    hyp, ref = rng.integers(5, 12, size=(3, 300)), rng.integers(5, 12, size=(3, 310))
    hl, rl = [300, 256, 10], [310, 300, 0]
    er = asrx.ErrorRate(drop=(PAD,))
    er.update(torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev), torch.tensor(hl), torch.tensor(rl))
    er.update(torch.from_numpy(hyp[:, :200]).to(dev), torch.from_numpy(ref[:, :255]).to(dev))     # the short entry
    got = er.compute()
    want = [long_align(hyp[b, :hl[b]].tolist(), ref[b, :rl[b]].tolist()) for b in range(3)] + \
        [long_align(hyp[b, :200].tolist(), ref[b, :255].tolist()) for b in range(3)]
    assert got["n_edits"] == sum(w[0] for w in want) and got["n_sub"] == sum(w[1] for w in want)
    assert got["n_del"] == sum(w[2] for w in want) and got["n_ins"] == sum(w[3] for w in want)
    assert got["n_ref"] == sum(rl) + 3 * 255 and got["n_samples"] == 6
    d = asrx.edit_distance(torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev), torch.tensor(hl),
                           torch.tensor(rl))
    assert d.dist.tolist() == [w[0] for w in want[:3]] and d.sub.tolist() == [w[1] for w in want[:3]]
    # beyond the long bound the message names it
    er = asrx.ErrorRate(drop=())
    wide = torch.from_numpy(rng.integers(5, 12, size=(1, 4100))).to(dev)
    er.update(wide, wide)
    with pytest.raises(ValueError, match="sample 0 .*4095"):
        er.compute()
