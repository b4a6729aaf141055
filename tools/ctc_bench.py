"""CTC timing: asrx_ctc_loss against torch's own log_softmax + F.ctc_loss + backward, and the c3 training step with
and without the CTC term.

    python tools/ctc_bench.py [--reps 9] [--inner 10] [--no-step]

(a) asrx_ctc_loss alone (bf16 gradient, mean reduction, zero_infinity) at the c3 shape (B 64, T' 249, V 250, ld 256,
    target lengths U[20, 62]) and the c5 shape (B 16, T' 999, target lengths U[100, 254]): a captured graph of `inner`
    calls, replayed; ms per call.
(b) torch on the same device tensors: F.log_softmax + F.ctc_loss (lengths as host lists: no synchronisation) +
    backward to the logits, `inner` eager iterations between two device events (its kernels are long against the
    launch cost; (a) is also given in this eager form, `ours_eager`, for a like-for-like line).
(c) the c3 Trainer step (B 64, T 1000, bf16, dropout 0.1, graph replays) with ctc_weight 0 and 0.3 on one ctc=True
    model, and `new_launches`: the launches the CTC term adds to the step (head GEMM, asrx_ctc_targets, asrx_ctc_loss,
    head data-gradient GEMM; the head's weight gradient rides in the grouped launch) as a graph of their own.
Variants are interleaved; every figure is the median [min ... max] over --reps.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asr-transformer_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import asrx  # noqa: E402
from asrx import kernels as K  # noqa: E402
from oracle.ref_model import CONFIGS, synthetic_batch  # noqa: E402

dev = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def graphed(fn, inner):
    """fn() x inner captured once (after a warm-up call); returns the replay callable."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g.replay


def summary(ts, per=1):
    return {"ms": round(statistics.median(ts) / per, 4), "min": round(min(ts) / per, 4), "max": round(max(ts) / per, 4)}


def interleaved(variants, reps, per):
    times = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return {k: summary(v, per) for k, v in times.items()}


def loss_shape(name, B, T, V, ld, lo, hi, reps, inner):
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(B * T, ld)
    x[:, :V] = torch.randn(B * T, V, generator=g)
    x = x.to(dev)
    tl = torch.randint(lo, hi + 1, (B,), generator=g)
    tg = torch.randint(1, V, (B, hi), generator=g)
    tg_d, tl_d = tg.to(dev), tl.int().to(dev)
    xt = x.view(B, T, ld)[:, :, :V].detach().clone().requires_grad_(True)    # torch's own contiguous copy
    il_h, tl_h = [T] * B, tl.tolist()

    def ours():
        K.ctc_loss(x, V, T, tg_d, tl_d, max_target_len=hi, blank=0, reduction="mean", zero_infinity=True)

    def theirs():
        lp = F.log_softmax(xt, dim=-1).transpose(0, 1)
        loss = F.ctc_loss(lp, tg_d, il_h, tl_h, blank=0, reduction="mean", zero_infinity=True)
        torch.autograd.grad(loss, xt)

    replay = graphed(ours, inner)
    out = interleaved({"ours_graph": replay,
                       "ours_eager": lambda: [ours() for _ in range(inner)],
                       "torch_eager": lambda: [theirs() for _ in range(inner)]}, reps, inner)
    out["shape"] = dict(B=B, T=T, V=V, ld=ld, target_len=[lo, hi])
    return name, out


def step_delta(reps):
    from asrx.functions import make_ctx
    from asrx.train import Trainer
    spec = CONFIGS["c3"]
    cfg = spec["cfg"]
    torch.manual_seed(0)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.1, precision="bf16", ctc=True).to(dev).train()
    s, t, k = (x.to(dev) for x in synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=7))
    trainers = {"ctc_weight_0": Trainer(m, lr=1e-4, graph=True), "ctc_weight_0.3": Trainer(m, lr=1e-4, graph=True,
                                                                                         ctc_weight=0.3)}
    for tr in trainers.values():
        for _ in range(4):                     # eager warm-up steps, capture, one replay
            tr.step(s, t, k)
        assert tr._cap is not None
    variants = {name: (lambda tr=tr: tr.step(s, t, k)) for name, tr in trainers.items()}
    # the launches the CTC term adds, on tensors of the step's shapes
    B, Tp, d = spec["batch"], 249, cfg.d_model
    head = m.ctc_head
    C = make_ctx(m, 0.0)
    enc = torch.randn(B * Tp, d, device=dev).to(torch.bfloat16)
    denc = torch.randn(B * Tp, d, device=dev)
    ce = torch.ones(1, device=dev)

    def new_launches():
        logits = torch.empty(B * Tp, head.Vp, dtype=torch.float32, device=dev)
        K.linear(enc, C.W(head.weight), logits)
        tg, tl = K.ctc_targets(t, k, [1, cfg.eos_id, cfg.pad_id], m.ctc_blank)
        _, _, dl = K.ctc_loss(logits, head.V, Tp, tg, tl, max_target_len=min(tg.shape[1], 255), blank=m.ctc_blank,
                              reduction="mean", zero_infinity=True, grad_scale=0.3, loss_add=ce, loss_add_scale=0.7,
                              loss_scale=0.3)
        out = torch.empty_like(denc)
        K.linear_dgrad(dl, C.W(head.weight), out, resid=denc, ld_resid=d)

    variants["new_launches"] = graphed(new_launches, 1)
    return interleaved(variants, reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    out = {"reps": a.reps, "inner": a.inner}
    for args in (("c3", 64, 249, 250, 256, 20, 62), ("c5", 16, 999, 250, 256, 100, 254)):
        name, r = loss_shape(*args, a.reps, a.inner)
        out[name] = r
    if not a.no_step:
        out["c3_step"] = step_delta(a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
