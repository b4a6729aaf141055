"""Gradient parity of the bf16 training path the c3 bench actually runs (asrx.train.Trainer: fused resident-K/V
attention forward/backward at d_head = 64, grouped weight-gradient GEMMs written with beta = 0 into unzeroed
buffers (FreshGrads), fused conv2-dgrad + conv1-wgrad) against the reference's own gradients (golden fixtures
at d_head = 64, tests/golden/make_golden.py) and against the oracle's autograd at the c2 / c3 model dims.

Reference step: train.py:28-34 (forward, CE over text[:, 1:], backward); model.py:194-198.

Tolerances (bf16 operands, fp32 accumulation; the fp32 reference path is the comparator):
  * per-parameter gradient: relative error in the Frobenius norm ||g - ref|| / ||ref|| <= 5e-2 (GRAD_TOL), and
    in the max norm max|g - ref| / max|ref| <= 1.5e-1 (MAX_TOL).  The max norm is looser because bf16 rounding of
    the FFN pre-activations flips individual ReLU gates near zero, and each flip moves one row of dpre by a whole
    upstream-gradient value (the worst tensors are the FFN squeeze weight gradients);
  * gradients that are mathematically zero (the attention K bias: softmax is invariant to a per-query shift of
    the scores) hold only rounding noise in the reference: they must match in absolute terms at the scale of the
    largest gradient (<= GRAD_TOL * 1e-2 * global max);
  * at the c2 / c3 model dims (6 + 6 and 12 + 12 layers) the oracle also runs under torch's bf16 autocast (the
    reference's own bf16 path): a tensor may exceed GRAD_TOL only while its error stays within 1.5x
    (BF16_FACTOR) of that path's error against fp32, in both norms;
  * loss <= 1e-2 relative.
"""
import os

import numpy as np
import pytest
import torch

from oracle.ref_model import CONFIGS, det_params, synthetic_batch, train_step_grads
from tests.golden_io import load_golden

pytestmark = pytest.mark.gpu
dev = "cuda"
GRAD_TOL = 5e-2
MAX_TOL = 1.5e-1
BF16_FACTOR = 1.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def frorel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build(name, dropout=0.0):
    import asrx
    cfg = CONFIGS[name]["cfg"]
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=dropout, precision="bf16", attention="fused")
    sd = m.state_dict()
    sd.update(det_params(cfg, 0))
    m.load_state_dict(sd)
    assert cfg.d_model // cfg.n_heads == 64, "these tests pin the d_head = 64 (resident / tiled) kernels"
    return m.to(dev).train(), cfg


def ref_key_grads(m, cfg):
    """Gradients of the asrx model under the reference state_dict keys (the twin module's load/save hooks undo
    the fused Q/K/V packing, the lin_in column permutation and the classifier padding)."""
    import asrx
    twin = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=0.0)
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.grad.cpu() if p1.grad is not None else torch.zeros_like(p2))
    return twin.state_dict()


def trainer_grads(m, s, t, k):
    """Two Trainer.forward_backward calls without an optimizer step: the first binds / zeroes the flat gradient
    buffer, the second runs the steady-state path (Linear-weight gradients unzeroed, written with beta = 0)."""
    from asrx.train import Trainer
    tr = Trainer(m)
    tr.store.grad.fill_(float("nan"))
    tr.forward_backward(s, t, k)
    tr.store.grad.fill_(float("nan"))        # stale values must never leak into the steady-state gradients
    loss = tr.forward_backward(s, t, k)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.store.grad).all()
    return float(loss), tr


def check_grads(gsd, ref, names, label, ref_bf16=None):
    """ref_bf16 (optional): the same reference computed under bf16 autocast — the reference's own bf16 path.  A
    tensor whose error exceeds GRAD_TOL still passes if it is within BF16_FACTOR x that path's own error in the
    same norm (deep stacks: the bf16 rounding of 24 layers of activations, not this build, sets the floor)."""
    gmax = max(float(torch.as_tensor(ref[k]).abs().max()) for k in names)
    worst = []
    for key in names:
        r = torch.as_tensor(ref[key])
        if float(r.abs().max()) < 1e-6 * gmax:
            err = float((gsd[key].double() - r.double()).abs().max())
            assert err < GRAD_TOL * 1e-2 * gmax, (label, key, err)
            continue
        e, em = frorel(gsd[key], r), relerr(gsd[key], r)
        tol, mtol = GRAD_TOL, MAX_TOL
        if ref_bf16 is not None:
            tol = max(tol, BF16_FACTOR * frorel(ref_bf16[key], r))
            mtol = max(mtol, BF16_FACTOR * relerr(ref_bf16[key], r))
        worst.append((e, em, tol, key))
        assert e < tol and em < mtol, (label, key, e, em, tol, mtol)
    worst.sort(reverse=True)
    print(f"\n{label}: {len(worst)} gradients, worst rel err (frobenius / max / allowed frobenius) " +
          ", ".join(f"{k} {e:.2e}/{em:.2e}/{t:.2e}" for e, em, t, k in worst[:4]))


@pytest.mark.parametrize("name", ["g64", "g64l"])
def test_trainer_grads_vs_reference_golden(golden_dir, name):
    """g64: T' = 49 -> resident-K/V attention kernels; g64l: T' = 274 -> tiled attention kernels (encoder self and
    cross attention).  Full gradient tensors from the reference itself (norms where the fixture holds only those)."""
    g = load_golden(golden_dir, f"grads_{name}.npz")
    m, cfg = build(name)
    s, t, k = (torch.from_numpy(g[x]).to(dev) for x in ("spectrum", "text", "mask"))
    loss, _ = trainer_grads(m, s, t, k)
    assert abs(loss - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    gsd = ref_key_grads(m, cfg)
    full = [n for n in g["grad_names"] if "grad/" + n in g.files]
    check_grads(gsd, {n: g["grad/" + n] for n in full}, full, name)
    gmax = max(float(x) for x in g["grad_norms"])
    for key, n in zip(g["grad_names"], g["grad_norms"]):
        gn = float(gsd[key].double().norm())
        assert abs(gn - n) <= GRAD_TOL * n + 1e-4 * gmax, (key, gn, n)
    for key in g["nograd_names"]:
        assert float(gsd[key].abs().max()) == 0.0, key


@pytest.mark.parametrize("name,batch,frames", [("c2", 4, 512), ("c3", 2, 1000)])
def test_trainer_grads_vs_oracle(name, batch, frames):
    """The c2 (d256 h4, 6+6) and c3 (d512 h8, 12+12, T = 1000) model dims: every parameter gradient of the bf16
    Trainer step vs the oracle's fp32 autograd on the host."""
    m, cfg = build(name)
    spec = CONFIGS[name]
    s, t, k = synthetic_batch(cfg, batch, frames, spec["text_len"] + 1, seed=2024)
    loss, _ = trainer_grads(m, s.to(dev), t.to(dev), k.to(dev))
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    P = {kk: v.clone().requires_grad_(True) for kk, v in det_params(cfg, 0).items()}
    ref_loss, ref = train_step_grads(P, s, t, k, cfg, training=False)
    assert abs(loss - float(ref_loss)) < 1e-2 * abs(float(ref_loss))
    P16 = {kk: v.clone().requires_grad_(True) for kk, v in det_params(cfg, 0).items()}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        _, ref16 = train_step_grads(P16, s, t, k, cfg, training=False)
    gsd = ref_key_grads(m, cfg)
    names = [kk for kk, v in ref.items() if v is not None]
    check_grads(gsd, ref, names, name, ref_bf16=ref16)
    for kk, v in ref.items():
        if v is None:
            assert float(gsd[kk].abs().max()) == 0.0, kk


def test_trainer_c3_full_batch_properties():
    """c3 at the bench's full size (B = 64, T = 1000, dropout 0.1): gradients finite, the unzeroed (FreshGrads) step
    equal bit for bit to a whole-buffer-zero step, and 5 fused AdamW steps on one batch drive the loss down."""
    from asrx.train import Trainer
    m, cfg = build("c3", dropout=0.1)
    spec = CONFIGS["c3"]
    s, t, k = synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=77)
    s, t, k = s.to(dev), t.to(dev), k.to(dev)
    tr = Trainer(m, lr=3e-4)
    tr.forward_backward(s, t, k)                 # binds and zeroes
    torch.manual_seed(5)
    tr.forward_backward(s, t, k)                 # unzeroed Linear-weight gradients, beta = 0
    g_fresh = tr.store.grad.clone()
    assert torch.isfinite(g_fresh).all()
    wonly, tr._wonly = tr._wonly, []
    torch.manual_seed(5)
    tr.forward_backward(s, t, k)                 # whole-buffer zero, same dropout masks
    assert torch.equal(g_fresh, tr.store.grad)
    tr._wonly = wonly
    losses = [float(tr.step(s, t, k)) for _ in range(5)]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


def _plan_log(fn):
    """Run fn() with a KernelProbe that logs every GEMM launch (kernel instantiation, m, n, k, batch, splitk)."""
    from asrx import kernels as K
    probe = K.KernelProbe(target="", log=[])
    probe.active = True
    K.PROBE = probe
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        K.PROBE = None
    return out, probe.log


def _assert_bench_plan(log, rows):
    """The GEMM kernels of a c3 step at B = 64 (bench.py's workload): the wide encoder projections (FFN1 forward,
    the gated FFN2 data gradient, the Q/K/V projection forward, the all-layer cross K/V) on the warp-specialised
    kernel family p4 (FFN) / ws (Q/K/V), every 512-wide encoder output on the ws kernel, the weight gradients in one
    grouped ws launch."""
    by_shape = {}
    for name, m, n, k, *_ in log:
        by_shape.setdefault((m, n, k), set()).add(name.split("<")[0])
    fam = {nm for names in by_shape.values() for nm in names}
    assert by_shape[(rows, 2048, 512)] == {"gemm_bf16_p4_kernel"}, by_shape[(rows, 2048, 512)]   # FFN1 fwd + FFN2 dX
    assert by_shape[(rows, 1536, 512)] == {"gemm_bf16_ws_kernel"}, by_shape[(rows, 1536, 512)]   # Q/K/V fwd
    for kk in (512, 1216, 1536, 2048):                                                          # N = 512 outputs
        assert by_shape[(rows, 512, kk)] <= {"gemm_bf16_ws_kernel"}, (kk, by_shape[(rows, 512, kk)])
    assert fam & {"gemm_bf16_wsg_kernel", "gemm_bf16_wsgq_kernel", "gemm_bf16_wsgqa_kernel"}, fam


def test_trainer_grads_vs_oracle_bench_batch():
    """The bench's GEMM plan pinned at model level: c3 at B = 64, T = 1000 (15 936 encoder rows, the exact kernel
    plan bench.py times — asserted from the launch log), dropout 0: every parameter gradient and the loss of the
    steady-state bf16 Trainer step vs the oracle's fp32 autograd (GRAD_TOL / MAX_TOL, or within BF16_FACTOR of the
    reference's own bf16-autocast path), and the teacher-forced bf16 forward vs the oracle's fp32 forward."""
    m, cfg = build("c3")
    spec = CONFIGS["c3"]
    B = spec["batch"]
    s, t, k = synthetic_batch(cfg, B, spec["frames"], spec["text_len"] + 1, seed=2025)
    (loss, _), log = _plan_log(lambda: trainer_grads(m, s.to(dev), t.to(dev), k.to(dev)))
    rows = B * 249
    _assert_bench_plan(log, rows)
    gsd = ref_key_grads(m, cfg)
    m.eval()
    with torch.no_grad():
        logits, flog = _plan_log(lambda: m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)).cpu())
    assert {nm.split("<")[0] for nm, mm, n, kk, *_ in flog if (mm, n) == (rows, 512)} <= {"gemm_bf16_ws_kernel"}
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    P = {kk: v.clone().requires_grad_(True) for kk, v in det_params(cfg, 0).items()}
    ref_loss, ref = train_step_grads(P, s, t, k, cfg, training=False)
    assert abs(loss - float(ref_loss)) < 1e-2 * abs(float(ref_loss))
    P16 = {kk: v.clone().requires_grad_(True) for kk, v in det_params(cfg, 0).items()}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        _, ref16 = train_step_grads(P16, s, t, k, cfg, training=False)
    names = [kk for kk, v in ref.items() if v is not None]
    check_grads(gsd, ref, names, "c3 B=64", ref_bf16=ref16)
    del P, P16, ref, ref16
    from tests.bf16_check import check_bf16_forward
    check_bf16_forward(logits, det_params(cfg, 0), s, t[:, :-1], k[:, :-1], cfg, "c3 B=64")
