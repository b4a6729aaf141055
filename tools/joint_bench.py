"""Decode timing of joint CTC/attention beam search on the c3 decoder (12 layers, d 512, 8 heads), bf16, against the
attention-only search of the same tree.

    python tools/joint_bench.py [--beams 4,8] [--lams 0,0.3] [--batch 8] [--te 249] [--steps 64] [--reps 7]
    python tools/joint_bench.py --prefix-only --te 999 [--beams 4,8,16]

Default: whole decodes timed with device events (warm-up first, the variants interleaved), one JSON line with the
median [min, max] total ms and ms per step of every (beam, ctc_weight) variant.  --prefix-only times the two per-step
prefix kernels alone (asrx_ctc_prefix_score, asrx_ctc_prefix_advance: 50 back-to-back launches between two events,
median of the repetitions, per launch) at any frame count, e.g. c5's T' = 999.  For per-launch times inside a decode
run one variant alone under the profiler and read prefix_score_kernel, prefix_advance_kernel and beam_step_kernel:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python tools/joint_bench.py --beams 8 --lams 0.3 --reps 1
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asr-transformer_amd")]

import torch  # noqa: E402

import asrx  # noqa: E402
from asrx import kernels as K  # noqa: E402
from oracle.ref_model import CONFIGS  # noqa: E402


def head_logits(B, T, V, Vp, blank):
    """Random fp32 head logits [B*T, Vp] that emit mostly blank, as a trained head does."""
    x = 2 * torch.randn(B * T, Vp, device="cuda")
    x[:, blank] += 5.0 + math.log(V)
    return x


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ts, per=1):
    return {"median": round(statistics.median(ts) / per, 4), "min": round(min(ts) / per, 4),
            "max": round(max(ts) / per, 4)}


def prefix_only(a, cfg):
    V, blank, eos, n = cfg.vocab_size, cfg.pad_id, cfg.eos_id, 50
    out = {"mode": "prefix-only", "batch": a.batch, "te": a.te, "reps": a.reps, "launches_per_rep": n, "unit": "us"}
    for W in (int(x) for x in a.beams.split(",") if x):
        R = a.batch * W
        pf = K.CtcPrefix(head_logits(a.batch, a.te, V, 256, blank), a.batch, W, a.te, V, blank)
        delta = torch.empty(R, 256, dtype=torch.float32, device="cuda")
        parent = torch.randint(0, W, (R,), device="cuda").to(torch.int32)
        tok = torch.randint(5, V, (R,), device="cuda")
        fin = torch.zeros(R, dtype=torch.uint8, device="cuda")
        for _ in range(3):                      # hypotheses of a few labels, not the root
            pf.advance(eos, parent, tok, fin)

        def scores():
            for _ in range(n):
                pf.score(eos, delta)

        def advances():
            for _ in range(n):
                pf.advance(eos, parent, tok, fin)

        scores(), advances()
        torch.cuda.synchronize()
        ts, ta = [], []
        for _ in range(a.reps):
            ts.append(timed(scores) * 1e3)
            ta.append(timed(advances) * 1e3)
        out[f"beam{W}"] = {"score_us": summary(ts, n), "advance_us": summary(ta, n)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--lams", default="0,0.3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--te", type=int, default=249)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prefix-only", action="store_true")
    a = ap.parse_args()
    cfg = CONFIGS["c3"]["cfg"]
    torch.manual_seed(0)
    if a.prefix_only:
        return prefix_only(a, cfg)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision="bf16", ctc=True).cuda().eval()
    dec = m.decoder
    dec._seq_len = a.steps
    enc = torch.randn(a.batch, a.te, cfg.d_model, device="cuda")
    bos = torch.ones(a.batch, 1, dtype=torch.int64, device="cuda")
    ctc = (head_logits(a.batch, a.te, cfg.vocab_size, m.ctc_head.Vp, m.ctc_blank), a.te, m.ctc_blank, None)
    variants = {}
    for w in (int(x) for x in a.beams.split(",") if x):
        for lam in (float(x) for x in a.lams.split(",") if x):
            variants[f"beam{w}_lam{lam:g}"] = lambda w=w, lam=lam: dec.beam_search(
                bos, enc, beam=w, max_len=a.steps, poll=0, ctc=ctc if lam > 0 else None, ctc_weight=lam)
    times = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():          # warm-up: code objects, allocator pools
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn))
    out = {"batch": a.batch, "te": a.te, "steps": a.steps, "reps": a.reps, "unit": "ms"}
    for name, ts in times.items():
        out[name] = {"total_ms": summary(ts), "ms_per_step": summary(ts, a.steps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
