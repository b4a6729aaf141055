"""Decode timing on the c3 decoder (12 layers, d 512, 8 heads), bf16: greedy `evaluate` against beam search.

    python tools/beam_bench.py [--beams 1,4,8] [--batch 8] [--te 249] [--steps 64] [--reps 5] [--no-greedy]

Times whole decode calls with device events (warm-up first, the variants interleaved) and prints one JSON line:
total ms and ms per step, median over the repetitions.  For the kernels' share run one variant alone under the
profiler and sum by kernel name (beam_step_kernel, gather_rows_kernel):

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \
        python tools/beam_bench.py --beams 4 --no-greedy --reps 1
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asr-transformer_amd")]

import torch  # noqa: E402

import asrx  # noqa: E402
from asrx.decode import _decoder_evaluate_cached  # noqa: E402
from oracle.ref_model import CONFIGS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="1,4,8")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--te", type=int, default=249)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-greedy", action="store_true")
    a = ap.parse_args()
    cfg = CONFIGS["c3"]["cfg"]
    torch.manual_seed(0)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision="bf16").cuda().eval()
    dec = m.decoder
    dec._seq_len = a.steps
    enc = torch.randn(a.batch, a.te, cfg.d_model, device="cuda")
    bos = torch.ones(a.batch, 1, dtype=torch.int64, device="cuda")
    variants = {}
    if not a.no_greedy:
        variants["greedy"] = lambda: _decoder_evaluate_cached(dec, bos, enc)
    for w in (int(x) for x in a.beams.split(",") if x):
        variants[f"beam{w}"] = lambda w=w: dec.beam_search(bos, enc, beam=w, max_len=a.steps, poll=0)
    times = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():          # warm-up: code objects, allocator pools
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
    out = {"batch": a.batch, "te": a.te, "steps": a.steps, "reps": a.reps}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"total_ms": round(med, 3), "ms_per_step": round(med / a.steps, 4),
                     "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
