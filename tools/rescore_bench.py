"""Decode timing of two-pass decoding (CTC prefix beam search + attention rescoring) on the c3 decoder (12 layers,
d 512, 8 heads), bf16, against the joint CTC/attention beam search of the same tree on the same box.

    python tools/rescore_bench.py [--beam 8] [--batch 8] [--te 249] [--steps 64] [--reps 7]
    python tools/rescore_bench.py --first-pass-only --te 999 [--beams 4,8,16] [--reps 3]

Default: whole decodes timed with device events (one warm-up, the variants interleaved), one JSON line with the median
[min, max] ms of
    joint     Decoder.beam_search(beam, ctc_weight=0.3), `steps` positions, poll=0
    rescore   Decoder.rescore(beam): first pass, one decoder forward over batch * beam rows of `steps` positions, rank
    ctc_beam  the first pass alone
each ending in its one host copy.  --first-pass-only launches asrx_ctc_prefix_beam alone for every beam of --beams;
for per-launch kernel times run it, and one default run, under the profiler in runs of their own and read
ctc_prefix_beam_kernel, hyp_tokens_kernel, seq_logprob_kernel and rescore_rank_kernel:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python tools/rescore_bench.py --first-pass-only --te 999 --beams 4,8,16 --reps 3
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
from asrx import decode  # noqa: E402
from asrx import kernels as K  # noqa: E402
from oracle.ref_model import CONFIGS  # noqa: E402
from tools.joint_bench import head_logits, summary, timed  # noqa: E402


def first_pass_only(a, cfg):
    V, blank = cfg.vocab_size, cfg.pad_id
    out = {"mode": "first-pass-only", "batch": a.batch, "te": a.te, "max_labels": a.steps - 1, "reps": a.reps,
           "unit": "ms"}
    x = head_logits(a.batch, a.te, V, 256, blank)
    for W in (int(v) for v in a.beams.split(",") if v):
        fn = lambda W=W: K.ctc_prefix_beam(x, V, a.te, blank, W, a.steps - 1)   # noqa: E731
        fn()
        torch.cuda.synchronize()
        out[f"beam{W}"] = summary([timed(fn) for _ in range(a.reps)])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--beams", default="4,8,16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--te", type=int, default=249)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--first-pass-only", action="store_true")
    a = ap.parse_args()
    cfg = CONFIGS["c3"]["cfg"]
    torch.manual_seed(0)
    if a.first_pass_only:
        return first_pass_only(a, cfg)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision="bf16", ctc=True).cuda().eval()
    dec = m.decoder
    dec._seq_len = a.steps
    enc = torch.randn(a.batch, a.te, cfg.d_model, device="cuda")
    bos = torch.ones(a.batch, 1, dtype=torch.int64, device="cuda")
    ctc = (head_logits(a.batch, a.te, cfg.vocab_size, m.ctc_head.Vp, m.ctc_blank), a.te, m.ctc_blank, None)
    W = a.beam
    variants = {
        "joint": lambda: dec.beam_search(bos, enc, beam=W, max_len=a.steps, poll=0, ctc=ctc, ctc_weight=0.3),
        "rescore": lambda: dec.rescore(enc, ctc, beam=W, max_len=a.steps),
        "ctc_beam": lambda: decode.decoder_ctc_beam_search(dec, ctc, a.batch, beam=W, max_len=a.steps),
    }
    times = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():          # warm-up: code objects, allocator pools
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn))
    out = {"batch": a.batch, "te": a.te, "steps": a.steps, "beam": W, "reps": a.reps, "unit": "ms"}
    for name, ts in times.items():
        out[name] = summary(ts)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
