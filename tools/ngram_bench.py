"""Decode timing of n-gram LM shallow fusion on the c3 decoder (12 layers, d 512, 8 heads), bf16, against the same
search without the LM (lm=None issues exactly the launches of a build without the feature: that is the baseline).

    python tools/ngram_bench.py [--beams 4,8] [--lams 0,0.3] [--batch 8] [--te 249] [--steps 64] [--reps 7]
    python tools/ngram_bench.py --kernels-only [--beams 4,8] [--vocab 250,5400,16384]

Default: whole decodes timed with device events (warm-up first, the variants interleaved within every repetition), one
JSON line with the median [min, max] total ms and ms per step of every (beam, ctc_weight, lm on / off) variant.
--kernels-only times the three kernels alone (asrx_ngram_score, asrx_ngram_advance, asrx_ngram_seq_logprob: 50
back-to-back launches between two events, median of the repetitions, per launch).  For per-launch times inside a
decode run one variant alone under the profiler and read ngram_score_kernel, ngram_advance_kernel, ngram_seq_kernel:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python tools/ngram_bench.py --beams 8 --lams 0.3 --reps 1 --lm-only

The LM is NgramLM.estimate (order 3) over random token sequences: 400 sequences of 5 .. 30 tokens."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asr-transformer_amd"), os.path.join(REPO, "tools")]

import torch  # noqa: E402

import asrx  # noqa: E402
from asrx import kernels as K  # noqa: E402
from joint_bench import head_logits, summary, timed  # noqa: E402
from oracle.ref_model import CONFIGS  # noqa: E402


def make_lm(V, order, bos, eos, pad, n_seq=400):
    g = torch.Generator().manual_seed(0)
    ids = [v for v in range(V) if v not in (bos, eos, pad)]
    seqs = []
    for _ in range(n_seq):
        L = int(torch.randint(5, 31, (1,), generator=g))
        seqs.append([ids[i] for i in torch.randint(0, min(len(ids), 200), (L,), generator=g).tolist()])
    return asrx.NgramLM.estimate(seqs, order, V, bos_id=bos, eos_id=eos, exclude=(pad,)).to("cuda")


def kernels_only(a):
    n = 50
    out = {"mode": "kernels-only", "batch": a.batch, "order": a.order, "reps": a.reps, "launches_per_rep": n,
           "unit": "us"}
    for V in (int(x) for x in a.vocab.split(",") if x):
        lm = make_lm(V, a.order, 1, 2, 4)
        for W in (int(x) for x in a.beams.split(",") if x):
            R = a.batch * W
            st = K.NgramState(lm, a.batch, W)
            extra = torch.empty(R, V + 6, dtype=torch.float32, device="cuda")
            delta = torch.randn(R, V + 6, device="cuda")
            parent = torch.randint(0, W, (R,), device="cuda").to(torch.int32)
            tok = torch.randint(5, min(V, 200), (R,), device="cuda")
            fin = torch.zeros(R, dtype=torch.uint8, device="cuda")
            tgt = torch.randint(5, min(V, 200), (R, 64), device="cuda")
            for _ in range(3):                      # hypotheses of a few tokens, not the root
                st.advance(2, parent, tok, fin)

            def scores():
                for _ in range(n):
                    st.score(extra, delta, 0.3, 0.5, 0.0)

            def advances():
                for _ in range(n):
                    st.advance(2, parent, tok, fin)

            def seqs():
                for _ in range(n):
                    K.ngram_seq_logprob(lm, tgt, -1)

            fns = (scores, advances, seqs)
            for f in fns:
                f()
            torch.cuda.synchronize()
            ts = [[] for _ in fns]
            for _ in range(a.reps):
                for t, f in zip(ts, fns):
                    t.append(timed(f) * 1e3)
            out[f"V{V}_beam{W}"] = {"score_us": summary(ts[0], n), "advance_us": summary(ts[1], n),
                                    "seq_logprob_L64_us": summary(ts[2], n)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--lams", default="0,0.3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--te", type=int, default=249)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--vocab", default="250,5400,16384")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--lm-only", action="store_true", help="run the variants with the LM only (profiler runs)")
    a = ap.parse_args()
    cfg = CONFIGS["c3"]["cfg"]
    torch.manual_seed(0)
    if a.kernels_only:
        return kernels_only(a)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision="bf16", ctc=True).cuda().eval()
    dec = m.decoder
    dec._seq_len = a.steps
    lm = make_lm(cfg.vocab_size, a.order, 1, cfg.eos_id, cfg.pad_id)
    enc = torch.randn(a.batch, a.te, cfg.d_model, device="cuda")
    bos = torch.ones(a.batch, 1, dtype=torch.int64, device="cuda")
    ctc = (head_logits(a.batch, a.te, cfg.vocab_size, m.ctc_head.Vp, m.ctc_blank), a.te, m.ctc_blank, None)
    variants = {}
    for w in (int(x) for x in a.beams.split(",") if x):
        for lam in (float(x) for x in a.lams.split(",") if x):
            for use in ((True,) if a.lm_only else (False, True)):
                variants[f"beam{w}_lam{lam:g}_{'lm' if use else 'nolm'}"] = lambda w=w, lam=lam, use=use: dec.beam_search(
                    bos, enc, beam=w, max_len=a.steps, poll=0, ctc=ctc if lam > 0 else None, ctc_weight=lam,
                    lm=lm if use else None, lm_weight=0.5 if use else 0.0)
    times = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():          # warm-up: code objects, allocator pools
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn))
    out = {"batch": a.batch, "te": a.te, "steps": a.steps, "reps": a.reps, "order": a.order, "lm_nodes": lm.n_nodes,
           "unit": "ms"}
    for name, ts in times.items():
        out[name] = {"total_ms": summary(ts), "ms_per_step": summary(ts, a.steps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
