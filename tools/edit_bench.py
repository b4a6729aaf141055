"""Kernel timing of asrx_edit_distance (token error rates, MBR distances) next to the search that produces the beam.

    python tools/edit_bench.py [--batch 64] [--beam 8] [--launches 50] [--reps 7] [--no-host]

Device-event timings, one JSON line, microseconds per launch (median [min, max] over --reps windows of --launches
launches each, after a warm-up), eager and as a captured graph of the same launches:
    group64 / cross64     batch * beam hypotheses of 64 tokens against batch references (batch * beam pairs) and
                          all beam x beam pairs per sample (batch * beam^2 pairs); hypotheses are the reference with a
                          tenth of the tokens substituted, deleted or inserted
    group255 / cross255   the same with 255-token rows (the longest supported)
    mbr_rank              asrx_mbr_rank on the cross64 distances
    ctc_prefix_beam       asrx_ctc_prefix_beam at the c3 shape (T' 249, V 250, 63 labels) for the same batch and beam,
                          and for batch 8: what producing the beam costs
    host_group64 / host_cross64   the path this replaces, once, in ms: copy the rows to the host, strip them, and run
                          asrx.new.train._edit_distance per pair
For the kernel alone run it under the profiler in a run of its own and read edit_distance_kernel:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/edit_bench.py --no-host --reps 2
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asr-transformer_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from asrx import kernels as K  # noqa: E402
from asrx.new.train import _edit_distance  # noqa: E402
from tools.joint_bench import head_logits, summary, timed  # noqa: E402

PAD = 4


def make_rows(B, W, n, seed):
    """ref [B, n], hyp [B * W, n] (PAD-filled where edits shortened a row): each hypothesis is its reference with
    about a tenth of the tokens edited."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(5, 250, size=(B, n))
    hyp = np.full((B * W, n), PAD, dtype=np.int64)
    for r in range(B * W):
        h = list(ref[r // W])
        for _ in range(max(1, n // 10)):
            k, p = int(rng.integers(0, 3)), int(rng.integers(0, len(h)))
            if k == 0:
                h[p] = int(rng.integers(5, 250))
            elif k == 1:
                h.insert(p, int(rng.integers(5, 250)))
            else:
                del h[p]
        h = h[:n]
        hyp[r, :len(h)] = h
    return torch.from_numpy(ref).cuda(), torch.from_numpy(hyp).cuda()


def window(fn, launches, reps):
    """us per launch: eager windows of `launches` launches, and replays of a graph that holds the same launches."""
    def many():
        for _ in range(launches):
            fn()
    many()
    torch.cuda.synchronize()
    eager = [timed(many) for _ in range(reps)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        many()
    g.replay()
    torch.cuda.synchronize()
    graph = [timed(g.replay) for _ in range(reps)]
    return {"eager_us": summary(eager, launches / 1e3), "graph_us": summary(graph, launches / 1e3)}


def host_path(hyp, ref, W, cross):
    """ms of the host loop over the same pairs, the device-to-host copy included."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = [[t for t in row if t != PAD] for row in hyp.cpu().tolist()]
    if cross:
        total = sum(_edit_distance(h[g * W + i], h[g * W + j]) for g in range(len(h) // W) for i in range(W)
                    for j in range(W))
    else:
        r = ref.cpu().tolist()
        total = sum(_edit_distance(a, r[k // W]) for k, a in enumerate(h))
    return round((time.perf_counter() - t0) * 1e3, 2), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    B, W = a.batch, a.beam
    out = {"batch": B, "beam": W, "launches": a.launches, "reps": a.reps}
    check = {}
    for n in (64, 255):
        ref, hyp = make_rows(B, W, n, n)
        bufs = {m: (torch.empty(N, dtype=torch.int32, device="cuda"),
                    torch.empty(N, 4, dtype=torch.int32, device="cuda"))
                for m, N in (("group", B * W), ("cross", B * W * W))}
        for mode in ("group", "cross"):
            def fn(mode=mode):
                K.edit_distance(hyp, None if mode == "cross" else ref, drop=(PAD,), mode=mode, W=W, out=bufs[mode])
            out[f"{mode}{n}"] = dict(pairs=bufs[mode][0].numel(), **window(fn, a.launches, a.reps))
            check[f"{mode}{n}"] = int(bufs[mode][0].sum())
        if n == 64:
            score = torch.randn(B * W, device="cuda")
            out["mbr_rank"] = window(lambda: K.mbr_rank(bufs["cross"][0], score, B, W, 1.0), a.launches, a.reps)
            if not a.no_host:
                for mode in ("group", "cross"):
                    ms, total = host_path(hyp, ref, W, mode == "cross")
                    assert total == check[f"{mode}64"], (mode, total, check)      # the same distances, summed
                    out[f"host_{mode}64_ms"] = ms
    out["sum_of_distances"] = check
    for b in sorted({B, 8}):
        x = head_logits(b, 249, 250, 256, PAD)
        out[f"ctc_prefix_beam_b{b}"] = window(lambda: K.ctc_prefix_beam(x, 250, 249, PAD, W, 63),
                                              max(a.launches // 10, 2), a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
