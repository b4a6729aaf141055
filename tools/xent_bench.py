"""Cross-entropy micro-benchmark, built the way tools/fbank_bench.py is.

Shape: 4096 rows (c3's B * L = 64 * 64) of V = 250, 1000, 5000 and 16384 classes, ld = V rounded up to 64, fp32 logits
in, bf16 dlogits out, label smoothing 0.1, argmax and statistics on.
  xent_ls   asrx_cross_entropy_ls: its three launches (count, rows, final)
  xent_old  asrx_cross_entropy, the one-wave-per-row kernel (ld <= 1024 only), the same three launches
  cast      dst_bf16.copy_(src_fp32) over [rows, ld]: a device copy moving the bytes of the rows kernel (fp32 rows * ld
            read — the kernel reads rows * V of them — and bf16 rows * ld written)
Every variant is LAUNCHES calls captured in a HIP graph (no host gaps); the graphs of a group are replayed in turn
between HIP events after warm-up rounds; cold = buffer sets rotating beyond the 256 MiB Infinity Cache, warm = one set
repeated; median [min .. max] over the rounds, and the whole measurement is repeated --runs times.

    python tools/xent_bench.py [--rounds 9] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asr-transformer_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import asrx  # noqa: E402
from asrx import kernels as K  # noqa: E402
from asrx._lib import BF16  # noqa: E402

COLD_BYTES = 768 << 20   # rotating buffer sets this large read from HBM, not from the 256 MiB Infinity Cache
ROWS = 4096
VOCABS = (250, 1000, 5000, 16384)
EPS = 0.1
LAUNCHES = 16


def _graph(fns, launches):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(launches):
            fns[i % len(fns)]()
    g.replay()
    torch.cuda.synchronize()
    return g


def _interleaved_us(graphs, rounds, launches):
    """{name: [us per call, one per round]}: the graphs replayed in turn, each between its own pair of events"""
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            out[k].append(s.elapsed_time(e) * 1e3 / launches)
    return out


def _row(us):
    return {k: {"us": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            for k, v in us.items()}


def vocab_bench(V, rounds, gen):
    ld = (V + 63) // 64 * 64
    moved = ROWS * V * 4 + ROWS * ld * 2                       # the rows kernel's reads and writes
    nsets = max(2, -(-COLD_BYTES // (ROWS * ld * 6)))
    sets = []
    for _ in range(nsets):
        x = torch.randn(ROWS, ld, device="cuda", generator=gen) * 3
        t = torch.randint(0, V, (ROWS,), device="cuda", generator=gen)
        t[5::7] = -100
        sets.append(dict(x=x, t=t, dl=torch.empty(ROWS, ld, device="cuda", dtype=torch.bfloat16),
                         am=torch.empty(ROWS, device="cuda", dtype=torch.int64),
                         loss=torch.empty(1, device="cuda"), stats=torch.empty(2, device="cuda"),
                         ws=torch.empty(K.xent_workspace_elems(ROWS), device="cuda")))
    torch.cuda.synchronize()

    def ls(b):
        K.call("asrx_cross_entropy_ls", b["x"].data_ptr(), ROWS, V, ld, b["t"].data_ptr(), -100, EPS, 1.0,
               b["loss"].data_ptr(), b["stats"].data_ptr(), BF16, b["dl"].data_ptr(), b["am"].data_ptr(),
               b["ws"].data_ptr(), K.stream())

    def old(b):
        K.call("asrx_cross_entropy", b["x"].data_ptr(), ROWS, V, ld, b["t"].data_ptr(), -100, 1.0,
               b["loss"].data_ptr(), b["dl"].data_ptr(), b["am"].data_ptr(), b["ws"].data_ptr(), K.stream())

    def make(use):
        g = {"xent_ls": [lambda b=b: ls(b) for b in use],
             "cast": [lambda b=b: b["dl"].copy_(b["x"]) for b in use]}
        if ld <= K.CE_OLD_MAXLD:
            g["xent_old"] = [lambda b=b: old(b) for b in use]
        return g

    res = {"V": V, "ld": ld, "buffer_sets": nsets, "bytes_moved": moved}
    for state, use in (("cold", sets), ("warm", sets[:1])):
        graphs = {k: _graph(fns, LAUNCHES) for k, fns in make(use).items()}
        _interleaved_us(graphs, 2, LAUNCHES)                   # warm-up rounds
        row = _row(_interleaved_us(graphs, rounds, LAUNCHES))
        row["xent_ls"]["GBps"] = round(moved / row["xent_ls"]["us"] / 1e3, 0)
        row["cast"]["GBps"] = round(ROWS * ld * 6 / row["cast"]["us"] / 1e3, 0)
        row["ls_vs_cast"] = round(row["xent_ls"]["us"] / row["cast"]["us"], 3)
        if "xent_old" in row:
            row["ls_vs_old"] = round(row["xent_ls"]["us"] / row["xent_old"]["us"], 3)
        res[state] = row
        del graphs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xent_bench needs the GPU: nothing is measured without one")
    assert asrx.native().asrx_version() >= 14
    out = []
    for run in range(args.runs):
        gen = torch.Generator(device="cuda").manual_seed(run)
        res = {"run": run, "rows": ROWS, "eps": EPS, "rounds": args.rounds, "launches": LAUNCHES}
        for V in VOCABS:
            res[f"V{V}"] = vocab_bench(V, args.rounds, gen)
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


if __name__ == "__main__":
    main()
