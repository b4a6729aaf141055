"""SpecAugment micro-benchmark: asrx_specaug against the copy it replaces, and the c3 step with and
without an augmenter.

  kernel: the c3 input (64, 1, 80, 1000) fp32, masks only and with a warp of 40, each against `dst.copy_(src)` of the
          same tensors.  Every variant is 24 launches captured in a HIP graph (no host gaps), the graphs replayed in
          turn between HIP events after a warm-up, cold (rotating buffer sets beyond the Infinity Cache) and warm (one
          set); median and min .. max over the rounds; kernel_vs_copy = copy time / kernel time, as bench.py's.
  step:   one c3 trainer and its one captured graph, blocks of steps alternating between no augmenter, masks only and
          a warp of 40 (the augmenter is switched between blocks; the graph is the same).

    python tools/specaug_bench.py [--rounds 9] [--blocks 6] [--steps 10] [--no-step]
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
from oracle.ref_model import CONFIGS, synthetic_batch  # noqa: E402

COLD_BYTES = 768 << 20   # rotating buffer sets this large read from HBM, not from the 256 MiB Infinity Cache
LAUNCHES = 24


def _graph(fns):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            fns[i % len(fns)]()
    g.replay()
    torch.cuda.synchronize()
    return g


def _interleaved_us(graphs, rounds):
    """{name: [us per launch, one per round]}: the graphs replayed in turn, each between its own pair of events"""
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            out[k].append(s.elapsed_time(e) * 1e3 / LAUNCHES)
    return out


def kernel_bench(rounds):
    B, F, T = 64, 80, 1000
    nbytes = 2 * B * F * T * 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    nsets = max(2, -(-COLD_BYTES // nbytes))
    sets = [(torch.randn(B, 1, F, T, device="cuda", generator=gen), torch.empty(B, 1, F, T, device="cuda"))
            for _ in range(nsets)]
    masks = asrx.SpecAugment(seed=1)                   # the defaults: 2 x 27 rows, 2 x 100 frames
    warp = asrx.SpecAugment(seed=1, time_warp=40)
    res = {"shape": [B, 1, F, T], "bytes_copy": nbytes, "buffer_sets": nsets, "launches_per_replay": LAUNCHES,
           "rounds": rounds}
    for state, use in (("cold", sets), ("warm", sets[:1])):
        graphs = {
            "copy": _graph([lambda s=s, d=d: d.copy_(s) for s, d in use]),
            "masks": _graph([lambda s=s, d=d: masks.augment(s, out=d, step=3) for s, d in use]),
            "warp40": _graph([lambda s=s, d=d: warp.augment(s, out=d, step=3) for s, d in use]),
        }
        _interleaved_us(graphs, 2)                     # warm-up rounds
        us = _interleaved_us(graphs, rounds)
        row = {}
        for k, v in us.items():
            row[k] = {"us": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        for k in ("masks", "warp40"):
            row[k]["kernel_vs_copy"] = round(row["copy"]["us"] / row[k]["us"], 3)
        row["copy"]["GBps"] = round(nbytes / row["copy"]["us"] / 1e3, 0)
        res[state] = row
        del graphs
    return res


def step_bench(blocks, steps):
    from asrx.train import Trainer
    spec = CONFIGS["c3"]
    cfg = spec["cfg"]
    s, t, k = (x.cuda() for x in synthetic_batch(cfg, spec["batch"], spec["frames"], spec["text_len"] + 1, seed=1))
    lens = torch.full((spec["batch"],), spec["frames"], dtype=torch.int32, device="cuda")
    # ONE trainer and one captured graph: the augmenter is read at every replay, so switching it between blocks
    # compares the launch with the copy and nothing else (two trainers differ in where their buffers lie as well)
    augs = {"plain": None, "specaug": asrx.SpecAugment(seed=1), "specaug_warp40": asrx.SpecAugment(seed=1, time_warp=40)}
    torch.manual_seed(0)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, precision="bf16").cuda().train()
    tr = Trainer(m, lr=1e-4, graph=True)

    def run(name, n):
        tr.spec_augment = augs[name]
        for _ in range(n):
            if tr.spec_augment is None:
                tr.step(s, t, k)
            else:
                tr.step(s, t, k, input_lengths=lens)

    for name in augs:
        run(name, 6)                                   # eager steps, the capture, first replays of every variant
    torch.cuda.synchronize()
    assert tr._cap is not None
    ms = {name: [] for name in augs}
    for _ in range(blocks):
        for name in augs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, steps)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    return {"config": "c3", "steps_per_block": steps,
            **{name: {"ms": round(statistics.median(v), 3), "blocks": [round(x, 3) for x in v]} for name, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specaug_bench needs the GPU: nothing is measured without one")
    out = {"kernel": kernel_bench(args.rounds)}
    print(json.dumps(out["kernel"]), flush=True)
    if not args.no_step:
        out["step"] = step_bench(args.blocks, args.steps)
        print(json.dumps(out["step"]), flush=True)
    return out


if __name__ == "__main__":
    main()
