"""Run every case of tests/test_attn_plan_table.py's table (b) once, forward and backward, to compare a kernel trace
with the names asrx_attn_kernel_name predicts.

    rocprofv3 --kernel-trace -d OUT -o run --output-format csv -- python tools/attn_plan_trace.py run [--out PRED.json]
    python tools/attn_plan_trace.py check OUT/.../run_kernel_trace.csv [--pred PRED.json] [--other TRACE.csv]

run    B = H = 2, random operands, the tests' own run_fwd / run_bwd and mask layouts (a second or two).  Where the loaded
       library has the name query, every attention call is preceded by the query on the very descriptor it launches,
       and the predictions are printed (and written to --out) in launch order.
check  The attn_* / ln_dropgen / dq_finish kernels of the trace, in start order, against the table's expected names,
       the names tests/golden/attn_plan_table.json recorded for these cases, --pred, and those of another trace
       (--other).  Exits nonzero on any difference.
"""
import argparse
import csv
import ctypes
import json
import os
import re
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "asr-transformer_amd")]


def expected():
    """[(case id, direction, names)] in the order `run` launches them."""
    import test_attn_plan_table as T
    out = []
    for cid, var, args, fwd, bwd in T.cases():
        out.append((cid, "fwd", fwd))
        if bwd is not None:
            out.append((cid, "bwd", bwd))
    return out


def run(args):
    import torch
    import test_attn_plan_table as T
    import test_gpu_attention_keymask as KM
    import test_gpu_attention_peaked as P
    from asrx import kernels
    from asrx._lib import lib

    has_query = hasattr(lib(), "asrx_attn_kernel_name")
    predicted, real_call = [], kernels.call

    def call(name, *a):
        if has_query and name in ("asrx_attention_fwd", "asrx_attention_bwd"):
            buf = ctypes.create_string_buffer(128)
            rc = lib().asrx_attn_kernel_name(a[0], int(name.endswith("bwd")), buf, 128)
            predicted.append(buf.value.decode() if rc == 0 else f"error {rc}")
        return real_call(name, *a)

    kernels.call = call
    g = torch.Generator().manual_seed(1)
    with T.attn_kernel_env() as env:
        for cid, var, (dh, Lq, Lk, mask, drop, with_lo), fwd, bwd in T.cases():
            env.set(var)      # ("auto" reads as no choice)
            d = P.H * dh
            qb = torch.randn(P.B, Lq, d, generator=g).bfloat16()
            kvb = torch.randn(P.B, Lk, 2 * d, generator=g).bfloat16()
            if mask in ("keys", "decoder_padded"):
                valid = torch.ones(P.B, Lk, dtype=torch.bool)
                valid[0, Lk - 1] = False
                spec = KM.spec_of(valid, "padded", "decoder" if mask == "decoder_padded" else "keys")
            else:
                spec = P.mask_and_spec({"decoder_tight": "decoder"}.get(mask, mask), Lq, Lk)[1]
            r = P.run_fwd(qb, kvb, dh, spec, drop != "none", drop != "nowords", with_lo)
            if bwd is not None:
                dOb = torch.randn(P.B, Lq, d, generator=g).bfloat16()
                P.run_bwd(r, types.SimpleNamespace(Lq=Lq, Lk=Lk), dh, dOb, drop != "nowords")
            torch.cuda.synchronize()
    kernels.call = real_call
    exp = expected()
    print(f"{len(exp)} calls, library {'with' if has_query else 'without'} the name query")
    if has_query:
        diff = [(c, dr, e, p) for (c, dr, e), p in zip(exp, predicted) if e != p]
        for (c, dr, e), p in zip(exp, predicted):
            print(f"{c:40s} {dr}  {p}")
        print(f"predictions vs the table's expected names: {len(predicted)} calls, {len(diff)} differences")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(predicted, f, indent=0)
        if diff or len(predicted) != len(exp):
            print(diff)
            sys.exit(1)


def trace_kernels(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")).strip()
             for r in rows]
    return [n for n in names if n.startswith(("attn_", "ln_dropgen", "dq_finish"))]


def check(args):
    got = trace_kernels(args.trace)
    status = 0

    def compare(what, want):
        nonlocal status
        n = sum(a != b for a, b in zip(got, want)) + abs(len(got) - len(want))
        print(f"trace vs {what}: {len(got)} / {len(want)} kernels, {n} differences")
        if n:
            status = 1
            print([(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:10])

    exp = expected()
    compare(f"the table's expected names ({len(exp)} calls)", [k for _, _, names in exp for k in names.split(" + ")])
    with open(os.path.join(REPO, "tests", "golden", "attn_plan_table.json")) as f:
        fx = json.load(f)
    compare(f"the names recorded from {fx['commit']}",
            [k for cid in dict.fromkeys(c for c, _, _ in exp) for names in fx["test_cases"][cid] for k in names.split(" + ")])
    if args.pred:
        with open(args.pred) as f:
            compare("the library's predictions", [k for names in json.load(f) for k in names.split(" + ")])
    if args.other:
        compare("the other trace", trace_kernels(args.other))
    sys.exit(status)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out")
    c = sub.add_parser("check")
    c.add_argument("trace")
    c.add_argument("--pred")
    c.add_argument("--other")
    a = ap.parse_args()
    run(a) if a.cmd == "run" else check(a)
