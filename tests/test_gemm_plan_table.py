"""GEMM plan parity without a GPU: the kernel name asrx_gemm_kernel_name reports for a table of descriptors (fake,
aligned pointers; host logic only) against names recorded from the library of commit ac50840, the last one before
the planner was rewritten around one named plan.  The fixture is a record of that commit: it is never regenerated
from a later library.

The table is a sub-table of the product SHAPES x layouts x EPIS x KERNELS x TILES x SPLIT_BATCH x ALIGN (2,371,200
descriptors, 104 distinct names at ac50840, compared once case by case when the planner was rewritten).  Per
(shape, layout) block it walks three slices of that product, so every value of every axis appears and, as the test
asserts, every kernel name of the full product is reached."""
import hashlib
import itertools
import json
import os

SHAPES = [(15936, 512, 512), (15936, 1536, 512), (15936, 2048, 512), (15936, 512, 2048), (15936, 12288, 512),
          (15936, 512, 12288), (4096, 512, 512), (4096, 1536, 512), (4096, 2048, 512), (4096, 512, 2048),
          (2048, 512, 512), (8192, 512, 64), (1024, 512, 2048), (1000, 4160, 256), (200, 136, 96), (1000, 250, 64),
          (129, 64, 576), (64, 1536, 512), (33, 17, 40), (8, 8, 64), (7, 8, 64), (64, 576, 302784), (64, 128, 16421),
          (2048, 512, 15936), (512, 512, 15936)]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
EPIS = ["none", "bias", "bias_relu", "bias_relu_drop", "bias_relu_mask", "bias_relu_drop_mask", "f32", "bias_f32",
        "bias_resid_f32", "bias_drop_resid_f32", "bias_rowadd_f32", "gate_bf16", "gate_bf16_alpha", "gate_bits",
        "gate_bits_alpha", "beta1_f32", "beta_half_f32", "drop_only", "rowsum"]
KERNELS = list(range(13))
TILES = [0, 64, 128, 3]
SPLIT_BATCH = [(1, 1), (5, 1), (256, 1), (1, 8)]
ALIGN = ["ok", "a_off2", "lda_odd", "c_off4", "ldc_odd", "bias_off4"]

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_table.json")


def desc(m, n, k, at, bt, epi, kernel, tile, splitk, batch, align):
    from asrx._lib import BF16, BITS, F32, GemmDesc
    d = GemmDesc()
    d.m, d.n, d.k, d.in_dtype = m, n, k, BF16
    d.a, d.lda, d.a_trans = 1 << 20, (m if at else k), at
    d.b, d.ldb, d.b_trans = 2 << 20, (n if bt else k), bt
    d.c, d.ldc, d.c_dtype = 3 << 20, n, BF16
    d.alpha, d.batch, d.batch_inner, d.splitk = 1.0, batch, 1, splitk
    d.kernel, d.tile = kernel, tile
    if splitk > 1:
        d.workspace, d.workspace_elems = 6 << 20, splitk * m * n
    p = set(epi.split("_"))
    if "bias" in p:
        d.bias = 4 << 20
    if "relu" in p:
        d.relu = 1
    if "drop" in p:
        d.dropout_p = 0.1
    if "mask" in p:
        d.mask_out, d.ld_mask = 7 << 20, (n + 31) // 32
    if "f32" in p:
        d.c_dtype = F32
    if "resid" in p:
        d.resid, d.ld_resid, d.resid_dtype = 5 << 20, n, F32
    if "rowadd" in p:
        d.rowadd, d.ld_rowadd, d.rowadd_mod = 8 << 20, n, 249
    if "gate" in p:
        d.gate = 9 << 20
        if "bits" in p:
            d.gate_dtype, d.ld_gate = BITS, (n + 31) // 32
        else:
            d.gate_dtype, d.ld_gate = BF16, n
    if "alpha" in p:
        d.alpha = 0.125
    if "beta1" in p:
        d.beta = 1.0
    if "beta" in p and "half" in p:
        d.beta = 0.5
    if "rowsum" in p:
        d.rowsum_a, d.rowsum_ws = 10 << 20, 11 << 20
    if align == "a_off2":
        d.a += 2
    elif align == "lda_odd":
        d.lda += 1
    elif align == "c_off4":
        d.c += 4
    elif align == "ldc_odd":
        d.ldc += 1
    elif align == "bias_off4" and d.bias:
        d.bias += 4
    return d


def full_block():
    """One (shape, layout) block of the full product, in its fixed order."""
    return itertools.product(EPIS, KERNELS, TILES, SPLIT_BATCH, ALIGN)


def sub_block():
    """The committed slices of one (shape, layout) block: every epilogue under every kernel code; every epilogue on
    the auto planner under every tile, split / batch and alignment; every kernel code under every tile, split /
    batch and alignment for bias + ReLU (the epilogue p4 runs as its dropout instantiation)."""
    yield from itertools.product(EPIS, KERNELS, TILES[:1], SPLIT_BATCH[:1], ALIGN[:1])
    yield from itertools.product(EPIS, KERNELS[:1], TILES, SPLIT_BATCH, ALIGN)
    yield from itertools.product(("bias_relu",), KERNELS[1:], TILES, SPLIT_BATCH, ALIGN)


def block_names(shape, layout, block):
    from asrx.kernels import kernel_name
    return [kernel_name(desc(*shape, *layout, epi, kern, tile, sk, ba, al)) for epi, kern, tile, (sk, ba), al in block]


def digest(names):
    return hashlib.sha256("\n".join(names).encode()).hexdigest()[:24]


def test_gemm_plan_table_matches_recorded_names():
    with open(FIXTURE) as f:
        fx = json.load(f)
    recorded = set(fx["names"])
    seen, differ = set(), []
    for shape in SHAPES:
        for layout in LAYOUTS:
            names = block_names(shape, layout, sub_block())
            seen.update(names)
            key = "%d,%d,%d,%d,%d" % (shape + layout)
            if digest(names) != fx["blocks"][key]:
                differ.append((key, sorted(set(names) - recorded)))
    assert not differ, f"(shape, layout) blocks whose names differ from {fx['commit']} (and their new names): {differ}"
    # the sub-table reaches every kernel the full product reached on the recorded commit, and nothing else
    assert seen == recorded, (sorted(recorded - seen), sorted(seen - recorded))
    assert len(recorded) == fx["full_product"]["distinct"]
    # bias + ReLU (+ mask bits) on p4 only ever runs as the dropout instantiation with threshold 0
    assert not seen & {"gemm_bf16_p4_kernel<false, false, 3>", "gemm_bf16_p4_kernel<false, false, 1027>"}
