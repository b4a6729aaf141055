"""Attention plan parity without a GPU: the kernels asrx_attn_kernel_name reports for tables of descriptors (fake,
torch-like pointers; host logic only).

(a) The product ENVS x DHS x LQS x LKS x MASKS x DROPS x O_LO x ALIGN x direction (712,800 descriptors, B = H = 2)
    against the names — or the error code — recorded from commit 82d90bb, the last one before the dispatch was rewritten
    around one named plan.  That commit had no name query: the fixture was recorded from its library with a query
    appended to csrc/attention.hip that walks its asrx_attention_fwd / asrx_attention_bwd condition by condition and
    names a kernel where they launch one (no existing line changed; a kernel trace of the cases of (b) on that library
    agreed with it).  The fixture is a record of that commit: it is never regenerated from a later library.
(b) The cases of tests/test_gpu_attention_peaked.py and tests/attn_keymask_ref.py, with the descriptors their run_fwd /
    run_bwd build, and the kernels each case is there to reach: CASES below is the table those files point to, and
    every forward and backward instantiation the library compiles is the expected name of at least one case.
(c) The keep-word invariant over the whole of (a): wherever the backward reads keep words, the forward of the same
    descriptor (its gradients removed) wrote them."""
import ctypes
import hashlib
import itertools
import json
import os

import attn_keymask_ref as M
import test_gpu_attention_peaked as P

B, H = P.B, P.H
ENVS = [None, "tiled", "resident"]
DHS = [32, 64]
LQS = [1, 5, 33, 64, 65, 100, 249, 256, 257, 300, 1031]
LKS = [1, 17, 32, 33, 64, 65, 100, 128, 129, 200, 249, 256, 257, 300, 1031]
# decoder: causal + both validity rows, word-aligned; keys*: key validity only — word-aligned rows, the base off by 1,
# an odd valid_bstride
MASKS = ["none", "decoder", "keys", "keys_off1", "keys_oddstride", "dense"]
DROPS = ["none", "words", "words_ready", "nowords"]
O_LO = [False, True]
ALIGN_FWD = ["ok", "o_off4", "o_rstride4", "k_off8", "k_rstride_2p23"]
ALIGN_BWD = ALIGN_FWD + ["do_rstride_2p31", "dq_off4", "dq_rstride4", "do_rstride4", "no_dq_acc"]

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plan_table.json")

# one 4 GiB-aligned fake address per tensor, as separate torch allocations would be (at least 256-byte aligned)
Q, KV, O, LSE, VALID, MASK, DM, LO, DO, DQ, DKV, DELTA, ACC = ((i + 1) << 32 for i in range(13))


def ceil4(n):
    return (n + 3) // 4 * 4


def desc(dh, Lq, Lk, mask, drop, with_lo, backward):
    """The descriptor run_fwd / run_bwd of test_gpu_attention_peaked.py build: q [B, Lq, H dh], K | V interleaved in
    one [B, Lk, 2 H dh] tensor (and dK | dV likewise), dense outputs; dq_acc where asrx_attn_dq_acc_elems asks for it."""
    from asrx._lib import AttnDesc
    d, dm = AttnDesc(), H * dh
    d.batch, d.heads, d.lq, d.lk, d.dh = B, H, Lq, Lk, dh
    d.q, d.q_rstride, d.q_bstride = Q, dm, Lq * dm
    d.k, d.k_rstride, d.k_bstride = KV, 2 * dm, Lk * 2 * dm
    d.v, d.v_rstride, d.v_bstride = KV + 2 * dm, 2 * dm, Lk * 2 * dm
    d.o, d.o_rstride, d.o_bstride = O, dm, Lq * dm
    d.lse, d.scale = LSE, dm ** -0.5
    if mask == "dense":
        d.mask_mode, d.mask, d.mask_sb, d.mask_sq, d.mask_sk = 2, MASK, Lq * Lk, Lk, 1
    elif mask == "decoder":          # word-aligned rows, kvalid = qvalid
        d.mask_mode, d.causal, d.kvalid, d.qvalid, d.valid_bstride = 1, 1, VALID, VALID, ceil4(max(Lq, Lk))
    elif mask == "decoder_tight":    # MaskSpec.decoder(valid [B, Lq]): rows Lq bytes apart
        d.mask_mode, d.causal, d.kvalid, d.qvalid, d.valid_bstride = 1, 1, VALID, VALID, Lq
    elif mask == "decoder_padded":   # test_gpu_attention_keymask.py's padded layout, the decoder's form
        d.mask_mode, d.causal, d.kvalid, d.qvalid, d.valid_bstride = 1, 1, VALID + 8, VALID + 8, ceil4(Lk) + 4
    elif mask.startswith("keys"):    # keys: the padded layout of test_gpu_attention_keymask.py
        d.mask_mode, d.kvalid, d.valid_bstride = 1, VALID + 8, ceil4(Lk) + 4
        if mask == "keys_off1":
            d.kvalid += 1
        elif mask == "keys_oddstride":
            d.valid_bstride += 1
    if drop != "none":
        d.dropout_p, d.seed = P.P_DROP, P.SEED
        if drop != "nowords":
            d.dropmask, d.dropmask_ready = DM, int(drop == "words_ready")
    if with_lo:
        d.o_lo = LO
    if backward:
        d.dout, d.do_rstride, d.do_bstride = DO, dm, Lq * dm
        d.dq, d.dq_rstride, d.dq_bstride = DQ, dm, Lq * dm
        d.dk, d.dk_rstride, d.dk_bstride = DKV, 2 * dm, Lk * 2 * dm
        d.dv, d.dv_rstride, d.dv_bstride = DKV + 2 * dm, 2 * dm, Lk * 2 * dm
        d.delta = DELTA
        if Lk > 128:
            d.dq_acc = ACC
    return d


def misaligned(d, align):
    """A copy of d with one alignment or bound of the ALIGN axis broken."""
    d = type(d).from_buffer_copy(d)
    if align == "o_off4":
        d.o += 4
    elif align == "o_rstride4":
        d.o_rstride += 4
    elif align == "k_off8":
        d.k += 8
    elif align == "k_rstride_2p23":
        d.k_rstride = 1 << 23
    elif align == "do_rstride_2p31":       # (Lq + 32) * stride >= 2^31, the stride a multiple of 8
        d.do_rstride = ((1 << 31) // (d.lq + 32) + 8) // 8 * 8
    elif align == "dq_off4":
        d.dq += 4
    elif align == "dq_rstride4":
        d.dq_rstride += 4
    elif align == "do_rstride4":
        d.do_rstride += 4
    elif align == "no_dq_acc":
        d.dq_acc = None
    return d


def without_grads(d):
    """The forward descriptor of a backward one: the gradients and the backward's workspaces removed."""
    d = type(d).from_buffer_copy(d)
    d.dout = d.dq = d.dk = d.dv = d.delta = d.dq_acc = None
    d.do_rstride = d.do_bstride = d.dq_rstride = d.dq_bstride = 0
    d.dk_rstride = d.dk_bstride = d.dv_rstride = d.dv_bstride = 0
    return d


_BUF = ctypes.create_string_buffer(128)


def name_or_code(d, backward):
    """What asrx_attn_kernel_name reports for d: the names, or "error <code>" where the call returns one."""
    from asrx._lib import lib
    rc = lib().asrx_attn_kernel_name(ctypes.byref(d), int(backward), _BUF, 128)
    return _BUF.value.decode() if rc == 0 else f"error {rc}"


class attn_kernel_env:
    """ASRX_ATTN_KERNEL for a block of queries (None: unset), restored afterwards."""

    def __init__(self, value=None):
        self.value = value

    def set(self, value):
        if value is None:
            os.environ.pop("ASRX_ATTN_KERNEL", None)
        else:
            os.environ["ASRX_ATTN_KERNEL"] = value

    def __enter__(self):
        self.old = os.environ.get("ASRX_ATTN_KERNEL")
        self.set(self.value)
        return self

    def __exit__(self, *exc):
        self.set(self.old)


def block_names(dh, Lq, Lk, env, unwritten=None):
    """The names of one (dh, Lq, Lk) block of the product, in its fixed order.  unwritten (a list) collects the cases
    that break the keep-word invariant (c)."""
    names = []
    for mask, drop, with_lo, backward in itertools.product(MASKS, DROPS, O_LO, (False, True)):
        base = desc(dh, Lq, Lk, mask, drop, with_lo, backward)
        for align in (ALIGN_BWD if backward else ALIGN_FWD):
            d = misaligned(base, align)
            fwd = without_grads(d) if backward and drop != "none" else None
            for e in ENVS:
                env.set(e)
                name = name_or_code(d, backward)
                names.append(name)
                if fwd is not None and "attn_bwd_res_kernel" in name and unwritten is not None:
                    # (a forward that returns an error wrote no output either: there is no backward of it to run)
                    wrote = name_or_code(fwd, False)
                    if not (wrote.startswith("error") or drop == "words_ready" or "attn_dropgen_kernel" in wrote):
                        unwritten.append((dh, Lq, Lk, mask, drop, with_lo, align, e, name, wrote))
    return names


def digest(names):
    return hashlib.sha256("\n".join(names).encode()).hexdigest()[:24]


def test_attn_plan_table_matches_recorded_names():
    with open(FIXTURE) as f:
        fx = json.load(f)
    recorded = set(fx["names"])
    seen, differ, unwritten, count = set(), [], [], 0
    with attn_kernel_env() as env:
        for dh, Lq, Lk in itertools.product(DHS, LQS, LKS):
            names = block_names(dh, Lq, Lk, env, unwritten)
            seen.update(names)
            count += len(names)
            key = f"{dh},{Lq},{Lk}"
            if digest(names) != fx["blocks"][key]:
                differ.append((key, sorted(set(names) - recorded)))
    assert not differ, f"(dh, Lq, Lk) blocks whose names differ from {fx['commit']} (and their new names): {differ}"
    assert count == fx["cases"] and seen == recorded, (count, sorted(recorded - seen), sorted(seen - recorded))
    # (c) a backward that reads keep words follows a forward that wrote them
    assert not unwritten, unwritten[:10]


# ------------------------------------------------------------------------------------------------ (b) the tests' cases

KQ, RES, STREAM, TILED = "attn_fwd_kq_kernel", "attn_fwd_res_kernel", "attn_fwd_stream_kernel", "attn_fwd_kernel"
GEN, BRES, FIN = "attn_dropgen_kernel + ", "attn_bwd_res_kernel", " + dq_finish_kernel"


def tiled_bwd(dh, blocks):
    return f"attn_delta_kernel<{dh}> + attn_bwd_kernel<{dh}>" + (FIN if blocks > 1 else "")


# test_gpu_attention_peaked.FWD_CASES: id -> the forward's kernels
PEAKED_FWD = {
    "kq-64x249": KQ + "<false>", "kq-5x17": KQ + "<false>", "kq-33x256": KQ + "<false>", "kq-64x100": KQ + "<false>",
    "kqdrop-64x249": GEN + KQ + "<true>",
    "res0-100x200": RES + "<0, false>", "res0-249x249": RES + "<0, false>",
    "res0drop-64x100": GEN + RES + "<0, false>",          # four keep words per query: neither kq<true> nor W8
    "res0w8drop-249x249": GEN + RES + "<0, true>",
    "res1-70x70": RES + "<1, false>", "res1-33x33": RES + "<1, false>", "res2-40x40": RES + "<2, false>",
    "stream0-57x1031": STREAM + "<0, false>", "stream0-300x300": STREAM + "<0, false>",
    "stream0-64x257": STREAM + "<0, false>", "stream0-100x200": STREAM + "<0, false>",     # (100, 200): two chunks
    "stream0drop-57x1031": GEN + STREAM + "<0, true>", "stream0drop-300x300": GEN + STREAM + "<0, true>",
    "stream1-300x300": STREAM + "<1, false>", "stream1drop-300x300": GEN + STREAM + "<1, true>",
    "tiled64-64x249": TILED + "<64>", "tiled64-300x300": TILED + "<64>",
    "tiled64drop-64x249": TILED + "<64>",                 # dropout without keep words
    "tiled64dense-300x300": TILED + "<64>", "tiled32-64x249": TILED + "<32>",
}
# test_gpu_attention_peaked.BWD_CASES: id -> (the forward's kernels, the backward's)
PEAKED_BWD = {
    "res0n2-64x64": (KQ + "<false>", BRES + "<0, 2, false>"),
    "res0n4-64x100": (KQ + "<false>", BRES + "<0, 4, false>"),
    "res0n8-64x249": (KQ + "<false>", BRES + "<0, 8, false>"),
    "res0n8-64x249-drop": (GEN + KQ + "<true>", BRES + "<0, 8, false>"),
    "res0n8-64x249-drop-lo": (GEN + KQ + "<true>", BRES + "<0, 8, false>"),
    "res1n2-33x33": (RES + "<1, false>", BRES + "<1, 2, false>"),
    "res1n4-70x70": (RES + "<1, false>", BRES + "<1, 4, false>"),
    "res1n8-249x249": (RES + "<1, false>", BRES + "<1, 8, false>"),   # validity rows 249 bytes apart: not streamed
    "res2n2-40x40": (RES + "<2, false>", BRES + "<2, 2, false>"),
    "res2n4-100x100": (RES + "<2, false>", BRES + "<2, 4, false>"),
    "res2n8-200x200": (RES + "<2, false>", BRES + "<2, 8, false>"),
    "multi0-57x1031": (STREAM + "<0, false>", BRES + "<0, 8, true>" + FIN),
    "multi0-57x1031-drop-lo": (GEN + STREAM + "<0, true>", BRES + "<0, 8, true>" + FIN),
    "multi0-300x300": (STREAM + "<0, false>", BRES + "<0, 8, true>" + FIN),
    "multi0-300x300-drop": (GEN + STREAM + "<0, true>", BRES + "<0, 8, true>" + FIN),
    "multi0-300x300-ramp": (STREAM + "<0, false>", BRES + "<0, 8, true>" + FIN),
    "multi1-300x300": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "multi1-300x300-drop-lo": (GEN + STREAM + "<1, true>", BRES + "<1, 8, true>" + FIN),
    "multi1-300x300-ramp": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "tiled64-64x249": (TILED + "<64>", tiled_bwd(64, 1)),
    "tiled64-300x300": (TILED + "<64>", tiled_bwd(64, 2)),
    "tiled64-300x300-ramp": (TILED + "<64>", tiled_bwd(64, 2)),
    "tiled64-64x249-drop-nowords": (TILED + "<64>", tiled_bwd(64, 1)),
    "tiled64-300x300-drop-nowords": (TILED + "<64>", tiled_bwd(64, 2)),
    "tiled32-64x249": (TILED + "<32>", tiled_bwd(32, 1)),
    "tiled32-300x300-drop": (TILED + "<32>", tiled_bwd(32, 2)),
}
# attn_keymask_ref.SHAPES / DROP_SHAPES with word-aligned validity rows (the padded layout of
# test_gpu_attention_keymask.py; dropout carries keep words and o_lo): id -> (the forward's kernels, the backward's).
# Rows off a word boundary take attn_fwd_res_kernel<1, false> up to 256 keys and the tiled pair past that.
KEYMASK = {
    "self-249": (STREAM + "<1, false>", BRES + "<1, 8, false>"),          # two 128-key chunks
    "self-129": (STREAM + "<1, false>", BRES + "<1, 8, false>"),
    "self-190": (STREAM + "<1, false>", BRES + "<1, 8, false>"),
    "self-255": (STREAM + "<1, false>", BRES + "<1, 8, false>"),
    "self-257": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),     # Lk > 256: the key-block backward
    "self-386": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "self-999": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "cross-16x249": (RES + "<1, false>", BRES + "<1, 8, false>"),         # control: it reads bytes
    "cross-70x249": (STREAM + "<1, false>", BRES + "<1, 8, false>"),      # more than 64 queries: two chunks
    "cross-16x257": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "cross-16x999": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "dec-249": (STREAM + "<1, false>", BRES + "<1, 8, false>"),           # causal
    "dec-257": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "dec-302": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "dec-303": (STREAM + "<1, false>", BRES + "<1, 8, true>" + FIN),
    "ctl-252": (STREAM + "<1, false>", BRES + "<1, 8, false>"),           # controls: Lk % 4 == 0; tiled; resident
    "ctl-tiled-259": (TILED + "<64>", tiled_bwd(64, 2)),
    "ctl-resident-249": (RES + "<1, false>", BRES + "<1, 8, false>"),
    "drop-self-249": (GEN + STREAM + "<1, true>", BRES + "<1, 8, false>"),
    "drop-self-259": (GEN + STREAM + "<1, true>", BRES + "<1, 8, true>" + FIN),
    "drop-cross-16x257": (GEN + STREAM + "<1, true>", BRES + "<1, 8, true>" + FIN),
    "drop-dec-303": (GEN + STREAM + "<1, true>", BRES + "<1, 8, true>" + FIN),
}

# every instantiation of the forward and backward kernels in csrc/attention.hip: 12 + 11 + 2
INSTANTIATIONS = (
    [KQ + "<false>", KQ + "<true>", RES + "<0, false>", RES + "<0, true>", RES + "<1, false>", RES + "<2, false>"] +
    [f"{STREAM}<{m}, {d}>" for m in (0, 1) for d in ("false", "true")] + [TILED + "<64>", TILED + "<32>"] +
    [f"{BRES}<{m}, {n}, false>" for m in (0, 1, 2) for n in (2, 4, 8)] + [BRES + "<0, 8, true>", BRES + "<1, 8, true>"] +
    ["attn_bwd_kernel<64>", "attn_bwd_kernel<32>"])


def cases():
    """(case id, ASRX_ATTN_KERNEL, (dh, Lq, Lk, mask, drop, with_lo), expected forward, expected backward or None)."""
    def drop_of(drop, keep_words):
        return "none" if not drop else ("words" if keep_words else "nowords")

    def mask_of(kind):
        return {"none": "none", "decoder": "decoder_tight", "dense": "dense"}[kind]

    for cid, var, Lq, Lk, dh, mask, drop, kw in P.FWD_CASES:
        yield "peaked-fwd-" + cid, var, (dh, Lq, Lk, mask_of(mask), drop_of(drop, kw), False), PEAKED_FWD[cid], None
    for cid, var, Lq, Lk, dh, mask, drop, kw, lo, _ in P.BWD_CASES:
        yield "peaked-bwd-" + cid, var, (dh, Lq, Lk, mask_of(mask), drop_of(drop, kw), lo), *PEAKED_BWD[cid]
    for shapes, drop in ((M.SHAPES, False), (M.DROP_SHAPES, True)):
        for cid, var, Lq, Lk, form in shapes:
            mask = "decoder_padded" if form == "decoder" else "keys"
            yield "keymask-" + cid, var, (M.DH, Lq, Lk, mask, drop_of(drop, True), drop), *KEYMASK[cid]


def test_attn_test_cases_reach_their_kernels():
    """Table (b): each case of the two GPU test files reaches the kernels it is there for, and together they reach
    every instantiation."""
    assert len(PEAKED_FWD) == len(P.FWD_CASES) and len(PEAKED_BWD) == len(P.BWD_CASES)
    assert len(KEYMASK) == len(M.SHAPES) + len(M.DROP_SHAPES)
    with open(FIXTURE) as f:
        recorded = json.load(f)["test_cases"]      # the same cases on the recorded commit
    wrong, reached = [], set()
    with attn_kernel_env() as env:
        for cid, var, args, fwd, bwd in cases():
            assert recorded[cid] == [fwd] + ([bwd] if bwd else []), (cid, recorded[cid])
            env.set(None if var == "auto" else var)
            for backward, expected in ((False, fwd), (True, bwd)):
                if expected is None:
                    continue
                got = name_or_code(desc(*args, backward), backward)
                reached.update(expected.split(" + "))
                if got != expected:
                    wrong.append((cid, "bwd" if backward else "fwd", expected, got))
    assert not wrong, wrong
    assert not set(INSTANTIATIONS) - reached, sorted(set(INSTANTIATIONS) - reached)


def test_attn_kernel_name_wrapper():
    """kernels.attn_kernel_name returns the same names and raises where the call itself would return an error."""
    import pytest
    from asrx import kernels
    with attn_kernel_env():
        d = desc(64, 64, 249, "none", "words", False, True)
        assert kernels.attn_kernel_name(d) == GEN + KQ + "<true>"
        assert kernels.attn_kernel_name(d, backward=True) == BRES + "<0, 8, false>"
        with pytest.raises(RuntimeError, match="unsupported"):
            kernels.attn_kernel_name(misaligned(d, "o_off4"))
