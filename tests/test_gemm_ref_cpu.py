"""The exact GEMM reference and its case table (tests/gemm_ref.py), checked without a GPU: the reference's own
exactness and poison hygiene, and — through the host-only asrx_gemm_kernel_name — that every case plans the kernel it
declares, so that tests/test_gpu_gemm_exact.py runs every family, layout and instantiated epilogue it claims to."""
import collections
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as R
import rng_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asr-transformer_amd", "csrc")


@pytest.fixture(scope="module")
def built():
    return [(c, R.make_case(c)) for c in R.all_cases()]


def _planned(b):
    from asrx.kernels import kernel_name
    return kernel_name(b.desc(R.fake_bases(b)))


def test_reference_is_exact_and_never_sees_the_poison(built):
    """make_case asserts that every intermediate is a multiple of 0.5 below 2^24 (it would have raised); here: the
    expected C is finite and equals the float64 value (bf16 C: its nearest-even rounding), the operands hold exactly
    their logical elements and NaN everywhere else, GUARD_ROWS rows of it on either side."""
    rounds = 0
    for c, b in built:
        want = torch.from_numpy(b.exact)
        assert torch.isfinite(b.expect_c.float()).all(), c.id
        if c.c_f32:
            assert torch.equal(b.expect_c.double(), want), c.id
        else:
            assert torch.equal(b.expect_c, want.float().to(torch.bfloat16)), c.id   # numpy's rounding is torch's
            err = (b.expect_c.double() - want).abs()
            ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)).log2().floor().exp2() * 2.0 ** -7
            assert (err <= ulp / 2).all(), c.id
            rounds += int((err > 0).any())
        for name in ("a", "b"):
            buf, lay = b.bufs[name].float(), b.lay[name]
            idx = torch.from_numpy(lay.index().reshape(-1))
            assert len(torch.unique(idx)) == idx.numel(), c.id
            assert torch.isfinite(buf[idx]).all() and buf[idx].abs().max() <= 3, c.id
            assert int(torch.isnan(buf).sum()) == buf.numel() - idx.numel(), c.id
            lo, hi = int(idx.min()), int(idx.max())
            assert lo >= R.GUARD_ROWS * lay.ld and buf.numel() - 1 - hi >= R.GUARD_ROWS * lay.ld, c.id
        cb = b.bufs["c"].float()
        inside = torch.zeros(cb.numel(), dtype=torch.bool)
        inside[b.c_index.reshape(-1)] = True
        assert (cb[~inside] == R.SENTINEL).all(), c.id
        assert torch.isnan(cb[inside]).all() if c.beta == 0.0 else torch.isfinite(cb[inside]).all(), c.id
    assert rounds >= 5   # bf16 outputs that really round (the cast's rounding mode is under test)


def test_bf16_rounding_is_nearest_even():
    x = torch.tensor([257.0, 259.0, 261.0, -771.0, 1028.0, 1036.0])   # ties (spacing 2 and 8) and one non-tie
    assert x.to(torch.bfloat16).float().tolist() == [256.0, 260.0, 260.0, -772.0, 1024.0, 1040.0]


def test_odd_n_hash_pairs_straddle_rows(built):
    """With odd N the pair (2p, 2p + 1) of one 32-bit hash falls on the last column of a row and the first of the
    next: the table has dropout cases where such a pair takes two different decisions and both elements are
    observable (non-zero before the dropout), in batch 0 and in a batch z > 0."""
    seen = collections.Counter()
    for c, b in built:
        if not c.drop or c.n % 2 == 0:
            continue
        nb, m, n = b.keep.shape
        flat_keep, flat_pre = b.keep.reshape(-1), b.pre_drop.reshape(-1)
        assert np.array_equal(flat_keep, rng_ref.elem_keep(R.SEED, nb * m * n, R.DROP_P))
        p = np.arange(flat_keep.size // 2)
        straddle = (2 * p) // n != (2 * p + 1) // n
        assert straddle.any(), c.id
        good = straddle & (flat_keep[2 * p] != flat_keep[2 * p + 1]) & (flat_pre[2 * p] != 0) & (flat_pre[2 * p + 1] != 0)
        seen["z0"] += int(good[2 * p < m * n].any())
        seen["z>0"] += int(good[2 * p >= m * n].any())
    assert seen["z0"] >= 2 and seen["z>0"] >= 1, seen
    assert R.SEED >> 32 != 0


def test_bit_layout_matches_the_header():
    """pack_bits against the formula of include/asrx.h, bit by bit."""
    rs = np.random.RandomState(0)
    pos = rs.rand(5, 96) > 0.5
    w = R.pack_bits(pos, 3, 0)
    for m in range(5):
        for n in range(96):
            c = n % 32
            bit = 8 * ((c & 15) >> 2) + 4 * (c >> 4) + (c & 3)
            assert (int(w[m, n // 32]) >> bit) & 1 == int(pos[m, n])
    assert sorted(R.mask_bit_pos(np.arange(32)).tolist()) == list(range(32))


def test_empty_split_table():
    """fill_args rounds k_per_split up to whole K-steps: the (K, splitk) pairs of the table and their empty splits"""
    assert R.empty_splits(320, 5) == []
    assert R.empty_splits(576, 7) == [5, 6]
    assert R.empty_splits(320, 4) == [3]
    assert R.empty_splits(640, 8) == [5, 6, 7]
    assert R.empty_splits(64, 2) == [1] and R.empty_splits(64, 3) == [1, 2]
    assert R.empty_splits(200, 3) == [2]   # 128 + a ragged 72, then nothing
    for k in (64 * 32, 64 * 32 + 37):
        assert len(R.empty_splits(k, 64)) >= 31 and len(R.empty_splits(k, 256)) >= 223


def test_every_case_plans_the_kernel_it_declares(built):
    wrong = []
    for c, b in built:
        name = _planned(b)
        prefix, epi = R.expected_family(c)
        if name != R.expected_name(c) or not name.startswith(prefix) or (epi is not None and f", {epi}" not in name):
            wrong.append((c.id, name, R.expected_name(c)))
        # a request the planner cannot honour is declared as such, and only those are
        asked = {"p3": "p3", "p4": "p4", "ring": "ring", "ring128": "ring128", "ws": "ws", "ws64": "ws64"}.get(c.kernel)
        if asked is not None and c.family != asked:
            assert c.fallback and c.family in ("reg64", "reg128"), c.id
        if c.fallback:
            assert c.family in ("reg64", "reg128"), c.id
    assert not wrong, wrong


def _source_lists():
    """The instantiation lists of the sources: macro name -> epilogue numbers."""
    out = {}
    for fn in ("gemm_common.h", "gemm.hip", "gemm_ws.hip"):
        with open(os.path.join(CSRC, fn)) as f:
            text = f.read().replace("\\\n", " ")
        for m in re.finditer(r"^#define\s+(ASRX_EPI\w*)\(X\)(.*)$", text, re.M):
            out[m.group(1)] = [eval(e, {"__builtins__": {}}, dict(R.E_NAMES)) for e in re.findall(r"X\(([^()]*)\)", m.group(2))]
    return out


def test_restated_epilogue_lists_match_the_sources():
    src = _source_lists()
    assert sorted(src) == ["ASRX_EPI4_NN", "ASRX_EPI4_NT", "ASRX_EPI4_TT", "ASRX_EPIWS_NN", "ASRX_EPIWS_NT",
                           "ASRX_EPI_NN", "ASRX_EPI_NT", "ASRX_EPI_TT"]
    for name, mine in (("ASRX_EPI_NT", R.EPI_NT), ("ASRX_EPI_NN", R.EPI_NN), ("ASRX_EPI_TT", R.EPI_TT),
                       ("ASRX_EPI4_NT", R.EPI4_NT), ("ASRX_EPI4_NN", R.EPI4_NN), ("ASRX_EPI4_TT", R.EPI4_TT),
                       ("ASRX_EPIWS_NT", R.EPIWS_NT), ("ASRX_EPIWS_NN", R.EPIWS_NN)):
        assert sorted(src[name]) == sorted(mine), name


def test_table_reaches_every_family_layout_and_epilogue(built, capsys):
    """Every family name, every instantiated epilogue on each family that has it (from the planned names, not the
    declarations), and the layouts each family takes.  Prints the coverage per family."""
    reached = collections.defaultdict(lambda: collections.defaultdict(set))   # family -> layout -> epilogue numbers
    for c, b in built:
        name = _planned(b)
        fam, epi = R.parse_name(name)
        reached[fam][R._lname(c.at, c.bt)].add(epi)
    assert set(R.FAMILIES) <= set(reached), sorted(set(R.FAMILIES) - set(reached))
    src = _source_lists()
    lists = {"p3": ("ASRX_EPI_NT", "ASRX_EPI_NN", "ASRX_EPI_TT"), "p4": ("ASRX_EPI4_NT", "ASRX_EPI4_NN", "ASRX_EPI4_TT"),
             "ring": ("ASRX_EPI_NT", "ASRX_EPI_NN"), "ring128": ("ASRX_EPI_NT", "ASRX_EPI_NN"),
             "ws": ("ASRX_EPIWS_NT", "ASRX_EPIWS_NN"), "ws64": ("ASRX_EPIWS_NT", "ASRX_EPIWS_NN")}
    missing = []
    for fam, names in lists.items():
        for name in names:
            lay = name[-2:]
            missing += [(fam, lay, e) for e in src[name] if e not in reached[fam][lay]]
        if fam in ("p3", "ring", "ring128"):
            assert R.E_GENERIC in set().union(*reached[fam].values()), fam   # and the generic epilogue
    assert not missing, missing
    for fam in ("reg64", "reg128"):
        assert set(reached[fam]) == {"NT", "NN", "TN", "TT"}, fam
    assert set(reached["p3"]) == {"NT", "NN", "TN", "TT"} and set(reached["p4"]) == {"NT", "NN", "TT"}
    with capsys.disabled():
        print()
        for fam in list(R.FAMILIES) + ["f32"]:
            per = ", ".join(f"{lay}: {['generic' if e == R.E_GENERIC else e for e in sorted(e for e in es if e is not None)] or '-'}" for lay, es in sorted(reached[fam].items()))
            print(f"  {fam:8s} {sum(1 for c, _ in built if c.family == fam):4d} cases  {per}")


def test_grouped_references():
    for beta in (0.0, 1.0):
        groups = R.make_groups(beta, 7)
        assert len(groups) == 5 and sum(g.expect_b is not None for g in groups) == 3
        for g in groups:
            assert torch.isfinite(g.expect_w).all()
            for name in ("dy", "x"):
                idx = torch.from_numpy(g.lay[name].index().reshape(-1))
                assert int(torch.isnan(g.bufs[name].float()).sum()) == g.bufs[name].numel() - idx.numel()
