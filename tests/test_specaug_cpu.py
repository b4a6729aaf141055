"""SpecAugment, host side (no GPU): the invariants of the numpy restatement (tests/specaug_ref.py) that the device
tests compare against, asrx_specaug's argument checks (made before any HIP call), and the Python module's validation,
eval-mode identity and per-rank seed."""
import ctypes

import numpy as np
import pytest
import torch

from tests import specaug_ref as R

BASE = dict(freq_masks=2, freq_width=3, time_masks=2, time_width=10, time_ratio=0.2)


def test_reference_plans_stay_in_range():
    """Over 300 (seed, step) pairs: W <= w0 < L - W and 1 <= c <= L - 1 where a warp applies, none where L <= 2W,
    f0 + w <= F, w <= min(Wf, F), t0 + w <= L, w <= min(Wt, floor(ratio * L))."""
    F, T, W = 5, 40, 5
    lengths = [40, 11, 12, 39, 10, 0, 55]
    warped = 0
    for seed in range(100):
        for step in (0, 1, 77):
            P = R.plan(len(lengths), F, T, lengths, time_warp=W, seed=seed, step=step, **BASE)
            for b, row in enumerate(P):
                L, w0, c, zero = (int(v) for v in row[:4])
                assert L == min(max(lengths[b], 0), T) and zero == 0
                if L > 2 * W:
                    assert W <= w0 < L - W and 1 <= c <= L - 1 and w0 - W + 1 <= c <= w0 + W
                    warped += 1
                else:
                    assert (w0, c) == (0, 0)
                for j in range(2):
                    f0, w = (int(v) for v in row[4 + 2 * j:6 + 2 * j])
                    assert 0 <= w <= 3 and 0 <= f0 and f0 + w <= F
                    t0, w = (int(v) for v in row[8 + 2 * j:10 + 2 * j])
                    assert 0 <= w <= min(10, int(np.floor(np.float32(0.2) * np.float32(L)))) and 0 <= t0 and t0 + w <= L
    assert warped == 300 * 5   # lengths 40, 11, 12, 39 and 55 (clamped to 40); 10 and 0 are too short


def test_reference_steps_differ_and_short_rows_are_not_warped():
    """The base case of the device tests: the plans of steps 1-4 all differ, and the row of length 7 gets no warp."""
    plans = [R.plan(3, 5, 61, [61, 30, 7], time_warp=5, seed=1234, step=n, **BASE) for n in (1, 2, 3, 4)]
    assert len({p.tobytes() for p in plans}) == 4
    for p in plans:
        assert tuple(p[2, :3]) == (7, 0, 0) and p[0, 2] > 0 and p[1, 2] > 0
    # the step folds into the seed the way the dropout seed offset does; step 0 leaves the seed alone
    assert R.step_seed(1234, 0) == 1234 and R.step_seed(1234, 1) != R.step_seed(1234, 2)
    assert R.plan(2, 5, 61, seed=R.step_seed(9, 3), step=0, **BASE).tobytes() == \
        R.plan(2, 5, 61, seed=9, step=3, **BASE).tobytes()


def test_reference_skipped_warp_draws_keep_the_other_indices():
    """The masks of an utterance are the same draws with and without a warp (indices 0 and 1 stay reserved)."""
    a = R.plan(3, 5, 61, [61, 30, 7], time_warp=0, seed=5, step=2, **BASE)
    b = R.plan(3, 5, 61, [61, 30, 7], time_warp=5, seed=5, step=2, **BASE)
    assert np.array_equal(a[:, 4:], b[:, 4:]) and not np.array_equal(a[:, :4], b[:, :4])


def test_reference_warp_sources_and_identity():
    """Every source index lies in [0, L), i is monotone in t, the anchor frame c reads w0 exactly, and c == w0 is the
    identity warp (frac 0 everywhere)."""
    rng = np.random.default_rng(0)
    for _ in range(300):
        L = int(rng.integers(2, 200))
        w0 = int(rng.integers(0, L))
        c = int(rng.integers(1, L))
        i, i1, frac = R.warp_sources(L, w0, c)
        assert i.min() >= 0 and i.max() < L and i1.max() < L and (np.diff(i) >= 0).all()
        assert i[0] == 0 and frac[0] == 0 and i[c] == w0 and frac[c] == 0
        assert (frac >= 0).all() and (frac < 1).all()
        i, i1, frac = R.warp_sources(L, c, c)
        assert np.array_equal(i, np.arange(L)) and not frac.any()
    x = rng.standard_normal((1, 3, 20))
    P = np.array([[17, 6, 6, 0]], dtype=np.int32)
    out, mag = R.apply(x, P)
    assert np.array_equal(out, x)


def test_reference_leaves_padding_untouched():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 1, 5, 61)).astype(np.float32)
    lengths = [61, 30, 7]
    for seed in range(50):
        out, mag, P = R.specaug(x, lengths, time_warp=5, seed=seed, step=seed % 3, mask_value=-1.5, **BASE)
        for b, L in enumerate(lengths):
            assert np.array_equal(out[b, 0, :, L:], x[b, 0, :, L:].astype(np.float64))
            assert not mag[b, 0, :, L:].any()
        assert out.shape == x.shape and (out[1, 0, :, :30] != x[1, 0, :, :30]).any()


def _specaug(lib, src=4096, dst=1 << 20, B=2, F=5, T=61, sb=5 * 61, db=5 * 61, lengths=None, nF=2, Wf=3, nT=2, Wt=10,
             ratio=0.2, W=0, mask_value=0.0, seed=1, step=1, plan=None):
    return lib.asrx_specaug(src, dst, B, F, T, sb, db, lengths, nF, Wf, nT, Wt, ratio, W, mask_value, seed, step, plan,
                            None)


def test_abi_rejects_bad_arguments_without_gpu():
    """Every refusal of the header's list comes before any HIP call (fake, disjoint device addresses; no GPU here)."""
    import asrx
    lib = asrx.native()
    assert lib.asrx_version() >= 11
    ARG, UNSUP = -1, -3
    assert _specaug(lib, src=None) == ARG
    assert _specaug(lib, dst=None) == ARG
    assert _specaug(lib, dst=4096) == ARG                       # dst == src
    assert _specaug(lib, dst=4096 + 4 * 100) == ARG             # dst starts inside src's extent
    assert _specaug(lib, src=1 << 20, dst=(1 << 20) - 4 * 610 + 4) == ARG   # src starts inside dst's last element
    assert _specaug(lib, src=4098) == ARG                       # not an fp32 address
    assert _specaug(lib, F=0) == ARG
    assert _specaug(lib, T=0) == ARG
    assert _specaug(lib, B=-1) == ARG
    for k in ("nF", "Wf", "nT", "Wt", "W"):
        assert _specaug(lib, **{k: -1}) == ARG, k
    for ratio in (-0.01, 1.01, float("nan"), float("inf")):
        assert _specaug(lib, ratio=ratio) == ARG, ratio
    assert _specaug(lib, sb=5 * 61 - 1) == ARG                  # utterances overlap each other
    assert _specaug(lib, db=5 * 61 - 1) == ARG
    assert _specaug(lib, nF=9) == UNSUP
    assert _specaug(lib, nT=9) == UNSUP
    assert _specaug(lib, B=65536, dst=1 << 40) == UNSUP
    assert _specaug(lib, B=0) == 0                              # nothing to do, nothing launched
    assert _specaug(lib, B=0, dst=4096 + 4) == 0


def test_signature_matches_the_header():
    """The ctypes signature has one entry per parameter of the header's declaration, in its types."""
    import os
    import re
    from asrx._lib import SIGNATURES, SPECAUG_MAX_MASKS, SPECAUG_RUN
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "asrx.h")).read()
    decl = re.search(r"int asrx_specaug\((.*?)\);", src, re.S).group(1)
    kinds = []
    for p in decl.split(","):
        p = " ".join(p.split())
        if "*" in p:
            kinds.append(ctypes.c_void_p)
        else:
            kinds.append({"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
                          "float": ctypes.c_float}[p.split()[0]])
    assert SIGNATURES["asrx_specaug"] == kinds
    assert int(re.search(r"#define ASRX_SPECAUG_MAX_MASKS (\d+)", src).group(1)) == SPECAUG_MAX_MASKS
    assert int(re.search(r"#define ASRX_SPECAUG_RUN (\d+)", src).group(1)) == SPECAUG_RUN


def test_module_validates_its_arguments():
    import asrx
    aug = asrx.SpecAugment(seed=3)
    assert (aug.freq_masks, aug.freq_width, aug.time_masks, aug.time_width, aug.time_ratio, aug.time_warp,
            aug.mask_value, aug.seed, aug.calls) == (2, 27, 2, 100, 1.0, 0, 0.0, 3, 1)
    for bad in (dict(freq_masks=9), dict(time_masks=9), dict(freq_masks=-1), dict(time_masks=-1), dict(freq_width=-1),
                dict(time_width=-1), dict(time_warp=-1), dict(time_ratio=1.5), dict(time_ratio=-0.1),
                dict(time_ratio=float("nan")), dict(freq_masks=1.5), dict(time_warp=True), dict(seed=1.5)):
        with pytest.raises(ValueError):
            asrx.SpecAugment(**bad)
    assert asrx.SpecAugment(seed=-1).seed == (1 << 64) - 1
    assert asrx.SpecAugment(freq_masks=8, time_masks=8, time_ratio=0.0).time_masks == 8


def test_module_default_seed_is_torchs_and_advances_no_generator():
    import asrx
    torch.manual_seed(4321)
    state = torch.get_rng_state()
    aug = asrx.SpecAugment()
    assert aug.seed == 4321 == torch.initial_seed()
    assert torch.equal(torch.get_rng_state(), state)


def test_module_eval_is_the_identity_and_training_needs_a_gpu():
    import asrx
    aug = asrx.SpecAugment(seed=3)
    x = torch.randn(2, 1, 5, 61)
    assert aug.eval()(x) is x and aug.calls == 1
    aug.train()
    with pytest.raises(RuntimeError):
        aug(x)
    with pytest.raises(RuntimeError):
        aug.augment(x)


def test_rank_seed():
    from asrx.augment import rank_seed
    assert rank_seed(7, 0) == 7 and rank_seed(7, 3) == 10
    assert rank_seed((1 << 64) - 1, 2) == 1                    # wraps like the kernel's u64
    assert len({rank_seed(1234, r) for r in range(8)}) == 8
    with pytest.raises(ValueError):
        rank_seed(7, -1)
    # different ranks, different plans of the same step
    kw = dict(freq_masks=2, freq_width=3, time_masks=2, time_width=10, time_ratio=0.2, time_warp=5, step=1)
    assert R.plan(3, 5, 61, seed=rank_seed(1234, 0), **kw).tobytes() != \
        R.plan(3, 5, 61, seed=rank_seed(1234, 1), **kw).tobytes()


def test_trainer_rank_of_the_reducer():
    """The rank the trainer adds to the augmenter's seed: 0 without a process group; an injected all-reduce may carry
    its own."""
    import inspect
    from asrx.augment import rank_seed
    from asrx.dist import GradAllReduce
    from asrx.train import Trainer, reducer_rank
    assert reducer_rank(GradAllReduce(torch.zeros(8))) == 0

    def fake(view):
        pass
    assert reducer_rank(GradAllReduce(torch.zeros(8), allreduce_fn=fake)) == 0
    fake.rank = 3
    assert rank_seed(11, reducer_rank(GradAllReduce(torch.zeros(8), allreduce_fn=fake))) == 14
    assert inspect.signature(Trainer.__init__).parameters["spec_augment"].default is None
    assert inspect.signature(Trainer.step).parameters["input_lengths"].default is None
