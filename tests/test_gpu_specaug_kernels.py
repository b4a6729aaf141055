"""asrx_specaug on the device against the numpy restatement (tests/specaug_ref.py): every plan and every masks-only
output bitwise, warped frames within 8 * 2^-24 * (|a| + |b|) of the float64 reference — one rounding each in frac, the
difference, the product (or the FMA the build's -ffp-contract=fast makes of it) and the sum, with margin — and the
padding bit for bit the input."""
import numpy as np
import pytest
import torch

from tests import specaug_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"

BASE = dict(freq_masks=2, freq_width=3, time_masks=2, time_width=10, time_ratio=0.2)
BASE_LENGTHS = [61, 30, 7]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _x(B, F, T, seed=0):
    return np.random.default_rng(seed).standard_normal((B, 1, F, T)).astype(np.float32)


@pytest.fixture(scope="module")
def base_x():
    return _x(3, 5, 61)


def _run(x, lengths=None, *, mask_value=0.0, seed=0, step=0, src=None, **kw):
    """(device output as numpy, device plan as numpy, reference output, reference |a| + |b|, reference plan)"""
    import asrx
    aug = asrx.SpecAugment(mask_value=mask_value, seed=seed, **kw)
    xs = torch.from_numpy(x).to(dev) if src is None else src
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    got = aug(xs, lengths=lens, step=step)
    plan = aug.plan(x.shape[0], x.shape[2], x.shape[3], lengths=lens, step=step)
    torch.cuda.synchronize()
    assert _bitwise(xs.cpu().numpy(), x), "the input was written"
    want, mag, P = R.specaug(x, lengths, mask_value=mask_value, seed=seed, step=step, **kw)
    return got.cpu().numpy(), plan.cpu().numpy(), want, mag, P


def _bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                          np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _check(got, plan, want, mag, P, x, lengths):
    """plan bitwise; copied and masked elements bitwise; warped ones within the bound; padding the input's bits"""
    assert np.array_equal(plan, P)
    exact = mag == 0
    assert _bitwise(np.where(exact, got, 0), np.where(exact, want, 0))
    err = np.abs(got.astype(np.float64) - want)
    bound = 8 * 2.0 ** -24 * mag
    assert (err <= bound).all(), float((err - bound).max())
    for b in range(x.shape[0]):
        L = x.shape[3] if lengths is None else min(max(lengths[b], 0), x.shape[3])
        assert _bitwise(got[b, :, :, L:], x[b, :, :, L:])


def test_base_case_masks_only(base_x):
    got, plan, want, mag, P = _run(base_x, BASE_LENGTHS, seed=1234, step=1, **BASE)
    assert not mag.any() and np.array_equal(plan, P)
    assert _bitwise(got, want)
    assert (got != base_x).any()
    _check(got, plan, want, mag, P, base_x, BASE_LENGTHS)


def test_base_case_with_warp(base_x):
    got, plan, want, mag, P = _run(base_x, BASE_LENGTHS, seed=1234, step=1, time_warp=5, **BASE)
    assert P[0, 2] > 0 and P[1, 2] > 0 and tuple(P[2, :3]) == (7, 0, 0)   # the row of length 7 gets no warp
    assert mag[0].any() and mag[1].any() and not mag[2].any()
    _check(got, plan, want, mag, P, base_x, BASE_LENGTHS)
    # the warp moved something: frames differ from the masks-only result
    plain = _run(base_x, BASE_LENGTHS, seed=1234, step=1, **BASE)[0]
    assert (plain[0] != got[0]).any() and _bitwise(plain[2], got[2])


def test_vector_and_scalar_paths_agree_bitwise():
    """(2, 8, 64) without lengths: 16-B aligned rows take the 16-B path; the same data through a view that starts one
    element into a larger buffer takes the 4-B path.  Both equal the reference bit for bit."""
    x = _x(2, 8, 64, seed=3)
    kw = dict(freq_masks=2, freq_width=3, time_masks=2, time_width=10, time_ratio=1.0)
    got, plan, want, mag, P = _run(x, None, seed=77, step=2, **kw)
    assert got.shape == x.shape and _bitwise(got, want) and np.array_equal(plan, P)
    assert (got != x).any()
    big = torch.zeros(x.size + 8, dtype=torch.float32, device=dev)
    view = big[1:1 + x.size].view(2, 1, 8, 64)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4
    got2 = _run(x, None, seed=77, step=2, src=view, **kw)[0]
    assert _bitwise(got2, want)
    # and into a misaligned destination
    import asrx
    out = torch.zeros(x.size + 8, dtype=torch.float32, device=dev)
    dst = out[3:3 + x.size].view(2, 1, 8, 64)
    asrx.SpecAugment(seed=77, **kw)(torch.from_numpy(x).to(dev), out=dst, step=2)
    assert _bitwise(dst.cpu().numpy(), want)
    assert not out[:3].any() and not out[3 + x.size:].any()


@pytest.mark.parametrize("warp", [0, 5])
def test_utterance_longer_than_one_run(warp):
    """T = one workgroup's run of frames + 7, F = 3 (fewer rows than a workgroup covers): with seed 3728 (found with
    the reference) the warp point c and a time mask both lie beyond the first run."""
    from asrx._lib import SPECAUG_RUN
    T = SPECAUG_RUN + 7
    x = _x(1, 3, T, seed=4)
    kw = dict(freq_masks=1, freq_width=1, time_masks=8, time_width=6, time_ratio=1.0, time_warp=warp)
    got, plan, want, mag, P = _run(x, None, seed=3728, step=1, **kw)
    tm = P[0, 6:].reshape(8, 2)
    assert any(t0 >= SPECAUG_RUN and w >= 1 for t0, w in tm)
    if warp:
        assert P[0, 2] >= SPECAUG_RUN and mag[0, 0, :, SPECAUG_RUN:].any()
    _check(got, plan, want, mag, P, x, None)
    assert (got[0, 0, :, SPECAUG_RUN:] != x[0, 0, :, SPECAUG_RUN:]).any()


def test_nothing_to_do_is_a_bitwise_copy(base_x):
    x = base_x.copy()
    x.view(np.uint32)[0, 0, 0, :3] = [0x7FC01234, 0xFF800000, 0x80000000]   # a NaN payload, -inf, -0.0
    got, plan, want, mag, P = _run(x, BASE_LENGTHS, seed=5, step=3, freq_masks=0, time_masks=0, time_warp=0)
    assert plan.shape == (3, 4) and np.array_equal(plan, P)
    assert _bitwise(got, x)


def test_eight_masks_of_each_kind():
    x = _x(2, 40, 200, seed=5)
    kw = dict(freq_masks=8, freq_width=4, time_masks=8, time_width=12, time_ratio=1.0)
    lengths = [200, 150]
    got, plan, want, mag, P = _run(x, lengths, seed=99, step=1, mask_value=-2.5, **kw)
    assert plan.shape == (2, 36)
    assert (P[:, 5:20:2] > 0).any() and (P[:, 21:36:2] > 0).any()
    _check(got, plan, want, mag, P, x, lengths)
    assert (got == -2.5).any()
    got, plan, want, mag, P = _run(x, lengths, seed=99, step=1, mask_value=-2.5, time_warp=30, **kw)
    _check(got, plan, want, mag, P, x, lengths)


def test_frequency_width_above_the_rows(base_x):
    kw = dict(freq_masks=2, freq_width=27, time_masks=0, time_width=0)
    seen = set()
    for seed in range(6):
        got, plan, want, mag, P = _run(base_x, BASE_LENGTHS, seed=seed, step=1, **kw)
        assert (P[:, 5] <= 5).all() and (P[:, 4] + P[:, 5] <= 5).all()
        seen |= set(P[:, 5].tolist()) | set(P[:, 7].tolist())
        _check(got, plan, want, mag, P, base_x, BASE_LENGTHS)
    assert 5 in seen    # a mask over every row occurs (the reference says so: no device result decides this)


@pytest.mark.parametrize("warp", [0, 5])
def test_lengths_of_zero_and_above_t(base_x, warp):
    lengths = [0, 100, 61]
    got, plan, want, mag, P = _run(base_x, lengths, seed=1234, step=2, time_warp=warp, **BASE)
    assert P[:, 0].tolist() == [0, 61, 61]
    _check(got, plan, want, mag, P, base_x, lengths)
    assert _bitwise(got[0], base_x[0])        # nothing valid: the whole utterance is padding
    lengths = [-3, 61, 2_000_000_000]
    got, plan, want, mag, P = _run(base_x, lengths, seed=1234, step=2, time_warp=warp, **BASE)
    assert P[:, 0].tolist() == [0, 61, 61]
    _check(got, plan, want, mag, P, base_x, lengths)


def test_overlapping_masks(base_x):
    """Seed 8 (found with the reference): utterance 0's two frequency masks share row 4 and its two time masks share
    frames 27 .. 30."""
    got, plan, want, mag, P = _run(base_x, BASE_LENGTHS, seed=8, step=1, **BASE)
    assert P[0, 4:].tolist() == [4, 1, 2, 3, 26, 6, 27, 4]
    assert _bitwise(got, want) and np.array_equal(plan, P)
    assert not got[0, 0, 2:5, :61].any() and not got[0, 0, :, 26:32].any()
    assert got[0, 0, :2, :26].all() and got[0, 0, :2, 32:].all()


def test_same_seed_and_step_repeat_bitwise(base_x):
    kw = dict(seed=1234, step=3, time_warp=5, **BASE)
    a = _run(base_x, BASE_LENGTHS, **kw)
    b = _run(base_x, BASE_LENGTHS, **kw)
    assert _bitwise(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_steps_one_to_four_differ(base_x):
    import asrx
    aug = asrx.SpecAugment(seed=1234, time_warp=5, **BASE)
    lens = torch.tensor(BASE_LENGTHS, dtype=torch.int32, device=dev)
    plans = [aug.plan(3, 5, 61, lengths=lens, step=n).cpu().numpy() for n in (1, 2, 3, 4)]
    for n, p in zip((1, 2, 3, 4), plans):
        assert np.array_equal(p, R.plan(3, 5, 61, BASE_LENGTHS, seed=1234, step=n, time_warp=5, **BASE))
    assert len({p.tobytes() for p in plans}) == 4


def test_module_call_counter_and_modes(base_x):
    """step=None counts the module's own calls from 1; eval mode hands the input back; a non-dense view is taken
    through a dense copy; a wrong dtype or rank raises."""
    import asrx
    aug = asrx.SpecAugment(seed=1234, **BASE)
    x = torch.from_numpy(base_x).to(dev)
    a, b = aug(x), aug(x)
    assert aug.calls == 3
    assert _bitwise(a.cpu().numpy(), R.specaug(base_x, seed=1234, step=1, **BASE)[0])
    assert _bitwise(b.cpu().numpy(), R.specaug(base_x, seed=1234, step=2, **BASE)[0])
    assert aug.eval()(x) is x and aug.calls == 3
    aug.train()
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)       # frequency innermost in memory
    assert _bitwise(aug(xt, step=1).cpu().numpy(), a.cpu().numpy())
    with pytest.raises(ValueError):
        aug(x.double())
    with pytest.raises(ValueError):
        aug(x[:, 0])
    with pytest.raises(RuntimeError):
        aug(x, out=x)                                          # in place: refused by the library
