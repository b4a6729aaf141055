"""asrx_logmel, asrx_cmvn and asrx_feature_stats on the device against the float64 numpy restatement
(tests/fbank_ref.py; the rule is DESIGN.md §17).

Bounds.  Linear mel energies: max|out - ref| / max|ref| < 2e-5, the criterion tests/test_features.py applies to the
spectrogram.  Log output, elementwise: |out - ref| <= log_mul * (4e-5 * max(e_ref) / (e_ref + log_eps) + 1e-6) — the
linear bound with a factor 2 pushed through the derivative of the log; where the reference energy is exactly 0 the
output equals log_mul * log(log_eps) to 1e-6 relative.  Fused global CMVN: that bound times istd[m], plus
1e-6 * (1 + |ref|).  asrx_cmvn: |out - ref| <= 5e-5 * (1 + |ref|) (a tree reduction over at most 2^12 frames costs
about 12 roundings of 2^-24 on quantities up to (|mean| + 4 sigma) / sigma <= 10: about 7e-6, taken with a factor 7;
the longer row of the off-chip case adds one rounding).  asrx_feature_stats: 1e-12 relative on the fp64 sums."""
import functools
import math

import numpy as np
import pytest
import torch

import fbank_ref as R

pytestmark = pytest.mark.gpu

# name: (shape, n_fft, hop, n_mels, LogMel keywords beyond those)
CASES = {
    "c1": ((3, 7001), 400, 160, 23, {}),          # 42 frames (ragged 2nd frame tile), 201 bins (ragged chunk), 23 mels
    "c2": ((2, 16000), 1024, 512, 80, {}),        # the headline geometry, 30 frames
    "c3": ((2, 4000), 64, 32, 40, {}),            # 33 bins < one chunk, 7 empty filters, one-bin filters
    "c4": ((1, 400), 400, 160, 23, {}),           # exactly one frame
    "c5": ((2, 7001), 400, 160, 80, dict(norm="slaney", mel_scale="slaney", power=1, normalized=True)),
}
LOG_COMBOS = [(log, mode, eps) for log in ("ln", "log10") for mode in ("add", "clamp") for eps in (1e-6, 1e-10)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(waveform fp32 numpy, float64 filterbank, reference mel energies float64 (B, n_mels, frames))"""
    shape, n_fft, hop, n_mels, kw = CASES[name]
    x = R.waveform(shape, seed=list(CASES).index(name) + 1)
    fb = R.melscale_fbanks(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000, kw.get("norm"), kw.get("mel_scale", "htk"))
    e = R.mel_energies(x, fb, n_fft, hop, power=float(kw.get("power", 2)), normalized=kw.get("normalized", False))
    e.setflags(write=False)
    return x, fb, e


def _module(name, **extra):
    from asrx.features import LogMel
    _, n_fft, hop, n_mels, kw = CASES[name]
    return LogMel(n_fft=n_fft, hop_length=hop, n_mels=n_mels, **{**kw, **extra})


def _np(t):
    return t.detach().cpu().double().numpy()


def _log_bound(e_ref, log, eps):
    return R.log_mul(log) * (4e-5 * e_ref.max() / (e_ref + eps) + 1e-6)


def _check_log(out, e_ref, log, mode, eps, what):
    ref = R.apply_log(e_ref, log, eps, mode)
    err = np.abs(out - ref)
    bound = _log_bound(e_ref, log, eps)
    worst = float((err / bound).max())
    print(f"{what} {log} {mode} eps={eps:g}: max err/bound {worst:.3g}")
    assert (err <= bound).all(), (what, log, mode, eps, worst)
    zero = e_ref == 0.0
    if zero.any():
        want = R.log_mul(log) * math.log(eps)
        assert np.abs(out[zero] - want).max() <= 1e-6 * abs(want), (what, log, mode, eps)


@pytest.mark.parametrize("name", list(CASES))
def test_linear_mel_energies(name):
    _gpu()
    x, _, e_ref = _case(name)
    out = _module(name, log=None)(torch.from_numpy(x).cuda())
    assert out.dtype == torch.float32 and tuple(out.shape) == e_ref.shape
    err = np.abs(_np(out) - e_ref).max() / np.abs(e_ref).max()
    print(f"{name}: linear max|out - ref| / max|ref| = {err:.3g}")
    assert err < 2e-5, err
    if name == "c3":
        empty = ~R.melscale_fbanks(33, 0.0, 8000.0, 40, 16000).any(axis=0)
        assert int(empty.sum()) == 7 and float(out[:, torch.from_numpy(empty).cuda()].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_log_mel(name):
    _gpu()
    x, _, e_ref = _case(name)
    xg = torch.from_numpy(x).cuda()
    for log, mode, eps in LOG_COMBOS:
        out = _module(name, log=log, log_mode=mode, log_eps=eps)(xg)
        _check_log(_np(out), e_ref, log, mode, eps, name)


@pytest.mark.parametrize("name", ["c1", "c3", "c5"])
def test_channel_dimension(name):
    """(B, 1, time) in gives (B, 1, n_mels, frames) out, the same numbers as the 2-D call."""
    _gpu()
    x, _, e_ref = _case(name)
    m = _module(name)
    xg = torch.from_numpy(x).cuda()
    flat = m(xg)
    out = m(xg.unsqueeze(1))
    assert tuple(out.shape) == (e_ref.shape[0], 1) + e_ref.shape[1:]
    assert torch.equal(out[:, 0], flat)
    _check_log(_np(flat), e_ref, "ln", "add", 1e-6, name + " 3-D")
    out, fl = m(xg.unsqueeze(1), lengths=[x.shape[-1]] * x.shape[0])
    assert fl.dtype == torch.int32 and fl.is_cuda and fl.tolist() == [e_ref.shape[-1]] * x.shape[0]
    assert torch.equal(out[:, 0], flat)


def test_custom_filterbanks():
    """Case 6: a dense random filterbank (ranges [0, nbins)) and one with negative entries, case 1's geometry."""
    _gpu()
    x, _, _ = _case("c1")
    xg = torch.from_numpy(x).cuda()
    g = torch.Generator().manual_seed(6)
    dense = torch.rand(201, 23, generator=g) + 0.01
    signed = torch.randn(201, 23, generator=g)
    signed[:40, 3] = 0.0
    signed[:, 7] = 0.0
    for fb, logs in ((dense, [None, "ln"]), (signed, [None])):
        e_ref = R.mel_energies(x, fb.double().numpy(), 400, 160)
        for log in logs:
            m = _module("c1", filterbank=fb, log=log)
            if fb is dense:
                assert m.fb_range.tolist() == [[0, 201]] * 23
            else:
                assert m.fb_range[3].tolist() == [40, 201] and m.fb_range[7].tolist() == [0, 0]
            out = _np(m(xg))
            if log is None:
                err = np.abs(out - e_ref).max() / np.abs(e_ref).max()
                print(f"custom filterbank linear: {err:.3g}")
                assert err < 2e-5, err
            else:
                _check_log(out, e_ref, "ln", "add", 1e-6, "dense")


def test_second_passes_alone():
    """asrx_logmel_pass on the workspace asrx_logmel left gives asrx_logmel's output bit for bit, and
    asrx_stft_power on it gives Spectrogram's."""
    _gpu()
    from asrx import kernels as K
    from asrx.features import Spectrogram
    x, _, _ = _case("c1")
    xg = torch.from_numpy(x).cuda()
    m = _module("c1")
    basis, fb = m._constants(xg.device)
    B, frames, nb = 3, 42, 201
    ws = torch.empty(B * frames * 2 * nb, device="cuda")
    out = torch.empty(B, 23, frames, device="cuda")
    wl = torch.tensor([7001, 399, 560], dtype=torch.int32, device="cuda")
    kw = dict(n_fft=400, hop=160, wave_lengths=wl, log_mode=1, pad_value=-7.5)
    K.logmel(xg, basis, fb, m.fb_range, out, ws, **kw)
    again, fl = torch.empty_like(out), torch.empty(B, dtype=torch.int32, device="cuda")
    K.logmel_pass(ws, fb, m.fb_range, again, frame_lengths=fl, **kw)
    assert torch.equal(again, out) and fl.tolist() == [42, 0, 2]
    spec = torch.empty(B, nb, frames, device="cuda")
    K.stft_power(ws, spec)
    assert torch.equal(spec, Spectrogram(n_fft=400, hop_length=160, center=False)(xg))


@pytest.mark.parametrize("pad_value", [0.0, -7.5])
def test_lengths_and_padding(pad_value):
    _gpu()
    x, _, e_ref = _case("c1")
    xg = torch.from_numpy(x).cuda()
    lengths = [7001, 399, 560]
    want = [42, 0, 2]
    for log in (None, "ln"):
        m = _module("c1", log=log, pad_value=pad_value)
        out, fl = m(xg, lengths=torch.tensor(lengths))
        assert fl.dtype == torch.int32 and fl.is_cuda and fl.tolist() == want
        assert m.frame_lengths(lengths) == want
        full = m(xg)
        assert torch.equal(out[0], full[0])                      # a full-length row: bit-identical
        o = _np(out)
        for b, n in enumerate(want):
            assert (o[b, :, n:] == pad_value).all()
            if n == 0:
                continue
            if log is None:
                assert np.abs(o[b, :, :n] - e_ref[b, :, :n]).max() / np.abs(e_ref).max() < 2e-5
            else:
                ref = R.apply_log(e_ref, "ln", 1e-6, "add")
                assert (np.abs(o[b, :, :n] - ref[b, :, :n]) <= _log_bound(e_ref, "ln", 1e-6)[b, :, :n]).all()
    # frame lengths longer than the batch clamp to its frames
    _, fl = _module("c1")(xg, lengths=[99999, 7001, 400])
    assert fl.tolist() == [42, 42, 1]


def _global_cmvn(mean, istd):
    """A finalised global CMVN holding the given statistics (through its state_dict)."""
    from asrx.features import CMVN
    n = len(mean)
    cm = CMVN(n, mode="global", norm_var=istd is not None)
    cm.load_state_dict({"sum": torch.zeros(n, dtype=torch.float64), "sumsq": torch.zeros(n, dtype=torch.float64),
                        "count": torch.ones(1, dtype=torch.int64), "mean": torch.from_numpy(mean),
                        "istd": torch.from_numpy(istd) if istd is not None else torch.ones(n),
                        "finalized": torch.ones(1, dtype=torch.uint8)})
    return cm.cuda()


@pytest.mark.parametrize("with_istd", [True, False])
def test_fused_global_cmvn(with_istd):
    _gpu()
    x, fb, e_ref = _case("c1")
    rng = np.random.default_rng(5)
    mean = rng.uniform(-4.0, 1.0, 23).astype(np.float32)
    istd = rng.uniform(0.3, 2.5, 23).astype(np.float32) if with_istd else None
    lengths = [7001, 399, 560]
    m = _module("c1", cmvn=_global_cmvn(mean, istd), pad_value=-7.5)
    out, fl = m(torch.from_numpy(x).cuda(), lengths=lengths)
    ref, _, rfl = R.logmel(x, fb, 400, 160, mean=mean, istd=istd, lengths=lengths, pad_value=-7.5)
    assert fl.tolist() == rfl.tolist()
    o = _np(out)
    scale = istd.astype(np.float64)[None, :, None] if with_istd else 1.0
    bound = _log_bound(e_ref, "ln", 1e-6) * scale + 1e-6 * (1.0 + np.abs(ref))
    for b, n in enumerate(rfl):
        assert (o[b, :, n:] == -7.5).all()
        assert (np.abs(o[b, :, :n] - ref[b, :, :n]) <= bound[b, :, :n]).all()


# ------------------------------------------------------------------------------------------- asrx_cmvn

def _features(shape, seed):
    """Random features whose rows have a mean in [-3, 3] and a sigma in [0.5, 2]; fp32."""
    rng = np.random.default_rng(seed)
    B, F, T = shape
    mu = rng.uniform(-3.0, 3.0, (B, F, 1))
    sd = rng.uniform(0.5, 2.0, (B, F, 1))
    return (mu + sd * rng.standard_normal(shape)).astype(np.float32)


CMVN_SHAPES = [((3, 23, 42), [42, 0, 1]), ((2, 80, 1000), [1000, 777]), ((1, 5, 1), None),
               ((2, 3, 5000), [5000, 4097])]     # rows beyond the 4096 frames a workgroup holds in registers


@pytest.mark.parametrize("shape,lengths", CMVN_SHAPES, ids=[str(s[0]) for s in CMVN_SHAPES])
@pytest.mark.parametrize("norm_var", [True, False])
def test_cmvn_utterance(shape, lengths, norm_var):
    _gpu()
    from asrx.features import CMVN
    x = _features(shape, seed=sum(shape))
    xg = torch.from_numpy(x).cuda()
    cm = CMVN(shape[1], mode="utterance", norm_var=norm_var, pad_value=-2.0).cuda()
    out = cm(xg, lengths=lengths)
    again = cm(xg, lengths=lengths)
    assert torch.equal(out, again)                               # deterministic
    assert torch.equal(xg, torch.from_numpy(x).cuda())           # the input is left alone
    inplace = xg.clone()
    assert cm(inplace, lengths=lengths, out=inplace) is inplace and torch.equal(inplace, out)
    four = cm(xg.unsqueeze(1), lengths=lengths)
    assert tuple(four.shape) == (shape[0], 1) + shape[1:] and torch.equal(four[:, 0], out)
    ref = R.cmvn_utterance(x, lengths, norm_var=norm_var, eps=1e-5, pad_value=-2.0)
    o = _np(out)
    valid = np.zeros(shape, dtype=bool)
    for b in range(shape[0]):
        valid[b, :, :(shape[2] if lengths is None else lengths[b])] = True
    assert (o[~valid] == -2.0).all()                             # pad frames exact, a length-0 row all pad
    err = np.abs(o - ref)[valid] / (1.0 + np.abs(ref[valid]))
    print(f"cmvn {shape} norm_var={norm_var}: max err / (1 + |ref|) = {err.max():.3g}")
    assert (err <= 5e-5).all(), float(err.max())
    if lengths is not None and 1 in lengths:
        assert (o[lengths.index(1), :, 0] == 0.0).all()          # a length-1 row gives zeros
    if shape[2] == 1:
        assert (o == 0.0).all()


def test_cmvn_global_module_matches_the_restatement():
    _gpu()
    rng = np.random.default_rng(9)
    x = _features((2, 23, 42), seed=11)
    mean = rng.uniform(-3.0, 3.0, 23).astype(np.float32)
    istd = rng.uniform(0.5, 2.0, 23).astype(np.float32)
    for sd in (istd, None):
        cm = _global_cmvn(mean, sd)
        out = _np(cm(torch.from_numpy(x).cuda(), lengths=[42, 17]))
        ref = R.cmvn_global(x, mean, sd, lengths=[42, 17], pad_value=0.0)
        assert (out[1, :, 17:] == 0.0).all()
        assert (np.abs(out - ref) <= 1e-6 * (1.0 + np.abs(ref))).all()


# ---------------------------------------------------------------------------------- asrx_feature_stats

def test_feature_stats_and_finalize():
    _gpu()
    from asrx.features import CMVN
    batches = [(_features((3, 23, 42), seed=1), [42, 0, 17]), (_features((2, 23, 1000), seed=2), [1000, 777]),
               (_features((1, 23, 5), seed=3), None)]
    runs = []
    for _ in range(2):
        cm = CMVN(23, mode="global").cuda()
        for x, lengths in batches:
            cm.accumulate(torch.from_numpy(x).cuda(), lengths=lengths)
        runs.append((cm.sum.clone(), cm.sumsq.clone(), cm.count.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))          # two runs bit-identical
    s, q, n = R.feature_sums(batches)
    assert int(cm.count) == n == 42 + 17 + 1777 + 5
    rel_s, rel_q = np.abs(_np(cm.sum) - s) / np.abs(s), np.abs(_np(cm.sumsq) - q) / np.abs(q)
    print(f"feature_stats: max relative error {rel_s.max():.3g} (sum), {rel_q.max():.3g} (sum of squares)")
    assert (rel_s <= 1e-12).all() and (rel_q <= 1e-12).all()
    with pytest.raises(RuntimeError):
        cm(torch.from_numpy(batches[0][0]).cuda())                # global CMVN before finalize()
    cm.finalize()
    mean, istd = R.finalize(s, q, n)
    assert np.abs(_np(cm.mean) - mean).max() <= 1e-6 and (np.abs(_np(cm.istd) - istd) <= 1e-6 * istd).all()


# --------------------------------------------------------------------------------------- argument checks

def test_argument_checks_return_before_any_launch():
    _gpu()
    import asrx
    lib = asrx.native()
    B, S, n_fft, hop, nb, M = 2, 2000, 400, 160, 201, 23
    frames = (S - n_fft) // hop + 1
    dev = dict(device="cuda", dtype=torch.float32)
    audio, basis, fb = torch.zeros(B, S, **dev), torch.zeros(2 * nb, n_fft, **dev), torch.zeros(nb, M, **dev)
    ws, out = torch.zeros(B * frames * 2 * nb, **dev), torch.zeros(B, M, frames, **dev)
    rng = torch.tensor([[0, nb]] * 257, dtype=torch.int32)
    torch.cuda.synchronize()

    def logmel(**kw):
        a = dict(audio=audio.data_ptr(), batch=B, samples=S, stride=S, wl=None, basis=basis.data_ptr(), n_fft=n_fft,
                 hop=hop, nbins=nb, power=2, scale=1.0, fb=fb.data_ptr(), rng=rng.data_ptr(), n_mels=M, log_mode=1,
                 log_mul=1.0, log_eps=1e-6, mean=None, istd=None, pad=0.0, ws=ws.data_ptr(), ws_elems=ws.numel(),
                 out=out.data_ptr(), fl=None)
        a.update(kw)
        return lib.asrx_logmel(*a.values(), None)

    assert lib.asrx_version() >= 12
    assert logmel() == 0 and logmel(batch=0) == 0
    for name in ("audio", "basis", "fb", "rng", "ws", "out"):
        assert logmel(**{name: None}) == -1, name
    assert logmel(n_mels=257) == -3 and logmel(n_mels=0) == -1
    for bad in ([5, 4], [0, nb + 1], [-1, 3]):
        r = rng.clone()
        r[M - 1] = torch.tensor(bad, dtype=torch.int32)
        assert logmel(rng=r.data_ptr()) == -1, bad
    r = rng.clone()
    r[M] = torch.tensor([9, 2], dtype=torch.int32)                # beyond n_mels: not read
    assert logmel(rng=r.data_ptr()) == 0
    assert logmel(ws_elems=ws.numel() - 1) == -1
    assert logmel(log_eps=0.0) == -1 and logmel(log_eps=-1.0) == -1 and logmel(log_mode=0, log_eps=0.0) == 0
    assert logmel(log_mode=3) == -1 and logmel(power=3) == -1 and logmel(samples=n_fft - 1) == -1
    assert logmel(istd=fb.data_ptr()) == -1                       # istd without mean
    assert logmel(batch=65536, ws_elems=1 << 40) == -3

    def second(**kw):
        a = dict(ws=ws.data_ptr(), batch=B, frames=frames, wl=None, n_fft=n_fft, hop=hop, nbins=nb, power=2, scale=1.0,
                 fb=fb.data_ptr(), rng=rng.data_ptr(), n_mels=M, log_mode=1, log_mul=1.0, log_eps=1e-6, mean=None,
                 istd=None, pad=0.0, out=out.data_ptr(), fl=None)
        a.update(kw)
        return lib.asrx_logmel_pass(*a.values(), None)

    assert second() == 0 and second(batch=0) == 0
    assert second(ws=None) == -1 and second(out=None) == -1 and second(fb=None) == -1 and second(rng=None) == -1
    assert second(frames=0) == -1 and second(n_mels=257) == -3 and second(log_eps=0.0) == -1
    spec = torch.zeros(B, nb, frames, **dev)
    assert lib.asrx_stft_power(ws.data_ptr(), B, frames, nb, 2, 1.0, spec.data_ptr(), None) == 0
    assert lib.asrx_stft_power(None, B, frames, nb, 2, 1.0, spec.data_ptr(), None) == -1
    assert lib.asrx_stft_power(ws.data_ptr(), B, frames, nb, 3, 1.0, spec.data_ptr(), None) == -1
    assert lib.asrx_stft_power(ws.data_ptr(), 0, frames, nb, 2, 1.0, spec.data_ptr(), None) == 0

    buf = torch.zeros(2 * 5 * 8 + 8, **dev)
    x = buf.data_ptr()

    def cmvn(xp=x, op=x, B=2, F=5, T=8, xb=40, ob=40, mean=None, istd=None, norm_var=1, eps=1e-5):
        return lib.asrx_cmvn(xp, op, B, F, T, xb, ob, None, mean, istd, norm_var, eps, 0.0, None)

    assert cmvn() == 0 and cmvn(B=0) == 0                         # in place is allowed
    assert cmvn(op=x + 16) == -1 and cmvn(xp=x + 16, op=x) == -1  # overlapping, unequal
    assert cmvn(xp=None) == -1 and cmvn(op=None) == -1 and cmvn(op=x + 2) == -1
    assert cmvn(F=0) == -1 and cmvn(T=0) == -1 and cmvn(xb=39) == -1 and cmvn(eps=0.0) == -1
    assert cmvn(istd=x) == -1 and cmvn(B=65536) == -3
    acc = torch.zeros(5, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def stats(xp=x, s=acc.data_ptr(), q=acc.data_ptr(), c=cnt.data_ptr(), B=2, F=5, T=8, xb=40):
        return lib.asrx_feature_stats(xp, B, F, T, xb, None, s, q, c, None)

    assert stats(B=0) == 0
    assert stats(xp=None) == -1 and stats(s=None) == -1 and stats(q=None) == -1 and stats(c=None) == -1
    assert stats(F=0) == -1 and stats(xb=39) == -1
    torch.cuda.synchronize()
