"""Host side of the log-mel / CMVN features without a GPU: the product's mel filterbank against the
numpy restatement (tests/fbank_ref.py), the filterbank's structural properties, the bin ranges the kernel walks, the
frame-length rule, constructor validation and CMVN.finalize()'s arithmetic."""
import math

import numpy as np
import pytest
import torch

import fbank_ref as R

# (n_freqs, f_min, f_max, n_mels, sample_rate, norm, mel_scale)
CONFIGS = [
    (513, 0.0, 8000.0, 80, 16000, None, "htk"),
    (201, 0.0, 8000.0, 23, 16000, None, "htk"),
    (201, 0.0, 8000.0, 80, 16000, "slaney", "slaney"),
    (33, 0.0, 8000.0, 40, 16000, None, "htk"),
    (257, 20.0, 7600.0, 80, 16000, None, "htk"),
]
_ids = [f"{c[0]}-{c[3]}-{c[6]}" for c in CONFIGS]


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_melscale_fbanks_matches_the_restatement(cfg):
    from asrx.features import melscale_fbanks
    fb = melscale_fbanks(*cfg)
    assert fb.dtype == torch.float32 and fb.device.type == "cpu" and tuple(fb.shape) == (cfg[0], cfg[3])
    ref = R.melscale_fbanks(*cfg)
    assert np.abs(fb.double().numpy() - ref).max() < 1e-6


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_filterbank_structure(cfg):
    """Checked on the restatement: at most two filters on a bin, contiguous nonzeros, and with norm=None a partition
    of unity between the first and the last centre frequency."""
    n_freqs, f_min, f_max, n_mels, sr, norm, scale = cfg
    fb = R.melscale_fbanks(*cfg)
    assert ((fb != 0).sum(axis=1) <= 2).all()
    rng = R.filterbank_ranges(fb)
    for m in range(n_mels):
        lo, hi = rng[m]
        assert (fb[lo:hi, m] != 0).all() and not fb[:lo, m].any() and not fb[hi:, m].any()
    if norm is None:
        pts = R.mel_points(f_min, f_max, n_mels, scale)
        freqs = np.linspace(0, sr // 2, n_freqs)
        mid = (freqs >= pts[1]) & (freqs <= pts[-2])
        assert mid.any()
        assert np.abs(fb[mid].sum(axis=1) - 1.0).max() < 1e-12


def test_filterbank_widths_of_the_known_cases():
    from asrx.features import filterbank_ranges, melscale_fbanks
    rng = R.filterbank_ranges(R.melscale_fbanks(*CONFIGS[3]))           # 33 bins, 40 filters
    assert int((rng[:, 1] == rng[:, 0]).sum()) == 7
    rng = R.filterbank_ranges(R.melscale_fbanks(*CONFIGS[0]))           # 513 bins, 80 filters
    w = rng[:, 1] - rng[:, 0]
    assert (int(w.min()), int(w.max())) == (2, 34)
    for cfg in CONFIGS:                                                 # the product's ranges on its own matrices
        fb = melscale_fbanks(*cfg)
        got = filterbank_ranges(fb)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and tuple(got.shape) == (cfg[3], 2)
        assert np.array_equal(got.numpy(), R.filterbank_ranges(fb.numpy()))


def test_filterbank_ranges_dense_and_empty_columns():
    from asrx.features import filterbank_ranges
    g = torch.Generator().manual_seed(0)
    dense = torch.rand(33, 5, generator=g) + 0.1
    assert filterbank_ranges(dense).tolist() == [[0, 33]] * 5
    fb = torch.zeros(10, 4)
    fb[3:6, 0] = 1.0
    fb[9, 2] = -2.0          # negative entries count; column 1 and 3 stay empty
    fb[0, 3] = 0.0
    fb[2, 0] = 0.5
    fb[7, 0] = 0.25          # a hole inside the range stays inside it
    assert filterbank_ranges(fb).tolist() == [[2, 8], [0, 0], [9, 10], [0, 0]]
    assert np.array_equal(R.filterbank_ranges(fb.numpy()), filterbank_ranges(fb).numpy())


def test_mel_scales_round_trip_and_agree_below_1khz():
    from asrx.features import hz_to_mel, mel_to_hz
    f = np.linspace(0.0, 8000.0, 161)
    for scale in ("htk", "slaney"):
        for h2m, m2h in ((R.hz_to_mel, R.mel_to_hz),
                         (lambda v, s: hz_to_mel(torch.from_numpy(v), s).numpy(),
                          lambda v, s: mel_to_hz(torch.from_numpy(v), s).numpy())):
            back = m2h(np.asarray(h2m(f, scale)), scale)
            assert np.abs(back - f).max() < 1e-8
        assert np.abs(hz_to_mel(torch.from_numpy(f), scale).numpy() - R.hz_to_mel(f, scale)).max() < 1e-9
    low = f[f < 1000.0]
    assert np.abs(R.hz_to_mel(low, "slaney") - low / (200.0 / 3.0)).max() < 1e-12     # linear, 200/3 Hz per mel
    assert abs(float(R.hz_to_mel(1000.0, "slaney")) - 15.0) < 1e-12
    assert abs(float(R.hz_to_mel(6400.0, "slaney")) - 42.0) < 1e-9                    # 27 log steps of ln(6.4)/27
    assert abs(float(R.hz_to_mel(700.0, "htk")) - 2595.0 * math.log10(2.0)) < 1e-9


def test_frame_lengths_rule():
    from asrx.features import frame_lengths
    assert frame_lengths(399, 400, 160) == 0
    assert frame_lengths(400, 400, 160) == 1
    assert frame_lengths(559, 400, 160) == 1 and frame_lengths(560, 400, 160) == 2
    assert frame_lengths(0, 400, 160) == 0
    assert frame_lengths([7001, 399, 560], 400, 160) == [42, 0, 2]
    t = frame_lengths(torch.tensor([7001, 399, 560, 16000]), 400, 160)
    assert t.tolist() == [42, 0, 2, 98]
    assert R.frame_lengths([7001, 399, 560, 16000], 400, 160).tolist() == [42, 0, 2, 98]


def test_constructor_validation():
    from asrx.features import CMVN, LogMel, MelSpectrogram
    with pytest.raises(NotImplementedError):
        LogMel(center=True)
    with pytest.raises(ValueError):
        LogMel(log="log2")
    with pytest.raises(ValueError):
        LogMel(log_mode="floor")
    with pytest.raises(ValueError):
        LogMel(log_eps=0.0)
    with pytest.raises(ValueError):
        LogMel(sample_rate=16000, f_max=8000.5)
    with pytest.raises(ValueError):
        LogMel(n_fft=400, filterbank=torch.ones(200, 23))
    with pytest.raises(ValueError):
        LogMel(n_mels=257)
    with pytest.raises(ValueError):
        LogMel(n_mels=80, cmvn=CMVN(80, mode="utterance"))
    with pytest.raises(ValueError):
        LogMel(n_mels=80, cmvn=CMVN(40))
    with pytest.raises(ValueError):
        CMVN(80, mode="batch")
    m = LogMel()
    assert (m.n_fft, m.win_length, m.hop_length, m.n_mels, m.f_max, m.log) == (400, 400, 200, 80, 8000.0, "ln")
    assert tuple(m.fb.shape) == (201, 80) and tuple(m.fb_range.shape) == (80, 2)
    ms = MelSpectrogram()
    assert ms.n_mels == 128 and ms.log is None
    custom = LogMel(n_fft=64, filterbank=torch.ones(33, 7))
    assert custom.n_mels == 7 and custom.fb_range.tolist() == [[0, 33]] * 7
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1000))                     # no CPU fallback
    import asrx
    assert asrx.LogMel is LogMel and asrx.CMVN is CMVN


def test_cmvn_finalize_arithmetic():
    from asrx.features import CMVN
    # three features over n = 4 frames: values {1, 2, 3, 4}, a constant 5 (var = 0), and {-1, 1, -1, 1}
    rows = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 5.0, 5.0, 5.0], [-1.0, 1.0, -1.0, 1.0]])
    s, q, n = rows.sum(axis=1), (rows ** 2).sum(axis=1), rows.shape[1]
    for norm_var in (True, False):
        cm = CMVN(3, mode="global", norm_var=norm_var, eps=1e-5)
        with pytest.raises(RuntimeError):
            cm.statistics()                          # not finalised
        with pytest.raises(RuntimeError):
            cm.finalize()                            # nothing accumulated
        cm.sum.copy_(torch.from_numpy(s))
        cm.sumsq.copy_(torch.from_numpy(q))
        cm.count.fill_(n)
        cm.finalize()
        mean, istd = R.finalize(s, q, n, norm_var=norm_var, eps=1e-5)
        assert np.allclose(cm.mean.double().numpy(), mean, rtol=0, atol=1e-6)
        assert np.allclose(cm.istd.double().numpy(), istd, rtol=1e-6, atol=0)
        assert cm.mean.tolist() == [2.5, 5.0, 0.0]
        if norm_var:
            want = [1.0 / math.sqrt(1.25), 1.0 / 1e-5, 1.0]      # var = 0: istd = 1 / eps
            assert np.allclose(cm.istd.double().numpy(), want, rtol=1e-6, atol=0)
            assert cm.statistics()[1] is cm.istd
        else:
            assert cm.istd.tolist() == [1.0, 1.0, 1.0] and cm.statistics()[1] is None
        # the buffers travel in state_dict, the finalised flag with them
        fresh = CMVN(3, mode="global", norm_var=norm_var)
        fresh.load_state_dict(cm.state_dict())
        assert torch.equal(fresh.statistics()[0], cm.mean) and torch.equal(fresh.istd, cm.istd)
        assert set(cm.state_dict()) == {"sum", "sumsq", "count", "mean", "istd", "finalized"}
