"""Test oracle (never imported by the product): float64 numpy restatement of the log-mel / CMVN rule of DESIGN.md §17
(asrx_logmel, asrx_cmvn, asrx_feature_stats), written from the rule, not from the product code.

The filterbank follows torchaudio's published torchaudio.functional.melscale_fbanks (torchaudio 2.x; not installed
here): bin frequencies linspace(0, sample_rate // 2, n_freqs), n_mels + 2 points equally spaced on the mel scale,
triangles max(0, min(down, up)), norm="slaney" scaling filter m by 2 / (f[m + 2] - f[m]).  The STFT is
oracle.features.spectrogram.
"""
import math

import numpy as np

from oracle import features as OF

F_SP = 200.0 / 3.0
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = MIN_LOG_HZ / F_SP
LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f, mel_scale="htk"):
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    assert mel_scale == "slaney"
    return np.where(f >= MIN_LOG_HZ, MIN_LOG_MEL + np.log(np.maximum(f, MIN_LOG_HZ) / MIN_LOG_HZ) / LOGSTEP, f / F_SP)


def mel_to_hz(m, mel_scale="htk"):
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    assert mel_scale == "slaney"
    return np.where(m >= MIN_LOG_MEL, MIN_LOG_HZ * np.exp(LOGSTEP * (np.maximum(m, MIN_LOG_MEL) - MIN_LOG_MEL)),
                    F_SP * m)


def mel_points(f_min, f_max, n_mels, mel_scale="htk"):
    """The n_mels + 2 corner frequencies in Hz."""
    return mel_to_hz(np.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2), mel_scale)


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    """float64 [n_freqs, n_mels]"""
    freqs = np.linspace(0, sample_rate // 2, n_freqs)
    pts = mel_points(f_min, f_max, n_mels, mel_scale)
    fb = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        up = (freqs - left) / (centre - left)
        down = (right - freqs) / (right - centre)
        fb[:, m] = np.maximum(0.0, np.minimum(up, down))
        if norm == "slaney":
            fb[:, m] *= 2.0 / (right - left)
    return fb


def filterbank_ranges(fb):
    """int [n_mels, 2]: first and one-past-last nonzero row of each column, (0, 0) for an all-zero column."""
    fb = np.asarray(fb)
    out = np.zeros((fb.shape[1], 2), dtype=np.int64)
    for m in range(fb.shape[1]):
        nz = np.nonzero(fb[:, m])[0]
        if len(nz):
            out[m] = (nz[0], nz[-1] + 1)
    return out


def frame_lengths(sample_lengths, n_fft, hop):
    return np.array([(n - n_fft) // hop + 1 if n >= n_fft else 0 for n in sample_lengths], dtype=np.int64)


def mel_energies(audio, fb, n_fft, hop, win_length=None, power=2.0, normalized=False):
    """audio (B, T) -> float64 (B, n_mels, frames): the filterbank applied to the (power) spectrogram."""
    spec = OF.spectrogram(np.asarray(audio, dtype=np.float64), n_fft=n_fft, win_length=win_length, hop_length=hop,
                          power=power, normalized=normalized)          # (B, nbins, frames)
    return np.einsum("bnf,nm->bmf", spec, np.asarray(fb, dtype=np.float64))


def log_mul(log):
    return {None: None, "ln": 1.0, "log10": 1.0 / math.log(10.0)}[log]


def apply_log(e, log="ln", log_eps=1e-6, log_mode="add"):
    if log is None:
        return e
    arg = e + log_eps if log_mode == "add" else np.maximum(e, log_eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        return log_mul(log) * np.log(arg)


def logmel(audio, fb, n_fft, hop, win_length=None, power=2.0, normalized=False, log="ln", log_eps=1e-6,
           log_mode="add", mean=None, istd=None, lengths=None, pad_value=0.0):
    """(features float64 (B, n_mels, frames), energies, frame lengths): log, global CMVN, then the pad."""
    e = mel_energies(audio, fb, n_fft, hop, win_length, power, normalized)
    v = apply_log(e, log, log_eps, log_mode)
    if mean is not None:
        v = v - np.asarray(mean, dtype=np.float64)[None, :, None]
        if istd is not None:
            v = v * np.asarray(istd, dtype=np.float64)[None, :, None]
    B, _, frames = v.shape
    fl = np.full(B, frames, dtype=np.int64)
    if lengths is not None:
        fl = np.minimum(frame_lengths(lengths, n_fft, hop), frames)
        v = v.copy()
        for b in range(B):
            v[b, :, fl[b]:] = pad_value
    return v, e, fl


def cmvn_utterance(x, lengths=None, norm_var=True, eps=1e-5, pad_value=0.0):
    """x (B, F, T) -> float64: per (b, f) row over t < L_b, population variance, istd = 1 / max(sqrt(var), eps)."""
    x = np.asarray(x, dtype=np.float64)
    B, F, T = x.shape
    out = np.full((B, F, T), float(pad_value))
    for b in range(B):
        L = T if lengths is None else int(min(max(lengths[b], 0), T))
        if L == 0:
            continue
        row = x[b, :, :L]
        mean = row.mean(axis=1, keepdims=True)
        d = row - mean
        if norm_var:
            var = (d * d).mean(axis=1, keepdims=True)
            d = d / np.maximum(np.sqrt(var), eps)
        out[b, :, :L] = d
    return out


def feature_sums(batches):
    """[(x (B, F, T), lengths or None)] -> (sum [F], sumsq [F], count) in float64 over the valid frames."""
    s = q = None
    n = 0
    for x, lengths in batches:
        x = np.asarray(x, dtype=np.float64)
        B, F, T = x.shape
        if s is None:
            s, q = np.zeros(F), np.zeros(F)
        for b in range(B):
            L = T if lengths is None else int(min(max(lengths[b], 0), T))
            s += x[b, :, :L].sum(axis=1)
            q += (x[b, :, :L] ** 2).sum(axis=1)
            n += L
    return s, q, n


def finalize(s, q, n, norm_var=True, eps=1e-5):
    """(mean, istd) float64 from the sums: var = max(q / n - mean^2, 0), istd = 1 / max(sqrt(var), eps)."""
    mean = np.asarray(s, dtype=np.float64) / n
    var = np.maximum(np.asarray(q, dtype=np.float64) / n - mean * mean, 0.0)
    istd = 1.0 / np.maximum(np.sqrt(var), eps) if norm_var else np.ones_like(mean)
    return mean, istd


def cmvn_global(x, mean, istd=None, lengths=None, pad_value=0.0):
    x = np.asarray(x, dtype=np.float64)
    v = x - np.asarray(mean, dtype=np.float64)[None, :, None]
    if istd is not None:
        v = v * np.asarray(istd, dtype=np.float64)[None, :, None]
    if lengths is not None:
        for b in range(x.shape[0]):
            v[b, :, int(min(max(lengths[b], 0), x.shape[2])):] = pad_value
    return v


def waveform(shape, seed, sample_rate=16000):
    """The tests' waveform: 0.3 * randn plus one sine, seeded; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(shape[-1], dtype=np.float64) / sample_rate
    x = 0.3 * rng.standard_normal(shape) + 0.5 * np.sin(2.0 * math.pi * (440.0 + 37.0 * seed) * t)
    return x.astype(np.float32)
