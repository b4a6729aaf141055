"""GPU featuriser: the power spectrogram of the reference's data pipeline (modules/dataset.py:34-55).

`Spectrogram` mirrors torchaudio.transforms.Spectrogram for the configuration the reference builds
(dataset.py:34-35: n_fft=1024, center=False; torchaudio's defaults win_length=n_fft, hop_length=win_length//2,
periodic Hann window, power=2.0, normalized=False, onesided) and its forward contract: (..., time) fp32 waveform
-> (..., n_fft//2 + 1, frames), frequency-major with time innermost — the layout the model's front-end reads
(dataset.py:51-55 -> model.py:168).  It runs in libasrx.so (asrx_spectrogram: one fp32 MFMA GEMM of the framed
waveform against the windowed DFT basis, then a square/transpose pass); `pad_spectrum` is the dataset's padding and
frame mask (dataset.py:42-55).

`LogMel` (and `MelSpectrogram`, the same without the log) is the 80-bin input every configuration of the model
takes: the same STFT, then ONE pass that squares, applies the mel filterbank (`melscale_fbanks`, torchaudio's
algorithm), the log, an optional global CMVN and the padding of short utterances (asrx_logmel); the
linear spectrogram is never written.  `CMVN` normalises per utterance (asrx_cmvn) or by statistics gathered over a
training set (asrx_feature_stats).  Frame lengths come out of `LogMel` once, as the int32 device tensor that
SpecAugment, Trainer.step(input_lengths=), the CTC decoders and align take.

Not covered: center=True (reflect padding), complex output (power=None), window functions other than Hann, Kaldi's
dither / pre-emphasis / DC removal / Povey window, delta features, waveform decoding and resampling.
"""
import math

import torch
from torch import nn

from . import kernels as K
from ._lib import LOGMEL_MAX_MELS, call


def _hann_periodic(n):
    k = torch.arange(n, dtype=torch.float64)
    return 0.5 - 0.5 * torch.cos(2.0 * math.pi * k / n)


def dft_basis(n_fft, win_length, device):
    """[2 * (n_fft//2 + 1), n_fft] fp32: rows 2n, 2n+1 = w[k] cos(2 pi n k / n_fft), -w[k] sin(...), with the
    periodic Hann window of win_length zero-padded to n_fft centred (torch.stft's window placement)."""
    nb = n_fft // 2 + 1
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = _hann_periodic(win_length)
    k = torch.arange(n_fft, dtype=torch.float64)
    n = torch.arange(nb, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(n, k).remainder(n_fft) / n_fft   # exact phase: (n k) mod n_fft first
    basis = torch.empty(2 * nb, n_fft, dtype=torch.float64)
    basis[0::2] = torch.cos(ang) * w
    basis[1::2] = -torch.sin(ang) * w
    return basis.to(device=device, dtype=torch.float32).contiguous()


class Spectrogram(nn.Module):
    """torchaudio.transforms.Spectrogram(n_fft=400, win_length=None, hop_length=None, pad=0, power=2.0,
    normalized=False, center=True, onesided=True) restricted to center=False (the reference's setting), Hann
    window, power 1 or 2."""

    def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, power=2.0, normalized=False,
                 center=True, onesided=True):
        super().__init__()
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        if center:
            raise NotImplementedError("asrx.features.Spectrogram: center=True (reflect padding) is not built; "
                                      "the reference uses center=False (dataset.py:34-35)")
        if power not in (1, 1.0, 2, 2.0):
            raise NotImplementedError("asrx.features.Spectrogram: power must be 1 or 2")
        if not onesided:
            raise NotImplementedError("asrx.features.Spectrogram: onesided=False is not built")
        if self.win_length > n_fft:
            raise ValueError("win_length must be <= n_fft")
        self.pad, self.power, self.normalized, self.center = pad, int(power), normalized, center
        self._basis = {}

    def basis(self, device):
        key = str(device)
        if key not in self._basis:
            self._basis[key] = dft_basis(self.n_fft, self.win_length, device)
        return self._basis[key]

    def forward(self, waveform):
        if not waveform.is_cuda:
            raise RuntimeError("asrx.features.Spectrogram computes on the GPU (libasrx.so); move the waveform "
                               "with .cuda()")
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1]).float()
        if self.pad > 0:
            x = torch.nn.functional.pad(x, (self.pad, self.pad))
        x = x.contiguous()
        B, T = x.shape
        nb = self.n_fft // 2 + 1
        if T < self.n_fft:
            raise ValueError(f"waveform of {T} samples is shorter than n_fft={self.n_fft}")
        frames = (T - self.n_fft) // self.hop_length + 1
        out = torch.empty(B, nb, frames, device=x.device, dtype=torch.float32)
        ws = torch.empty(B * frames * 2 * nb, device=x.device, dtype=torch.float32)
        # normalized=True (torchaudio "window"): divide the STFT by the window's L2 norm (power applies after)
        scale = 1.0
        if self.normalized:
            wn = float(_hann_periodic(self.win_length).pow(2).sum().sqrt())
            scale = 1.0 / wn ** self.power
        call("asrx_spectrogram", x.data_ptr(), B, T, x.stride(0), self.basis(x.device).data_ptr(), self.n_fft,
             self.hop_length, nb, self.power, scale, ws.data_ptr(), ws.numel(), out.data_ptr(), K.stream())
        return out.reshape(shape[:-1] + (nb, frames))


def spectrum_len(n_samples, win_length=1024, hop_length=512):
    """dataset.py:40-41 (_calculate_spectrum_len)."""
    return math.floor((n_samples - win_length) / hop_length) + 1


def frame_lengths(sample_lengths, n_fft, hop_length):
    """Frames of center=False framing for the given sample counts (an int, a sequence or an integer tensor; host
    arithmetic, the rule asrx_logmel applies on the device): 0 below n_fft, else (len - n_fft) // hop_length + 1."""
    if isinstance(sample_lengths, int):
        return (sample_lengths - n_fft) // hop_length + 1 if sample_lengths >= n_fft else 0
    if torch.is_tensor(sample_lengths):
        n = torch.div(sample_lengths - n_fft, hop_length, rounding_mode="floor") + 1
        return torch.where(sample_lengths >= n_fft, n, torch.zeros_like(n))
    return [frame_lengths(int(v), n_fft, hop_length) for v in sample_lengths]


# ---------------------------------------------------------------------------------- mel filterbank

_F_SP = 200.0 / 3.0                  # Slaney scale: Hz per mel below 1 kHz
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP   # 15
_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(freq, mel_scale="htk"):
    """float64 tensor of mels for frequencies in Hz (torchaudio's _hz_to_mel, elementwise)."""
    if mel_scale not in ("htk", "slaney"):
        raise ValueError('mel_scale should be one of "htk" or "slaney"')
    f = torch.as_tensor(freq, dtype=torch.float64)
    if mel_scale == "htk":
        return 2595.0 * torch.log10(1.0 + f / 700.0)
    log_part = _MIN_LOG_MEL + torch.log(f.clamp(min=_MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP
    return torch.where(f >= _MIN_LOG_HZ, log_part, f / _F_SP)


def mel_to_hz(mels, mel_scale="htk"):
    """The inverse of hz_to_mel (torchaudio's _mel_to_hz)."""
    if mel_scale not in ("htk", "slaney"):
        raise ValueError('mel_scale should be one of "htk" or "slaney"')
    m = torch.as_tensor(mels, dtype=torch.float64)
    if mel_scale == "htk":
        return 700.0 * (torch.pow(10.0, m / 2595.0) - 1.0)
    log_part = _MIN_LOG_HZ * torch.exp(_LOGSTEP * (m.clamp(min=_MIN_LOG_MEL) - _MIN_LOG_MEL))
    return torch.where(m >= _MIN_LOG_MEL, log_part, _F_SP * m)


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    """torchaudio.functional.melscale_fbanks: fp32 CPU tensor [n_freqs, n_mels] of triangular filters (computed in
    float64): n_mels + 2 points equally spaced on the mel scale between f_min and f_max, filter m rising from point m
    to m + 1 and falling to m + 2 over the bin frequencies linspace(0, sample_rate // 2, n_freqs); norm="slaney"
    scales filter m by 2 / (f[m + 2] - f[m])."""
    if norm is not None and norm != "slaney":
        raise ValueError('norm must be one of None or "slaney"')
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_min, m_max = float(hz_to_mel(float(f_min), mel_scale)), float(hz_to_mel(float(f_max), mel_scale))
    f_pts = mel_to_hz(torch.linspace(m_min, m_max, n_mels + 2, dtype=torch.float64), mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)          # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0)
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb.to(torch.float32)


def filterbank_ranges(fb):
    """int32 CPU tensor [n_mels, 2]: the first and one-past-last nonzero row of each column of fb [n_freqs, n_mels],
    (0, 0) for an all-zero column — the half-open bin range asrx_logmel sums for that filter."""
    nz = (torch.as_tensor(fb).detach().cpu() != 0)
    n_freqs, n_mels = nz.shape
    idx = torch.arange(n_freqs).unsqueeze(1)
    big = n_freqs + 1
    lo = torch.where(nz, idx, torch.full_like(idx, big)).amin(dim=0)
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).amax(dim=0)
    lo = torch.where(hi == 0, torch.zeros_like(lo), lo)
    return torch.stack([lo, hi], dim=1).to(torch.int32).contiguous()


# ------------------------------------------------------------------------------------------- CMVN

class CMVN(nn.Module):
    """Cepstral mean and variance normalisation of fp32 (B, F, T) / (B, 1, F, T) features over their valid frames.

    mode="utterance": every (b, f) row by its own mean and population variance (asrx_cmvn; two passes, fixed
    reduction tree).  mode="global": by statistics gathered with accumulate() over a training set (asrx_feature_stats,
    fp64 sums) and fixed by finalize(); the buffers travel in state_dict.  istd = 1 / max(sqrt(var), eps), or 1 with
    norm_var=False.  Frames at or beyond an utterance's length take pad_value."""

    def __init__(self, n_feats, mode="global", norm_var=True, eps=1e-5, pad_value=0.0):
        super().__init__()
        if mode not in ("global", "utterance"):
            raise ValueError(f'CMVN: mode {mode!r} must be "global" or "utterance"')
        if isinstance(n_feats, bool) or not isinstance(n_feats, int) or n_feats < 1:
            raise ValueError(f"CMVN: n_feats {n_feats!r} must be a positive int")
        if not eps > 0:
            raise ValueError(f"CMVN: eps {eps!r} must be positive")
        self.n_feats, self.mode, self.norm_var, self.eps = n_feats, mode, bool(norm_var), float(eps)
        self.pad_value = float(pad_value)
        self.register_buffer("sum", torch.zeros(n_feats, dtype=torch.float64))
        self.register_buffer("sumsq", torch.zeros(n_feats, dtype=torch.float64))
        self.register_buffer("count", torch.zeros(1, dtype=torch.int64))
        self.register_buffer("mean", torch.zeros(n_feats, dtype=torch.float32))
        self.register_buffer("istd", torch.ones(n_feats, dtype=torch.float32))
        self.register_buffer("finalized", torch.zeros(1, dtype=torch.uint8))
        self._finalized = False   # host copy of the `finalized` buffer (no device read per call)

    def extra_repr(self):
        return f"n_feats={self.n_feats}, mode={self.mode}, norm_var={self.norm_var}, eps={self.eps}"

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._finalized = bool(int(self.finalized.cpu()[0]))

    @staticmethod
    def _lengths(lengths, device):
        if lengths is None:
            return None
        return torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()

    def _check(self, x):
        if not x.is_cuda:
            raise RuntimeError("asrx.features.CMVN computes on the GPU (libasrx.so); move the features with .cuda()")
        if x.shape[-2] != self.n_feats:
            raise ValueError(f"CMVN: {x.shape[-2]} feature bins, built for {self.n_feats}")

    def statistics(self):
        """(mean, istd) fp32 [n_feats] of a finalised global CMVN (istd None with norm_var=False)."""
        if self.mode != "global":
            raise RuntimeError("CMVN: an utterance CMVN has no global statistics")
        if not self._finalized:
            raise RuntimeError("CMVN: global statistics are not finalised; call accumulate() over the training set, "
                               "then finalize() (or load a finalised state_dict)")
        return self.mean, (self.istd if self.norm_var else None)

    def accumulate(self, x, lengths=None):
        """Add the valid frames of x to the running sums (asrx_feature_stats)."""
        self._check(x)
        if self.sum.dtype != torch.float64 or self.sumsq.dtype != torch.float64:
            raise RuntimeError("CMVN: the running sums must stay float64 (the module was cast with .float()/.half())")
        K.feature_stats(_dense(x), self.sum, self.sumsq, self.count, lengths=self._lengths(lengths, x.device))
        self.finalized.zero_()
        self._finalized = False
        return self

    def finalize(self):
        """mean and istd from the fp64 sums (host arithmetic on the [n_feats] statistics)."""
        n = int(self.count.cpu()[0])
        if n < 1:
            raise RuntimeError("CMVN.finalize(): no frames were accumulated")
        mean = self.sum.detach().cpu().double() / n
        var = (self.sumsq.detach().cpu().double() / n - mean * mean).clamp(min=0.0)
        istd = 1.0 / var.sqrt().clamp(min=self.eps) if self.norm_var else torch.ones_like(mean)
        self.mean.copy_(mean.to(torch.float32))
        self.istd.copy_(istd.to(torch.float32))
        self.finalized.fill_(1)
        self._finalized = True
        return self

    def forward(self, x, lengths=None, out=None):
        self._check(x)
        x = _dense(x)
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        lengths = self._lengths(lengths, x.device)
        if self.mode == "global":
            mean, istd = self.statistics()
            K.cmvn(x, out, lengths=lengths, mean=mean, istd=istd, pad_value=self.pad_value)
        else:
            K.cmvn(x, out, lengths=lengths, norm_var=self.norm_var, eps=self.eps, pad_value=self.pad_value)
        return out


def _dense(x):
    """fp32 (B, F, T) / (B, 1, F, T) features with dense (F, T) planes: x itself, or a contiguous copy where its
    layout asks for one."""
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"CMVN takes fp32 (B, F, T) or (B, 1, F, T) features, got {x.dtype} {tuple(x.shape)}")
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    if (T == 1 or x.stride(-1) == 1) and (F == 1 or x.stride(-2) == T) and (B <= 1 or x.stride(0) >= F * T):
        return x
    return x.contiguous()


# ------------------------------------------------------------------------------------------ LogMel

_LOGS = {None: 0.0, "ln": 1.0, "log10": 1.0 / math.log(10.0)}
_LOG_MODES = {"add": 1, "clamp": 2}


class LogMel(nn.Module):
    """Waveform -> log-mel filterbank features in one native call (asrx_logmel): the STFT of
    `Spectrogram` (fp32 MFMA GEMM against the windowed DFT basis), then one pass that squares, applies the mel
    filterbank, the log, an optional global CMVN and the padding, and stores (..., n_mels, frames) — the layout the
    model's front end, SpecAugment and Trainer.step read.

    The arguments up to mel_scale are torchaudio.transforms.MelSpectrogram's (center=False only, Hann window, power 1
    or 2).  log: None | "ln" | "log10"; log_mode "add": log(e + log_eps), "clamp": log(max(e, log_eps)).  cmvn: a
    finalised global CMVN, fused into the launch.  filterbank: a [n_fft // 2 + 1, n_mels] matrix used instead of the
    computed one.  forward(waveform, lengths=None): with lengths (valid samples per row) the frames at or beyond
    frame_lengths(lengths, n_fft, hop_length) take pad_value and (features, frame_lengths) is returned,
    frame_lengths an int32 device tensor to hand to SpecAugment, Trainer.step(input_lengths=) and the decoders."""

    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0,
                 n_mels=80, power=2.0, normalized=False, center=False, norm=None, mel_scale="htk", log="ln",
                 log_eps=1e-6, log_mode="add", cmvn=None, pad_value=0.0, filterbank=None):
        super().__init__()
        self.sample_rate, self.n_fft = sample_rate, n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        if center:
            raise NotImplementedError("asrx.features.LogMel: center=True (reflect padding) is not built")
        if power not in (1, 1.0, 2, 2.0):
            raise NotImplementedError("asrx.features.LogMel: power must be 1 or 2")
        if self.win_length > n_fft:
            raise ValueError("win_length must be <= n_fft")
        if log not in _LOGS:
            raise ValueError(f'LogMel: log {log!r} must be None, "ln" or "log10"')
        if log_mode not in _LOG_MODES:
            raise ValueError(f'LogMel: log_mode {log_mode!r} must be "add" or "clamp"')
        if log is not None and not log_eps > 0:
            raise ValueError(f"LogMel: log_eps {log_eps!r} must be positive")
        self.f_min = float(f_min)
        self.f_max = float(f_max) if f_max is not None else float(sample_rate // 2)
        if self.f_max > sample_rate / 2:
            raise ValueError(f"LogMel: f_max {self.f_max} is above the Nyquist frequency {sample_rate / 2}")
        if not 0.0 <= self.f_min < self.f_max:
            raise ValueError(f"LogMel: need 0 <= f_min < f_max, got {self.f_min}, {self.f_max}")
        nb = n_fft // 2 + 1
        if filterbank is not None:
            fb = torch.as_tensor(filterbank).detach().to(device="cpu", dtype=torch.float32)
            if fb.dim() != 2 or fb.shape[0] != nb:
                raise ValueError(f"LogMel: filterbank must be [n_fft // 2 + 1 = {nb}, n_mels], got {tuple(fb.shape)}")
            n_mels = fb.shape[1]
        else:
            fb = melscale_fbanks(nb, self.f_min, self.f_max, n_mels, sample_rate, norm, mel_scale)
        if not 1 <= n_mels <= LOGMEL_MAX_MELS:
            raise ValueError(f"LogMel: n_mels {n_mels} outside [1, {LOGMEL_MAX_MELS}]")
        if cmvn is not None and (not isinstance(cmvn, CMVN) or cmvn.mode != "global" or cmvn.n_feats != n_mels):
            raise ValueError(f"LogMel: cmvn must be a global CMVN over {n_mels} features")
        self.n_mels, self.pad, self.power, self.normalized, self.center = n_mels, pad, int(power), normalized, center
        self.norm, self.mel_scale = norm, mel_scale
        self.log, self.log_eps, self.log_mode, self.pad_value = log, float(log_eps), log_mode, float(pad_value)
        self.cmvn = cmvn
        self.fb = fb.contiguous()                      # [nbins, n_mels] fp32, host
        self.fb_range = filterbank_ranges(self.fb)     # [n_mels, 2] int32, host (read by the launcher)
        self._dev = {}

    def _constants(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (dft_basis(self.n_fft, self.win_length, device), self.fb.to(device))
        return self._dev[key]

    def frame_lengths(self, sample_lengths):
        """Host arithmetic: the frames forward() gives rows of these sample counts."""
        if isinstance(sample_lengths, int):
            return frame_lengths(sample_lengths + 2 * self.pad, self.n_fft, self.hop_length)
        return frame_lengths([int(v) + 2 * self.pad for v in sample_lengths], self.n_fft, self.hop_length)

    def forward(self, waveform, lengths=None):
        if not waveform.is_cuda:
            raise RuntimeError("asrx.features.LogMel computes on the GPU (libasrx.so); move the waveform with .cuda()")
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1]).float()
        if self.pad > 0:
            x = torch.nn.functional.pad(x, (self.pad, self.pad))
        x = x.contiguous()
        B, T = x.shape
        if T < self.n_fft:
            raise ValueError(f"waveform of {T} samples is shorter than n_fft={self.n_fft}")
        nb = self.n_fft // 2 + 1
        frames = (T - self.n_fft) // self.hop_length + 1
        basis, fb = self._constants(x.device)
        out = torch.empty(B, self.n_mels, frames, device=x.device, dtype=torch.float32)
        ws = torch.empty(B * frames * 2 * nb, device=x.device, dtype=torch.float32)
        wl = fl = None
        if lengths is not None:
            wl = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).reshape(-1)
            if wl.numel() != B:
                raise ValueError(f"LogMel: {wl.numel()} lengths for {B} waveforms")
            if self.pad > 0:
                wl = wl + 2 * self.pad   # both pads count as signal, as without lengths
            wl = wl.contiguous()
            fl = torch.empty(B, device=x.device, dtype=torch.int32)
        scale = 1.0
        if self.normalized:   # torchaudio "window": the STFT over the window's L2 norm, power applied after
            scale = 1.0 / float(_hann_periodic(self.win_length).pow(2).sum().sqrt()) ** self.power
        mean = istd = None
        if self.cmvn is not None:
            mean, istd = self.cmvn.statistics()
            if mean.device != x.device:
                raise RuntimeError("LogMel: the fused CMVN's buffers live on another device")
        K.logmel(x, basis, fb, self.fb_range, out, ws, n_fft=self.n_fft, hop=self.hop_length, power=self.power,
                 scale=scale, wave_lengths=wl, log_mode=0 if self.log is None else _LOG_MODES[self.log_mode],
                 log_mul=_LOGS[self.log], log_eps=self.log_eps, mean=mean, istd=istd, pad_value=self.pad_value,
                 frame_lengths=fl)
        out = out.reshape(shape[:-1] + (self.n_mels, frames))
        if lengths is None:
            return out
        # one length per waveform; (B, 1, time) gives [B], what SpecAugment and Trainer.step take
        lead = shape[:-2] if len(shape) == 3 and shape[1] == 1 else shape[:-1]
        return out, fl.reshape(lead)


class MelSpectrogram(LogMel):
    """torchaudio.transforms.MelSpectrogram's arguments and defaults (n_mels=128; center=False only): LogMel without
    the log."""

    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0,
                 n_mels=128, power=2.0, normalized=False, center=False, norm=None, mel_scale="htk", **kw):
        super().__init__(sample_rate, n_fft, win_length, hop_length, f_min, f_max, pad, n_mels, power, normalized,
                         center, norm, mel_scale, log=None, **kw)


def pad_spectrum(spectrogram, max_frames_len, win_length=1024, hop_length=512):
    """dataset.py:47-55: pad (channels, freq, frames) with zero frames to spectrum_len(max_frames_len) and return
    (spectrogram, spectrum_mask) — ones for the real frames, zeros for the padding."""
    channels, freq, frames = spectrogram.shape
    padding_length = spectrum_len(max_frames_len, win_length, hop_length) - frames
    if padding_length < 0:
        raise ValueError(f"{frames} frames exceed the padded length {frames + padding_length} "
                         f"(dataset.py:50 would fail the same way)")
    dev = spectrogram.device
    mask = torch.cat([torch.ones(frames, device=dev), torch.zeros(padding_length, device=dev)])
    out = torch.cat([spectrogram, torch.zeros(channels, freq, padding_length, device=dev, dtype=spectrogram.dtype)],
                    dim=-1)
    return out, mask
