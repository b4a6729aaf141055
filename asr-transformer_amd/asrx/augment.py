"""SpecAugment on the device: a time warp plus frequency and time masks on the input spectrogram, applied by one
launch while the spectrogram is copied (asrx_specaug; the rule is DESIGN.md §16, restated in tests/specaug_ref.py).

Every random decision is a counter-based hash of (seed, step, utterance), so the augmentation of step n is a pure
function of those: the same in an eager step and in a replayed graph, and reproducible under torch.manual_seed.
`asrx.train.Trainer(..., spec_augment=SpecAugment(...))` launches it in place of the spectrogram's copy into the
captured input buffer; the module can also be called by hand on any fp32 (B, 1, F, T) tensor.
"""
import torch
from torch import nn

from . import kernels as K
from ._lib import SPECAUG_MAX_MASKS

_U64 = (1 << 64) - 1


def rank_seed(seed, rank):
    """The seed of data-parallel rank `rank`: seed + rank (mod 2^64), so ranks do not share plans."""
    if rank < 0:
        raise ValueError(f"rank {rank} is negative")
    return (int(seed) + int(rank)) & _U64


def _count(name, v, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (hi is not None and v > hi):
        raise ValueError(f"SpecAugment: {name} = {v!r} must be an int in [0, {hi if hi is not None else 'inf'})")
    return v


class SpecAugment(nn.Module):
    """freq_masks masks of up to freq_width rows, time_masks masks of up to min(time_width, time_ratio * length)
    frames, filled with mask_value, after a time warp of up to time_warp frames (0 = off).  seed=None takes
    torch.initial_seed() (no generator is advanced)."""

    def __init__(self, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, time_warp=0,
                 mask_value=0.0, seed=None):
        super().__init__()
        self.freq_masks = _count("freq_masks", freq_masks, SPECAUG_MAX_MASKS)
        self.time_masks = _count("time_masks", time_masks, SPECAUG_MAX_MASKS)
        self.freq_width = _count("freq_width", freq_width, 2 ** 31 - 2)
        self.time_width = _count("time_width", time_width, 2 ** 31 - 2)
        self.time_warp = _count("time_warp", time_warp, 2 ** 30)
        self.time_ratio = float(time_ratio)
        if not 0.0 <= self.time_ratio <= 1.0:
            raise ValueError(f"SpecAugment: time_ratio {time_ratio!r} outside [0, 1]")
        self.mask_value = float(mask_value)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError(f"SpecAugment: seed {seed!r} must be an int or None")
        self.seed = (torch.initial_seed() if seed is None else seed) & _U64
        self.calls = 1   # the step of the next forward() that is not given one

    def extra_repr(self):
        return (f"freq_masks={self.freq_masks}, freq_width={self.freq_width}, time_masks={self.time_masks}, "
                f"time_width={self.time_width}, time_ratio={self.time_ratio}, time_warp={self.time_warp}, "
                f"mask_value={self.mask_value}, seed={self.seed}")

    def _launch(self, src, dst, lengths, step, seed, plan_out=None):
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=src.device, dtype=torch.int32).contiguous()
        K.specaug(src, dst, lengths=lengths, freq_masks=self.freq_masks, freq_width=self.freq_width,
                  time_masks=self.time_masks, time_width=self.time_width, time_ratio=self.time_ratio,
                  time_warp=self.time_warp, mask_value=self.mask_value, seed=self.seed if seed is None else seed,
                  step=step, plan_out=plan_out)

    def augment(self, spectrum, out=None, lengths=None, step=0, seed=None):
        """The augmented copy of fp32 (B, 1, F, T) `spectrum` for `step`, whatever the module's mode; written into
        `out` (same shape, disjoint from the input) when given.  seed: instead of the module's (a rank's seed)."""
        if not spectrum.is_cuda:
            raise RuntimeError("asrx: tensors must live on the GPU (no CPU fallback)")
        if spectrum.dim() != 4 or spectrum.shape[1] != 1 or spectrum.dtype != torch.float32:
            raise ValueError(f"SpecAugment takes an fp32 (B, 1, F, T) spectrogram, got {spectrum.dtype} "
                             f"{tuple(spectrum.shape)}")
        B, _, F, T = spectrum.shape
        dense = (T == 1 or spectrum.stride(3) == 1) and (F == 1 or spectrum.stride(2) == T) and \
            (B == 1 or spectrum.stride(0) >= F * T)
        src = spectrum if dense else spectrum.contiguous()
        if out is None:
            out = torch.empty((B, 1, F, T), dtype=torch.float32, device=spectrum.device)
        if B * F * T > 0:
            self._launch(src, out, lengths, step, seed)
        return out

    def forward(self, spectrum, lengths=None, out=None, step=None):
        if not self.training:
            return spectrum
        if not spectrum.is_cuda:
            raise RuntimeError("asrx: tensors must live on the GPU (no CPU fallback)")
        if step is None:
            step = self.calls
            self.calls += 1
        return self.augment(spectrum, out=out, lengths=lengths, step=step)

    def plan(self, B, F, T, lengths=None, step=0, seed=None, device="cuda"):
        """int32 [B, 4 + 2 * (freq_masks + time_masks)]: per utterance L, w0, c (0, 0 without a warp), 0, the
        frequency masks' (f0, w), the time masks' (t0, w) — what the launch of `step` applies (tests, logging)."""
        src = torch.zeros((B, 1, F, T), dtype=torch.float32, device=device)
        out = torch.empty((B, 4 + 2 * (self.freq_masks + self.time_masks)), dtype=torch.int32, device=device)
        if B > 0:
            self._launch(src, torch.empty_like(src), lengths, step, seed, plan_out=out)
        return out
