"""numpy restatement of asrx_length_mask (asr-transformer_amd/csrc/lengths.hip; the rule is DESIGN.md §18 and the
header's), written from the rule, not from the product code: test oracle only."""
import numpy as np


def conv_len(n):
    """Output length of an unpadded kernel-3 stride-2 convolution over n frames (0 where the kernel does not fit)."""
    n = np.asarray(n, dtype=np.int64)
    return np.where(n < 3, 0, (n - 3) // 2 + 1)


def rows(lengths, T, subsample=0):
    """int32 [B]: conv_len applied `subsample` times to the lengths, clamped to [0, T]; negative lengths give 0."""
    n = np.asarray(lengths, dtype=np.int64)
    for _ in range(int(subsample)):
        n = conv_len(n)
    return np.clip(n, 0, int(T)).astype(np.int32)


def length_mask(lengths, T, subsample=0):
    """(enc_lengths int32 [B], valid uint8 [B, T]) with valid[b, t] = t < enc_lengths[b]."""
    r = rows(lengths, T, subsample)
    return r, (np.arange(int(T))[None, :] < r[:, None]).astype(np.uint8)
