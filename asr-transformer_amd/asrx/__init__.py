"""asrx — MI355X-native (gfx950) Speech-Transformer attention path.

Drop-in modules for shockless/asr-transformer's modules/Transformer/{layers,model}.py backed by the C-ABI
library libasrx.so (hand-written HIP/CDNA4 kernels).  There is no CPU fallback: the modules require the
native library and a GPU.
"""
from .layers import MHA, FeedForward, LayerNorm, TrainablePositionalEncoding  # noqa: F401
from .decode import BeamResult, CtcInput, RescoreResult  # noqa: F401
from .kernels import CtcAlignment  # noqa: F401
from .augment import SpecAugment  # noqa: F401
from .ctc import CTCLoss  # noqa: F401
from .features import CMVN, LogMel  # noqa: F401
from .loss import CrossEntropyLoss  # noqa: F401
from .lm import NgramLM  # noqa: F401
from .model import Decoder, DecoderLayer, Encoder, EncoderLayer, FrontEnd, Transformer, subsampled  # noqa: F401
from .score import EditCounts, ErrorRate, MbrResult, edit_distance, mbr_rerank  # noqa: F401

__version__ = "0.1.0"


def frame_span(start, end):
    """Spectrogram frames [first, last) that the encoder frames [start, end) see (ints, or tensors elementwise; host
    arithmetic only).  The front end is two kernel-3 stride-2 convolutions without padding (`subsampled`), so encoder
    frame j sees spectrogram frames 4j .. 4j + 6 and a run [s, e) covers [4s, 4(e - 1) + 7).  An empty or absent run
    (end <= start, such as the -1 / -1 of a position past the target length) maps to (-1, -1).  Seconds are the
    caller's hop length times these."""
    if isinstance(start, int) and isinstance(end, int):
        return (4 * start, 4 * (end - 1) + 7) if end > start >= 0 else (-1, -1)
    ok = (end > start) & (start >= 0)
    return (4 * start).masked_fill(~ok, -1), (4 * (end - 1) + 7).masked_fill(~ok, -1)


def native():
    """The loaded ctypes library (raises if libasrx.so is missing)."""
    from ._lib import lib
    return lib()
