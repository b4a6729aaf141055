"""Padded batches, host side (no GPU): the numpy restatement of the length arithmetic (tests/lengths_ref.py) against
asrx.subsampled and against the convolution itself, asrx_length_mask's argument checks (made before any HIP call), its
derived signature, and the mask_padding flag of Transformer."""
import ctypes

import numpy as np
import torch

from tests import lengths_ref as R


def test_reference_matches_subsampled_and_the_convolutions():
    """n = 7 ... 64: two applications of the rule are asrx.subsampled(n) and the time length F.conv2d produces."""
    import asrx
    w1, w2 = torch.zeros(2, 1, 3, 3), torch.zeros(2, 2, 3, 3)
    for n in range(7, 65):
        y = torch.nn.functional.conv2d(torch.nn.functional.conv2d(torch.zeros(1, 1, 9, n), w1, stride=2), w2, stride=2)
        assert int(R.rows([n], 1 << 20, 2)[0]) == asrx.subsampled(n) == y.shape[-1], n
    assert R.rows([-3, 0, 2, 3, 6, 7, 10, 11], 100, 2).tolist() == [0, 0, 0, 0, 0, 1, 1, 2]
    assert R.rows([-3, 0, 5, 1100], 274, 0).tolist() == [0, 0, 5, 274]
    enc, valid = R.length_mask([7, 23, 0], 6, 2)
    assert enc.tolist() == [1, 5, 0] and valid.dtype == np.uint8
    assert valid.tolist() == [[1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0], [0] * 6]


def _length_mask(lib, lengths=4096, B=3, T=64, subsample=2, enc=8192, valid=1 << 20, vb=64):
    return lib.asrx_length_mask(lengths, B, T, subsample, enc, valid, vb, None)


def test_abi_rejects_bad_arguments_without_gpu():
    """Every refusal of the header's list comes before any HIP call (fake device addresses; no GPU here)."""
    import asrx
    lib = asrx.native()
    assert lib.asrx_version() >= 13
    ARG = -1
    assert _length_mask(lib, lengths=None) == ARG
    assert _length_mask(lib, B=-1) == ARG
    assert _length_mask(lib, T=0) == ARG
    assert _length_mask(lib, T=-5) == ARG
    assert _length_mask(lib, subsample=-1) == ARG
    assert _length_mask(lib, subsample=9) == ARG
    assert _length_mask(lib, enc=None, valid=None) == ARG
    assert _length_mask(lib, vb=63) == ARG
    assert _length_mask(lib, enc=None, vb=63) == ARG
    assert _length_mask(lib, B=0) == 0                          # nothing to do, nothing launched
    assert _length_mask(lib, B=0, enc=None) == 0
    assert _length_mask(lib, B=0, valid=None, subsample=8) == 0


def test_signature_matches_the_header():
    """The derived ctypes signature has one entry per parameter of the header's declaration, in its types."""
    import os
    import re
    from asrx._lib import RESTYPES, SIGNATURES
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "asrx.h")).read()
    decl = re.search(r"int asrx_length_mask\((.*?)\);", src, re.S).group(1)
    kinds = []
    for p in decl.split(","):
        p = " ".join(p.split())
        scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
        kinds.append(ctypes.c_void_p if "*" in p else scalar[p.split()[0]])
    assert len(kinds) == 8
    assert SIGNATURES["asrx_length_mask"] == kinds
    assert RESTYPES["asrx_length_mask"] is ctypes.c_int


def test_mask_padding_is_a_plain_attribute():
    """mask_padding is keyword-only, stored on the model, and changes neither the parameters nor the state_dict."""
    import pytest
    import asrx
    args = (50, 40, 64, 8, 40, 1, 1, 2, 128)
    torch.manual_seed(0)
    a = asrx.Transformer(*args, ctc=True)
    torch.manual_seed(0)
    b = asrx.Transformer(*args, ctc=True, mask_padding=True)
    assert a.mask_padding is False and b.mask_padding is True
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    assert "mask_padding" not in dict(b.named_parameters())
    a.load_state_dict(sb)
    a.mask_padding = True                                       # may be set after loading
    assert a.mask_padding is True and list(a.state_dict()) == list(sb)
    with pytest.raises(TypeError):
        asrx.Transformer(*args, 0.1, 4, 2, True)                # keyword-only


def test_mask_spec_keys():
    from asrx.kernels import MaskSpec
    valid = torch.ones(3, 40, dtype=torch.uint8)[:, :33]
    s = MaskSpec.keys(valid)
    assert (s.mode, s.causal, s.qvalid, s.valid_bstride) == (1, False, None, 40) and s.kvalid is valid
