"""Transcripts beyond 255 labels, host side (no GPU): the `_long` entry points are exported and refuse bad arguments
with the short entries' codes before any launch (the pointers here are not mapped), their size helpers follow the
stated rules in int64, and the Python layers choose between the short and the long entries from a width alone."""
import ctypes

import pytest
import torch

from tests.test_ctc_align_cpu import _args as _align_args
from tests.test_ctc_cpu import _loss_args
from tests.test_edit_cpu import _ed

ERR_ARG, ERR_UNSUPPORTED = -1, -3
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _size(fn, B, T, L):
    """(return code, count) of a `_long` size helper: an int result, the int64 count through a pointer."""
    n = ctypes.c_int64(12345)
    return fn(B, T, L, ctypes.byref(n)), n.value


def test_symbols_constants_and_version():
    import asrx
    from asrx import _lib
    lib = asrx.native()
    assert lib.asrx_version() >= 16
    for name, short in (("asrx_ctc_loss_long", "asrx_ctc_loss"), ("asrx_ctc_align_long", "asrx_ctc_align"),
                        ("asrx_edit_distance_long", "asrx_edit_distance")):
        assert getattr(lib, name) is not None
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[short], name      # the same parameter lists
    for name in ("asrx_ctc_long_workspace_elems", "asrx_ctc_align_long_workspace_words"):
        assert _lib.SIGNATURES[name] == [ctypes.c_int32] * 3 + [ctypes.c_void_p] and _lib.RESTYPES[name] is ctypes.c_int
    assert _lib.CONSTS["ASRX_CTC_LONG_MAX_TARGET"] == _lib.CTC_LONG_MAX_TARGET == 4095
    assert _lib.CONSTS["ASRX_ED_LONG_MAX_TOKENS"] == _lib.ED_LONG_MAX_TOKENS == 4095


def test_loss_long_refuses_bad_arguments_without_gpu():
    import asrx
    f = asrx.native().asrx_ctc_loss_long
    big = dict(tgt_stride=5000, ws_elems=1 << 40)
    assert f(*_loss_args(max_target_len=4096, **big)) == ERR_UNSUPPORTED
    assert f(*_loss_args(max_target_len=4096, logits=None, ws=None, **big)) == ERR_UNSUPPORTED   # whatever else is wrong
    assert f(*_loss_args(max_target_len=4095, tgt_stride=4094, ws_elems=1 << 40)) == ERR_ARG    # rows shorter than that
    assert f(*_loss_args(blank=10)) == ERR_ARG and f(*_loss_args(blank=-1)) == ERR_ARG
    assert f(*_loss_args(blank=10, max_target_len=4096, **big)) == ERR_ARG      # ctc_check_target_args' order
    for bad in (dict(logits=None), dict(target_lengths=None), dict(nll=None), dict(loss=None), dict(ws=None),
                dict(targets=None), dict(B=0), dict(T=0), dict(V=0), dict(ld=9), dict(max_target_len=-1),
                dict(reduction=2), dict(dlogits_dtype=2), dict(ws_elems=100), dict(ws=P0 + 4)):
        assert f(*_loss_args(**bad)) == ERR_ARG, bad
    assert f(*_loss_args(B=65536, ws_elems=1 << 50)) == ERR_UNSUPPORTED
    assert f(*_loss_args(B=30000, T=30000, ws_elems=1 << 60)) == ERR_UNSUPPORTED     # the B * T bound
    assert f(*_loss_args(V=9000, ld=9000)) == ERR_UNSUPPORTED                        # asrx_ctc_loss's row limit
    # the workspace rule is the helper's own: one element short is refused
    rc, n = _size(asrx.native().asrx_ctc_long_workspace_elems, 2, 8, 300)
    assert rc == 0 and f(*_loss_args(max_target_len=300, ws_elems=n - 1)) == ERR_ARG


def test_align_long_refuses_bad_arguments_without_gpu():
    import asrx
    f = asrx.native().asrx_ctc_align_long
    null = dict(logits=None, targets=None, target_lengths=None, ws=None, frame_pos=None, score=None)
    assert f(*_align_args(max_target_len=4096, tgt_stride=4096, **null)) == ERR_UNSUPPORTED
    assert f(*_align_args(max_target_len=4095, tgt_stride=4095, **null)) == ERR_ARG
    assert f(*_align_args(max_target_len=4095, tgt_stride=4094)) == ERR_ARG
    assert f(*_align_args(B=65536, ws_words=1 << 40)) == ERR_UNSUPPORTED
    for bad in (dict(blank=-1), dict(blank=10), dict(T=0), dict(B=0), dict(V=0), dict(ld=9), dict(max_target_len=-1),
                dict(tgt_stride=6), dict(logits=None), dict(targets=None), dict(target_lengths=None), dict(ws=None),
                dict(ws=P0 + 0x3002), dict(frame_pos=None), dict(frame_logp=None), dict(tok_start=None),
                dict(tok_end=None), dict(tok_conf=None), dict(score=None)):
        assert f(*_align_args(**bad)) == ERR_ARG, bad
    words = 2 * 2 * 9 + 32 * 2 * 9          # B 2, T 9, NW 1
    assert f(*_align_args(ws_words=words - 1)) == ERR_ARG


def test_edit_distance_long_refuses_bad_arguments_without_gpu():
    import asrx
    f = asrx.native().asrx_edit_distance_long
    for bad in (dict(N=0), dict(hyp_cols=0), dict(ref_cols=0), dict(ld_hyp=11), dict(ld_ref=7), dict(ndrop=-1),
                dict(ndrop=1, drop=None), dict(hyp=None), dict(dist=None), dict(ref=None), dict(mode=1, W=0),
                dict(mode=2, W=17, N=17 * 17), dict(mode=2, W=2), dict(mode=3)):
        assert f(*_ed(**bad)) == ERR_ARG, bad


def test_size_helpers():
    """Loss: row statistics, 4100 ints per sample, -log2 P, then alpha and beta rows of 512 * NW floats, NW =
    ceil((L + 1) / 256).  Alignment: 2 B T words and one 16-bit backpointer word per thread and frame."""
    import asrx
    from asrx import kernels as K
    lib = asrx.native()

    def r4(x):
        return (x + 3) // 4 * 4
    prev_l = prev_a = 0
    for L, nw in ((0, 1), (255, 1), (256, 2), (511, 2), (512, 3), (1023, 4), (1024, 5), (2047, 8), (4095, 16)):
        rc, n = _size(lib.asrx_ctc_long_workspace_elems, 16, 999, L)
        assert rc == 0 and n == r4(2 * 16 * 999) + r4(4100 * 16) + r4(16) + 2 * 16 * 999 * 512 * nw, L
        rc, w = _size(lib.asrx_ctc_align_long_workspace_words, 16, 999, L)
        assert rc == 0 and w == 2 * 16 * 999 + 32 * nw * 16 * 999, L
        assert n >= prev_l and w >= prev_a and (nw == 1 or L % 256 or (n > prev_l and w > prev_a))   # grows with NW
        prev_l, prev_a = n, w
        assert K.ctc_workspace_elems(16, 999, L, long=True) == n and K.ctc_align_workspace_words(16, 999, L, long=True) == w
    for fn in (lib.asrx_ctc_long_workspace_elems, lib.asrx_ctc_align_long_workspace_words):
        for bad in ((0, 5, 5), (-1, 5, 5), (5, 0, 5), (5, 5, -1), (5, 5, 4096), (5, 5, 100000)):
            assert _size(fn, *bad) == (-1, -1), bad
        assert fn(5, 5, 5, None) == -1
    # beyond 2^31 without overflow
    rc, n = _size(lib.asrx_ctc_long_workspace_elems, 64, 4000, 4095)
    assert rc == 0 and n == r4(2 * 64 * 4000) + 4100 * 64 + 64 + 2 * 64 * 4000 * 8192 and n > 2 ** 31
    rc, w = _size(lib.asrx_ctc_align_long_workspace_words, 64, 4000, 4095)
    assert rc == 0 and w == 2 * 64 * 4000 + 512 * 64 * 4000 and w > 2 ** 26
    rc, w = _size(lib.asrx_ctc_align_long_workspace_words, 65535, 8000, 4095)
    assert rc == 0 and w == 514 * 65535 * 8000 and w > 2 ** 37
    for fn in (K.ctc_workspace_elems, K.ctc_align_workspace_words):
        with pytest.raises(RuntimeError):
            fn(1, 10, 4096, long=True)
        with pytest.raises(RuntimeError):
            fn(1, 10, 256)                      # the default is the short rule


def test_the_dispatch_rule():
    """A teacher-forced row holds BOS and EOS beside its labels (framing 2); a target row holds labels only."""
    from asrx import kernels as K
    text = {255: (False, 255), 256: (False, 255), 257: (False, 255), 258: (True, 258), 4095: (True, 4095),
            4097: (True, 4095)}
    for width, want in text.items():
        assert K.ctc_path(width, framing=2) == want, width
    labels = {0: (False, 0), 255: (False, 255), 256: (True, 256), 257: (True, 257), 258: (True, 258),
              4095: (True, 4095), 4097: (True, 4095)}
    for width, want in labels.items():
        assert K.ctc_path(width) == want, width
    assert K.edit_path(255, 255) == (False, 255) and K.edit_path(256, 3) == (True, 4095)
    assert K.edit_path(3, 300) == (True, 4095) and K.edit_path(10) == (False, 255) and K.edit_path(5000) == (True, 4095)


def test_python_layers_name_the_bound():
    import asrx
    from asrx.score import reduce_counts
    crit = asrx.CTCLoss()
    with pytest.raises(ValueError, match="4095"):
        crit(torch.zeros(1, 3, 4), torch.ones(1, 4096, dtype=torch.int64), torch.tensor([3]), torch.tensor([1]))
    with pytest.raises(RuntimeError, match="GPU"):          # 4095 columns pass that check: the device rule is next
        crit(torch.zeros(1, 3, 4), torch.ones(1, 4095, dtype=torch.int64), torch.tensor([3]), torch.tensor([1]))
    d0, c0 = torch.tensor([[0], [2], [1]]), torch.tensor([[[0, 0, 0, 4]], [[1, 1, 0, 5]], [[0, 0, 1, 3]]])
    bad = (torch.tensor([[1, 0], [0, -2]]), -torch.ones(2, 2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="sample 4 .*4095"):
        reduce_counts([(d0, c0), bad], max_tokens=4095)
    with pytest.raises(ValueError, match="sample 4 .*4095"):
        reduce_counts([(d0, c0), bad], max_tokens=[255, 4095])
    with pytest.raises(ValueError, match="sample 4 .*255"):
        reduce_counts([(d0, c0), bad])
    assert reduce_counts([(d0, c0)], max_tokens=4095)["n_edits"] == 3
