"""CTC, host side (no GPU): the new entry points are exported and validate their arguments before any device
access, the workspace size rule, the Transformer's CTC head leaves the reference state_dict schema alone, and the
test reference (torch's fp64 CPU path) agrees with a brute-force enumeration of all alignments."""
import json
import math
import os

import pytest
import torch

from oracle.ref_model import CONFIGS, det_params
from tests import ctc_ref

ERR_ARG, ERR_UNSUPPORTED = -1, -3
P0 = 0x10000   # never dereferenced: validation returns before any launch


def _loss_args(**kw):
    a = dict(logits=P0, B=2, T=8, V=10, ld=16, targets=P0 + 0x1000, tgt_stride=300, input_lengths=None,
             target_lengths=P0 + 0x2000, max_target_len=4, blank=0, reduction=1, zero_infinity=0, grad_scale=1.0,
             nll=P0 + 0x3000, loss=P0 + 0x4000, dlogits=P0 + 0x5000, dlogits_dtype=0, loss_add=None,
             loss_add_scale=0.0, loss_scale=1.0, ws=P0 + 0x100000, ws_elems=1 << 30, stream=None)
    a.update(kw)
    return list(a.values())


def test_ctc_symbols_are_exported_and_version_is_5():
    import asrx
    from asrx._lib import SIGNATURES
    lib = asrx.native()
    for s in ("asrx_ctc_loss", "asrx_ctc_targets", "asrx_ctc_greedy", "asrx_ctc_workspace_elems"):
        assert hasattr(lib, s), s
        assert s in SIGNATURES, s
    assert lib.asrx_version() >= 5
    assert asrx.CTCLoss is not None


@pytest.mark.parametrize("B,T,L", [(64, 249, 62), (64, 249, 63), (64, 249, 64), (16, 999, 254), (16, 999, 255),
                                   (1, 1, 0), (3, 7, 127), (3, 7, 128), (5, 11, 191), (5, 11, 192)])
def test_ctc_workspace_size_rule(B, T, L):
    """Row statistics (2 per row), the per-sample tables (260 words), -log2 P per sample, then log2 alpha and beta:
    128 * ceil((L + 1) / 64) values per row each; every region rounded up to 4 elements."""
    import asrx
    lib = asrx.native()

    def r4(x):
        return (x + 3) // 4 * 4
    kp = (L + 1 + 63) // 64
    assert 1 <= kp <= 4
    assert lib.asrx_ctc_workspace_elems(B, T, L) == r4(2 * B * T) + r4(260 * B) + r4(B) + 2 * B * T * 128 * kp


def test_ctc_workspace_size_rule_rejects_bad_arguments():
    import asrx
    lib = asrx.native()
    for B, T, L in [(0, 5, 3), (-1, 5, 3), (2, 0, 3), (2, -4, 3), (2, 5, -1), (2, 5, 256), (2, 5, 1000)]:
        assert lib.asrx_ctc_workspace_elems(B, T, L) == -1, (B, T, L)
    # large but legal: the result does not wrap at 2^31
    assert lib.asrx_ctc_workspace_elems(4096, 4000, 255) > 2 ** 31


def test_ctc_loss_refuses_a_256_token_target_and_a_bad_blank_without_gpu():
    """Both checks sit before any device access: the pointers here are not mapped."""
    import asrx
    lib = asrx.native()
    assert lib.asrx_ctc_loss(*_loss_args(max_target_len=256)) == ERR_UNSUPPORTED
    assert lib.asrx_ctc_loss(*_loss_args(max_target_len=255, tgt_stride=254)) == ERR_ARG   # rows shorter than the bound
    assert lib.asrx_ctc_loss(*_loss_args(blank=10)) == ERR_ARG      # blank >= V
    assert lib.asrx_ctc_loss(*_loss_args(blank=-1)) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(logits=None), dict(target_lengths=None), dict(nll=None), dict(loss=None),
                                 dict(ws=None), dict(targets=None), dict(B=0), dict(T=0), dict(V=0), dict(ld=9),
                                 dict(max_target_len=-1), dict(reduction=2), dict(dlogits_dtype=2), dict(ws_elems=100),
                                 dict(ws=P0 + 4)])
def test_ctc_loss_rejects_bad_arguments_without_gpu(bad):
    import asrx
    assert asrx.native().asrx_ctc_loss(*_loss_args(**bad)) == ERR_ARG


def test_ctc_targets_and_greedy_reject_bad_arguments_without_gpu():
    import ctypes
    import asrx
    lib = asrx.native()
    drop = (ctypes.c_int64 * 4)(1, 2, 4, 0)
    ok = dict(text=P0, ld_text=9, mask=P0 + 0x1000, ld_mask=9, B=2, n=9, drop=drop, ndrop=3, blank=4,
              targets=P0 + 0x2000, ld_targets=9, target_lengths=P0 + 0x3000, stream=None)
    for bad in (dict(text=None), dict(mask=None), dict(targets=None), dict(target_lengths=None), dict(B=0), dict(n=0),
                dict(ld_text=8), dict(ld_mask=8), dict(ld_targets=8), dict(ndrop=5), dict(ndrop=-1),
                dict(drop=None)):
        assert lib.asrx_ctc_targets(*{**ok, **bad}.values()) == ERR_ARG, bad
    ok = dict(logits=P0, B=2, T=8, V=10, ld=16, input_lengths=None, blank=0, tok=P0 + 0x1000, len=P0 + 0x2000,
              stream=None)
    for bad in (dict(logits=None), dict(tok=None), dict(len=None), dict(B=0), dict(T=0), dict(V=0), dict(ld=9),
                dict(blank=10), dict(blank=-1)):
        assert lib.asrx_ctc_greedy(*{**ok, **bad}.values()) == ERR_ARG, bad
    assert lib.asrx_ctc_greedy(*{**ok, **dict(T=20000)}.values()) == ERR_UNSUPPORTED


def test_ctc_loss_module_refuses_cpu_tensors_and_long_targets():
    import asrx
    crit = asrx.CTCLoss()
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.zeros(1, 3, 4), torch.ones(1, 1, dtype=torch.int64), torch.tensor([3]), torch.tensor([1]))
    with pytest.raises(ValueError):
        asrx.CTCLoss(reduction="batchmean")


# ---------------------------------------------------------------------------------------------- model schema

def _build(name, **kw):
    import asrx
    cfg = CONFIGS[name]["cfg"]
    return asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                            cfg.n_dec, cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, **kw), cfg


def test_ctc_false_keeps_the_reference_schema(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "ref_state_dict_schema.json")))
    m, cfg = _build("c1", ctc=False)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["c1"]
    assert not hasattr(m, "ctc_head")


def test_ctc_true_adds_exactly_one_key(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "ref_state_dict_schema.json")))
    m, cfg = _build("c1", ctc=True)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got[:-1] == ref["c1"]
    assert got[-1] == ["ctc_head.weight", [cfg.vocab_size, cfg.d_model]]
    assert m.ctc_blank == cfg.pad_id                       # the default blank: the padding id, never a target
    assert _build("c1", ctc=True, ctc_blank=0)[0].ctc_blank == 0
    with pytest.raises(ValueError):
        _build("c1", ctc=True, ctc_blank=cfg.vocab_size)


def test_ctc_head_does_not_move_the_other_parameters():
    """Same seed: every shared parameter of a ctc=True model starts from the values of the ctc=False model, and the
    flat store keeps them at the same offsets (the head is registered last)."""
    from asrx.functions import param_order
    torch.manual_seed(3)
    m0, _ = _build("micro")
    torch.manual_seed(3)
    m1, _ = _build("micro", ctc=True)
    p0, p1 = dict(m0.named_parameters()), dict(m1.named_parameters())
    assert set(p1) - set(p0) == {"ctc_head.weight"}
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    o0, o1 = param_order(m0), param_order(m1)
    assert len(o1) == len(o0) + 1 and o1[-1] is m1.ctc_head.weight
    assert [tuple(p.shape) for p in o1[:-1]] == [tuple(p.shape) for p in o0]


def test_loading_a_reference_checkpoint_leaves_the_head_alone():
    m0, cfg = _build("c1")
    sd = m0.state_dict()
    sd.update(det_params(cfg, 5))
    m1, _ = _build("c1", ctc=True)
    head0 = m1.ctc_head.weight.detach().clone()
    res = m1.load_state_dict(sd, strict=False)
    assert list(res.missing_keys) == ["ctc_head.weight"] and not res.unexpected_keys
    assert torch.equal(m1.ctc_head.weight, head0)
    assert float(head0[:cfg.vocab_size].abs().max()) > 0 and float(head0[cfg.vocab_size:].abs().max()) == 0
    got = m1.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    with pytest.raises(RuntimeError):
        m1.load_state_dict(sd, strict=True)


def test_trainer_argument_rules():
    """A positive ctc_weight needs a head — refused before the Trainer touches the device."""
    from asrx.train import Trainer
    m, _ = _build("micro")
    with pytest.raises(ValueError, match="ctc=True"):
        Trainer(m, ctc_weight=0.3)
    with pytest.raises(ValueError):
        Trainer(m, ctc_weight=1.0)


# ---------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("T,target", [(1, []), (1, [1]), (2, [1]), (3, [1, 2]), (3, [1, 1]), (4, [1, 1]), (5, [2, 2]),
                                      (5, [1, 2]), (4, []), (2, [1, 1]), (1, [1, 2])])
def test_reference_equals_enumeration(T, target):
    """V = 3, T <= 5, L <= 2, repeats included (T = 3, [1, 1] is the only feasible length; T = 2 has no alignment)."""
    g = torch.Generator().manual_seed(100 * T + len(target))
    logits = torch.randn(1, T, 3, generator=g, dtype=torch.float64) * 2
    tg = torch.tensor([target + [0] * (2 - len(target))], dtype=torch.int64)
    nll, grad = ctc_ref.ctc_reference(logits, tg, None, torch.tensor([len(target)]), blank=0)
    want = ctc_ref.brute_force_nll(logits[0], target, blank=0)
    if math.isinf(want):
        assert math.isinf(float(nll[0])) and float(grad.abs().max()) == 0.0
    else:
        assert abs(float(nll[0]) - want) < 1e-12 * max(1.0, abs(want))
        # the gradient rows sum to zero (softmax minus an occupancy that sums to one)
        assert float(grad.sum(-1).abs().max()) < 1e-12


def test_reference_blank_position_and_python_loops():
    logits = torch.randn(1, 4, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    for blank, target in ((2, [0, 1]), (1, [0, 2])):
        nll, _ = ctc_ref.ctc_reference(logits, torch.tensor([target]), None, torch.tensor([2]), blank=blank)
        assert abs(float(nll[0]) - ctc_ref.brute_force_nll(logits[0], target, blank=blank)) < 1e-12
    text = torch.tensor([[1, 7, 7, 9, 2, 4], [1, 2, 4, 4, 4, 4], [1, 5, 6, 7, 8, 9]])
    mask = (text != 4).float()
    tg, ln = ctc_ref.targets_loop(text, mask, (1, 2, 4), 4)
    assert tg.tolist() == [[7, 7, 9, 4, 4, 4], [4] * 6, [5, 6, 7, 8, 9, 4]] and ln.tolist() == [3, 0, 5]
    lg = torch.zeros(1, 6, 3)
    for t, s in enumerate([1, 1, 0, 1, 2, 2]):
        lg[0, t, s] = 1.0
    tok, n = ctc_ref.greedy_loop(lg, 0)
    assert tok.tolist() == [[1, 1, 2, 0, 0, 0]] and n.tolist() == [3]
    tok, n = ctc_ref.greedy_loop(lg, 0, torch.tensor([2]))
    assert tok.tolist() == [[1, 0, 0, 0, 0, 0]] and n.tolist() == [1]
