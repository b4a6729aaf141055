"""Label-smoothed cross-entropy, host side (no GPU): the fp64 restatement of the formulas (tests/xent_ref.py) against
torch.nn.functional.cross_entropy and its autograd gradient, asrx_cross_entropy_ls's argument checks (made before any
HIP call), the derived signatures, and the Python front ends' own validation."""
import ctypes
import os
import re

import pytest
import torch

from tests import xent_ref as R


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_reference_is_torch_cross_entropy(eps, ignore_index):
    """Loss and gradient to 1e-12 in fp64, with ignored rows (a stride of them, or the class-0 rows)."""
    g = torch.Generator().manual_seed(7)
    rows, V = 23, 37
    x = torch.randn(rows, V, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, V, (rows,), generator=g)
    t[0], t[1] = 0, V - 1
    if ignore_index != 0:
        t[3::5] = ignore_index
    else:
        t[4::6] = 0
    assert 0 < int((t == ignore_index).sum()) < rows
    xr = x.clone().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(xr, t, ignore_index=ignore_index, label_smoothing=eps)
    want.backward()
    want = want.detach()
    got = R.cross_entropy(x, t, ignore_index=ignore_index, eps=eps)
    assert abs(float(got.loss) - float(want)) < 1e-12 * max(1.0, abs(float(want)))
    assert float((got.grad - xr.grad).abs().max()) < 1e-12
    assert bool((got.grad[t == ignore_index] == 0).all())
    assert torch.equal(got.argmax, x.argmax(-1))
    plain = torch.nn.functional.cross_entropy(x, t, ignore_index=ignore_index)
    assert abs(float(got.nll) - float(plain)) < 1e-12
    scaled = R.cross_entropy(x, t, ignore_index=ignore_index, eps=eps, grad_scale=0.125)
    assert float((scaled.grad - 0.125 * xr.grad).abs().max()) < 1e-12


def test_reference_with_every_row_ignored():
    x = torch.randn(4, 9, dtype=torch.float64)
    got = R.cross_entropy(x, torch.full((4,), -100), eps=0.1)
    assert float(got.loss) == 0.0 and float(got.nll) == 0.0 and got.acc == 0.0 and bool((got.grad == 0).all())


def _xent(lib, logits=4096, rows=8, V=100, ld=128, target=8192, ignore=-100, eps=0.1, gs=1.0, loss=12288,
          stats=16384, gdt=0, dl=1 << 20, am=1 << 21, ws=1 << 22):
    return lib.asrx_cross_entropy_ls(logits, rows, V, ld, target, ignore, eps, gs, loss, stats, gdt, dl, am, ws, None)


def test_abi_rejects_bad_arguments_without_gpu():
    """Every refusal of the header's list comes before any HIP call (fake device addresses; no GPU here)."""
    import asrx
    from asrx._lib import CONSTS
    lib = asrx.native()
    assert lib.asrx_version() >= 14
    ARG, UNSUPPORTED = -1, -3
    for null in ("logits", "target", "loss", "ws"):
        assert _xent(lib, **{null: None}) == ARG, null
    assert _xent(lib, V=0) == ARG
    assert _xent(lib, V=-3) == ARG
    assert _xent(lib, V=129) == ARG                       # ld < V
    assert _xent(lib, rows=-1) == ARG
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        assert _xent(lib, eps=eps) == ARG, eps
    for gdt in (-1, 2, 7):
        assert _xent(lib, gdt=gdt) == ARG, gdt
    assert _xent(lib, V=(1 << 20) + 1, ld=(1 << 20) + 64) == UNSUPPORTED
    assert _xent(lib, V=(1 << 20) + 1, ld=(1 << 20) + 64, eps=1.0) == ARG    # the argument checks come first
    assert lib.asrx_xent_workspace_elems(-1) == -1
    assert lib.asrx_xent_workspace_elems(0) >= 1
    assert lib.asrx_xent_workspace_elems(4096) >= 3 * 4096 + 1
    # the count is an int: the most rows it can size, and one more (refused by both functions)
    top = CONSTS["ASRX_XENT_MAX_ROWS"]
    assert lib.asrx_xent_workspace_elems(top) == 3 * top + 4 <= 2 ** 31 - 1 < 3 * (top + 1) + 4
    assert lib.asrx_xent_workspace_elems(top + 1) == -1
    assert _xent(lib, rows=top + 1) == UNSUPPORTED


def _kinds(decl):
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    kinds = []
    for p in decl.split(","):
        p = " ".join(p.split())
        kinds.append(ctypes.c_void_p if "*" in p else scalar[p.split()[0]])
    return kinds


def test_signatures_match_the_header():
    """The derived ctypes signatures have one entry per parameter of the header's declarations, in their types."""
    from asrx._lib import RESTYPES, SIGNATURES
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(repo, "include", "asrx.h")).read(), flags=re.S)
    decl = re.search(r"int asrx_cross_entropy_ls\((.*?)\);", src, re.S).group(1)
    names = [" ".join(p.split()).split()[-1].lstrip("*") for p in decl.split(",")]
    assert names == ["logits", "rows", "V", "ld", "target", "ignore_index", "label_smoothing", "grad_scale", "loss",
                     "stats", "grad_dtype", "dlogits", "argmax", "ws", "stream"]
    c = ctypes
    assert _kinds(decl) == [c.c_void_p, c.c_int64, c.c_int32, c.c_int64, c.c_void_p, c.c_int64, c.c_float, c.c_float,
                            c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    assert SIGNATURES["asrx_cross_entropy_ls"] == _kinds(decl)
    assert RESTYPES["asrx_cross_entropy_ls"] is ctypes.c_int
    # (an int, not the int64_t of the other size helpers: tests/test_host_cpu.py pins which entry points return one)
    decl = re.search(r"\bint asrx_xent_workspace_elems\((.*?)\);", src, re.S).group(1)
    assert SIGNATURES["asrx_xent_workspace_elems"] == _kinds(decl) == [ctypes.c_int64]
    assert RESTYPES["asrx_xent_workspace_elems"] is ctypes.c_int
    # the old entry point's declaration is as it was
    assert len(SIGNATURES["asrx_cross_entropy"]) == 12


def test_python_front_ends_validate_label_smoothing():
    import asrx
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError):
            asrx.CrossEntropyLoss(label_smoothing=bad)
    ce = asrx.CrossEntropyLoss(ignore_index=4, label_smoothing=0.1)
    assert (ce.ignore_index, ce.label_smoothing, ce.last_stats) == (4, 0.1, None)
    with pytest.raises(RuntimeError):                     # no CPU fallback
        ce(torch.zeros(2, 5, 3), torch.zeros(2, 3, dtype=torch.int64))
    import inspect
    from asrx.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["label_smoothing"].default == 0.0
    sig = inspect.signature(asrx.kernels.cross_entropy).parameters
    assert (sig["label_smoothing"].default, sig["grad_dtype"].default, sig["want_stats"].default) == \
        (0.0, torch.bfloat16, False)
