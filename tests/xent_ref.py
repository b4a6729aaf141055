"""Label-smoothed cross-entropy in fp64, the formulas of include/asrx.h (asrx_cross_entropy_ls) written out: what the
kernels are compared with.  tests/test_xent_cpu.py holds it against torch.nn.functional.cross_entropy."""
from typing import NamedTuple

import torch


class Xent(NamedTuple):
    loss: torch.Tensor      # fp64 scalar
    grad: torch.Tensor      # fp64 [rows, V], d loss / d logits (times grad_scale)
    argmax: torch.Tensor    # int64 [rows], first index of the row maximum
    nll: torch.Tensor       # fp64 scalar, mean unsmoothed nll over the valid rows
    acc: float              # (#valid rows with argmax == target) / n


def cross_entropy(x, t, ignore_index=-100, eps=0.0, grad_scale=1.0):
    """x [rows, V] (any float dtype, read as fp64), t int64 [rows].  n = #rows with t != ignore_index;
    row = (1 - eps) (lse - x[t]) + eps (lse - mean_c x[c]); loss = sum row / n; grad = grad_scale / n (softmax -
    (1 - eps) onehot - eps / V) on valid rows, 0 on ignored ones; n == 0: loss 0, grad 0, nll 0, acc 0."""
    x = x.detach().double()
    rows, V = x.shape
    valid = t != ignore_index
    n = int(valid.sum())
    lse = torch.logsumexp(x, dim=-1)
    ts = torch.where(valid, t, torch.zeros_like(t))
    nll = lse - x.gather(1, ts[:, None])[:, 0]
    smooth = lse - x.mean(dim=-1)
    row = (1.0 - eps) * nll + eps * smooth if eps > 0 else nll
    am = x.argmax(dim=-1)
    if n == 0:
        z = torch.zeros((), dtype=torch.float64)
        return Xent(z, torch.zeros_like(x), am, z, 0.0)
    loss = row[valid].sum() / n
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), ts] = 1.0
    g = (torch.softmax(x, dim=-1) - (1.0 - eps) * onehot - eps / V) * (grad_scale / n)
    g = g * valid[:, None].double()
    return Xent(loss, g, am, nll[valid].sum() / n, float((am == t)[valid].sum()) / n)
