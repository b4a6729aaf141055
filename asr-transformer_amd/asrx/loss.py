"""Cross-entropy as an nn.Module over the native kernels (asrx_cross_entropy_ls): loss, gradient and the step's
statistics from one read of the logits, label smoothing included.  GPU tensors only, like the rest of the package."""
import torch
from torch import nn

from . import kernels as K


def _rows(x, V):
    """x (rows, V) as fp32 rows the kernel can walk in place (unit column stride, row stride >= V), or a contiguous
    copy."""
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= V):
        return x
    return x.contiguous()


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, label_smoothing, owner):
        x = logits.detach()
        if x.dim() == 3:   # (N, V, L): class dimension second, as nn.CrossEntropyLoss takes it
            N, V, L = x.shape
            y = x.transpose(1, 2)
            try:   # the transposed view of a (N, L, ld)[:, :, :V] buffer is [N * L, ld] rows where it lies
                y = y.view(N * L, V)
            except RuntimeError:
                y = y.contiguous().view(N * L, V)
        else:
            y = x
        V = y.shape[1]
        y = _rows(y, V)
        want_grad = logits.requires_grad
        loss, dl, _, stats = K.cross_entropy(y, V, target, ignore_index=ignore_index, want_grad=want_grad,
                                             label_smoothing=label_smoothing, grad_dtype=torch.float32,
                                             want_stats=True, strided=True)
        owner.last_stats = stats
        ctx.shape, ctx.in_dtype = tuple(logits.shape), logits.dtype
        ctx.save_for_backward(dl)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_out):
        (dl,) = ctx.saved_tensors
        if dl is None:
            return (None,) * 5
        shape = ctx.shape
        V = shape[1]
        g = dl[:, :V] * grad_out
        if len(shape) == 3:
            g = g.view(shape[0], shape[2], V).transpose(1, 2)
        return g.to(ctx.in_dtype), None, None, None, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(ignore_index=, label_smoothing=) with mean reduction, on the GPU kernels:

        loss = asrx.CrossEntropyLoss(label_smoothing=0.1)(logits.transpose(1, 2), text[:, 1:])

      input   (N, V, L) or (rows, V) float logits on the GPU, the class dimension second.  The reference's
              `logits.transpose(1, 2)` of this package's model output is recognised by its strides and read in place;
              any other layout is made contiguous first.
      target  (N, L) or (rows,) integer class indices; ignore_index rows count for nothing.

    One call computes the loss and, where the input requires a gradient, the gradient; backward multiplies it by the
    incoming gradient.  All rows ignored gives 0 (torch: NaN).  last_stats: device fp32 [2] of the last call, the mean
    unsmoothed negative log-likelihood (log perplexity) and the token accuracy over the rows that count.
    Deterministic (no atomics).  CPU tensors raise: there is no fallback."""

    def __init__(self, ignore_index=-100, label_smoothing=0.0):
        super().__init__()
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"asrx.CrossEntropyLoss: label_smoothing {label_smoothing} outside [0, 1)")
        self.ignore_index, self.label_smoothing = int(ignore_index), float(label_smoothing)
        self.last_stats = None

    def forward(self, input, target):
        for t in (input, target):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise RuntimeError("asrx.CrossEntropyLoss: tensors must live on the GPU (no CPU fallback)")
        if input.dim() not in (2, 3) or not input.is_floating_point():
            raise ValueError("asrx.CrossEntropyLoss: input must be float (N, V, L) or (rows, V)")
        want = (input.shape[0], input.shape[2]) if input.dim() == 3 else (input.shape[0],)
        if tuple(target.shape) != want or target.is_floating_point():
            raise ValueError(f"asrx.CrossEntropyLoss: target must be integer class indices of shape {want}")
        tgt = target.to(torch.int64).reshape(-1).contiguous()
        return _CrossEntropyFn.apply(input, tgt, self.ignore_index, self.label_smoothing, self)
