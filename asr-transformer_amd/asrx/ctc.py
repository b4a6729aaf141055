"""CTC loss as an nn.Module over the native kernels (asrx_ctc_loss, and asrx_ctc_loss_long for targets wider than 255):
negative log-likelihood and gradient in one call, the log-softmax fused.  GPU tensors only, like the rest of the
package."""
import torch
from torch import nn

from . import kernels as K
from ._lib import CTC_LONG_MAX_TARGET


class _CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank, reduction, zero_infinity):
        B, T, V = logits.shape
        use_long, _ = K.ctc_path(targets.shape[1])
        x = logits.detach().to(torch.float32).contiguous().view(B * T, V)
        want_grad = logits.requires_grad
        # 'none' is the sum's kernel call: per-sample weight 1, the per-sample factors applied in backward
        loss, nll, dl = K.ctc_loss(x, V, T, targets, target_lengths, input_lengths, blank=blank,
                                   reduction="mean" if reduction == "mean" else "sum", zero_infinity=zero_infinity,
                                   grad_dtype=torch.float32, want_grad=want_grad, long=use_long)
        ctx.reduction = reduction
        ctx.shape = (B, T, V)
        ctx.in_dtype = logits.dtype
        ctx.save_for_backward(dl)
        if reduction == "none":
            return torch.where(torch.isinf(nll), torch.zeros_like(nll), nll) if zero_infinity else nll
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_out):
        (dl,) = ctx.saved_tensors
        if dl is None:
            return (None,) * 7
        B, T, V = ctx.shape
        g = dl.view(B, T, V)
        g = g * (grad_out.view(B, 1, 1) if ctx.reduction == "none" else grad_out)
        return g.to(ctx.in_dtype), None, None, None, None, None, None


class CTCLoss(nn.Module):
    """Connectionist temporal classification loss on **logits**.

        loss = CTCLoss(blank=0, reduction="mean", zero_infinity=False)(logits, targets, input_lengths, target_lengths)

    computes what

        F.ctc_loss(F.log_softmax(logits, -1).transpose(0, 1), targets, input_lengths, target_lengths,
                   blank=blank, reduction=reduction, zero_infinity=zero_infinity)

    computes — note the two differences from F.ctc_loss(log_probs (T, B, V), ...): the input is unnormalised logits
    (the log-softmax is part of the kernel; do not apply one), and it is batch-first, (B, T, V).

      logits          (B, T, V) float, on the GPU
      targets         (B, Lmax) int64, padded; Lmax <= 4095.  Up to 255 columns take the one-wave kernel, 256 .. 4095
                      the workgroup-per-sample one (asrx_ctc_loss_long); the width decides, not the lengths
      input_lengths   (B,) integer tensor, or None for T everywhere
      target_lengths  (B,) integer tensor
      reduction       "mean" (torch's: mean over the batch of nll / max(target length, 1)), "sum", or "none" (the
                      per-sample values)

    Deterministic (no atomics), unlike torch's device implementation.  CPU tensors raise: there is no fallback."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"asrx.CTCLoss: unknown reduction {reduction!r}")
        self.blank, self.reduction, self.zero_infinity = int(blank), reduction, bool(zero_infinity)

    def forward(self, logits, targets, input_lengths, target_lengths):
        # (first, and whatever device the tensors are on: a width no kernel takes)
        if torch.is_tensor(targets) and targets.dim() == 2 and targets.shape[1] > CTC_LONG_MAX_TARGET:
            raise ValueError(f"asrx.CTCLoss: targets longer than {CTC_LONG_MAX_TARGET} are not supported")
        for t in (logits, targets, input_lengths, target_lengths):
            if t is not None and not (torch.is_tensor(t) and t.is_cuda):
                raise RuntimeError("asrx.CTCLoss: tensors must live on the GPU (no CPU fallback)")
        if logits.dim() != 3:
            raise ValueError("asrx.CTCLoss: logits must be (B, T, V)")
        if targets.dim() != 2 or targets.shape[0] != logits.shape[0] or targets.dtype != torch.int64:
            raise ValueError("asrx.CTCLoss: targets must be int64 (B, Lmax)")
        il = None if input_lengths is None else input_lengths.to(torch.int32).contiguous()
        tl = target_lengths.to(torch.int32).contiguous()
        return _CTCLossFn.apply(logits, targets.contiguous(), il, tl, self.blank, self.reduction, self.zero_infinity)
