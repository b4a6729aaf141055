"""CTC test reference (host only): torch's CPU log_softmax + ctc_loss with autograd, in fp64 (the reference) or fp32
(to measure the error of torch's own single-precision path, from which the kernel tolerances derive), a brute-force
enumeration of all alignments for tiny cases, and the Python loops the target builder and the best-path decoder are
checked against."""
import itertools
import math

import torch
import torch.nn.functional as F


def ctc_reference(logits, targets, input_lengths, target_lengths, blank=0, dtype=torch.float64):
    """logits (B, T, V), targets (B, Lmax), lengths (B,) or None -> (nll (B,) per sample, +inf where no alignment
    exists; dlogits (B, T, V): gradient of sum_b nll_b over the samples with a finite nll, zero rows elsewhere).
    Every reduction and grad_scale is a per-sample weight on these."""
    B, T, V = logits.shape
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    il = torch.full((B,), T, dtype=torch.long) if input_lengths is None else input_lengths.cpu().long()
    tl = target_lengths.cpu().long()
    lp = F.log_softmax(x, dim=-1).transpose(0, 1)
    nll = F.ctc_loss(lp, targets.cpu().long(), il, tl, blank=blank, reduction="none", zero_infinity=False)
    finite = torch.isfinite(nll)
    (g,) = torch.autograd.grad(torch.where(finite, nll, torch.zeros_like(nll)).sum(), x)
    g = torch.where(finite.view(B, 1, 1), g, torch.zeros_like(g))   # (torch leaves NaN in the rows of an inf sample)
    return nll.detach(), g


def sample_weights(target_lengths, B, reduction):
    """The per-sample weight w_b of a reduction: 'sum' 1, 'mean' 1 / (B * max(L_b, 1))."""
    tl = target_lengths.cpu().double()
    return torch.ones(B, dtype=torch.float64) if reduction == "sum" else 1.0 / (B * tl.clamp_min(1.0))


def collapse(path, blank):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return out


def brute_force_nll(logits, target, blank=0):
    """-log of the total probability of every length-T path over V symbols that collapses to `target` (fp64).
    logits (T, V)."""
    T, V = logits.shape
    lp = F.log_softmax(logits.double(), dim=-1)
    total = 0.0
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) == list(target):
            total += math.exp(sum(float(lp[t, s]) for t, s in enumerate(path)))
    return math.inf if total == 0.0 else -math.log(total)


def targets_loop(text, mask, drop, blank):
    """asrx_ctc_targets in Python: per row the tokens with mask >= 1 that are not in `drop`, left-packed."""
    B, n = text.shape
    out = torch.full((B, n), blank, dtype=torch.int64)
    lens = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        keep = [int(text[b, p]) for p in range(n) if float(mask[b, p]) >= 1.0 and int(text[b, p]) not in drop]
        out[b, :len(keep)] = torch.tensor(keep, dtype=torch.int64)
        lens[b] = len(keep)
    return out, lens


def greedy_loop(logits, blank, input_lengths=None):
    """asrx_ctc_greedy in Python: logits (B, T, V) -> (tokens (B, T) padded with blank, lengths (B,))."""
    B, T, V = logits.shape
    am = logits.argmax(dim=-1)     # first index of the maximum
    out = torch.full((B, T), blank, dtype=torch.int64)
    lens = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n = T if input_lengths is None else max(0, min(T, int(input_lengths[b])))
        seq = collapse([int(a) for a in am[b, :n]], blank)
        out[b, :len(seq)] = torch.tensor(seq, dtype=torch.int64)
        lens[b] = len(seq)
    return out, lens
