"""Accumulate a gradient over K micro-batches: the CPU twin of ``csrc/kernels/accum.hip``.

``--accum-steps K``: a step runs K micro-batches of ``batch_size`` images and updates once, from
the mean of their gradients.  With ``g`` the gradient buffer after micro-batch ``j`` (0-based) and
``A`` the fp32 accumulator of the same size, over the payload ranges only:

* ``j = 0`` (K >= 2): ``A[i] := g[i]``, the bits copied (a ``-0.0`` stays ``-0.0``);
* ``0 < j < K - 1``: ``A[i] := A[i] + g[i]``, one float32 add;
* ``j = K - 1``: ``g[i] := (A[i] + g[i]) * r`` with ``r = float32(1.0 / K)`` formed in float64 and
  rounded once: one rounded add, then one rounded multiply.

The alignment padding of ``g`` and of ``A`` keeps its bits.  Afterwards ``g`` holds the effective
gradient (the loss head divides by the batch, so this is the mean-loss gradient of K * B images)
and everything downstream reads it as it reads a single step's gradient.  Plain torch float32
ops, one per rounding, so the kernel and the twin give the same bits.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from .clip import check_ranges

FIRST, ADD, FINISH = 0, 1, 2   # api.h kAccumFirst / kAccumAdd / kAccumFinish


def check_accum_steps(k: int) -> None:
    """Refuse a micro-batch count below 1 (or not an integer); 1 switches accumulation off."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"--accum-steps must be an integer of at least 1 (got {k})")


def mode_of(j: int, k: int) -> int:
    """The pass that follows micro-batch ``j`` of ``k`` (``k`` >= 2)."""
    if k < 2 or not 0 <= j < k:
        raise ValueError(f"accum: micro-batch {j} of {k}")
    return FINISH if j == k - 1 else (FIRST if j == 0 else ADD)


def recip(k: int) -> torch.Tensor:
    """``float32(1.0 / k)``: the quotient formed in float64, rounded once."""
    return torch.tensor(1.0 / float(k), dtype=torch.float64).to(torch.float32)


def accum_grads_(grads: torch.Tensor, acc: torch.Tensor, ranges: Sequence[Tuple[int, int]],
                 mode: int, k: int) -> None:
    """One pass of ``mode`` over ``ranges`` [(lo, n)] of the CPU tensors ``grads`` and ``acc``,
    in place."""
    if k < 2:
        raise ValueError("accum: K must be at least 2")
    if mode not in (FIRST, ADD, FINISH):
        raise ValueError("accum: mode 0 (first), 1 (add) or 2 (finish)")
    if acc.numel() != grads.numel() or acc.dtype != torch.float32 or \
            grads.dtype != torch.float32:
        raise ValueError("accum: acc must be a float32 buffer of the size of grads")
    r = recip(k)
    for lo, n in check_ranges(ranges, grads.numel()):
        g, a = grads[lo:lo + n], acc[lo:lo + n]
        if mode == FIRST:
            a.copy_(g)
        elif mode == ADD:
            a.add_(g)
        else:
            g.copy_((a + g) * r)
