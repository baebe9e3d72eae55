"""Clip a gradient by its global norm: the CPU twin of ``csrc/kernels/clip.hip``.

``tf.clip_by_global_norm`` on the worker, ahead of ``apply_gradients``: ``norm`` is the square
root of the sum of squares over the payload ranges of the flat gradient buffer, ``coef`` is
``C / norm`` when ``norm > C`` and exactly 1 otherwise (also when the norm is zero or not
finite), and the gradient is scaled in place unless ``coef == 1``.

The sum is not left to a library reduction: every addition has the place the kernel gives it, so
both give the same bits for the same (contents, ranges, C).

* Work is cut into chunks of ``CHUNK`` elements, enumerated range by range; a range's last chunk
  may be short.
* Element ``j`` of a chunk is widened to float64 (its square is then exact) and added to slot
  ``j % SLOTS``, in increasing ``j``, each slot starting from +0.
* The ``SLOTS`` = 4 x 256 slots fold to 256 as ``(s[i] + s[i+256]) + (s[i+512] + s[i+768])``, the
  256 to one by halving: ``s[i] += s[i+h]`` for ``h`` = 128, 64, .. 1.
* The chunk sums add into 256 running sums (``partial[i]`` into sum ``i % 256``, increasing
  ``i``), folded by the same halving.
* ``sqrt`` and ``C / norm`` are formed in float64 and rounded once to float32.

Only float64 summation rounds, so the float32 norm is within 1 ulp of the exact one.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

CHUNK = 8192      # clip_ranges.h kClipChunk
SLOTS = 1024      # clip_ranges.h kClipSlots
LANES = 256       # clip_ranges.h kClipThreads
MAX_RANGES = 16


def payload_ranges(tensor_offsets: Sequence[int]) -> List[Tuple[int, int]]:
    """The ``(lo, n)`` ranges of the 14 tensors in a plan buffer, in plan order.  The alignment
    padding between them is not part of the norm."""
    from ..models.layout import TENSORS
    return sorted((int(tensor_offsets[t.index]), int(t.numel)) for t in TENSORS)


def check_ranges(ranges: Sequence[Tuple[int, int]], total: int) -> List[Tuple[int, int]]:
    out = [(int(lo), int(n)) for lo, n in ranges]
    if len(out) > MAX_RANGES:
        raise ValueError("clip: more than 16 ranges")
    for lo, n in out:
        if lo < 0 or n < 0 or lo + n > total:
            raise ValueError(f"clip: range ({lo}, {n}) outside the buffer of {total}")
    return out


def _fold(s: torch.Tensor) -> torch.Tensor:
    """[..., 256] float64 -> [...]: the halving fold, s[i] += s[i+h]."""
    h = s.shape[-1] // 2
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def chunk_sums(grads: torch.Tensor, ranges: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """The float64 sum of squares of every chunk, in chunk order."""
    parts = []
    for lo, n in ranges:
        if n == 0:
            continue
        x = grads[lo:lo + n].detach().to("cpu", torch.float64)
        nch = (n + CHUNK - 1) // CHUNK
        sq = torch.zeros(nch * CHUNK, dtype=torch.float64)
        sq[:n] = x * x
        sq = sq.view(nch, CHUNK // SLOTS, SLOTS)
        acc = torch.zeros(nch, SLOTS, dtype=torch.float64)
        for k in range(CHUNK // SLOTS):   # increasing j within every slot
            acc = acc + sq[:, k, :]
        a = acc.view(nch, 4, LANES)
        parts.append(_fold((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])))
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64)


def grad_norm_coef(grads: torch.Tensor, ranges: Sequence[Tuple[int, int]],
                   max_norm: float) -> Tuple[float, float]:
    """``(norm, coef)`` as float32 values (returned as Python floats), in the kernel's order."""
    if not max_norm > 0.0:
        raise ValueError("clip: max_norm must be positive")
    ranges = check_ranges(ranges, grads.numel())
    p = chunk_sums(grads, ranges)
    rows = (p.numel() + LANES - 1) // LANES
    pad = torch.zeros(max(rows, 1) * LANES, dtype=torch.float64)
    pad[:p.numel()] = p
    pad = pad.view(-1, LANES)
    s = torch.zeros(LANES, dtype=torch.float64)
    for r in range(pad.shape[0]):
        s = s + pad[r]
    nd = torch.sqrt(_fold(s))
    norm = nd.to(torch.float32)
    c = torch.tensor(float(torch.tensor(max_norm, dtype=torch.float32)), dtype=torch.float64)
    coef = torch.tensor(1.0, dtype=torch.float32)
    if bool(torch.isfinite(norm)) and bool(nd > c):
        coef = (c / nd).to(torch.float32)
    return float(norm), float(coef)


def clip_grads_(grads: torch.Tensor, ranges: Sequence[Tuple[int, int]],
                max_norm: float) -> Tuple[float, float]:
    """Clip ``grads`` (a CPU tensor) in place over ``ranges``; returns ``(norm, coef)``.  With
    ``coef == 1`` no element is rewritten."""
    norm, coef = grad_norm_coef(grads, ranges, max_norm)
    if coef != 1.0:
        a = torch.tensor(coef, dtype=torch.float32)
        for lo, n in check_ranges(ranges, grads.numel()):
            grads[lo:lo + n].mul_(a)
    return norm, coef
