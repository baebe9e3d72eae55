"""Shuffled, shift-augmented batches: the index rule and the CPU twin of ``csrc/kernels/batch.hip``.

``--shuffle`` reads every pass over the training set in a fresh pseudo-random order, without
replacement; ``--augment-shift S`` translates every training image by a per-draw ``(dx, dy)``, each
uniform in ``[-S, S]``, zero-filled.  Both are stateless functions of a few integers, so every rank
derives the same thing, a resumed run is the uninterrupted run, and the device evaluates them per
row: no index array, no host-to-device copy, no RNG state.

**The permutation.**  ``perm(i; N, key)`` is a bijection on ``[0, N)``: a balanced Feistel network
of ``ROUNDS`` rounds over ``b`` bits, ``b`` the smallest even number ``>= max(2, bitlength(N - 1))``,
with cycle-walking (re-applied until the value is ``< N``; the walk stays on the cycle of the
network's permutation through ``i < N``, so it ends).  With ``h = b / 2`` and ``x = (L << h) | R``,
round ``j`` maps ``(L, R)`` to ``(R, L ^ (mix32(R ^ k_j) & (2^h - 1)))`` and ``k_j = mix32(key +
j * GOLDEN)``; ``mix32`` is the dropout RNG's lowbias32 (``ops/rng.py``).

**The keys.**  ``batch_key(seed, epoch, wrap, salt)`` chains ``mix32`` over the run's seed, the
epoch (``global_step // steps_per_epoch``) and the wrap (how often the raw batch number has gone
round the set inside the epoch); the rank is not part of it.  ``PERM_SALT`` gives the permutation's
key and ``SHIFT_SALT`` the shift's.

**A batch.**  Row ``n`` of the batch at ``base = slot * B`` is training row ``perm(base + n)`` (or
``base + n`` unshuffled), moved by ``shift_of(base + n, key_shift, S)``: ``out[r][c] =
in[r - dy][c - dx]`` inside the 28 x 28 image, else ``0.0``.  Pure data movement: the kernel and
the twin give equal bits.  The same constants appear in ``csrc/kernels/batch.h``.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from .rng import GOLDEN, M32, _mix, mix_scalar

ROUNDS = 4
PERM_SALT = 0x243F6A88
SHIFT_SALT = 0x85A308D3
MAX_SHIFT = 8
IMAGE = 28
ROW = IMAGE * IMAGE
MAX_ROWS = (1 << 31) - 1   # the launcher's row counts are signed 32-bit


def check_augment_shift(s: int) -> None:
    """Refuse a shift that is no integer in 0..MAX_SHIFT; 0 switches the augmentation off."""
    if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s <= MAX_SHIFT:
        raise ValueError(f"--augment-shift must be an integer in 0..{MAX_SHIFT} (got {s})")


def half_bits(n: int) -> int:
    """Bits of one Feistel half for a domain of ``n`` rows."""
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(f"shuffle: the number of rows must be in 1..2^31 - 1 (got {n})")
    return (max(2, (n - 1).bit_length()) + 1) // 2


def round_keys(key: int) -> List[int]:
    return [mix_scalar((key + j * GOLDEN) & M32) for j in range(ROUNDS)]


def batch_key(seed: int, epoch: int, wrap: int, salt: int) -> int:
    """The 32-bit key of one (epoch, wrap) of the run with ``seed``; the same on every rank."""
    k = mix_scalar((seed + salt) & M32)
    k = mix_scalar((k + epoch * GOLDEN) & M32)
    return mix_scalar((k + wrap * GOLDEN) & M32)


def perm(i: int, n: int, key: int) -> int:
    """Where position ``i`` of ``[0, n)`` reads from under ``key``."""
    if not 0 <= i < n:
        raise ValueError(f"shuffle: position {i} outside [0, {n})")
    h = half_bits(n)
    mask = (1 << h) - 1
    ks = round_keys(key)
    x = i
    while True:
        left, right = x >> h, x & mask
        for k in ks:
            left, right = right, left ^ (mix_scalar(right ^ k) & mask)
        x = (left << h) | right
        if x < n:
            return x


def perm_indices(idx: torch.Tensor, n: int, key: int) -> torch.Tensor:
    """``perm`` of every element of the int64 tensor ``idx`` at once."""
    if idx.numel() and not (int(idx.min()) >= 0 and int(idx.max()) < n):
        raise ValueError(f"shuffle: positions outside [0, {n})")
    h = half_bits(n)
    mask = (1 << h) - 1
    ks = round_keys(key)
    x = idx.to(torch.int64).clone()
    todo = torch.ones_like(x, dtype=torch.bool)
    while bool(todo.any()):
        v = x[todo]
        left, right = v >> h, v & mask
        for k in ks:
            left, right = right, left ^ (_mix(right ^ k) & mask)
        x[todo] = (left << h) | right
        todo = x >= n
    return x


def permutation(n: int, key: int) -> torch.Tensor:
    """The whole order of one pass: element ``i`` is ``perm(i; n, key)``."""
    return perm_indices(torch.arange(n, dtype=torch.int64), n, key)


def shift_of(i: int, key_shift: int, s: int) -> Tuple[int, int]:
    """The ``(dx, dy)`` of the draw at position ``i`` (before permutation)."""
    if s == 0:
        return 0, 0
    h = mix_scalar((i ^ key_shift) & M32)
    m = 2 * s + 1
    return (h & 0xFFFF) % m - s, (h >> 16) % m - s


def source_rows(n: int, b: int, base: int, key: int, shuffle: bool) -> torch.Tensor:
    """The training rows of the batch of ``b`` at position ``base``."""
    if b < 1 or base < 0 or base + b > n:
        raise ValueError(f"shuffle: batch [{base}, {base + b}) outside the {n} rows")
    pos = torch.arange(base, base + b, dtype=torch.int64)
    return perm_indices(pos, n, key) if shuffle else pos


def shift_image_(out: torch.Tensor, img: torch.Tensor, dx: int, dy: int) -> None:
    """``out[r][c] = img[r - dy][c - dx]`` inside the image, else 0 (both [28, 28])."""
    out.zero_()
    r0, r1 = max(0, dy), IMAGE + min(0, dy)
    c0, c1 = max(0, dx), IMAGE + min(0, dx)
    out[r0:r1, c0:c1] = img[r0 - dy:r1 - dy, c0 - dx:c1 - dx]


def assemble_batch(x_train: torch.Tensor, y_train: torch.Tensor, xb: torch.Tensor,
                   yb: torch.Tensor, b: int, base: int, key: int, key_shift: int, s: int,
                   shuffle: bool) -> None:
    """Fill rows ``[0, b)`` of ``xb`` [>= b, 784] and of ``yb`` [>= b] from the CPU training set;
    rows from ``b`` on keep their contents."""
    check_augment_shift(s)
    n = x_train.shape[0]
    if x_train.shape[1:] != (ROW,) or y_train.shape != (n,) or xb.shape[1:] != (ROW,) or \
            xb.shape[0] < b or yb.shape[0] < b:
        raise ValueError("assemble_batch: shapes")
    rows = source_rows(n, b, base, key, shuffle)
    yb[:b] = y_train[rows]
    if s == 0:
        xb[:b] = x_train[rows]
        return
    for j in range(b):
        dx, dy = shift_of(base + j, key_shift, s)
        shift_image_(xb[j].view(IMAGE, IMAGE), x_train[int(rows[j])].view(IMAGE, IMAGE), dx, dy)


def batch_rule(seed: int, epoch: int, step: int, batch: int, total: int, rank: int = 0,
               world: int = 1, sharding: str = "replicate") -> Tuple[int, int, int]:
    """``(base, key, key_shift)`` of the micro-batch a worker trains on at ``step`` of ``epoch``.

    The raw batch number is ``utils/data.batch_indices``'s before its ``% nb``: ``step`` under
    ``replicate``, ``step * world + rank`` under ``stride``.  ``wrap = b_raw // nb`` goes into the
    keys beside the epoch, ``slot = b_raw % nb`` gives ``base = slot * batch``."""
    if sharding == "replicate":
        b_raw = step
    elif sharding == "stride":
        b_raw = step * world + rank
    else:
        raise ValueError(sharding)
    nb = total // batch
    wrap, slot = b_raw // nb, b_raw % nb
    return (slot * batch, batch_key(seed, epoch, wrap, PERM_SALT),
            batch_key(seed, epoch, wrap, SHIFT_SALT))
