"""Shared by tests/test_shuffle_cpu.py and tests/test_shuffle_gpu.py (helper module, not a
conftest): the ramp set on which any misplaced element shows, a batch written out element by
element from the scalar index rule, a shift key with a draw in a corner of its range, and a
dataset in the order a shuffled pass reads it.
"""
import numpy as np
import torch

from ddl_amd.ops import shuffle as S

ROW = 784
POISON = -7.0
LABEL_POISON = -5


def ramp_set(n):
    """x[i][p] = i * 784 + p (exact in float32 up to N = 20000), y[i] = 3 i + 1."""
    assert n <= 20000
    x = torch.arange(n * ROW, dtype=torch.float32).reshape(n, ROW)
    y = torch.arange(n, dtype=torch.int64) * 3 + 1
    return x, y


def expected_batch(n, b, base, key, key_shift, s, shuffle):
    """The batch of the ramp set by the scalar rule: (x [b,784], y [b], the draws (dx, dy))."""
    r, c = np.meshgrid(np.arange(28), np.arange(28), indexing="ij")
    xs, ys, draws = [], [], []
    for j in range(b):
        row = S.perm(base + j, n, key) if shuffle else base + j
        dx, dy = S.shift_of(base + j, key_shift, s)
        sr, sc = r - dy, c - dx
        inside = (sr >= 0) & (sr < 28) & (sc >= 0) & (sc < 28)
        img = np.where(inside, row * ROW + sr * 28 + sc, 0).astype(np.float32)
        xs.append(torch.from_numpy(img.reshape(ROW)))
        ys.append(row * 3 + 1)
        draws.append((dx, dy))
    return torch.stack(xs), torch.tensor(ys, dtype=torch.int64), draws


def corner_key(base, b, s, start=0):
    """A shift key under which some draw of the batch has |dx| = |dy| = s."""
    for k in range(start, start + 100000):
        if any(abs(dx) == s and abs(dy) == s
               for dx, dy in (S.shift_of(base + j, k, s) for j in range(b))):
            return k
    raise AssertionError("no corner draw found")


def poisoned(b, device="cpu"):
    """A destination two rows longer than the batch, poisoned."""
    return (torch.full((b + 2, ROW), POISON, device=device),
            torch.full((b + 2,), LABEL_POISON, dtype=torch.int64, device=device))


def keeps_poison(xb, yb, b):
    return bool((xb[b:] == POISON).all()) and bool((yb[b:] == LABEL_POISON).all())


def bases(n, b):
    """The first batch of the set, its last whole one and the one that ends on the last row."""
    return sorted({0, (n // b - 1) * b, n - b})


def pre_permuted(data, seed, epoch=0, wrap=0):
    """The set in the order the shuffled pass (epoch, wrap) of the run with `seed` reads it."""
    from ddl_amd.utils.data import Dataset
    order = S.permutation(data.total_batch, S.batch_key(seed, epoch, wrap, S.PERM_SALT))
    order = order.to(data.x_train.device)
    return Dataset(data.x_train[order].contiguous(), data.y_train[order].contiguous(),
                   data.x_test, data.y_test, data.source)
