"""Eval inputs whose predictions are known (helper module, not a conftest).

With glorot-sized weights, bias noise of 0.05 and ``torch.rand`` images the bias noise decides the
argmax: the model predicts one class for every row, and a count over such rows cannot tell a
correct eval forward from one that returns zeros or mixes rows up
(tests/test_eval_reference_cpu.py test_old_setups_predict_one_class).  ``eval_case`` fits the last
layer instead, so that row r's prediction is a target T[r] drawn for that row:

1. P = make_real_params(), x = torch.rand(n, 784), T = randperm(n) % 10;
2. h2 = the eval forward (no dropout) up to fc2, in fp64;
3. W3 = lstsq(h2 - mean, onehot(T) - 0.1), an exact fit while n < 512, b3 = -(mean @ W3);
4. W3 and b3 go into P[12] and P[13] as fp32.

The fp64 logits of row r are then 0.9 at T[r] and -0.1 elsewhere, up to the fp32 rounding of W3 and
b3.  A second target vector T_B with its own W3 / b3 on the same h2 gives a second parameter set
that differs from the first in fc3 alone.  Everything here comes from torch on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import torch
import torch.nn.functional as F

from ddl_amd.models.mnist_cnn import torch_forward
from oracle_common import make_real_params

N_ROWS = 168
SEED = 21
ROW_BITS = 8   # bits of a row index below 256
GAP_FACTOR = 1024.0


@dataclass
class EvalCase:
    P: List[torch.Tensor]        # the 14 fp32 parameter tensors, fc3 fitted to T
    P_B: List[torch.Tensor]      # the same with fc3 fitted to T_B
    x: torch.Tensor              # [n, 784] fp32 images
    T: torch.Tensor              # [n] int64: the class every row is fitted to
    T_B: torch.Tensor
    logits64: torch.Tensor       # [n, 10] fp64 logits of P
    logits64_B: torch.Tensor

    @property
    def n(self) -> int:
        return self.x.shape[0]


def features64(P, x):
    """h2 of the eval forward in fp64: torch_forward with fc3 replaced by the identity."""
    p = [t.double() for t in P[:12]] + [torch.eye(512, dtype=torch.float64),
                                        torch.zeros(512, dtype=torch.float64)]
    return torch_forward(p, x.double(), 1.0, 0)


def fit_fc3(h2, T):
    """fp32 (W3, b3) with h2 @ W3 + b3 = onehot(T) - 0.1 (exact in fp64 while rows < 512)."""
    mean = h2.mean(0)
    target = F.one_hot(T, 10).double() - 0.1
    w3 = torch.linalg.lstsq(h2 - mean, target).solution
    return w3.float(), (-(mean @ w3)).float()


def logits64(P, x):
    return torch_forward([t.double() for t in P], x.double(), 1.0, 0)


def logits32(P, x):
    """The fp32 CPU forward: the yardstick for what fp32 rounding does to the logits."""
    return torch_forward(list(P), x, 1.0, 0)


_CACHE = {}


def eval_case(n: int = N_ROWS, seed: int = SEED) -> EvalCase:
    """The case of the module docstring, computed once per (n, seed) and shared: treat it as
    read-only."""
    if (n, seed) in _CACHE:
        return _CACHE[(n, seed)]
    assert n < 512
    g = torch.Generator().manual_seed(seed)
    P = make_real_params()
    x = torch.rand(n, 784, generator=g)
    T = torch.randperm(n, generator=g) % 10
    T_B = torch.randperm(n, generator=g) % 10
    h2 = features64(P, x)
    sets = []
    for t in (T, T_B):
        w3, b3 = fit_fc3(h2, t)
        sets.append([p.clone() for p in P[:12]] + [w3, b3])
    case = EvalCase(sets[0], sets[1], x, T, T_B, logits64(sets[0], x), logits64(sets[1], x))
    _CACHE[(n, seed)] = case
    return case


def top_two_gap(lg):
    top = lg.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


# ---- reading per-row predictions out of a count ------------------------------------------------
def label_sets(T, gen_seed: int = 33):
    """The label vectors of the row-by-row audit as (name, y, expected count): a count is all an
    eval returns, so each vector asks it one question about the predictions.  `T` is the
    prediction every row must have."""
    n = T.shape[0]
    sets = [("y=T", T.clone(), n), ("y=T+1", (T + 1) % 10, 0)]
    for c in range(10):
        sets.append((f"y={c}", torch.full((n,), c, dtype=torch.int64), int((T == c).sum())))
    sets += bit_sets(T)
    y = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(gen_seed))
    sets.append(("y=random", y, int((T == y).sum())))
    return sets


def bit_sets(T):
    """For each bit k of the row index: y = T where bit k is set (then where it is clear),
    (T + 1) % 10 elsewhere; the count is the number of such rows."""
    n = T.shape[0]
    assert n <= 1 << ROW_BITS
    wrong = (T + 1) % 10
    rows = torch.arange(n)
    sets = []
    for k in range(ROW_BITS):
        for val in (1, 0):
            sel = ((rows >> k) & 1) == val
            sets.append((f"bit{k}={val}", torch.where(sel, T, wrong), int(sel.sum())))
    return sets


def read_failures(count_fn, sets, n):
    """Run `count_fn(y) -> int` on every label set; returns the failure messages.  When bit sets
    fail, the message names the rows they single out: a row r whose prediction is wrong (and is
    not (T[r] + 1) % 10 either) lowers exactly the sets `bit k = (bit k of r)`."""
    fails, low = [], {}
    for name, y, want in sets:
        got = int(count_fn(y))
        if got != want:
            fails.append(f"{name}: count {got}, expected {want}")
            if name.startswith("bit"):
                k, val = name[3:].split("=")
                low[(int(k), int(val))] = got < want
    if low:
        rows = [r for r in range(n)
                if all(low.get((k, (r >> k) & 1), False) for k in range(ROW_BITS))]
        failing = sorted({(k, v) for (k, v) in low})
        fails.append(f"failing bit sets {failing} single out rows {rows}" if rows else
                     f"failing bit sets {failing}: more than one row is wrong")
    return fails


def host_counter(pred):
    """count_fn of a prediction vector held on the host: what a correct counter returns."""
    return lambda y: int((pred == y).sum())
