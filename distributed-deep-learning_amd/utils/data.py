"""MNIST data: the reference pickle, an npz file, or a learnable synthetic stand-in.

Reference loader (``mnist_sync/model/model.py:7-14``): unpickles ``data/mnist.pkl`` as
``(train, valid, test)``, keeps train (50k) and test (10k), one-hot encodes labels with
pandas, never shuffles, and every worker walks the *same* batches
(``mnist_sync/worker.py:27-28``).

MI355X-first: the whole dataset (157 MB train + 31 MB test in fp32) is copied to HBM
once and stays resident; a batch is a view, so there is no per-step host->device copy
and no loader thread in the hot loop.  With ``--shuffle`` or ``--augment-shift`` one kernel
assembles the batch from the resident set instead (``ops/shuffle.py``), still without a copy
from the host.

There is no network in this environment, so unless a data file is supplied we use a
*synthetic* MNIST-shaped set: 10 smooth random class prototypes, each sample a randomly
shifted prototype plus noise.  It is learnable, so accuracy and time-to-accuracy are
meaningful, and it has exactly the reference shapes.
"""
from __future__ import annotations

import gzip
import os
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..models.layout import INPUT_DIM, NUM_CLASSES, IMAGE

TRAIN_SIZE = 50000
TEST_SIZE = 10000


@dataclass
class Dataset:
    x_train: torch.Tensor   # [N,784] f32
    y_train: torch.Tensor   # [N] int64
    x_test: torch.Tensor
    y_test: torch.Tensor
    source: str = "synthetic"

    def to(self, device) -> "Dataset":
        return Dataset(self.x_train.to(device), self.y_train.to(device),
                       self.x_test.to(device), self.y_test.to(device), self.source)

    @property
    def total_batch(self) -> int:
        # The reference ships "total_batch": x_train.shape[0] in its metadata dict
        # (mnist_sync/worker.py:50).
        return self.x_train.shape[0]

    def one_hot_train(self) -> torch.Tensor:
        return F.one_hot(self.y_train, NUM_CLASSES).float()


def synthetic_mnist(n_train: int = TRAIN_SIZE, n_test: int = TEST_SIZE,
                    seed: int = 1234, noise: float = 0.45, mix: float = 0.25) -> Dataset:
    """Difficulty tuned so the reference recipe (Adam 1e-4, batch 100) learns it on an
    MNIST-like curve: ~0.5 accuracy after 50 steps, ~0.97 after 200 (gaussian pixel
    noise ``noise``, distractor-class blend ``mix``, +-3 px shifts)."""
    g = torch.Generator().manual_seed(seed)
    # Smooth prototypes: low-res random field upsampled, thresholded into strokes.
    low = torch.rand(NUM_CLASSES, 1, 7, 7, generator=g)
    proto = F.interpolate(low, size=(IMAGE, IMAGE), mode="bicubic", align_corners=False)
    proto = (proto - proto.mean(dim=(2, 3), keepdim=True)) * 3.0
    proto = proto.clamp(0.0, 1.0)  # [10,1,28,28]

    shift = 3

    def make(n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        y = torch.randint(0, NUM_CLASSES, (n,), generator=g)
        other = torch.randint(0, NUM_CLASSES, (n,), generator=g)
        # own class prototype blended with a random distractor class
        img = proto[y, 0] * (1.0 - mix) + proto[other, 0] * mix  # [n,28,28]
        # random translation by up to +-3 px via roll (cheap, deterministic)
        sx = torch.randint(-shift, shift + 1, (n,), generator=g)
        sy = torch.randint(-shift, shift + 1, (n,), generator=g)
        out = torch.empty(n, IMAGE, IMAGE)
        for dx in range(-shift, shift + 1):
            for dy in range(-shift, shift + 1):
                sel = (sx == dx) & (sy == dy)
                if sel.any():
                    out[sel] = torch.roll(img[sel], shifts=(dy, dx), dims=(1, 2))
        out = out + noise * torch.randn(n, IMAGE, IMAGE, generator=g)
        return out.clamp(0.0, 1.0).reshape(n, INPUT_DIM).contiguous(), y

    xtr, ytr = make(n_train)
    xte, yte = make(n_test)
    return Dataset(xtr, ytr, xte, yte, "synthetic")


# The "hard" synthetic set: the default set is separable enough that the
# reference recipe ends its epoch at ~0.998 and crosses 95 % after ~0.14 s, so it cannot show
# what async staleness or the replicate protocol cost in convergence.  Here every class has
# several writing STYLES (independent prototypes), samples blend two styles of their class with a
# distractor of another class, translate by up to +-4 px, get a random contrast and heavier pixel
# noise — intra-class variety and inter-class confusion instead of one template per class.
# Calibrated on MI355X (scripts/tta_calibrate.py, profiles/r6_tta_calibration*.txt) so the
# reference recipe (one epoch: 500 steps of batch 100, Adam 1e-4, keep 0.5) ends near MNIST's
# ~0.97-0.98: two styles per class at the default set's noise / mix / shift end the epoch at
# 0.980 (0.53 / 0.83 / 0.93 / 0.96 after 100 / 200 / 300 / 400 steps; 95 % after ~0.28 s),
# against 0.998 for the default set; four styles, more noise or a random contrast did not
# learn within the epoch (0.10-0.37).
HARD = dict(styles=2, noise=0.45, mix=0.25, shift=3, contrast=0.0)


def synthetic_mnist_hard(n_train: int = TRAIN_SIZE, n_test: int = TEST_SIZE, seed: int = 4321,
                         styles: int = HARD["styles"], noise: float = HARD["noise"],
                         mix: float = HARD["mix"], shift: int = HARD["shift"],
                         contrast: float = HARD["contrast"]) -> Dataset:
    """MNIST-shaped set on which the reference recipe converges like MNIST (see HARD)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(NUM_CLASSES * styles, 1, 7, 7, generator=g)
    proto = F.interpolate(low, size=(IMAGE, IMAGE), mode="bicubic", align_corners=False)
    proto = ((proto - proto.mean(dim=(2, 3), keepdim=True)) * 3.0).clamp(0.0, 1.0)
    proto = proto.reshape(NUM_CLASSES, styles, IMAGE, IMAGE)

    def make(n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        y = torch.randint(0, NUM_CLASSES, (n,), generator=g)
        s1 = torch.randint(0, styles, (n,), generator=g)
        s2 = torch.randint(0, styles, (n,), generator=g)
        a = torch.rand(n, 1, 1, generator=g)
        own = proto[y, s1] * a + proto[y, s2] * (1.0 - a)  # a point between two styles
        other = torch.randint(1, NUM_CLASSES, (n,), generator=g)
        other = (y + other) % NUM_CLASSES                   # a different class
        so = torch.randint(0, styles, (n,), generator=g)
        img = own * (1.0 - mix) + proto[other, so] * mix
        gain = 1.0 - contrast * torch.rand(n, 1, 1, generator=g)
        img = img * gain
        sx = torch.randint(-shift, shift + 1, (n,), generator=g)
        sy = torch.randint(-shift, shift + 1, (n,), generator=g)
        out = torch.empty(n, IMAGE, IMAGE)
        for dx in range(-shift, shift + 1):
            for dy in range(-shift, shift + 1):
                sel = (sx == dx) & (sy == dy)
                if sel.any():
                    out[sel] = torch.roll(img[sel], shifts=(dy, dx), dims=(1, 2))
        out = out + noise * torch.randn(n, IMAGE, IMAGE, generator=g)
        return out.clamp(0.0, 1.0).reshape(n, INPUT_DIM).contiguous(), y

    xtr, ytr = make(n_train)
    xte, yte = make(n_test)
    return Dataset(xtr, ytr, xte, yte, "synthetic-hard")


# The only globals a pickle of numpy arrays needs (numpy 1.x and 2.x module paths): the array
# reconstructor, the ndarray / dtype types and the buffer constructor of newer protocols, plus
# _codecs.encode, which protocol-2 pickles written by python 3 use to rebuild a bytes object
# (it only encodes a string).
_NUMPY_GLOBALS = {
    ("_codecs", "encode"),
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy", "ndarray"), ("numpy", "dtype"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
}


class _ArrayOnlyUnpickler:
    """``pickle.Unpickler`` that reconstructs numpy arrays, tuples, lists and scalars and
    refuses every other global: a crafted ``mnist.pkl`` cannot run code (the reference
    unpickles without restriction, ``mnist_sync/model/model.py:8-9``)."""

    def __new__(cls, f):
        import pickle

        class _U(pickle.Unpickler):
            def find_class(self, module, name):
                if (module, name) in _NUMPY_GLOBALS:
                    return super().find_class(module, name)
                raise pickle.UnpicklingError(
                    f"refusing global {module}.{name} in a dataset pickle (numpy arrays only)")
        return _U(f, encoding="latin1")


def load_pickle_arrays(f):
    """Unpickle a dataset file that may hold only numpy arrays (tuples / lists of them)."""
    return _ArrayOnlyUnpickler(f).load()


def load_file(path: str) -> Dataset:
    """Load ``.npz`` (x_train, y_train, x_test, y_test) or the reference ``mnist.pkl[.gz]``.

    The pickle format is read only from a user-supplied path (the reference tree ships no
    data) and only through an unpickler that admits numpy arrays (load_pickle_arrays)."""
    if path.endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        xtr, ytr, xte, yte = d["x_train"], d["y_train"], d["x_test"], d["y_test"]
    else:
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rb") as f:
            (xtr, ytr), _, (xte, yte) = load_pickle_arrays(f)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt)  # noqa: E731
    return Dataset(t(xtr, torch.float32).reshape(-1, INPUT_DIM), t(ytr, torch.int64),
                   t(xte, torch.float32).reshape(-1, INPUT_DIM), t(yte, torch.int64),
                   os.path.basename(path))


def get_dataset(spec: str = "synthetic", seed: int = 1234) -> Dataset:
    if spec in ("synthetic", "", None):
        return synthetic_mnist(seed=seed)
    if spec == "synthetic-hard":
        return synthetic_mnist_hard()
    if spec.startswith("synthetic:"):
        n = int(spec.split(":", 1)[1])
        return synthetic_mnist(n_train=n, n_test=max(n // 5, 100), seed=seed)
    return load_file(spec)


def batch_indices(step: int, batch: int, total: int, rank: int = 0, world: int = 1,
                  sharding: str = "replicate") -> Tuple[int, int]:
    """[start, end) of the batch a worker trains on at ``step``.

    ``replicate`` reproduces the reference (every worker the same slice,
    ``mnist_sync/worker.py:27-28``); ``stride`` gives worker w batch ``step*W + w``."""
    if sharding == "replicate":
        b = step
    elif sharding == "stride":
        b = step * world + rank
    else:
        raise ValueError(sharding)
    nb = total // batch
    b %= nb
    return b * batch, (b + 1) * batch
