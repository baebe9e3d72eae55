"""One config dataclass + argparse for every entry point.

The reference hard-codes everything: ``epoch = 1``, ``batch_size = 100``
(``mnist_sync/worker.py:41-42``), Adam lr 1e-4 (``mnist_sync/model/model.py:93``),
keep_prob 0.5 (``mnist_sync/worker.py:30``), eval every 10 steps (``:71``), PS/worker
counts from ``sys.argv[2]`` (``-np N``, ``mnist_sync_sharding/parameter_server.py:95``).
Those are the defaults here; ``-np`` is accepted for command-line compatibility.
"""
from __future__ import annotations

import argparse
from dataclasses import dataclass, field, asdict
from typing import Optional

from . import VARIANTS


@dataclass
class TrainConfig:
    mode: str = "sync"              # sync | async | single
    shard: str = "contiguous"       # none | contiguous | greedy | lpt | flat
    num_ps: Optional[int] = None    # default: one PS per worker process (sharded), 1 for 'none'
    epochs: int = 1
    batch_size: int = 100
    steps: Optional[int] = None     # steps per epoch (default total_batch // (batch_size *
                                    # accum_steps) = 500)
    lr: float = 1e-4
    optimizer: str = "adam"         # adam | momentum | sgd
    momentum: float = 0.9
    weight_decay: float = 0.0       # decoupled (AdamW / SGDW): w -= lr * wd * w before each update
    nesterov: bool = False          # momentum only: step along mu * m' + g
    clip_norm: float = 0.0          # clip each worker's gradient to this global norm; 0 = off
    accum_steps: int = 1            # micro-batches of batch_size per step (one update); 1 = off
    shuffle: bool = False           # a fresh order of the training set every pass (ops/shuffle.py)
    augment_shift: int = 0          # translate each training image by up to this many pixels; 0 = off
    keep_prob: float = 0.5
    eval_every: int = 10            # 0 disables periodic eval
    data: str = "synthetic"
    data_sharding: str = "replicate"  # replicate (reference) | stride
    grad_reduce: str = "sum"        # sum (reference PS sums) | mean
    ref_quirks: bool = False        # reproduce SURVEY.md §2.10 Q1/Q2/Q4
    seed: int = 0
    engine: str = "auto"            # auto | hip | torch
    graph: bool = False             # replay the compute step as HIP graphs (eager is faster)
    overlap: bool = True            # bucketed grad push overlapped with backward
    native_exchange: bool = True    # sync step in the C++ SyncRunner (HIP engine on GPU)
    force_collectives: bool = False  # W = 1: native runner keeps RS/reduce units on a 1-rank comm
    # W > 1 data plane of the native sync runner: rccl (reduce-scatter / all-gather or reduce /
    # broadcast) or xgmi (flat plan: one fused push / owner-Adam / pull kernel per bucket over
    # IPC-mapped peer memory, csrc/kernels/xgmi.hip); auto = rccl
    exchange_backend: str = "auto"
    dist_eval: bool = True          # sync, W > 1: each rank scores 1/W of the test set
    eval_async: bool = False        # HIP engine: periodic eval on a side stream from a snapshot
    check_provenance: bool = False  # async: verify every applied push
    log_jsonl: Optional[str] = None
    checkpoint_dir: Optional[str] = None
    checkpoint_every: int = 0
    resume: bool = False            # continue from checkpoint_dir at its global step
    max_steps: Optional[int] = None  # stop after this many global steps (a preempted run)
    target_acc: Optional[float] = None
    quiet: bool = False
    watchdog_s: float = 600.0

    def __post_init__(self):
        check_optimizer_options(self.optimizer, self.momentum, self.weight_decay, self.nesterov)
        check_clip_norm(self.clip_norm)
        check_accum_steps(self.accum_steps)
        check_augment_shift(self.augment_shift)

    def to_dict(self):
        return asdict(self)


def check_optimizer_options(optimizer: str, momentum: float, weight_decay: float,
                            nesterov: bool) -> None:
    """Refuse the combinations no update rule implements."""
    if weight_decay < 0.0:
        raise ValueError(f"--weight-decay must not be negative (got {weight_decay})")
    if nesterov and optimizer != "momentum":
        raise ValueError(f"--nesterov needs --optimizer momentum (got '{optimizer}')")
    if nesterov and not momentum > 0.0:
        raise ValueError(f"--nesterov needs a momentum above 0 (got --momentum {momentum})")


def check_clip_norm(clip_norm: float) -> None:
    """Refuse a clip norm that is negative (or not a number); 0 switches clipping off."""
    if not clip_norm >= 0.0:
        raise ValueError(f"--clip-norm must not be negative (got {clip_norm})")


def check_accum_steps(accum_steps: int) -> None:
    """Refuse a micro-batch count below 1 (or not an integer); 1 switches accumulation off."""
    from .ops.accum import check_accum_steps as check
    check(accum_steps)


def check_augment_shift(augment_shift: int) -> None:
    """Refuse a shift that is no integer in 0..8; 0 switches the augmentation off."""
    from .ops.shuffle import check_augment_shift as check
    check(augment_shift)


def add_args(p: argparse.ArgumentParser, mode_default: str = "sync") -> argparse.ArgumentParser:
    d = TrainConfig()
    p.add_argument("-np", dest="np_compat", type=int, default=None,
                   help="reference compatibility: number of PS (parameter_server.py) or "
                        "workers (worker.py)")
    p.add_argument("--variant", choices=sorted(VARIANTS), default=None,
                   help="preset mode/shard named after the reference directories")
    p.add_argument("--mode", default=mode_default, choices=["sync", "async", "single"])
    p.add_argument("--shard", default=d.shard,
                   choices=["none", "contiguous", "greedy", "lpt", "flat"])
    p.add_argument("--num-ps", type=int, default=None)
    p.add_argument("--epochs", type=int, default=d.epochs)
    p.add_argument("--batch-size", type=int, default=d.batch_size)
    p.add_argument("--steps", type=int, default=None)
    p.add_argument("--lr", type=float, default=d.lr)
    p.add_argument("--optimizer", default=d.optimizer, choices=["adam", "momentum", "sgd"])
    p.add_argument("--momentum", type=float, default=d.momentum,
                   help="mu of --optimizer momentum")
    p.add_argument("--weight-decay", type=float, default=d.weight_decay,
                   help="decoupled weight decay (AdamW / SGDW): every parameter loses "
                        "lr * wd of itself ahead of each update; 0 = off")
    p.add_argument("--nesterov", action="store_true",
                   help="Nesterov momentum (with --optimizer momentum and --momentum > 0)")
    p.add_argument("--clip-norm", type=float, default=d.clip_norm,
                   help="clip each worker's mini-batch gradient to this global norm before it is "
                        "scaled, pushed, reduced or applied (tf.clip_by_global_norm on the "
                        "worker); the step then runs without backward/exchange overlap; 0 = off")
    p.add_argument("--accum-steps", type=int, default=d.accum_steps,
                   help="micro-batches of --batch-size images per step: each worker sums their "
                        "gradients on the device and pushes, reduces or applies only their mean "
                        "(an effective batch of K * B per worker, one update and one exchange "
                        "per K backward passes); steps, --eval-every, --checkpoint-every and "
                        "--max-steps stay in updates; K > 1 runs without backward/exchange "
                        "overlap; 1 = off")
    p.add_argument("--shuffle", action="store_true",
                   help="read every pass over the training set in a fresh pseudo-random order, "
                        "without replacement: a function of --seed, the epoch and the position, "
                        "the same on every rank and after --resume, evaluated on the device")
    p.add_argument("--augment-shift", type=int, default=d.augment_shift,
                   help="translate every training image by a per-draw (dx, dy), each uniform in "
                        "[-S, S] pixels, zero-filled (training stream only, never eval); "
                        "0..8, 0 = off")
    p.add_argument("--keep-prob", type=float, default=d.keep_prob)
    p.add_argument("--eval-every", type=int, default=d.eval_every)
    p.add_argument("--data", default=d.data)
    p.add_argument("--data-sharding", default=d.data_sharding, choices=["replicate", "stride"])
    p.add_argument("--grad-reduce", default=d.grad_reduce, choices=["sum", "mean"])
    p.add_argument("--ref-quirks", action="store_true")
    p.add_argument("--seed", type=int, default=d.seed)
    p.add_argument("--engine", default=d.engine, choices=["auto", "hip", "torch"])
    p.add_argument("--graph", action="store_true", help="replay the engine step as HIP graphs")
    p.add_argument("--no-graph", action="store_true", help="(default)")
    p.add_argument("--check-provenance", action="store_true",
                   help="async: checksum every push and verify order/provenance at the PS")
    p.add_argument("--no-dist-eval", action="store_true",
                   help="every worker scores the full test set (reference behaviour)")
    p.add_argument("--eval-async", action="store_true",
                   help="HIP engine: run the periodic test-set eval on a side stream from a "
                        "parameter snapshot, overlapped with training (same accuracies)")
    p.add_argument("--no-native-exchange", action="store_true",
                   help="drive the sync exchange from Python instead of the C++ SyncRunner")
    p.add_argument("--no-overlap", action="store_true")
    p.add_argument("--exchange", dest="exchange_backend", default=d.exchange_backend,
                   choices=["auto", "rccl", "xgmi"],
                   help="W > 1 sync data plane of the native runner: RCCL collectives or the "
                        "fused xGMI peer-memory exchange (flat plan)")
    p.add_argument("--log-jsonl", default=None)
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--checkpoint-every", type=int, default=0)
    p.add_argument("--resume", action="store_true",
                   help="continue from --checkpoint-dir: same data index, eval cadence and "
                        "dropout seeds as an uninterrupted run")
    p.add_argument("--max-steps", type=int, default=None,
                   help="stop after this many global steps (checkpointed if --checkpoint-dir)")
    p.add_argument("--target-acc", type=float, default=None)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--watchdog-s", type=float, default=d.watchdog_s)
    return p


def from_args(a: argparse.Namespace) -> TrainConfig:
    mode, shard = a.mode, a.shard
    if a.variant:
        mode, shard = VARIANTS[a.variant]["mode"], VARIANTS[a.variant]["shard"]
    return TrainConfig(
        mode=mode, shard=shard, num_ps=a.num_ps, epochs=a.epochs, batch_size=a.batch_size,
        steps=a.steps, lr=a.lr, optimizer=a.optimizer, momentum=a.momentum,
        weight_decay=a.weight_decay, nesterov=a.nesterov, clip_norm=a.clip_norm,
        accum_steps=a.accum_steps, shuffle=a.shuffle, augment_shift=a.augment_shift,
        keep_prob=a.keep_prob,
        eval_every=a.eval_every, data=a.data, data_sharding=a.data_sharding,
        grad_reduce=a.grad_reduce, ref_quirks=a.ref_quirks, seed=a.seed, engine=a.engine,
        graph=a.graph and not a.no_graph, native_exchange=not a.no_native_exchange,
        dist_eval=not a.no_dist_eval, eval_async=a.eval_async,
        check_provenance=a.check_provenance, overlap=not a.no_overlap, log_jsonl=a.log_jsonl,
        exchange_backend=a.exchange_backend,
        checkpoint_dir=a.checkpoint_dir, checkpoint_every=a.checkpoint_every,
        resume=a.resume, max_steps=a.max_steps, target_acc=a.target_acc, quiet=a.quiet, watchdog_s=a.watchdog_s)
