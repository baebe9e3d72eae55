#!/usr/bin/env python3
"""What --shuffle and --augment-shift cost the W = 1 step: three configurations timed in
alternating rounds on one GPU, and the batch kernel's own duration.

  off            both flags off: a batch is a view of the resident set, no launch;
  shuffle        --shuffle: one assemble_batch launch per micro-batch (the 16-byte copy path);
  shuffle_shift  --shuffle --augment-shift 3: the same launch on the element-wise path.

Each round runs every configuration for --steps steps between device synchronisations (host
clock), in turn, so drift of the box hits all three alike; the figure per configuration is the
median over rounds, with the min and max beside it (the run-to-run spread to read a difference
against).  The kernel is timed with device events around `ops.assemble_batch` on the trainer's own
buffers, one call per event pair, on both paths, over batches spread through the set.  Prints one
JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--kernel-reps", type=int, default=200)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("shuffle_cost.py measures on a GPU; none found")
    from ddl_amd.config import TrainConfig
    from ddl_amd.ops import native
    from ddl_amd.ops import shuffle as S
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import get_dataset
    dev = torch.device("cuda", 0)
    data = get_dataset("synthetic", seed=1234)
    configs = {"off": dict(), "shuffle": dict(shuffle=True),
               "shuffle_shift": dict(shuffle=True, augment_shift=3)}
    trainers = {}
    for name, kw in configs.items():
        cfg = TrainConfig(mode="sync", shard="flat", batch_size=a.batch_size, eval_every=0,
                          engine="hip", quiet=True, **kw)
        trainers[name] = Trainer(cfg, DistEnv(0, 1, 0, dev), dataset=data)
    step = {n: 0 for n in trainers}

    def run(name, k):
        t = trainers[name]
        for _ in range(k):
            t.train_step(step[name] % t.steps)
            step[name] += 1

    for name in trainers:
        run(name, a.warmup)
    torch.cuda.synchronize()
    ms = {n: [] for n in trainers}
    for _ in range(a.rounds):
        for name in trainers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    launches = {n: int(t.exchange.runner.update_launches()) for n, t in trainers.items()}

    # the kernel alone, on the trainer's own set and batch buffers
    t = trainers["shuffle_shift"]
    ops = native.ops()
    x, y, B = t.data.x_train, t.data.y_train, a.batch_size
    nb = t.data.total_batch // B
    kern = {}
    for name, s in (("copy_path", 0), ("shift_path", 3)):
        us = []
        for i in range(a.kernel_reps + 10):
            base, key, ks = S.batch_rule(0, i, (i * 37) % nb, B, t.data.total_batch)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.assemble_batch(x, y, t.batch_x, t.batch_y, B, base, key, ks, s, True)
            e1.record()
            e1.synchronize()
            if i >= 10:
                us.append(1e3 * e0.elapsed_time(e1))
        kern[name] = dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us))
    res = dict(batch_size=B, steps=a.steps, rounds=a.rounds,
               ms_per_step={n: dict(median=statistics.median(v), min=min(v), max=max(v))
                            for n, v in ms.items()},
               update_launches=launches, kernels=kern,
               bytes_per_batch=2 * B * (x.shape[1] * 4 + 8))
    for tr in trainers.values():
        tr.exchange.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
