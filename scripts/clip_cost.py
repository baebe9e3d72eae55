#!/usr/bin/env python3
"""What --clip-norm costs the W = 1 step: three configurations timed in alternating rounds on
one GPU, and the two clip kernels' own durations.

  off    clip_norm = 0: the unclipped step (update tails riding in the backward launches);
  huge   clip_norm = 1e30: pays the lost placement (no tails: stand-alone update after the
         backward), the norm kernel and the scale kernel's early exit; changes no bit;
  tiny   clip_norm = 1e-3: the same plus the real scale pass.

Each round runs every configuration for --steps steps between device synchronisations (host
clock), in turn, so drift of the box hits all three alike; the figure per configuration is the
median over rounds, with the min and max beside it (the run-to-run spread to read a difference
against).  The kernels are timed with device events around `ops.clip_grads` on the trainer's own
gradient buffer, one call per event pair: norm + early exit (huge), norm + scale (tiny); the
scale pass alone is their difference.  Prints one JSON line.
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
        raise SystemExit("clip_cost.py measures on a GPU; none found")
    from ddl_amd.config import TrainConfig
    from ddl_amd.ops import native
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import get_dataset
    dev = torch.device("cuda", 0)
    data = get_dataset("synthetic", seed=1234)
    configs = {"off": 0.0, "huge": 1e30, "tiny": 1e-3}
    trainers = {}
    for name, c in configs.items():
        cfg = TrainConfig(mode="sync", shard="flat", batch_size=a.batch_size, eval_every=0,
                          engine="hip", quiet=True, clip_norm=c)
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

    # the kernels alone, on a gradient buffer of the real plan
    t = trainers["off"]
    ops = native.ops()
    g0 = t.grads.clone()
    g = g0.clone()
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    kern = {}
    for name, c in (("norm_and_early_exit", 1e30), ("norm_and_scale", 1e-3)):
        us = []
        for i in range(a.kernel_reps + 10):
            g.copy_(g0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.clip_grads(g, t.clip_ranges, c, out)
            e1.record()
            e1.synchronize()
            if i >= 10:
                us.append(1e3 * e0.elapsed_time(e1))
        kern[name] = dict(median_us=statistics.median(us), min_us=min(us))
    kern["scale_pass_us"] = (kern["norm_and_scale"]["median_us"]
                             - kern["norm_and_early_exit"]["median_us"])
    res = dict(batch_size=a.batch_size, steps=a.steps, rounds=a.rounds,
               ms_per_step={n: dict(median=statistics.median(v), min=min(v), max=max(v))
                            for n, v in ms.items()},
               update_launches=launches, kernels=kern,
               grad_norm={n: tr.last_grad_norm() for n, tr in trainers.items()},
               payload_floats=sum(n for _, n in t.clip_ranges))
    for tr in trainers.values():
        tr.exchange.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
