#!/usr/bin/env python3
"""What --accum-steps costs per micro-batch: K = 1, 2, 4, 8 on three step paths of one GPU,
against a baseline tree's K = 1 step on the same box, and the accumulate kernel's own time.

  w1      sync, W = 1: the native runner, every update local;
  xgmi    sync, W = 1 with --force-collectives --exchange xgmi: the W > 1 step structure (comm
          stream, hand-offs, fused bucket kernels) on one card;
  async   async, W = 1 with --exchange xgmi: the native async runner, in-line applies.

Method: one worker process per tree and round, the trees alternating (--baseline-tree: a built
checkout of the commit to compare against, e.g. the parent; it runs K = 1 only), so drift of
the box hits both alike.  Inside a worker every (path, K) trainer in turn, one alive at a time,
is warmed up and timed in --windows windows of --steps steps, each between two device events
(the last one synchronised).  A step of K micro-batches counts K: the figure is ms per
micro-batch, the median over all windows of all rounds, with the min and max beside it.

The kernel: `rocprofv3 --kernel-trace --stats` around a worker of its own (--kernel-reps calls of
every mode on a gradient buffer of the real plan, nothing else on the device), read back from
the stats CSV.  Bytes per call: the payload read from g, read from A unless it is the first pass,
and written once.  Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {
    "w1": dict(mode="sync", shard="flat"),
    "xgmi": dict(mode="sync", shard="flat", force_collectives=True, exchange_backend="xgmi"),
    "async": dict(mode="async", shard="flat", num_ps=3, exchange_backend="xgmi"),
}


# ---- worker: one tree, every (path, K) ---------------------------------------------------------
def worker(a) -> dict:
    sys.path.insert(0, a.tree)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_probe.py measures on a GPU; none found")
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import get_dataset
    dev = torch.device("cuda", 0)
    data = get_dataset("synthetic", seed=1234)
    res = {}
    for path in a.paths:
        ms = {}
        for k in a.ks:
            kw = dict(PATHS[path])
            if k > 1:  # (a baseline tree from before the option takes K = 1 only)
                kw["accum_steps"] = k
            cfg = TrainConfig(batch_size=a.batch_size, eval_every=0, engine="hip", quiet=True,
                              **kw)
            # one trainer alive at a time: every native exchange owns streams, and a process's
            # streams share its few hardware queues (four live xGMI rehearsals in one process
            # tripled the K = 1 step)
            tr = Trainer(cfg, DistEnv(0, 1, 0, dev), dataset=data)
            if cfg.mode == "async":
                tr.exchange.steps = 1 << 30
                tr.exchange.start()
            n = 0

            def run(steps):
                nonlocal n
                for _ in range(steps):
                    tr.train_step(n % tr.steps)
                    n += 1

            run(a.warmup)
            torch.cuda.synchronize()
            ms[k] = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(a.steps)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / (a.steps * k))
            torch.cuda.synchronize()
            if cfg.mode == "async":
                tr.exchange.join()
            tr.exchange.close()
            del tr
        res[path] = {str(k): v for k, v in ms.items()}
    return res


def kernel_worker(a) -> dict:
    """Every mode of the accumulate kernel, alone on the device (run under rocprofv3)."""
    sys.path.insert(0, a.tree)
    import torch
    from ddl_amd.ops import clip as C
    from ddl_amd.ops import native
    from ddl_amd.parallel.sharding import make_plan
    dev = torch.device("cuda", 0)
    plan = make_plan("none", 1)
    ranges = C.payload_ranges(plan.tensor_offsets)
    g = torch.randn(plan.total, device=dev)
    acc = torch.zeros_like(g)
    ops = native.ops()
    for _ in range(a.kernel_reps):
        for mode in (0, 1, 2):
            ops.accum_grads(g, acc, ranges, mode, 4)
    torch.cuda.synchronize()
    return dict(payload_floats=sum(n for _, n in ranges), buffer_floats=plan.total)


# ---- driver ----------------------------------------------------------------------------------------
def spawn_worker(a, tree, ks, extra=(), pre=()):
    cmd = [*pre, sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree,
           "--ks", ",".join(map(str, ks)), "--paths", ",".join(a.paths),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--windows", str(a.windows),
           "--batch-size", str(a.batch_size), "--kernel-reps", str(a.kernel_reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker failed with status {r.returncode}: no further GPU work")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def summarise(samples):
    return dict(median=statistics.median(samples), min=min(samples), max=max(samples),
                windows=len(samples))


def kernel_stats(a) -> dict:
    out = tempfile.mkdtemp(prefix="accum_prof_", dir=a.prof_dir)
    pre = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "-o", "prof", "--"]
    info = spawn_worker(a, a.tree, [1], extra=["--kernel"], pre=pre)
    rows = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("Kernel_Name") or ""
                if "grad_accum_kernel" in name:
                    rows[name] = row
    payload = 4 * info["payload_floats"]
    passes = {"first": ("<0>", 2), "add": ("<1>", 3), "finish": ("<2>", 3)}
    res = dict(info, rows=len(rows))
    for label, (tag, streams) in passes.items():
        hit = [r for n, r in rows.items() if tag in n or f"Li{tag[1]}E" in n]
        if not hit:
            continue
        r = hit[0]
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
        res[label] = dict(calls=int(float(r.get("Calls", 0))), avg_us=avg_ns / 1e3,
                          min_us=float(r.get("MinNs", 0.0)) / 1e3,
                          bytes=streams * payload,
                          gb_per_s=(streams * payload / avg_ns) if avg_ns else None)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3, help="windows per (path, K) and worker")
    ap.add_argument("--rounds", type=int, default=2, help="workers per tree, alternating")
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--paths", default="w1,xgmi,async")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--tree", default=HERE, help="the tree under test (built)")
    ap.add_argument("--baseline-tree", default=None,
                    help="a built checkout of the commit to compare against (K = 1 only)")
    ap.add_argument("--no-kernel", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--prof-dir", default=None, help="where rocprofv3 writes (default: TMPDIR)")
    ap.add_argument("--worker-timeout", type=float, default=420.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kernel", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    a.ks = [int(k) for k in a.ks.split(",")]
    a.paths = [p for p in a.paths.split(",") if p]
    for p in a.paths:
        if p not in PATHS:
            raise SystemExit(f"unknown path '{p}' (one of {sorted(PATHS)})")
    if a.worker:
        print(json.dumps(kernel_worker(a) if a.kernel else worker(a)))
        return None
    trees = [("this", a.tree, a.ks)]
    if a.baseline_tree:
        trees.insert(0, ("baseline", os.path.abspath(a.baseline_tree), [1]))
    samples = {name: {} for name, _, _ in trees}
    for _ in range(a.rounds):
        for name, tree, ks in trees:
            got = spawn_worker(a, tree, ks)
            for path, by_k in got.items():
                for k, v in by_k.items():
                    samples[name].setdefault(path, {}).setdefault(k, []).extend(v)
    res = dict(batch_size=a.batch_size, steps=a.steps, rounds=a.rounds, windows=a.windows,
               ms_per_micro_batch={name: {path: {k: summarise(v) for k, v in by_k.items()}
                                          for path, by_k in by_path.items()}
                                   for name, by_path in samples.items()})
    if not a.no_kernel:
        res["kernel"] = kernel_stats(a)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return res


if __name__ == "__main__":
    main()
