#!/usr/bin/env python3
"""Step time of the W = 1 native runner with the optimizer tail (csrc/kernels/tail.h) off and
in several placements / block sizes, interleaved rounds in one process.

--optimizer takes one or more of adam / momentum / sgd: each gets a trainer of its own, and
every round visits every (optimizer, variant) pair in turn, so optimizers are compared under
the same conditions as tail variants.  --variants default keeps the comparison to the tail
off and the runner's default placement.

--weight-decay WD and --nesterov add, beside every optimizer's plain trainer, one with the
options on (adam+wd; momentum+nesterov+wd: Nesterov goes to the momentum trainers only), visited
in the same rounds: the cost of the update rule's modifiers (csrc/kernels/update.h).

usage: python scripts/tail_probe.py [--steps 300] [--rounds 3] [--optimizer momentum]
       python scripts/tail_probe.py --optimizer adam momentum sgd --variants default
       python scripts/tail_probe.py --optimizer adam momentum --variants default \
              --weight-decay 0.1 --nesterov
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shard", default="flat")
    ap.add_argument("--optimizer", nargs="+", default=["adam"],
                    choices=["adam", "momentum", "sgd"])
    ap.add_argument("--variants", default="sweep", choices=["sweep", "default"],
                    help="sweep: off + both placements x 4 block sizes; default: off + the "
                         "runner's default tail")
    ap.add_argument("--weight-decay", type=float, default=0.0,
                    help="also time every optimizer with this decoupled weight decay")
    ap.add_argument("--nesterov", action="store_true",
                    help="also time momentum with Nesterov's look-ahead (with --weight-decay: "
                         "both on one trainer)")
    a = ap.parse_args()
    import torch
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist

    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    data = synthetic_mnist()
    trainers = {}
    for opt in dict.fromkeys(a.optimizer):
        mods = [{}]
        on = dict(weight_decay=a.weight_decay) if a.weight_decay else {}
        if a.nesterov and opt == "momentum":
            on["nesterov"] = True
        if on:
            mods.append(on)
        for kw in mods:
            cfg = TrainConfig(mode="sync", shard=a.shard, steps=10 ** 6, batch_size=100,
                              eval_every=0, engine="hip", quiet=True, data_sharding="stride",
                              optimizer=opt, **kw)
            name = opt + ("+nesterov" if kw.get("nesterov") else "") + ("+wd" if "weight_decay" in kw else "")
            trainers[name] = Trainer(cfg, env, dataset=data)
    if a.variants == "default":
        variants = [("off", None), ("tail", ())]
    else:
        variants = [("off", None)] + [(f"{'first' if f else 'last'}-f4x{n}", (f, n))
                                      for f in (1, 0) for n in (512, 1024, 2048, 4096)]
    res = {(o, k): [] for o in trainers for k, _ in variants}
    launches = {}
    step = 0
    for _ in range(a.rounds):
        for name, v in variants:
            for opt, tr in trainers.items():
                run = tr.exchange.runner
                if v is None:
                    run.set_use_tail(False)
                else:
                    run.set_use_tail(True)
                    if v:
                        run.set_tail_cfg(*v)
                for _ in range(20):
                    tr.train_step(step)
                    step += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.train_step(step)
                    step += 1
                torch.cuda.synchronize()
                res[opt, name].append(1e6 * (time.perf_counter() - t0) / a.steps)
                launches[opt, name] = run.update_launches()
    for (opt, name), ts in res.items():
        print(f"{opt:21s}{name:16s} us/step min {min(ts):7.1f}  spread {max(ts) - min(ts):5.1f}  "
              f"all {' '.join(f'{t:.1f}' for t in ts)}  update launches/step "
              f"{launches[opt, name]}")


if __name__ == "__main__":
    main()
