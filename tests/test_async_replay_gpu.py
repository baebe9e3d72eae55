"""The asynchronous PS over xGMI at W > 1, replayed in its recorded apply order: equal bits.

The path under test is the native asynchronous step (csrc/kernels/async_runner.hip: push tails,
the GPU pull gate) with the peer-memory data plane (csrc/kernels/xgmi_async.hip: the inbox, the
arrival board, the host service, the apply kernel).  Its ordering is hand-rolled — write-through
stores and flags instead of events, a one-wave gate in front of the next forward, the local-push
elision (the apply reads the worker's live gradient buffer), one inbox slot per (PS, worker)
reused every round, the step size from an atomically advanced t — and the run is not
deterministic.  It can be replayed, though (tests/async_replay.py): each host's service issues
its applies serially on one stream, an apply stores the PS state it has just produced into the
pushing worker's buffer and only there, and a worker's forward of step s + 1 waits for every
apply of its step s.  So the per-PS apply orders, which the service logs with
``check_provenance=True``, fix every bit.

W ranks share one card (gloo process group, as tests/test_xgmi_gpu.py); each saves its initial
parameters, its final buffer, every hosted PS's parameters, m, v and t, and the log.  This
process then replays the run on the GPU: gradients from ``HipEngine.forward_backward`` on the
worker's batch and dropout seed, updates from ``ops.update_flat`` on the PS range with the step
size of the PS's own t — the bits the apply kernel is pinned to by
tests/test_exchange_kernels_gpu.py.  Every worker buffer and every PS's parameters, m, v and t
must be BIT-equal; a mismatch is reported per worker and per PS range (first index, tensor,
max |diff|).

The control cell (W = 1, the service path instead of the in-line applies: a fixed order)
separates the two causes of a mismatch: if it fails the replay's premise is off (the runner's
gradient bits differ from forward_backward's); if it passes and a W > 1 cell fails, the data
plane has raced.

Batches 33 and 5 (the step audit's edge batches), 6 steps; the ranks pass a barrier before
their first step, so that their pushes do meet at the PS.  The skew cell sleeps rank 1 for
0.2 s before its steps 2 and 4, a margin over the few milliseconds the six steps take, and must
show a worker served twice while another is left behind (async_replay.staleness_exercised).
Each W > 1 cell also replays its run once more with two adjacent applies of different workers
swapped in one PS and requires a different result.

Measured on one MI355X: all 13 cells bit-equal on the first run, no kernel changed.  The file
takes 41 s inside the whole suite (46 s alone); a cell 2.7 - 3.6 s, nearly all of it the ranks'
start-up (import, HIP context, the IPC self-test), the replay itself under 0.1 s (0.4 s in the
first cell, which loads the code objects).  Slowest: 4-greedy-b5, 3.6 s (five GPU processes).
The skew cell recorded 120120202020201111 on all three PS: workers 0 and 2 done with their six
steps before worker 1's third.  A swapped pair moved the parameters by 7.6e-4 to 1.6e-3 with
Adam, 4.8e-6 with momentum and 7.4e-7 with SGD (max abs).  docs/DESIGN.md "Async W > 1
replayed in apply order" lists every cell's orders.
"""
import os
import sys
import time
import traceback

import pytest
import torch

import async_replay as ar
from conftest import ROOT, free_port

pytestmark = [pytest.mark.gpu, pytest.mark.slow]

STEPS = 6
SLEEP_S = 0.2
ADAM, MOMENTUM = 0, 1  # update.h UpdKind


def _rank(rank, world, port, outdir, kw):
    """One rank: the set-up of tests/test_xgmi_gpu.py::_async_rank, the steps driven one by one
    (the skew cell sleeps between them)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    kw = dict(kw)
    extra_env = kw.pop("_env", {})
    skew = kw.pop("_skew", ())
    kw.pop("_ps", None)
    batch = kw.pop("_batch")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), DDL_DIST_BACKEND="gloo",
                      DDL_XGMI_TIMEOUT_S="20")
    os.environ.update(extra_env)
    try:
        import torch.distributed as dist
        from ddl_amd.config import TrainConfig
        from ddl_amd.parallel.async_xgmi import AsyncPeerExchange
        from ddl_amd.parallel.comm import init_distributed
        from ddl_amd.parallel.roles import Trainer
        from ddl_amd.utils.data import synthetic_mnist
        env = init_distributed()
        assert env.device.index == 0
        cfg = TrainConfig(mode="async", steps=STEPS, batch_size=batch, eval_every=0,
                          engine="hip", quiet=True, data_sharding="stride",
                          exchange_backend="xgmi", check_provenance=True, watchdog_s=120.0, **kw)
        tr = Trainer(cfg, env, dataset=synthetic_mnist(2000, 500, seed=5))
        ex = tr.exchange
        assert isinstance(ex, AsyncPeerExchange), type(ex)
        want_native = extra_env.get("DDL_ASYNC_NATIVE", "1") == "1"
        assert (ex.runner is not None) == want_native, "native async step not taken"
        init = tr.params.clone()
        ex.steps = STEPS
        ex.start()
        if tr.servers:
            assert ex.service_mode == "host", ex.service_mode  # (the control: not in-line)
        if world > 1:  # the ranks start together: their pushes do meet at the PS
            torch.cuda.synchronize()
            dist.barrier()
        for i in range(STEPS):
            if rank == 1 and i in skew:
                time.sleep(SLEEP_S)
            tr.train_step(i)
        ex.join()
        ex.verify_provenance()
        torch.cuda.synchronize()
        assert ex.peer.error() == 0, ex.peer.error()
        P = tr.plan.num_ps
        torch.save({"init": init.cpu(), "params": tr.params.cpu(),
                    "ps": {p: dict(w=s.params.cpu(), m=s.m.cpu(),
                                   v=None if s.v is None else s.v.cpu(), t=s.t)
                           for p, s in tr.servers.items()},
                    "provenance": list(ex.provenance), "served": ex.served,
                    "ranges": [tr.plan.ps_segments(p)[0] for p in range(P)],
                    "hosts": [tr.plan.host_rank(p, world) for p in range(P)],
                    "offsets": list(tr.plan.tensor_offsets), "total": tr.plan.total,
                    "cfg": cfg.to_dict()},
                   os.path.join(outdir, f"rank{rank}.pt"))
        if world > 1:
            dist.barrier()
        ex.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


_DATA = []


def _data():
    """The ranks' dataset on the card: made once, read by every cell's replay."""
    if not _DATA:
        from ddl_amd.utils.data import synthetic_mnist
        _DATA.append(synthetic_mnist(2000, 500, seed=5).to(torch.device("cuda", 0)))
    return _DATA[0]


def _replay(recs, world, order):
    """The run again in this process, in the recorded order, with the engine's gradients and
    ops.update_flat."""
    import numpy as np
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.ops import native, rng
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    from ddl_amd.utils.data import batch_indices
    dev = torch.device("cuda", 0)
    cfg = recs[0]["cfg"]
    B = cfg["batch_size"]
    data = _data()
    params = torch.zeros(recs[0]["total"], device=dev)
    grads = torch.zeros_like(params)
    eng = HipEngine(params, grads, recs[0]["offsets"], batch=B, graph=False, eval_chunk=B)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    # the xGMI service holds lr and the betas as float32 and widens them for the step size
    # (update.h adam_step_size; tests/test_numerics_cpu.py pins that to adam_coeffs on the same
    # operands)
    h = AdamHyper(lr=f32(cfg["lr"]), beta1=f32(0.9), beta2=f32(0.999))
    opt = cfg["optimizer"]
    mu = {"adam": 0.0, "momentum": cfg["momentum"], "sgd": 0.0}[opt]

    def grad_fn(r, s, params_r):
        params.copy_(params_r)
        lo, hi = batch_indices(s, B, data.total_batch, r, world, cfg["data_sharding"])
        eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg["keep_prob"],
                             rng.step_seed(cfg["seed"], r, s))
        return grads.clone()

    def update_fn(p, st, g, t):
        if opt == "adam":
            native.ops().update_flat(ADAM, st.w, g, st.m, st.v, adam_coeffs(h, t), 0.9, 0.999,
                                     1e-8, 0.0, 1.0)
        else:
            native.ops().update_flat(MOMENTUM, st.w, g, st.m, None, f32(cfg["lr"]), 0.0, 0.0,
                                     0.0, mu, 1.0)

    out = ar.replay(order, recs[0]["ranges"], recs[0]["init"].to(dev), world, STEPS, grad_fn,
                    update_fn)
    torch.cuda.synchronize()
    return out


def _spans(ranges, offsets):
    """Every PS range cut at the tensor boundaries: (lo, hi, 'PS p / v7 (conv4 bias)')."""
    from ddl_amd.models.layout import TENSORS
    out = []
    for p, (lo, hi) in enumerate(ranges):
        for t in TENSORS:
            a, b = max(lo, offsets[t.index]), min(hi, offsets[t.index] + t.numel)
            if a < b:
                out.append((a, b, f"PS {p} / {t.name} ({t.layer} {t.kind})"))
    return out


def _b(n):
    return dict(_batch=n)


CELLS = [
    # the control: one worker, the service path (a fixed order)
    pytest.param(1, dict(shard="flat", _ps=3, **_b(33), _env=dict(DDL_ASYNC_INLINE="0")),
                 id="1-flat-control"),
    pytest.param(2, dict(shard="contiguous", **_b(33)), id="2-contiguous-b33"),
    pytest.param(2, dict(shard="contiguous", **_b(5)), id="2-contiguous-b5"),
    pytest.param(3, dict(shard="contiguous", num_ps=5, **_b(33)), id="3-contiguous-5ps"),
    pytest.param(4, dict(shard="greedy", num_ps=4, **_b(5)), id="4-greedy-b5"),
    pytest.param(2, dict(shard="flat", _ps=4, **_b(33)), id="2-flat"),
    pytest.param(3, dict(shard="greedy", _skew=(2, 4), **_b(33)), id="3-greedy-skew"),
    pytest.param(2, dict(shard="contiguous", **_b(33), _env=dict(DDL_ASYNC_ELIDE_LOCAL="0")),
                 id="2-no-elide"),
    pytest.param(2, dict(shard="contiguous", **_b(33), _env=dict(DDL_ASYNC_GATE="0")),
                 id="2-no-gate"),
    pytest.param(2, dict(shard="contiguous", **_b(33), _env=dict(DDL_ASYNC_TAIL="0")),
                 id="2-no-tail"),
    pytest.param(2, dict(shard="greedy", **_b(33), _env=dict(DDL_ASYNC_NATIVE="0")),
                 id="2-python-push-pull"),
    pytest.param(2, dict(shard="contiguous", optimizer="momentum", **_b(33)), id="2-momentum"),
    pytest.param(2, dict(shard="contiguous", optimizer="sgd", **_b(33)), id="2-sgd"),
]


@pytest.mark.parametrize("world,kw", CELLS)
def test_async_xgmi_run_equals_its_replay(tmp_path, world, kw):
    import torch.multiprocessing as mp
    t_start = time.perf_counter()
    mp.spawn(_rank, args=(world, free_port(), str(tmp_path), kw), nprocs=world, join=True)
    t_run = time.perf_counter() - t_start
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    hosts, ranges, offsets = recs[0]["hosts"], recs[0]["ranges"], recs[0]["offsets"]
    num_ps = len(hosts)
    assert num_ps == kw.get("_ps", kw.get("num_ps", world))
    for rec in recs[1:]:
        assert torch.equal(rec["init"], recs[0]["init"])
        assert rec["ranges"] == ranges and rec["offsets"] == offsets
    log = [e for rec in recs for e in rec["provenance"]]
    assert len(log) == num_ps * world * STEPS  # the xGMI service logs every apply
    order = ar.apply_orders(log, world, STEPS)
    orders = {p: ar.order_string(o) for p, o in order.items()}
    if kw.get("_skew"):
        assert ar.staleness_exercised(order, STEPS), f"staleness not exercised: {orders}"
    params, state = _replay(recs, world, order)
    print(f"cell: run {t_run:.1f} s, replay {time.perf_counter() - t_start - t_run:.1f} s; "
          f"orders {orders}")
    fails = []
    spans = _spans(ranges, offsets)
    for r in range(world):
        got = recs[r]["params"]
        lines = ar.mismatch_report(f"worker {r}", got, params[r].cpu(), spans)
        if not lines and not torch.equal(got, params[r].cpu()):
            lines = [f"worker {r}: differs outside every tensor (alignment padding)"]
        fails += lines
    for p in range(num_ps):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        lo = ranges[p][0]
        inner = [(a - lo, b - lo, label) for (a, b, label) in spans if label.startswith(f"PS {p} ")]
        if got["t"] != t:
            fails.append(f"PS {p}: t {got['t']}, replay {t}")
        for name, a, b in (("params", got["w"], w), ("m", got["m"], m), ("v", got["v"], v)):
            if a is None:
                assert name == "v" and kw.get("optimizer") in ("momentum", "sgd")
                continue
            lines = ar.mismatch_report(f"PS {p} {name}", a, b.cpu(), inner)
            if not lines and not torch.equal(a, b.cpu()):
                lines = [f"PS {p} {name}: differs in the alignment padding"]
            fails += lines
    assert not fails, f"orders {orders}\n" + "\n".join(fails[:40])
    # the comparison is sharp on this very run: one pair of adjacent applies swapped moves it
    for p, i, sw in ar.adjacent_swaps(order):
        try:
            other, _ = _replay(recs, world, sw)
        except ar.ReplayError:
            continue
        moved = max(float((a - b).abs().max()) for a, b in zip(other, params))
        print(f"cell: PS {p}, applies {i} and {i + 1} swapped: max |diff| {moved:.1e}")
        assert moved > 0.0
        break
    else:
        assert world == 1, "no realisable swap in the recorded orders"
