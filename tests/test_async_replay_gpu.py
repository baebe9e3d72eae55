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
import time

import pytest
import torch

import async_replay as ar
import onecard as oc
from conftest import free_port

pytestmark = [pytest.mark.gpu, pytest.mark.slow]

STEPS = 6
SLEEP_S = 0.2


def _rank(rank, world, port, outdir, kw):
    """One rank, its steps driven one by one (the skew cell sleeps between them)."""
    kw = dict(kw)
    extra_env = kw.pop("_env", {})
    skew = kw.pop("_skew", ())
    kw.pop("_ps", None)
    batch = kw.pop("_batch")
    with oc.rank_session(rank, world, port, env=extra_env, on_device_0=True) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "async", STEPS, batch, synthetic_mnist(2000, 500, seed=5),
                             **kw)
        ex = tr.exchange
        want_native = extra_env.get("DDL_ASYNC_NATIVE", "1") == "1"
        assert (ex.runner is not None) == want_native, "native async step not taken"

        def started(ex):
            if tr.servers:
                assert ex.service_mode == "host", ex.service_mode  # (the control: not in-line)

        def maybe_sleep(i):
            if rank == 1 and i in skew:
                time.sleep(SLEEP_S)

        rec = oc.async_rank_record(tr, world, STEPS, before_step=maybe_sleep, after_start=started)
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        me.close_single(ex)


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
    t_start = time.perf_counter()
    oc.run_ranks(_rank, world, free_port(), str(tmp_path), kw, limit_s=oc.LIMIT_S)
    t_run = time.perf_counter() - t_start
    recs = oc.load_ranks(tmp_path, world)
    hosts, ranges, offsets = recs[0]["hosts"], recs[0]["ranges"], recs[0]["offsets"]
    assert len(hosts) == kw.get("_ps", kw.get("num_ps", world))
    for rec in recs[1:]:
        assert torch.equal(rec["init"], recs[0]["init"])
        assert rec["ranges"] == ranges and rec["offsets"] == offsets
    _, order = oc.recorded_orders(recs, world, STEPS)
    orders = {p: ar.order_string(o) for p, o in order.items()}
    if kw.get("_skew"):
        assert ar.staleness_exercised(order, STEPS), f"staleness not exercised: {orders}"
    params, state = oc.replay_async(recs, world, order, STEPS)
    print(f"cell: run {t_run:.1f} s, replay {time.perf_counter() - t_start - t_run:.1f} s; "
          f"orders {orders}")
    fails = oc.replay_mismatches(recs, world, params, state, _spans(ranges, offsets))
    assert not fails, f"orders {orders}\n" + "\n".join(fails[:40])
    # the comparison is sharp on this very run: one pair of adjacent applies swapped moves it
    for p, i, sw in ar.adjacent_swaps(order):
        try:
            other, _ = oc.replay_async(recs, world, sw, STEPS)
        except ar.ReplayError:
            continue
        moved = max(float((a - b).abs().max()) for a, b in zip(other, params))
        print(f"cell: PS {p}, applies {i} and {i + 1} swapped: max |diff| {moved:.1e}")
        assert moved > 0.0
        break
    else:
        assert world == 1, "no realisable swap in the recorded orders"
