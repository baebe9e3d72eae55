"""The asynchronous PS replayed in its recorded apply order (tests/async_replay.py), on the CPU.

Two halves.

HARNESS: the replay against a seeded random scheduler that obeys the run's three rules (serial
applies per PS, the shard back to the pusher only, one round of staleness) and computes its own
result as it goes; the replay of the scheduler's recorded orders must give exactly that.  With
it: the check is sharp (two adjacent applies of different workers swapped change the result),
orders that no run can produce are refused, and W = 1 is the plain sequential loop.

GLOO RUNS: W real processes of the Python ``AsyncExchange`` (parallel/comm.py) with the torch
engine, batch 10, 5 steps.  Every worker's final buffer and every PS's parameters, m, v and t
must be BIT-equal to the replay of the orders the services logged.  The update inside the replay
is written out here (the TF1 forms, three lines), not taken from ``ParameterServer``: that class
is under test.  The replay runs torch with one thread, as the ranks do (dist_helpers._setup):
the CPU convolutions of a multi-threaded torch differ from the ranks' by ~6e-7.

The ranks pass a barrier before their first step, so that their pushes do meet at the PS.  Each
cell also replays its run once more with two adjacent applies of different workers swapped in
one PS and requires a different result (the check is sharp on the recorded run itself).

Measured orders (the workers' digits in apply order, one string per PS) of one CPU run, with
the largest parameter change of the swapped replay; a run's orders are its own, and the test
replays whatever was recorded:

    2-contiguous          PS0 0101010101       PS1 0101010101                        1.1e-3
    3-greedy              021021021021021 on all three PS                            1.4e-3
    3-contiguous-2ps      PS0 201210210210201  PS1 210210210210210                   1.4e-3
    2-contiguous-5ps      0101010101 on PS0..3, PS4 0101010011                       6.3e-4
    2-none                PS0 0101010101                                             1.2e-3
    2-momentum            PS0 0110101010       PS1 1010101010                        9.5e-6
    2-sgd                 PS0 0110101010       PS1 1010101010                        1.6e-6
    3-greedy-skew         010202020121211 on all three PS                            1.4e-3
                          (rank 1 sleeps 0.3 s before its steps 1 and 3: workers 0 and 2 are
                          served three times each between two pushes of worker 1; another
                          run gave 020120202012111)

The skew cell must show that: some PS serves one worker at least twice in a row while another
worker still has pushes outstanding, "in a row" read relative to the worker left behind
(async_replay.staleness_exercised: with three workers the third one's applies fall in between,
as in the orders above, which never serve a worker twice back to back before the tail).
"""
import os
import random
import time
import traceback

import pytest
import torch

import async_replay as ar
from conftest import free_port
from dist_helpers import _setup, spawn

B1, B2, EPS, LR, MU = 0.9, 0.999, 1e-8, 1e-4, 0.9


# ---- the update rules, written out (fp32, the forms of parallel/ps.py ParameterServer.apply) ------
def adam_step_size(t, lr=LR):
    import math
    return lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


def update_adam(p, st, g, t, lr=LR):
    st.m.add_((g - st.m) * (1.0 - B1))
    st.v.add_((g * g - st.v) * (1.0 - B2))
    st.w.sub_(adam_step_size(t, lr) * st.m / (st.v.sqrt() + EPS))


def update_momentum(p, st, g, t, lr=LR):
    st.m.mul_(MU).add_(g, alpha=1.0)
    st.w.sub_(lr * st.m)


def update_sgd(p, st, g, t, lr=LR):
    st.w.sub_(g, alpha=lr)


UPDATES = {"adam": update_adam, "momentum": update_momentum, "sgd": update_sgd}


# ---- harness ---------------------------------------------------------------------------------------
N = 37


def synth_grad(r, s, params):
    """Cheap and nonlinear in the parameters, different per worker and step."""
    return (torch.sin(params * (1.0 + r)) + 0.5 * params * torch.roll(params, 1)
            + 0.1 * (s + 1) * torch.cos(params * 3.0 + r))


def synth_setup(seed, world, num_ps):
    gen = torch.Generator().manual_seed(seed)
    init = torch.rand(N, generator=gen) * 2.0 - 1.0
    rnd = random.Random(seed)
    cuts = sorted(rnd.sample(range(1, N), num_ps - 1))
    ranges = list(zip([0] + cuts, cuts + [N]))
    return init, ranges


# big steps, so that one apply moves the parameters far beyond rounding
HARNESS_LR = 0.05


def harness_update(kind):
    fn = UPDATES[kind]
    return lambda p, st, g, t: fn(p, st, g, t, lr=HARNESS_LR)


def random_run(seed, world, num_ps, steps, kind):
    """A random scheduler under the run's rules, computing the run itself as it schedules: at
    every tick one enabled event, drawn uniformly — a worker computing its next gradient (every
    PS has applied its previous step) or a PS applying one of the pushes waiting at it (ANY
    waiting worker: the ANY_SOURCE order).  Returns the per-PS orders and its own result."""
    init, ranges = synth_setup(seed, world, num_ps)
    upd = harness_update(kind)
    rnd = random.Random(seed * 7919 + 1)
    params = [init.clone() for _ in range(world)]
    state = [ar.PSState(init[lo:hi].clone()) for lo, hi in ranges]
    applied = [[0] * world for _ in range(num_ps)]
    grad, grad_step = [None] * world, [-1] * world
    order = {p: [] for p in range(num_ps)}
    while True:
        events = []
        for r in range(world):
            s = grad_step[r] + 1
            if s < steps and all(applied[p][r] >= s for p in range(num_ps)):
                events.append(("grad", r))
        for p in range(num_ps):
            for w in range(world):
                if grad_step[w] >= 0 and applied[p][w] == grad_step[w]:
                    events.append(("apply", p, w))
        if not events:
            break
        ev = rnd.choice(events)
        if ev[0] == "grad":
            r = ev[1]
            grad_step[r] += 1
            grad[r] = synth_grad(r, grad_step[r], params[r])
        else:
            _, p, w = ev
            lo, hi = ranges[p]
            st = state[p]
            st.t += 1
            upd(p, st, grad[w][lo:hi], st.t)
            params[w][lo:hi] = st.w
            order[p].append((w, grad_step[w]))
            applied[p][w] += 1
    assert all(len(o) == world * steps for o in order.values())
    return init, ranges, order, params, state


def same_result(res, params, state):
    got_params, got_state = res
    if not all(torch.equal(a, b) for a, b in zip(got_params, params)):
        return False
    for p, st in enumerate(state):
        w, m, v, t = got_state[p]
        if not (torch.equal(w, st.w) and torch.equal(m, st.m) and torch.equal(v, st.v)
                and t == st.t):
            return False
    return True


DRAWS = [(seed, world, 1 + (seed * 3 + world) % 5, 2 + seed % 3, ("adam", "momentum")[seed % 2])
         for world in (1, 2, 3, 4) for seed in range(15)]


def test_draws_cover_the_plan_sizes():
    assert len(DRAWS) >= 50
    for world in (1, 2, 3, 4):
        assert {d[2] for d in DRAWS if d[1] == world} == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_replay_reproduces_random_schedules(world):
    out_of_step = 0
    for seed, w, num_ps, steps, kind in [d for d in DRAWS if d[1] == world]:
        init, ranges, order, params, state = random_run(seed, w, num_ps, steps, kind)
        res = ar.replay(order, ranges, init, w, steps, synth_grad, harness_update(kind))
        assert same_result(res, params, state), (seed, w, num_ps, steps, kind, order)
        # and through the log: what the services record gives the same orders back
        recs = [(wk, p, s, t + 1) for p, od in order.items() for t, (wk, s) in enumerate(od)]
        random.Random(seed).shuffle(recs)
        assert ar.apply_orders(recs, w, steps) == order
        out_of_step += ar.staleness_exercised(order, steps)
    if world > 1:  # the scheduler does leave lock-step (else the draws would test little)
        assert out_of_step >= 5, out_of_step


def test_partial_log_is_completed_with_the_hosts_own_pushes():
    """The Python AsyncExchange logs remote pushes only: the missing t are the host's, in step
    order."""
    for seed, w, num_ps, steps, kind in [d for d in DRAWS if d[1] > 1][::4]:
        _, _, order, _, _ = random_run(seed, w, num_ps, steps, kind)
        hosts = [p % w for p in range(num_ps)]
        recs = [(wk, p, s, t + 1) for p, od in order.items() for t, (wk, s) in enumerate(od)
                if wk != hosts[p]]
        assert ar.apply_orders(recs, w, steps, hosts=hosts) == order
        with pytest.raises(ar.ReplayError, match="PS 0"):   # no host named: cannot complete
            ar.apply_orders(recs, w, steps)


def realisable_swaps(order, ranges, init, world, steps, upd):
    """Every order that differs from `order` by one swap of two adjacent applies of DIFFERENT
    workers in one PS and is still realisable, with its replay."""
    out = []
    for p, i, sw in ar.adjacent_swaps(order):
        try:
            out.append((p, i, ar.replay(sw, ranges, init, world, steps, synth_grad, upd)))
        except ar.ReplayError:
            pass
    return out


@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_swapping_two_adjacent_applies_changes_the_result(kind):
    # the smallest case, by hand: one PS, two workers, both orders of round 0 are runs
    init, ranges = synth_setup(3, 2, 1)
    upd = harness_update(kind)
    a = ar.replay({0: [(0, 0), (1, 0), (0, 1), (1, 1)]}, ranges, init, 2, 2, synth_grad, upd)
    b = ar.replay({0: [(1, 0), (0, 0), (0, 1), (1, 1)]}, ranges, init, 2, 2, synth_grad, upd)
    assert not torch.equal(a[0][0], b[0][0]) or not torch.equal(a[0][1], b[0][1])
    # and every realisable swap of drawn schedules
    n = 0
    for seed, w, num_ps, steps, k in [d for d in DRAWS if d[1] > 1 and d[4] == kind][:12]:
        init, ranges, order, params, state = random_run(seed, w, num_ps, steps, k)
        for p, i, res in realisable_swaps(order, ranges, init, w, steps, upd):
            n += 1
            assert not same_result(res, params, state), (seed, p, i)
    assert n >= 20, n


def test_unrealisable_orders_raise():
    init, ranges = synth_setup(5, 2, 2)
    upd = harness_update("adam")
    # PS 0 wants worker 0's step 1 before worker 1's step 0, PS 1 the other way round: worker
    # 0's step 1 needs PS 1 to apply its step 0, which is queued behind worker 1's step 1, which
    # needs PS 0 to apply worker 1's step 0, which is queued behind worker 0's step 1
    order = {0: [(0, 0), (0, 1), (1, 0), (1, 1)], 1: [(1, 0), (1, 1), (0, 0), (0, 1)]}
    with pytest.raises(ar.ReplayError, match=r"PS 0: stopped at entry 1 = \(worker 0, step 1\)"):
        ar.replay(order, ranges, init, 2, 2, synth_grad, upd)
    # the same orders pass the log's checks: each PS alone looks fine
    recs = [(w, p, s, t + 1) for p, od in order.items() for t, (w, s) in enumerate(od)]
    assert ar.apply_orders(recs, 2, 2) == order
    # a worker's step 1 before its step 0 at one PS
    bad = {0: [(0, 1), (0, 0), (1, 0), (1, 1)], 1: [(0, 0), (1, 0), (0, 1), (1, 1)]}
    with pytest.raises(ar.ReplayError, match="PS 0: entry 0"):
        ar.replay(bad, ranges, init, 2, 2, synth_grad, upd)
    # a worker two rounds ahead of a PS (its step 2 needs PS 1 to have applied its step 1)
    ahead = {0: [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)],
             1: [(0, 0), (1, 0), (1, 1), (1, 2), (0, 1), (0, 2)]}
    with pytest.raises(ar.ReplayError, match=r"PS 0: stopped at entry 2 = \(worker 0, step 2\)"):
        ar.replay(ahead, ranges, init, 2, 3, synth_grad, upd)
    # an order of the wrong length
    with pytest.raises(ar.ReplayError, match="PS 1: 3 applies"):
        ar.replay({0: order[0], 1: order[1][:3]}, ranges, init, 2, 2, synth_grad, upd)


def test_bad_logs_are_refused():
    order = {0: [(0, 0), (1, 0), (0, 1), (1, 1)], 1: [(1, 0), (0, 0), (1, 1), (0, 1)]}
    recs = [(w, p, s, t + 1) for p, od in order.items() for t, (w, s) in enumerate(od)]
    assert ar.apply_orders(recs, 2, 2) == order
    assert ar.apply_orders([(w, p, s, t + 10) for (w, p, s, t) in recs], 2, 2, t0=10) == order
    # duplicate t
    dup = [r for r in recs if r[:2] != (1, 1) or r[2] != 1] + [(1, 1, 1, 2)]
    with pytest.raises(ar.ReplayError, match="PS 1: t = 2 logged twice"):
        ar.apply_orders(dup, 2, 2)
    # an entry lost, from a log that logs every apply (the host's too)
    with pytest.raises(ar.ReplayError, match="PS 1: no apply logged for t = .3."):
        ar.apply_orders([r for r in recs if r != (1, 1, 1, 3)], 2, 2, hosts=[0, 1])
    with pytest.raises(ar.ReplayError, match="PS 1: no apply logged"):
        ar.apply_orders([r for r in recs if r != (1, 1, 1, 3)], 2, 2)
    # a remote-only log that lost a remote entry as well: three missing, the host pushes two
    remote = [r for r in recs if r[0] != r[1]]
    assert ar.apply_orders(remote, 2, 2, hosts=[0, 1]) == order
    with pytest.raises(ar.ReplayError, match="PS 0: no apply logged"):
        ar.apply_orders(remote[1:], 2, 2, hosts=[0, 1])
    # t outside the run
    with pytest.raises(ar.ReplayError, match="PS 0: t = 5 outside"):
        ar.apply_orders([r if r != (1, 0, 1, 4) else (1, 0, 1, 5) for r in recs], 2, 2)
    # steps of one (worker, ps) out of order, or repeated
    swapped = [(w, p, 1 - s if (w, p) == (0, 1) else s, t) for (w, p, s, t) in recs]
    with pytest.raises(ar.ReplayError, match=r"PS 1: worker 0's steps are applied as \[1, 0\]"):
        ar.apply_orders(swapped, 2, 2)
    twice = [(w, p, 0 if (w, p) == (1, 0) else s, t) for (w, p, s, t) in recs]
    with pytest.raises(ar.ReplayError, match=r"PS 0: worker 1's steps are applied as \[0, 0\]"):
        ar.apply_orders(twice, 2, 2)
    # a PS the plan does not have
    with pytest.raises(ar.ReplayError, match="PS 2"):
        ar.apply_orders(recs + [(0, 2, 0, 1)], 2, 2, hosts=[0, 1])


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_one_worker_is_the_sequential_loop(kind):
    steps, num_ps = 4, 3
    init, ranges = synth_setup(11, 1, num_ps)
    upd = harness_update(kind)
    order = ar.apply_orders([(0, p, s, s + 1) for p in range(num_ps) for s in range(steps)], 1,
                            steps)
    (got,), state = ar.replay(order, ranges, init, 1, steps, synth_grad, upd)
    w = init.clone()
    m, v = torch.zeros(N), torch.zeros(N)
    for s in range(steps):
        g = synth_grad(0, s, w)
        if kind == "adam":
            m.add_((g - m) * (1.0 - B1))
            v.add_((g * g - v) * (1.0 - B2))
            w.sub_(adam_step_size(s + 1, HARNESS_LR) * m / (v.sqrt() + EPS))
        elif kind == "momentum":
            m.mul_(MU).add_(g, alpha=1.0)
            w.sub_(HARNESS_LR * m)
        else:
            w.sub_(g, alpha=HARNESS_LR)
    assert torch.equal(got, w)
    for p, (lo, hi) in enumerate(ranges):
        sw, sm, sv, st = state[p]
        assert torch.equal(sw, w[lo:hi]) and torch.equal(sm, m[lo:hi]) and st == steps
        assert torch.equal(sv, v[lo:hi])


def test_staleness_exercised_reads_the_order():
    lockstep = [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert not ar.staleness_exercised({0: lockstep}, 2)
    # worker 1 twice in a row while worker 0's step 1 is still to come
    assert ar.staleness_exercised({0: lockstep, 1: [(0, 0), (1, 0), (1, 1), (0, 1)]}, 2)
    assert ar.staleness_exercised({0: [(0, 0), (0, 1), (1, 0), (1, 1)]}, 2)
    # three workers: "in a row" is relative to the worker left behind
    def od(digits):
        seen = {}
        return [(int(c), seen.setdefault(c, []).append(0) or len(seen[c]) - 1) for c in digits]
    assert not ar.staleness_exercised({0: od("012012012")}, 3)
    assert ar.staleness_exercised({0: od("021020202012111")}, 5)  # 0 and 2 ahead of 1
    assert ar.staleness_exercised({0: od("012012012"), 1: od("012020121")}, 3)
    assert ar.order_string(od("0210")) == "0210" and od("0210")[3] == (0, 1)


# ---- gloo runs ---------------------------------------------------------------------------------------
STEPS, BATCH, SLEEP_S = 5, 10, 0.3


def _gloo_rank(rank, world, port, outdir, kw, skew):
    """One rank, driven as tests/test_xgmi_gpu.py::_rank drives train_step (not Trainer.train:
    the skew cell sleeps between steps)."""
    _setup(rank, world, port)
    try:
        import torch.distributed as dist
        from ddl_amd.config import TrainConfig
        from ddl_amd.parallel.comm import AsyncExchange, init_distributed
        from ddl_amd.parallel.roles import Trainer
        from ddl_amd.utils.data import synthetic_mnist
        env = init_distributed(device="cpu")
        cfg = TrainConfig(mode="async", steps=STEPS, batch_size=BATCH, eval_every=0, quiet=True,
                          engine="torch", data="synthetic", check_provenance=True,
                          watchdog_s=120.0, **kw)
        tr = Trainer(cfg, env, dataset=synthetic_mnist(600, 200, seed=7))
        ex = tr.exchange
        assert type(ex) is AsyncExchange, type(ex)
        init = tr.params.clone()
        ex.steps = STEPS
        ex.start()
        dist.barrier()  # the ranks start together: their pushes do meet at the PS
        for i in range(STEPS):
            if rank == 1 and i in skew:
                time.sleep(SLEEP_S)
            tr.train_step(i)
        ex.join()
        ex.verify_provenance()
        torch.save({"init": init, "params": tr.params.clone(),
                    "ps": {p: dict(w=s.params.clone(), m=s.m.clone(),
                                   v=None if s.v is None else s.v.clone(), t=s.t)
                           for p, s in tr.servers.items()},
                    "provenance": list(ex.provenance), "served": ex.served,
                    "ranges": [tr.plan.ps_segments(p)[0] for p in range(tr.plan.num_ps)],
                    "hosts": [tr.plan.host_rank(p, world) for p in range(tr.plan.num_ps)],
                    "offsets": list(tr.plan.tensor_offsets), "total": tr.plan.total,
                    "cfg": cfg.to_dict()},
                   os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        ex.close()
        dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


def replay_gloo(recs, world, order):
    """The replay of a gloo run, in this process: TorchEngine gradients on each worker's own
    batch and dropout seed, the update written out above."""
    from ddl_amd.models.mnist_cnn import TorchEngine
    from ddl_amd.ops import rng
    from ddl_amd.utils.data import batch_indices, synthetic_mnist
    cfg = recs[0]["cfg"]
    data = synthetic_mnist(600, 200, seed=7)
    params = torch.zeros(recs[0]["total"])
    grads = torch.zeros_like(params)
    eng = TorchEngine(params, grads, recs[0]["offsets"], BATCH)

    def grad_fn(r, s, params_r):
        params.copy_(params_r)
        lo, hi = batch_indices(s, BATCH, data.total_batch, r, world, cfg["data_sharding"])
        eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg["keep_prob"],
                             rng.step_seed(cfg["seed"], r, s))
        return grads.clone()

    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as the ranks (dist_helpers._setup)
    try:
        return ar.replay(order, recs[0]["ranges"], recs[0]["init"], world, STEPS, grad_fn,
                         UPDATES[cfg["optimizer"]])
    finally:
        torch.set_num_threads(threads)


GLOO_CELLS = [
    pytest.param(2, dict(shard="contiguous"), (), id="2-contiguous"),
    pytest.param(3, dict(shard="greedy"), (), id="3-greedy"),
    pytest.param(3, dict(shard="contiguous", num_ps=2), (), id="3-contiguous-2ps"),
    pytest.param(2, dict(shard="contiguous", num_ps=5), (), id="2-contiguous-5ps"),
    pytest.param(2, dict(shard="none"), (), id="2-none"),
    pytest.param(2, dict(shard="contiguous", optimizer="momentum"), (), id="2-momentum"),
    pytest.param(2, dict(shard="contiguous", optimizer="sgd"), (), id="2-sgd"),
    pytest.param(3, dict(shard="greedy"), (1, 3), id="3-greedy-skew"),
]


@pytest.mark.slow
@pytest.mark.parametrize("world,kw,skew", GLOO_CELLS)
def test_gloo_run_equals_its_replay(tmp_path, world, kw, skew):
    spawn(_gloo_rank, world, free_port(), str(tmp_path), kw, skew)
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    num_ps = len(hosts)
    assert num_ps == (1 if kw["shard"] == "none" else kw.get("num_ps", world))
    for rec in recs[1:]:
        assert torch.equal(rec["init"], recs[0]["init"])
        assert rec["ranges"] == ranges and rec["offsets"] == recs[0]["offsets"]
    log = [e for rec in recs for e in rec["provenance"]]
    # the Python exchange logs remote pushes only; the host's own are the missing t
    assert len(log) == num_ps * (world - 1) * STEPS
    order = ar.apply_orders(log, world, STEPS, hosts=hosts)
    print("orders:", {p: ar.order_string(o) for p, o in order.items()})
    if skew:
        assert ar.staleness_exercised(order, STEPS), \
            f"staleness not exercised: {[ar.order_string(o) for o in order.values()]}"
    params, state = replay_gloo(recs, world, order)
    fails = []
    spans = [(lo, hi, f"range of PS {p}") for p, (lo, hi) in enumerate(ranges)]
    for r in range(world):
        fails += ar.mismatch_report(f"worker {r}", recs[r]["params"], params[r], spans)
    for p in range(num_ps):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        if got["t"] != t:
            fails.append(f"PS {p}: t {got['t']}, replay {t}")
        one = [(0, w.numel(), "shard")]
        fails += ar.mismatch_report(f"PS {p} params", got["w"], w, one)
        if kw.get("optimizer") != "sgd":  # (plain SGD keeps no slot: m stays as allocated)
            fails += ar.mismatch_report(f"PS {p} m", got["m"], m, one)
        else:
            assert not got["m"].any()
        if got["v"] is not None:
            fails += ar.mismatch_report(f"PS {p} v", got["v"], v, one)
        else:
            assert kw.get("optimizer") in ("momentum", "sgd")
    assert not fails, "\n".join(fails[:20])
    # the comparison is sharp on this very run: one pair of adjacent applies swapped moves it
    for p, i, sw in ar.adjacent_swaps(order):
        try:
            other, _ = replay_gloo(recs, world, sw)
        except ar.ReplayError:
            continue
        moved = max(float((a - b).abs().max()) for a, b in zip(other, params))
        print(f"PS {p}: applies {i} and {i + 1} swapped: max |diff| {moved:.1e}")
        assert moved > 0.0
        break
    else:
        pytest.fail("no realisable swap in the recorded orders")
    # the assertion the issue names, on top of the report above
    for r in range(world):
        assert torch.equal(recs[r]["params"], params[r])
    for p in range(num_ps):
        got = recs[hosts[p]]["ps"][p]
        assert torch.equal(got["w"], state[p][0]) and got["t"] == state[p][3] == world * STEPS
