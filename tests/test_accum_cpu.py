"""Gradient accumulation over K micro-batches on the CPU (--accum-steps): the twin of the
kernel's arithmetic (ddl_amd/ops/accum.py), the option, every Python-driven step path and resume.

The twin is one float32 operation per rounding (a copy, an add, or an add and a multiply by
float32(1 / K)), so every comparison below demands equal bits.
"""
import argparse
import os
import traceback

import numpy as np
import pytest
import torch

import async_replay as ar
import exchange_reference as xr
from conftest import free_port
from dist_helpers import _setup, spawn, train_rank
from onecard import f32
from oracle_common import bits

from ddl_amd.ops import accum as A
from ddl_amd.ops import clip as C


NEG0 = int(np.float32(-0.0).view(np.int32))


# ---- a. the twin's arithmetic ------------------------------------------------------------------------
def micro_grads(k, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (10.0 ** (i - 1)) for i in range(k)]


def run_twin(gs, ranges, total, pad=1e30):
    """The K passes on buffers whose padding holds `pad`: (g afterwards, A afterwards)."""
    k = len(gs)
    buf = torch.full((total,), pad)
    acc = torch.full((total,), pad)
    for j, g in enumerate(gs):
        for lo, n in ranges:
            buf[lo:lo + n] = g[lo:lo + n]
        A.accum_grads_(buf, acc, ranges, A.mode_of(j, k), k)
    return buf, acc


@pytest.mark.parametrize("k", [2, 3, 5])
def test_twin_is_one_rounding_per_operation(k):
    """Against numpy float32, written out: ((g0 + g1) + ... + g_{K-1}) * float32(1 / K), every
    operation rounded once; the padding of g and of A keeps its bits."""
    total = 300
    ranges = [(1, 7), (9, 64), (80, 0), (81, 200)]
    gs = micro_grads(k, total)
    got, acc = run_twin(gs, ranges, total)
    r = np.float32(1.0 / k)
    want = gs[0].numpy().copy()
    for g in gs[1:]:
        want = (want + g.numpy()).astype(np.float32)
    want = (want * r).astype(np.float32)
    mask = torch.ones(total, dtype=torch.bool)
    for lo, n in ranges:
        assert torch.equal(bits(got[lo:lo + n]), bits(torch.from_numpy(want[lo:lo + n])))
        mask[lo:lo + n] = False
    assert bool((got[mask] == 1e30).all()) and bool((acc[mask] == 1e30).all())
    assert int(mask.sum()) == total - sum(n for _, n in ranges)


def test_modes():
    assert [A.mode_of(j, 2) for j in range(2)] == [A.FIRST, A.FINISH]
    assert [A.mode_of(j, 4) for j in range(4)] == [A.FIRST, A.ADD, A.ADD, A.FINISH]
    for j, k in ((0, 1), (2, 2), (-1, 3)):
        with pytest.raises(ValueError):
            A.mode_of(j, k)
    g, a = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError):
        A.accum_grads_(g, a, [(0, 4)], A.ADD, 1)
    with pytest.raises(ValueError):
        A.accum_grads_(g, a, [(0, 4)], 3, 2)
    with pytest.raises(ValueError):
        A.accum_grads_(g, torch.zeros(5), [(0, 4)], A.ADD, 2)
    with pytest.raises(ValueError):
        A.accum_grads_(g, a, [(2, 4)], A.ADD, 2)


def test_negative_zero_survives_the_copy():
    """K = 2: A := g copies bits, so -0.0 + -0.0 = -0.0 and -0.0 * 0.5 = -0.0.  A memset or a
    0 + g would leave +0.0."""
    g0 = torch.tensor([-0.0, 1.0, -0.0, 0.0])
    g1 = torch.tensor([-0.0, 2.0, 0.0, -0.0])
    buf, acc = g0.clone(), torch.full((4,), 7.0)
    A.accum_grads_(buf, acc, [(0, 4)], A.FIRST, 2)
    assert bits(acc).tolist() == bits(g0).tolist()
    buf.copy_(g1)
    A.accum_grads_(buf, acc, [(0, 4)], A.FINISH, 2)
    assert int(bits(buf)[0]) == NEG0
    assert bits(buf).tolist() == bits(torch.tensor([-0.0, 1.5, 0.0, 0.0])).tolist()


def test_reciprocal_is_rounded_once():
    r3 = A.recip(3)
    assert r3.dtype == torch.float32
    assert float(r3) == float(np.float32(1.0 / 3.0))
    # the float nearest 1/3: no float32 neighbour is closer
    third = np.float64(1.0) / np.float64(3.0)
    near = np.float32(float(r3))
    for other in (np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(1))):
        assert abs(np.float64(near) - third) < abs(np.float64(other) - third)
    assert float(A.recip(2)) == 0.5 and float(A.recip(5)) == float(np.float32(0.2))


# ---- b. the option -------------------------------------------------------------------------------------
def test_config():
    from ddl_amd.config import TrainConfig, add_args, from_args
    assert TrainConfig().accum_steps == 1
    for bad in (0, -1):
        with pytest.raises(ValueError, match="accum-steps"):
            TrainConfig(accum_steps=bad)
    p = add_args(argparse.ArgumentParser())
    for bad in ("0", "-1"):
        with pytest.raises(ValueError, match="accum-steps"):
            from_args(p.parse_args(["--accum-steps", bad]))
    assert from_args(p.parse_args([])).accum_steps == 1
    cfg = from_args(p.parse_args(["--accum-steps", "4"]))
    assert cfg.accum_steps == 4 and TrainConfig(**cfg.to_dict()).accum_steps == 4


# ---- c. the torch-engine trainer against the hand loop -----------------------------------------------
N_TRAIN = 600
BASE = dict(eval_every=0, quiet=True, engine="torch", data="synthetic", watchdog_s=120.0, lr=1e-3)


@pytest.fixture
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as the spawned ranks (dist_helpers._setup): the engine's own sums
    yield
    torch.set_num_threads(threads)


def hand_loop(cfg_kw, world, clip_norm=0.0):
    """One process, the plan's own buffers: per step and rank, K engine gradients (batch
    cnt * K + j, dropout seed of micro-step s * K + j), the twin's passes, the twin clip if asked
    for, then the rank-order sum (exchange_reference.rank_order_sum) and one ParameterServer
    update per PS and step.  Returns (params, servers, per rank the effective gradients' norms,
    per rank the effective gradients, the plan)."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.models import make_engine
    from ddl_amd.models.mnist_cnn import init_params_
    from ddl_amd.ops import rng
    from ddl_amd.ops.adam import AdamHyper
    from ddl_amd.parallel.ps import ParameterServer
    from ddl_amd.parallel.roles import resolve_num_ps
    from ddl_amd.parallel.sharding import make_plan
    from ddl_amd.utils.data import batch_indices, synthetic_mnist
    cfg = TrainConfig(**cfg_kw)
    K = cfg.accum_steps
    data = synthetic_mnist(N_TRAIN, 200, seed=7)
    num_ps = resolve_num_ps(cfg, world)
    plan = make_plan("none" if cfg.mode == "single" else cfg.shard, num_ps)
    dev = torch.device("cpu")
    params, grads = torch.zeros(plan.total), torch.zeros(plan.total)
    acc = torch.zeros(plan.total)
    init_params_(params, plan.tensor_offsets, cfg.seed)
    eng = make_engine("torch", params, grads, plan.tensor_offsets, dev, cfg.batch_size)
    servers = [ParameterServer(plan, p, dev, AdamHyper(lr=cfg.lr), cfg.optimizer, cfg.momentum,
                               native_optim=False, weight_decay=cfg.weight_decay,
                               nesterov=cfg.nesterov) for p in range(num_ps)]
    ranges = C.payload_ranges(plan.tensor_offsets)
    norms = [[] for _ in range(world)]
    eff = [[] for _ in range(world)]
    for step in range(cfg.steps):
        gs = []
        for r in range(world):
            for j in range(K):
                lo, hi = batch_indices(step * K + j, cfg.batch_size, data.total_batch, r, world,
                                       cfg.data_sharding)
                eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg.keep_prob,
                                     rng.step_seed(cfg.seed, r, step * K + j))
                if K > 1:
                    A.accum_grads_(grads, acc, ranges, A.mode_of(j, K), K)
            norms[r].append(C.grad_norm_coef(grads, ranges, 1e30)[0])
            if clip_norm > 0:
                C.clip_grads_(grads, ranges, clip_norm)
            eff[r].append(grads.clone())
            gs.append(grads.clone())
        total = xr.rank_order_sum(gs)
        for ps in servers:
            ps.update_flat(params, total)
    return params, servers, norms, eff, plan


def trainer_steps(cfg_kw, steps):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    tr = Trainer(TrainConfig(**cfg_kw), DistEnv(), dataset=synthetic_mnist(N_TRAIN, 200, seed=7))
    for i in range(steps):
        tr.train_step(i)
    return tr


def same_state(tr, params, servers):
    ok = torch.equal(bits(tr.params), bits(params))
    for p, ps in tr.servers.items():
        ok &= ps.t == servers[p].t
        ok &= torch.equal(bits(ps.m), bits(servers[p].m))
        if ps.v is not None:
            ok &= torch.equal(bits(ps.v), bits(servers[p].v))
    return ok


@pytest.mark.parametrize("mode", ["sync", "single", "async"])
def test_trainer_w1_is_the_hand_loop(one_thread, mode):
    """W = 1, B = 5, K = 3, two steps: parameters and optimizer state equal three
    forward_backward calls with the micro-steps' batches and seeds, the twin's passes and the PS
    update; the same with clip_norm at half the effective gradient's norm; and K = 1 is the
    plain loop over today's batch indices and seeds.  async: the host-driven AsyncExchange (an
    explicit exchange backend keeps a one-worker run off the sync step path), whose one PS
    applies each push to its private copy, the same update."""
    kw = dict(BASE, mode=mode, shard="contiguous", steps=2, batch_size=5)
    if mode == "async":
        kw["exchange_backend"] = "rccl"
    k1 = trainer_steps(dict(kw, accum_steps=1), 2)
    assert type(k1.exchange).__name__ == ("AsyncExchange" if mode == "async" else "SyncExchange")
    ref1 = hand_loop(dict(kw, accum_steps=1), 1)
    assert k1.accum_buf is None and k1.steps == 2
    assert same_state(k1, ref1[0], ref1[1])

    kw3 = dict(kw, accum_steps=3)
    got = trainer_steps(kw3, 2)
    params, servers, norms, _, _ = hand_loop(kw3, 1)
    assert all(ps.t == 2 for ps in got.servers.values())   # steps, not micro-batches
    assert got.global_step == 2
    assert same_state(got, params, servers)
    assert not torch.equal(bits(got.params), bits(k1.params))

    c = f32(0.5 * min(norms[0]))
    assert c > 0
    got_c = trainer_steps(dict(kw3, clip_norm=c), 2)
    params_c, servers_c, _, _, _ = hand_loop(dict(kw3, clip_norm=c), 1, clip_norm=c)
    assert float(got_c.clip_out[1]) < 1.0
    assert same_state(got_c, params_c, servers_c)
    assert not torch.equal(bits(got_c.params), bits(got.params))


def test_steps_per_epoch_and_image_count(one_thread):
    """The default steps per epoch is total_batch // (batch_size * K): K = 1 today's, K = 2 half;
    the summary counts K * batch_size images per step."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    data = synthetic_mnist(N_TRAIN, 200, seed=7)
    kw = dict(BASE, mode="sync", shard="contiguous", batch_size=20)
    t1 = Trainer(TrainConfig(**kw), DistEnv(), dataset=data)
    t2 = Trainer(TrainConfig(accum_steps=2, **kw), DistEnv(), dataset=data)
    assert t1.steps == data.total_batch // 20 and t2.steps == t1.steps // 2
    t3 = Trainer(TrainConfig(accum_steps=3, steps=2, **kw), DistEnv(), dataset=data)
    s = t3.train()
    assert s["steps"] == 2 and s["images"] == 2 * 3 * 20


# ---- d. gloo, W = 2 --------------------------------------------------------------------------------------
GSTEPS, GBATCH = 4, 10


@pytest.mark.slow
def test_gloo_sync_w2_applies_each_ranks_effective_gradient(tmp_path):
    """W = 2 over gloo, K = 2, 4 steps: every replica equals the one-process PS simulation fed
    with each rank's effective gradient (rank-order sum of two addends), bit for bit, and every
    PS counted 4 steps."""
    kw = dict(BASE, mode="sync", shard="contiguous", steps=GSTEPS, batch_size=GBATCH,
              accum_steps=2)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref, servers, _, _, plan = hand_loop(kw, 2)
        plain = hand_loop(dict(kw, accum_steps=1), 2)[0]
    finally:
        torch.set_num_threads(threads)
    spawn(train_rank, 2, free_port(), kw, str(tmp_path), N_TRAIN)
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(2)]
    for r, rec in enumerate(recs):
        assert rec["plan_offsets"] == plan.tensor_offsets
        assert torch.equal(bits(rec["params"]), bits(ref)), r
        assert all(t == GSTEPS for t in rec["ps_t"].values())
        assert rec["summary"]["steps"] == GSTEPS
        assert rec["summary"]["images"] == GSTEPS * 2 * GBATCH
    assert all(ps.t == GSTEPS for ps in servers)
    assert not torch.equal(bits(plain), bits(ref))


def _gloo_async_rank(rank, world, port, outdir, kw):
    """One rank of an accumulated asynchronous run over gloo (the set-up of
    tests/test_async_replay_cpu.py::_gloo_rank), GSTEPS steps."""
    _setup(rank, world, port)
    try:
        import torch.distributed as dist
        from ddl_amd.config import TrainConfig
        from ddl_amd.parallel.comm import AsyncExchange, init_distributed
        from ddl_amd.parallel.roles import Trainer
        from ddl_amd.utils.data import synthetic_mnist
        env = init_distributed(device="cpu")
        cfg = TrainConfig(mode="async", steps=GSTEPS, batch_size=GBATCH, eval_every=0, quiet=True,
                          engine="torch", data="synthetic", check_provenance=True,
                          watchdog_s=120.0, **kw)
        tr = Trainer(cfg, env, dataset=synthetic_mnist(N_TRAIN, 200, seed=7))
        ex = tr.exchange
        assert type(ex) is AsyncExchange, type(ex)
        init = tr.params.clone()
        ex.steps = GSTEPS
        ex.start()
        dist.barrier()
        for i in range(GSTEPS):
            tr.train_step(i)
        ex.join()
        ex.verify_provenance()
        torch.save({"init": init, "params": tr.params.clone(),
                    "ps": {p: dict(w=s.params.clone(), m=s.m.clone(), v=s.v.clone(), t=s.t)
                           for p, s in tr.servers.items()},
                    "provenance": list(ex.provenance),
                    "ranges": [tr.plan.ps_segments(p)[0] for p in range(tr.plan.num_ps)],
                    "hosts": [tr.plan.host_rank(p, world) for p in range(tr.plan.num_ps)],
                    "offsets": list(tr.plan.tensor_offsets), "total": tr.plan.total,
                    "cfg": cfg.to_dict(), "global_step": tr.global_step},
                   os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        ex.close()
        dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


@pytest.mark.slow
def test_gloo_async_w2_equals_its_replay_with_effective_gradients(tmp_path):
    """W = 2 over gloo, async, K = 2, 4 steps: the run equals the replay of its recorded apply
    orders with a gradient function that accumulates two micro-batches from the same parameters;
    every PS applied W * 4 pushes (steps, not micro-batches)."""
    import test_async_replay_cpu as T
    from ddl_amd.models.mnist_cnn import TorchEngine
    from ddl_amd.ops import rng
    from ddl_amd.utils.data import batch_indices, synthetic_mnist
    world, K = 2, 2
    spawn(_gloo_async_rank, world, free_port(), str(tmp_path),
          dict(shard="contiguous", accum_steps=K))
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    order = ar.apply_orders([e for rec in recs for e in rec["provenance"]], world, GSTEPS,
                            hosts=hosts)
    cfg = recs[0]["cfg"]
    assert cfg["accum_steps"] == K and all(rec["global_step"] == GSTEPS for rec in recs)
    data = synthetic_mnist(N_TRAIN, 200, seed=7)
    params = torch.zeros(recs[0]["total"])
    grads = torch.zeros_like(params)
    acc = torch.zeros_like(params)
    eng = TorchEngine(params, grads, recs[0]["offsets"], GBATCH)
    table = C.payload_ranges(recs[0]["offsets"])

    def make_grad_fn(k):
        def grad_fn(r, s, params_r):
            params.copy_(params_r)
            for j in range(k):
                lo, hi = batch_indices(s * k + j, GBATCH, data.total_batch, r, world,
                                       cfg["data_sharding"])
                eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg["keep_prob"],
                                     rng.step_seed(cfg["seed"], r, s * k + j))
                if k > 1:
                    A.accum_grads_(grads, acc, table, A.mode_of(j, k), k)
            return grads.clone()
        return grad_fn

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        want, state = ar.replay(order, ranges, recs[0]["init"], world, GSTEPS, make_grad_fn(K),
                                T.UPDATES["adam"])
        plain, _ = ar.replay(order, ranges, recs[0]["init"], world, GSTEPS, make_grad_fn(1),
                             T.UPDATES["adam"])
    finally:
        torch.set_num_threads(threads)
    for r in range(world):
        assert torch.equal(bits(recs[r]["params"]), bits(want[r])), r
        assert not torch.equal(bits(recs[r]["params"]), bits(plain[r]))
    for p in range(len(hosts)):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        assert got["t"] == t == world * GSTEPS
        assert torch.equal(bits(got["w"]), bits(w))
        assert torch.equal(bits(got["m"]), bits(m)) and torch.equal(bits(got["v"]), bits(v))


# ---- e. resume ---------------------------------------------------------------------------------------------
def _train(cfg_kw):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    tr = Trainer(TrainConfig(**cfg_kw), DistEnv(), dataset=synthetic_mnist(400, 100, seed=11))
    tr.train()
    return tr


def test_resume_continues_an_accumulated_run(tmp_path, one_thread):
    """K = 2, stopped after step 2 of 4 and resumed: the uninterrupted run, bit for bit (the
    micro-steps' batches and seeds pick up at step 2); the manifest records K, and a resume under
    another K is refused."""
    import json
    base = dict(BASE, mode="sync", shard="contiguous", num_ps=3, steps=4, batch_size=20,
                accum_steps=2)
    full = _train(dict(base, checkpoint_dir=str(tmp_path / "full")))
    part = _train(dict(base, checkpoint_dir=str(tmp_path / "cut"), max_steps=2))
    assert part.global_step == 2
    man = json.load(open(os.path.join(str(tmp_path / "cut"), "manifest.json")))
    assert man["accum_steps"] == 2 and man["global_step"] == 2
    res = _train(dict(base, checkpoint_dir=str(tmp_path / "cut"), resume=True))
    assert res.global_step == 4
    assert torch.equal(bits(res.params), bits(full.params))
    for p, ps in full.servers.items():
        q = res.servers[p]
        assert q.t == ps.t == 4
        assert torch.equal(bits(q.m), bits(ps.m)) and torch.equal(bits(q.v), bits(ps.v))
    _train(dict(base, checkpoint_dir=str(tmp_path / "cut3"), max_steps=2))
    with pytest.raises(ValueError, match="accum-steps 2"):
        _train(dict(base, accum_steps=3, checkpoint_dir=str(tmp_path / "cut3"), resume=True))


def test_manifest_without_the_field_means_one(tmp_path, one_thread):
    import json
    base = dict(BASE, mode="sync", shard="contiguous", num_ps=3, steps=4, batch_size=20)
    full = _train(dict(base, checkpoint_dir=str(tmp_path / "full")))
    _train(dict(base, checkpoint_dir=str(tmp_path / "cut"), max_steps=2))
    mp = os.path.join(str(tmp_path / "cut"), "manifest.json")
    man = json.load(open(mp))
    assert man.pop("accum_steps") == 1
    json.dump(man, open(mp, "w"))
    res = _train(dict(base, checkpoint_dir=str(tmp_path / "cut"), resume=True))
    assert torch.equal(bits(res.params), bits(full.params))
    with pytest.raises(ValueError, match="accum-steps"):
        _train(dict(base, accum_steps=2, checkpoint_dir=str(tmp_path / "cut"), resume=True))
