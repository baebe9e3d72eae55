"""Clipping by the global norm on the CPU: the twin of the kernel's pinned order
(ddl_amd/ops/clip.py), its semantics, the option, and every Python-driven step path.

The twin widens every element to float64, where its square is exact, and adds in one fixed
order; only float64 summation rounds (relative error about n * 2^-53, far below half a float32
ulp), and one rounding to float32 follows.  So the all-double bound applies:
|norm - float32(norm64)| <= 1 ulp.  (No fp32 lane runs are used anywhere.)
"""
import argparse
import os

import numpy as np
import pytest
import torch

import async_replay as ar
from conftest import free_port
from dist_helpers import spawn, train_rank
from onecard import f32
from oracle_common import bits

from ddl_amd.ops import clip as C

CH = C.CHUNK


def ulp(x):
    return float(np.spacing(np.float32(x)))


@pytest.fixture(scope="module")
def noise():
    g = torch.Generator().manual_seed(3)
    return torch.randn(257 * CH + 16, generator=g)


# ---- a. against float64 numpy ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 5, 257 * CH + 1])
@pytest.mark.parametrize("scale", [1.0, 1e-12, 1e12])
def test_norm_against_float64(noise, n, scale):
    x = (noise[1:1 + n] * scale).contiguous()
    buf = torch.cat([torch.full((1,), 7.0), x, torch.full((2,), 7.0)])
    norm, coef = C.grad_norm_coef(buf, [(1, n)], 1e30)
    ref = np.float32(np.sqrt(np.sum(x.numpy().astype("f8") ** 2)))
    print(f"n {n} scale {scale}: norm {norm}, float32(norm64) {float(ref)}")
    assert coef == 1.0
    assert abs(norm - float(ref)) <= ulp(ref)


def test_ranges_are_summed_in_table_order_and_split_freely(noise):
    """A table of several ragged ranges against numpy; an empty range changes nothing."""
    ranges = [(3, 5), (10, CH + 1), (CH + 20, 0), (CH + 24, 2 * CH), (4 * CH, 77)]
    x = noise[:5 * CH].clone()
    norm, _ = C.grad_norm_coef(x, ranges, 1e30)
    ref = np.float32(np.sqrt(sum(np.sum(x[lo:lo + n].numpy().astype("f8") ** 2)
                                 for lo, n in ranges)))
    assert abs(norm - float(ref)) <= ulp(ref)
    assert C.grad_norm_coef(x, [r for r in ranges if r[1]], 1e30)[0] == norm
    with pytest.raises(ValueError):
        C.grad_norm_coef(x, [(0, 1)] * 17, 1.0)
    with pytest.raises(ValueError):
        C.grad_norm_coef(x, [(5 * CH - 1, 2)], 1.0)
    with pytest.raises(ValueError):
        C.grad_norm_coef(x, [(0, 4)], 0.0)


# ---- b. semantics ---------------------------------------------------------------------------------
def test_semantics_table(noise):
    n = CH + 9
    x = noise[:n].clone() * 1e-3
    x[5] = -0.0
    norm, _ = C.grad_norm_coef(x, [(0, n)], 1.0)
    # norm < C
    y = x.clone()
    got = C.clip_grads_(y, [(0, n)], f32(4.0 * norm))
    assert got == (norm, 1.0) and torch.equal(bits(y), bits(x))
    assert int(bits(y)[5]) == int(bits(torch.tensor([-0.0]))[0])
    # norm > C: coef = float32(C / norm), every element rounded once.  The clipped norm is off C
    # by the rounding of coef (2^-24), of the elements (2^-24 of the norm at most) and of the
    # measured norm itself (2^-24): 3 * 2^-24 relative
    c = f32(0.125 * norm)
    y = x.clone()
    got = C.clip_grads_(y, [(0, n)], c)
    want = c / np.sqrt(np.sum(x.numpy().astype("f8") ** 2))
    assert got[0] == norm and 0.0 < got[1] < 1.0 and abs(got[1] - want) <= 2.0 ** -24 * want
    assert torch.equal(bits(y), bits(x * torch.tensor(got[1], dtype=torch.float32)))
    after, _ = C.grad_norm_coef(y, [(0, n)], 1.0)
    assert abs(after - c) <= 3 * 2.0 ** -24 * c
    # all zero
    z = torch.zeros(n)
    assert C.clip_grads_(z, [(0, n)], 1.0) == (0.0, 1.0) and not z.any()
    # one inf (and a nan): coef 1, the norm reported, nothing rewritten
    for bad in (float("inf"), float("nan")):
        y = x.clone()
        y[77] = bad
        keep = y.clone()
        got = C.clip_grads_(y, [(0, n)], 1.0)
        assert got[1] == 1.0 and not np.isfinite(got[0]) and torch.equal(bits(y), bits(keep))
    assert C.grad_norm_coef(torch.cat([x[:77], torch.tensor([float("inf")])]), [(0, 78)],
                            1.0)[0] == float("inf")
    # padding of 1e30 around and between the ranges: not counted, not scaled
    p = torch.full((n + 12,), 1e30)
    p[4:4 + 100] = x[:100]
    p[108:108 + n - 100] = x[100:]
    two = [(4, 100), (108, n - 100)]
    clean = torch.zeros(n + 12)
    clean[4:104], clean[108:108 + n - 100] = x[:100], x[100:]
    assert C.grad_norm_coef(p, two, c) == C.grad_norm_coef(clean, two, c)
    C.clip_grads_(p, two, c)
    assert bool((p[:4] == 1e30).all() and (p[104:108] == 1e30).all() and (p[-4:] == 1e30).all())


def test_plan_ranges_are_the_14_tensors():
    from ddl_amd.models.layout import TENSORS, TOTAL_NUMEL
    from ddl_amd.parallel.sharding import make_plan
    for shard, n in (("none", 1), ("contiguous", 3), ("flat", 2)):
        plan = make_plan(shard, n)
        r = C.payload_ranges(plan.tensor_offsets)
        assert len(r) == len(TENSORS) == 14 and sum(k for _, k in r) == TOTAL_NUMEL
        assert all(a[0] + a[1] <= b[0] for a, b in zip(r, r[1:])) and r[-1][0] + r[-1][1] <= plan.total


# ---- c. the option ----------------------------------------------------------------------------------
def test_config():
    from ddl_amd.config import TrainConfig, add_args, from_args
    assert TrainConfig().clip_norm == 0.0
    with pytest.raises(ValueError, match="clip-norm"):
        TrainConfig(clip_norm=-1.0)
    p = add_args(argparse.ArgumentParser())
    with pytest.raises(ValueError, match="clip-norm"):
        from_args(p.parse_args(["--clip-norm", "-1"]))
    assert from_args(p.parse_args([])).clip_norm == 0.0
    cfg = from_args(p.parse_args(["--clip-norm", "2.5"]))
    assert cfg.clip_norm == 2.5 and TrainConfig(**cfg.to_dict()).clip_norm == 2.5


# ---- the range table under the sanitizers (host code only) ---------------------------------------
def test_range_table_asan_ubsan(tmp_path):
    """csrc/kernels/tests/clip_ranges_check.cpp: the table builder and the kernels' index
    arithmetic on the shapes of the GPU tests, as a stand-alone host program built with
    AddressSanitizer + UndefinedBehaviorSanitizer (hipcc's host compiler, else g++)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "distributed-deep-learning_amd", "csrc", "kernels", "tests",
                       "clip_ranges_check.cpp")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "clip_ranges_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if os.path.exists(hipcc):
        cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
               *[a for f in san for a in ("-Xarch_host", f)], src, "-o", exe]
    elif shutil.which("g++"):
        cmd = ["g++", "-std=c++17", "-O1", "-g", *san, src, "-o", exe]
    else:
        pytest.skip("needs hipcc or g++")
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK "), r.stdout


# ---- d, e. the step paths ---------------------------------------------------------------------------
BASE = dict(steps=3, batch_size=20, eval_every=0, quiet=True, engine="torch", data="synthetic",
            watchdog_s=120.0, lr=1e-3)
N_TRAIN = 600


def simulate(cfg_kw, world, clip_norm):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as the ranks (dist_helpers._setup): the engine's own sums
    try:
        return _simulate(cfg_kw, world, clip_norm)
    finally:
        torch.set_num_threads(threads)


def _simulate(cfg_kw, world, clip_norm):
    """One process, the plan's own buffers: every worker's engine gradient (own batch, own
    dropout seed), clipped by ops/clip.py, summed in rank order, one ParameterServer update
    (parallel/ps.py) per PS and step.  Returns the parameters and per rank the (norm, coef) of
    every step."""
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
    data = synthetic_mnist(N_TRAIN, 200, seed=7)
    num_ps = resolve_num_ps(cfg, world)
    plan = make_plan("none" if cfg.mode == "single" else cfg.shard, num_ps)
    dev = torch.device("cpu")
    params, grads = torch.zeros(plan.total), torch.zeros(plan.total)
    init_params_(params, plan.tensor_offsets, cfg.seed)
    eng = make_engine("torch", params, grads, plan.tensor_offsets, dev, cfg.batch_size)
    servers = [ParameterServer(plan, p, dev, AdamHyper(lr=cfg.lr), cfg.optimizer, cfg.momentum,
                               native_optim=False, weight_decay=cfg.weight_decay,
                               nesterov=cfg.nesterov) for p in range(num_ps)]
    ranges = C.payload_ranges(plan.tensor_offsets)
    seen = [[] for _ in range(world)]
    for step in range(cfg.steps):
        acc = None
        for r in range(world):
            lo, hi = batch_indices(step, cfg.batch_size, data.total_batch, r, world,
                                   cfg.data_sharding)
            eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg.keep_prob,
                                 rng.step_seed(cfg.seed, r, step))
            if clip_norm > 0:
                seen[r].append(C.clip_grads_(grads, ranges, clip_norm))
            acc = grads.clone() if acc is None else acc.add_(grads)
        for ps in servers:
            ps.update_flat(params, acc)
    return params, seen, plan


@pytest.fixture
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (as simulate)
    yield
    torch.set_num_threads(threads)


def test_single_torch_engine_is_the_hand_loop(one_thread):
    """Single, 3 steps: clip below the first step's norm = the hand loop (engine, clip_grads_,
    PS update), bit for bit; clip above every norm = the unclipped run, bit for bit."""
    from ddl_amd.parallel.roles import Single
    from ddl_amd.utils.data import synthetic_mnist
    kw = dict(BASE)
    kw.pop("steps"), kw.pop("batch_size")

    def run(clip_norm):
        tr = Single(1, BASE["batch_size"], steps=BASE["steps"], clip_norm=clip_norm, **kw)
        tr.data = synthetic_mnist(N_TRAIN, 200, seed=7)
        norms = []
        for i in range(BASE["steps"]):
            tr.train_step(i)
            norms.append(tr.last_grad_norm())
        return tr, norms

    plain, none = run(0.0)
    assert none == [None] * 3
    _, seen, _ = simulate(dict(BASE, mode="single"), 1, 1e30)
    norms = [n for n, _ in seen[0]]
    assert all(np.isfinite(n) and n > 0 for n in norms)
    c = f32(0.5 * norms[0])
    ref, seen, _ = simulate(dict(BASE, mode="single", clip_norm=c), 1, c)
    assert seen[0][0][1] < 1.0
    got, got_norms = run(c)
    print("norms", got_norms, "coefs", [k for _, k in seen[0]])
    assert got_norms == [n for n, _ in seen[0]]
    assert torch.equal(bits(got.params), bits(ref))
    assert not torch.equal(bits(got.params), bits(plain.params))
    hi = f32(2.0 * max(norms))
    loose, loose_norms = run(hi)
    assert torch.equal(bits(loose.params), bits(plain.params)) and loose_norms == norms


@pytest.mark.slow
@pytest.mark.parametrize("shard", ["contiguous"])
def test_gloo_sync_w2_applies_each_ranks_clipped_gradient(tmp_path, shard):
    """W = 2 over gloo, contiguous plan: every replica equals the one-process PS simulation fed
    with each rank's own clipped gradient (two addends: the sum has one order), bit for bit."""
    kw = dict(BASE, mode="sync", shard=shard)
    _, seen, _ = simulate(kw, 2, 1e30)
    c = f32(0.5 * min(n for r in seen for n, _ in r[:1]))
    kw["clip_norm"] = c
    ref, seen, plan = simulate(kw, 2, c)
    assert all(r[0][1] < 1.0 for r in seen)
    spawn(train_rank, 2, free_port(), kw, str(tmp_path), N_TRAIN)
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(2)]
    for r, rec in enumerate(recs):
        assert rec["plan_offsets"] == plan.tensor_offsets
        assert torch.equal(bits(rec["params"]), bits(ref)), r
        assert rec["summary"]["grad_norm"] == seen[r][-1][0]
    unclipped, _, _ = simulate(dict(kw, clip_norm=0.0), 2, 0.0)
    assert not torch.equal(bits(unclipped), bits(ref))


@pytest.mark.slow
def test_gloo_async_w2_equals_its_replay_with_clipped_gradients(tmp_path):
    """W = 2 over gloo, async: the run equals the replay of its recorded apply orders with a
    gradient function that clips, bit for bit."""
    import test_async_replay_cpu as T
    from ddl_amd.models.mnist_cnn import TorchEngine
    from ddl_amd.ops import rng
    from ddl_amd.utils.data import batch_indices, synthetic_mnist
    world, c = 2, 0.25
    spawn(T._gloo_rank, world, free_port(), str(tmp_path),
          dict(shard="contiguous", clip_norm=c), ())
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    order = ar.apply_orders([e for rec in recs for e in rec["provenance"]], world, T.STEPS,
                            hosts=hosts)
    cfg = recs[0]["cfg"]
    assert cfg["clip_norm"] == c
    data = synthetic_mnist(600, 200, seed=7)
    params = torch.zeros(recs[0]["total"])
    grads = torch.zeros_like(params)
    eng = TorchEngine(params, grads, recs[0]["offsets"], T.BATCH)
    table = C.payload_ranges(recs[0]["offsets"])
    coefs = []

    def make_grad_fn(clip):
        def grad_fn(r, s, params_r):
            params.copy_(params_r)
            lo, hi = batch_indices(s, T.BATCH, data.total_batch, r, world, cfg["data_sharding"])
            eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg["keep_prob"],
                                 rng.step_seed(cfg["seed"], r, s))
            if clip:
                coefs.append(C.clip_grads_(grads, table, c)[1])
            return grads.clone()
        return grad_fn

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        want, state = ar.replay(order, ranges, recs[0]["init"], world, T.STEPS,
                                make_grad_fn(True), T.UPDATES["adam"])
        plain, _ = ar.replay(order, ranges, recs[0]["init"], world, T.STEPS,
                             make_grad_fn(False), T.UPDATES["adam"])
    finally:
        torch.set_num_threads(threads)
    print("coefs", coefs)
    assert min(coefs) < 1.0
    for r in range(world):
        assert torch.equal(bits(recs[r]["params"]), bits(want[r])), r
        assert not torch.equal(bits(recs[r]["params"]), bits(plain[r]))
    for p in range(len(hosts)):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        assert got["t"] == t and torch.equal(bits(got["w"]), bits(w))
        assert torch.equal(bits(got["m"]), bits(m)) and torch.equal(bits(got["v"]), bits(v))
