"""Decoupled weight decay (AdamW / SGDW) and Nesterov momentum at every update site on the GPU.

1. the three stand-alone shapes (vector kernel, scalar kernel, Engine::flush_tail) on the span of
   tests/test_update_rule_gpu.py: same bits, each of 3 steps within the fp64 closed form of
   tests/update_rule_reference.py, nothing outside the span touched;
2. the W = 1 step's three placements (tails + reduce epilogues, tails + a launch, launches after
   the backward): same bits, and the options keep a step on the tail path;
3. the engine's other paths (no dual launches, conv1's weight gradient through the GEMM);
4. the asynchronous W = 1 step with in-line applies against update_flat on its own gradients;
5. the xGMI exchange kernels: one spawned W = 2 job per data plane on one card, the synchronous
   one against a one-process simulation, the asynchronous one against its replay
   (tests/async_replay.py).

update_flat / flush_update_tail / PeerExchange.launch take the decay as lr * wd (a double, rounded
to float once inside); the trainers take --weight-decay and form the same product.

Measured on one MI355X: the two spawned jobs 2.7 and 3.2 s (nearly all of it the ranks' start-up),
every other case under 0.5 s; against the closed form |w - ref| <= 2.3e-7, rel m <= 2.4e-7, rel v <= 1.9e-7
(bounds 1e-6)."""
import os
import sys
import time
import traceback

import pytest
import torch

import async_replay as ar
from conftest import ROOT, free_port
from update_rule_reference import adam_step_size, update_closed_form

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, ALIGNED, SHIFTED = 1023, 4, 5
ADAM, MOMENTUM = 0, 1  # update.h UpdKind
B1, B2, EPS, MU = 0.9, 0.999, 1e-8, 0.9
WD = 0.1
STEPS = 3
ADAMW = dict(optimizer="adam", weight_decay=WD)
NESTEROV_WD = dict(optimizer="momentum", nesterov=True, weight_decay=WD)
JOB_LIMIT_S = 150.0


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1. the stand-alone shapes -------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.models.layout import CANON_OFFSETS, TOTAL_NUMEL
    params = torch.zeros(TOTAL_NUMEL, device=DEV)
    return HipEngine(params, torch.zeros_like(params), CANON_OFFSETS, batch=8, graph=False,
                     eval_chunk=8).eng


@pytest.fixture(scope="module")
def span():
    """w, m, v of tests/test_update_rule_gpu.py's span and one gradient per step (CPU), the same
    for every case."""
    torch.manual_seed(7)
    w, g, m, v = torch.randn(N), torch.randn(N) * 1e-2, torch.randn(N) * 1e-3, torch.rand(N) * 1e-4
    gen = torch.Generator().manual_seed(8)
    grads = [g] + [torch.randn(N, generator=gen) * 1e-2 for _ in range(STEPS - 1)]
    return w, m, v, grads


def _placed(x, lo):
    buf = torch.full((N + 4 + 1,), float("nan"), device=DEV)
    buf[lo:lo + N] = x.to(DEV)
    assert buf[lo:].data_ptr() % 16 == (4 * lo) % 16
    return buf


def _outside_intact(buf, lo):
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + N:]).all())


# (kind, lr, mu, weight decay, nesterov)
VARIANTS = [
    pytest.param(ADAM, 3e-4, 0.0, WD, False, id="adamw"),
    pytest.param(MOMENTUM, 3e-2, MU, WD, False, id="momentum-wd"),
    pytest.param(MOMENTUM, 3e-2, MU, 0.0, True, id="nesterov"),
    pytest.param(MOMENTUM, 3e-2, MU, WD, True, id="nesterov-wd"),
    pytest.param(MOMENTUM, 3e-2, 0.0, WD, False, id="sgd-wd"),
]


def _steps(launch, span, lo, kind, lr, mu, wd, nesterov, scale, options=True):
    """STEPS updates of the span placed at `lo`; the (w, m, v) after each, on the CPU."""
    w, m, v, grads = span
    W, M, V = (_placed(t, lo) for t in (w, m, v))
    view = lambda b: b[lo:lo + N]  # noqa: E731
    out = []
    for k, g in enumerate(grads):
        G = _placed(g, lo)
        step = adam_step_size(lr, B1, B2, k + 1) if kind == ADAM else lr
        args = (kind, view(W), view(G), view(M), view(V) if kind == ADAM else None, step, B1, B2,
                EPS, mu, scale)
        if options:
            launch(*args, lr * wd, nesterov)
        else:
            launch(*args)
        torch.cuda.synchronize()
        assert all(_outside_intact(b, lo) for b in (W, G, M, V))
        assert torch.equal(view(G).cpu(), g)  # the gradient is read only
        if kind != ADAM:
            assert torch.equal(view(V).cpu(), v)  # no v stream under momentum
        out.append((view(W).cpu(), view(M).cpu(), view(V).cpu()))
    return out


@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("kind,lr,mu,wd,nesterov", VARIANTS)
def test_shapes_same_bits_and_closed_form(engine, span, kind, lr, mu, wd, nesterov, scale):
    from ddl_amd.ops import native
    a = (kind, lr, mu, wd, nesterov, scale)
    vec = _steps(native.ops().update_flat, span, ALIGNED, *a)
    sca = _steps(native.ops().update_flat, span, SHIFTED, *a)
    tail = _steps(engine.flush_update_tail, span, ALIGNED, *a)
    for k in range(STEPS):
        for name, x, y, z in zip("wmv", vec[k], sca[k], tail[k]):
            assert torch.equal(bits(x), bits(y)), f"step {k} {name}: vector vs scalar kernel"
            assert torch.equal(bits(x), bits(z)), f"step {k} {name}: vector kernel vs flushed tail"
    # each step within the closed form, restarted from the kernel's own previous state
    w0, m0, v0, grads = span
    before = (w0, m0, v0)
    name = "adam" if kind == ADAM else "momentum"
    for k in range(STEPS):
        w_ref, m_ref, v_ref = update_closed_form(
            name, before[0], before[1], before[2] if kind == ADAM else None, [grads[k]], lr,
            b1=B1, b2=B2, eps=EPS, mu=mu, weight_decay=wd, nesterov=nesterov, scale=scale, t0=k)
        w, m, v = vec[k]
        err_w = float((w.double() - w_ref).abs().max())
        err_m = rel_err(m, m_ref)
        err_v = rel_err(v, v_ref) if kind == ADAM else 0.0
        print(f"step {k}: |w - ref| {err_w:.3e}  rel m {err_m:.3e}  rel v {err_v:.3e}")
        assert err_w < 1e-6 and err_m < 1e-6 and err_v < 1e-6
        before = vec[k]
    # and the options did something: the same steps without them end elsewhere
    plain = _steps(native.ops().update_flat, span, ALIGNED, kind, lr, mu, 0.0, False, scale)
    assert float((plain[-1][0] - vec[-1][0]).abs().max()) > 1e-4


@pytest.mark.parametrize("kind,lr,mu", [(ADAM, 3e-4, 0.0), (MOMENTUM, 3e-2, MU),
                                        (MOMENTUM, 3e-2, 0.0)])
def test_options_off_is_the_call_without_them(engine, span, kind, lr, mu):
    """decay = 0 and nesterov = False passed explicitly give the bits of a call that does not pass
    them, on all three shapes; the span holds a -0.0 parameter with a zero gradient, which a
    decay executed with a zero factor would turn into +0.0."""
    from ddl_amd.ops import native
    w, m, v, grads = span
    w, m, v = w.clone(), m.clone(), v.clone()
    grads = [g.clone() for g in grads]
    w[3], m[3], v[3] = -0.0, 0.0, 1e-4
    for g in grads:
        g[3] = 0.0
    sp = (w, m, v, grads)
    for launch, lo in ((native.ops().update_flat, ALIGNED), (native.ops().update_flat, SHIFTED),
                       (engine.flush_update_tail, ALIGNED)):
        with_ = _steps(launch, sp, lo, kind, lr, mu, 0.0, False, 1.0 / 3.0, options=True)
        without = _steps(launch, sp, lo, kind, lr, mu, 0.0, False, 1.0 / 3.0, options=False)
        for k in range(STEPS):
            for x, y in zip(with_[k], without[k]):
                assert torch.equal(bits(x), bits(y))
        if kind == MOMENTUM:  # w' = fma(-lr, 0, -0.0) keeps the sign
            assert int(bits(with_[-1][0])[3]) == int(bits(torch.tensor([-0.0]))[0])


def test_bindings_refuse_bad_options(span):
    from ddl_amd.ops import native
    w, m, v, grads = span
    W, G, M = (t.to(DEV) for t in (w, grads[0], m))
    with pytest.raises(RuntimeError, match="Nesterov"):
        native.ops().update_flat(ADAM, W, G, M, M.clone(), 1e-4, B1, B2, EPS, 0.0, 1.0, 0.0, True)
    with pytest.raises(RuntimeError, match="negative"):
        native.ops().update_flat(MOMENTUM, W, G, M, None, 1e-2, 0.0, 0.0, 0.0, MU, 1.0, -1e-3,
                                 False)
    assert torch.equal(W.cpu(), w)


@pytest.mark.parametrize("optimizer,lr,wd,nesterov", [("adam", 3e-4, WD, False),
                                                       ("momentum", 3e-2, WD, True),
                                                       ("sgd", 3e-2, WD, False)])
def test_parameter_server_native_branches(span, optimizer, lr, wd, nesterov):
    """ParameterServer on the GPU (the Python exchanges' update) hands both options to
    update_flat: the same bits as the direct call, step by step."""
    from ddl_amd.ops import native
    from ddl_amd.ops.adam import AdamHyper
    from ddl_amd.parallel.ps import ParameterServer
    from ddl_amd.parallel.sharding import make_plan
    w0, m0, v0, grads = span
    ps = ParameterServer(make_plan("none", 1), 0, DEV, AdamHyper(lr=lr, beta1=B1, beta2=B2,
                                                                  eps=EPS), optimizer, MU,
                         weight_decay=wd, nesterov=nesterov)
    n = N - 3  # a multiple of 4, so views at offset 0 take the vector kernel
    ps.m[:n] = m0[:n].to(DEV)
    if ps.v is not None:
        ps.v[:n] = v0[:n].to(DEV)
    w = w0[:n].to(DEV)
    W, M, V = w0[:n].to(DEV), m0[:n].to(DEV), v0[:n].to(DEV)
    kind = ADAM if optimizer == "adam" else MOMENTUM
    mu = MU if optimizer == "momentum" else 0.0
    for k, g in enumerate(grads):
        G = g[:n].to(DEV)
        ps.begin()
        ps.apply(w, G, 0, 1.0 / 3.0)
        step = adam_step_size(lr, B1, B2, k + 1) if kind == ADAM else lr
        native.ops().update_flat(kind, W, G, M, V if kind == ADAM else None, step, B1, B2, EPS,
                                 mu, 1.0 / 3.0, lr * wd, nesterov)
        assert torch.equal(bits(w), bits(W)) and torch.equal(bits(ps.m[:n]), bits(M))
        if ps.v is not None:
            assert torch.equal(bits(ps.v[:n]), bits(V))
    plain = w0[:n].to(DEV)
    assert not torch.equal(w, plain)


# ---- 2, 3. the W = 1 step -----------------------------------------------------------------------
BATCH = 33


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(n_train=2000, n_test=500, seed=5)


def _run(data, opts, shard, tail=None, final=None, setup=None):
    """Parameters and every server's (m, v) after STEPS steps, and update_launches() of the last
    one.  tail / final None: the runner's default."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    cfg = TrainConfig(mode="sync", shard=shard, steps=STEPS, batch_size=BATCH, eval_every=0,
                      engine="hip", quiet=True, lr=1e-2, seed=0, **opts)
    tr = Trainer(cfg, env, dataset=data)
    runner = tr.exchange.runner
    if tail is not None:
        runner.set_use_tail(tail)
    if final is not None:
        runner.set_final_in_reduce(final)
    if setup is not None:
        setup(tr)
    p0 = tr.params.clone()
    for i in range(STEPS):
        tr.train_step(i)
    torch.cuda.synchronize()
    assert not torch.equal(tr.params, p0)  # it trained
    state = [(s.m.clone(), None if s.v is None else s.v.clone())
             for _, s in sorted(tr.servers.items())]
    out = tr.params.clone(), state, runner.update_launches()
    tr.exchange.close()
    return out


def _assert_same(a, b):
    (pa, sa, _), (pb, sb, _) = a, b
    assert torch.isfinite(pa).all()
    assert torch.equal(bits(pa), bits(pb))
    assert len(sa) == len(sb) > 0
    for (ma, va), (mb, vb) in zip(sa, sb):
        assert torch.equal(bits(ma), bits(mb))
        assert (va is None) == (vb is None)
        if va is not None:
            assert torch.equal(bits(va), bits(vb))


PLACEMENTS = ((True, True), (True, False), (False, False))  # (set_use_tail, set_final_in_reduce)


@pytest.mark.parametrize("shard", ["flat", "contiguous"])
@pytest.mark.parametrize("opts", [ADAMW, NESTEROV_WD], ids=["adamw", "nesterov-wd"])
def test_placements_bit_identical_and_on_the_tail_path(data, opts, shard):
    runs = [_run(data, opts, shard, t, f) for t, f in PLACEMENTS]
    for r in runs[:2]:
        _assert_same(r, runs[2])
    has_v = opts["optimizer"] == "adam"
    assert all((v is not None) == has_v for _, v in runs[0][1])
    # the default placement: as many stand-alone optimizer launches as without the options
    default = _run(data, opts, shard)
    off = _run(data, dict(optimizer=opts["optimizer"]), shard)
    print(f"update_launches: options on {default[2]}, off {off[2]}, tails off {runs[2][2]}")
    _assert_same(default, runs[2])
    assert default[2] == off[2]
    assert default[2] < runs[2][2]
    # and the options reach the update
    moved = float((default[0] - off[0]).abs().max())
    print(f"options on vs off: max |diff| {moved:.2e}")
    assert moved > 1e-4


@pytest.mark.parametrize("setting", ["set_dual", "set_conv1_wgrad_direct"])
def test_other_engine_paths(data, setting):
    """set_dual(False): every tail leaves through Engine::flush_tail.  set_conv1_wgrad_direct(False):
    the last segment's update goes through the split-K reduce tail.  AdamW, each against the
    launches after the backward under the same engine setting."""
    def setup(tr):
        getattr(tr.engine.eng, setting)(False)
    on = _run(data, ADAMW, "flat", True, True, setup)
    off = _run(data, ADAMW, "flat", False, False, setup)
    _assert_same(on, off)
    plain = _run(data, dict(optimizer="adam"), "flat", True, True, setup)
    assert not torch.equal(on[0], plain[0])


# ---- 4. the asynchronous W = 1 step with in-line applies --------------------------------------------
def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def test_async_inline_adamw(data, monkeypatch):
    """--mode async --exchange xgmi at one worker: each PS's AdamW as tail blocks of the next
    segment's launch.  No suite demands the bits of the synchronous run of this path (the step
    audit compares it with update_flat on the step's own gradients), so: bit-equal to
    update_flat, with the decay, from the state before the step and the step's gradients, with
    each PS's own step size as the runner forms it."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.ops import native
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    monkeypatch.delenv("DDL_ASYNC_INLINE", raising=False)
    lr = 1e-2
    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    cfg = TrainConfig(mode="async", shard="flat", steps=STEPS, batch_size=BATCH, eval_every=0,
                      engine="hip", quiet=True, exchange_backend="xgmi", lr=lr, **ADAMW)
    tr = Trainer(cfg, env, dataset=data.to(torch.device("cuda", 0)))
    ex = tr.exchange
    assert tr.num_ps == 3 and ex.runner is not None
    ex.steps = STEPS
    ex.start()
    fails = []
    try:
        assert ex.inline and ex.service_mode == "inline"
        for step in range(STEPS):
            w0 = tr.params.clone()
            st0 = {p: (ps.m.clone(), ps.v.clone()) for p, ps in tr.servers.items()}
            t0 = {p: ex.runner.inline_t(p) for p in tr.servers}
            tr.train_step(step)
            ex.drain_round()
            torch.cuda.synchronize()
            for p, ps in sorted(tr.servers.items()):
                lo, hi = ex.ranges[p]
                assert ex.runner.inline_t(p) == t0[p] + 1
                size = native.ops().adam_step_size(f32(lr), f32(B1), f32(B2), t0[p] + 1)
                for decay in (lr * WD, 0.0):
                    w, (m, v) = w0[lo:hi].clone(), tuple(t.clone() for t in st0[p])
                    native.ops().update_flat(ADAM, w, tr.grads[lo:hi], m, v, size, ps.h.beta1,
                                             ps.h.beta2, ps.h.eps, 0.0, 1.0, decay, False)
                    same = (torch.equal(bits(w), bits(tr.params[lo:hi]))
                            and torch.equal(bits(m), bits(ps.m)) and torch.equal(bits(v), bits(ps.v)))
                    if decay and not same:
                        fails.append(f"step {step} PS {p}: differs from update_flat with the decay")
                    if not decay and torch.equal(bits(w), bits(tr.params[lo:hi])):
                        fails.append(f"step {step} PS {p}: equals update_flat WITHOUT the decay")
                if not torch.equal(ps.params, tr.params[lo:hi]):
                    fails.append(f"step {step} PS {p}: private copy differs from the worker's")
    finally:
        ex.join()
        ex.close()
    assert all(ps.t == STEPS for ps in tr.servers.values())
    assert not fails, "\n".join(fails)


# ---- 5. the exchange kernels: W = 2 on one card -----------------------------------------------------
def _spawn(fn, world, *args):
    """fn(rank, world, *args) in `world` fresh processes under one time limit for the job."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    kids = [ctx.Process(target=fn, args=(r, world, *args)) for r in range(world)]
    for k in kids:
        k.start()
    deadline = time.monotonic() + JOB_LIMIT_S
    for k in kids:
        k.join(timeout=max(0.0, deadline - time.monotonic()))
    late = [k for k in kids if k.is_alive()]
    for k in late:
        k.kill()
        k.join()
    assert not late, f"{len(late)} rank(s) still running after {JOB_LIMIT_S:.0f} s"
    assert all(k.exitcode == 0 for k in kids), [k.exitcode for k in kids]


def _enter(rank, world, port):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), DDL_DIST_BACKEND="gloo",
                      DDL_XGMI_TIMEOUT_S="20", DDL_ASYNC_INLINE="0")


def _canon(params, offsets):
    from ddl_amd.models.layout import TENSORS
    return torch.cat([params[offsets[t.index]:offsets[t.index] + t.numel] for t in TENSORS])


SYNC_CELLS = [(shard, name, opts) for shard in ("flat", "contiguous")  # contiguous: owner buckets
              for name, opts in (("adamw", ADAMW), ("nesterov-wd", NESTEROV_WD))]
ASYNC_CELLS = [("adamw", ADAMW), ("nesterov-wd", NESTEROV_WD)]


def _sync_job(rank, world, port, outdir):
    _enter(rank, world, port)
    try:
        import torch.distributed as dist
        from ddl_amd.config import TrainConfig
        from ddl_amd.parallel.comm import init_distributed
        from ddl_amd.parallel.roles import Trainer
        from ddl_amd.utils.data import synthetic_mnist
        env = init_distributed()
        assert env.device.index == 0
        data = synthetic_mnist(2000, 500, seed=5)
        out = {}
        for shard, name, opts in SYNC_CELLS:
            cfg = TrainConfig(mode="sync", shard=shard, steps=STEPS, batch_size=BATCH,
                              eval_every=0, engine="hip", quiet=True, data_sharding="stride",
                              exchange_backend="xgmi", **opts)
            tr = Trainer(cfg, env, dataset=data)
            ex = tr.exchange
            assert getattr(ex, "native", False) and ex.peer is not None, "xgmi path not taken"
            owner = shard != "flat"
            assert all((ex.peer.owner(b) >= 0) == owner for b in range(len(ex.peer.nslices())))
            for i in range(STEPS):
                tr.train_step(i)
            torch.cuda.synchronize()
            ex.check()
            assert ex.peer.error() == 0, ex.peer.error()
            out[(shard, name)] = dict(params=_canon(tr.params, tr.plan.tensor_offsets).cpu(),
                                      t={p: s.t for p, s in tr.servers.items()})
            # unmap, barrier, close, barrier: no rank frees a buffer a peer still has mapped
            dist.barrier()
            ex.runner.close()
            ex.peer.unmap_peers()
            dist.barrier()
            ex.peer.close()
            dist.barrier()
            del tr, ex
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


def _simulate_sync(world, opts):
    """One process: every rank's gradient on its own batch and dropout seed, summed in rank order
    (the kernels' order), one update_flat with the options per global step."""
    from ddl_amd.models import engine_segments
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.models.mnist_cnn import init_params_
    from ddl_amd.ops import native, rng
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    from ddl_amd.parallel.sharding import make_plan
    from ddl_amd.utils.data import synthetic_mnist, batch_indices
    dev = torch.device("cuda", 0)
    data = synthetic_mnist(2000, 500, seed=5).to(dev)
    plan = make_plan("flat", world, buckets=engine_segments("hip", dev))
    params = torch.zeros(plan.total, device=dev)
    init_params_(params, plan.tensor_offsets, 0)
    grads = torch.zeros_like(params)
    acc, m, v = torch.zeros_like(params), torch.zeros_like(params), torch.zeros_like(params)
    eng = HipEngine(params, grads, plan.tensor_offsets, batch=BATCH, graph=False, eval_chunk=BATCH)
    h = AdamHyper()
    adam = opts["optimizer"] == "adam"
    decay = h.lr * opts.get("weight_decay", 0.0)
    for step in range(STEPS):
        acc.zero_()
        for r in range(world):
            lo, hi = batch_indices(step, BATCH, data.total_batch, r, world, "stride")
            eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], 0.5,
                                 rng.step_seed(0, r, step))
            acc.add_(grads)
        if adam:
            native.ops().update_flat(ADAM, params, acc, m, v, adam_coeffs(h, step + 1), h.beta1,
                                     h.beta2, h.eps, 0.0, 1.0, decay, False)
        else:
            native.ops().update_flat(MOMENTUM, params, acc, m, None, h.lr, 0.0, 0.0, 0.0, MU, 1.0,
                                     decay, bool(opts.get("nesterov", False)))
    torch.cuda.synchronize()
    return _canon(params, plan.tensor_offsets).cpu()


@pytest.mark.slow
def test_xgmi_sync_exchange_with_options(tmp_path):
    world = 2
    _spawn(_sync_job, world, free_port(), str(tmp_path))
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    sims = {}
    for shard, name, opts in SYNC_CELLS:
        a, b = recs[0][(shard, name)], recs[1][(shard, name)]
        assert torch.equal(bits(a["params"]), bits(b["params"])), f"{shard} {name}: replicas differ"
        assert all(t == STEPS for r in (a, b) for t in r["t"].values())
        if name not in sims:
            sims[name] = (_simulate_sync(world, opts),
                          _simulate_sync(world, dict(optimizer=opts["optimizer"])))
        ref, plain = sims[name]
        diff = float((a["params"] - ref).abs().max())
        assert torch.equal(bits(a["params"]), bits(ref)), f"{shard} {name}: max |diff| {diff}"
        assert not torch.equal(a["params"], plain), f"{shard} {name}: the options did nothing"


def _async_job(rank, world, port, outdir):
    _enter(rank, world, port)
    try:
        import torch.distributed as dist
        from ddl_amd.config import TrainConfig
        from ddl_amd.parallel.async_xgmi import AsyncPeerExchange
        from ddl_amd.parallel.comm import init_distributed
        from ddl_amd.parallel.roles import Trainer
        from ddl_amd.utils.data import synthetic_mnist
        env = init_distributed()
        assert env.device.index == 0
        data = synthetic_mnist(2000, 500, seed=5)
        out = {}
        for name, opts in ASYNC_CELLS:
            cfg = TrainConfig(mode="async", shard="contiguous", steps=STEPS, batch_size=BATCH,
                              eval_every=0, engine="hip", quiet=True, data_sharding="stride",
                              exchange_backend="xgmi", check_provenance=True, watchdog_s=120.0,
                              **opts)
            tr = Trainer(cfg, env, dataset=data)
            ex = tr.exchange
            assert isinstance(ex, AsyncPeerExchange) and ex.runner is not None
            init = tr.params.clone()
            ex.steps = STEPS
            ex.start()
            assert ex.service_mode == "host", ex.service_mode  # the board service
            torch.cuda.synchronize()
            dist.barrier()  # the ranks start together: their pushes do meet at the PS
            for i in range(STEPS):
                tr.train_step(i)
            ex.join()
            ex.verify_provenance()
            torch.cuda.synchronize()
            assert ex.peer.error() == 0, ex.peer.error()
            P = tr.plan.num_ps
            out[name] = {"init": init.cpu(), "params": tr.params.cpu(),
                         "ps": {p: dict(w=s.params.cpu(), m=s.m.cpu(),
                                        v=None if s.v is None else s.v.cpu(), t=s.t)
                                for p, s in tr.servers.items()},
                         "provenance": list(ex.provenance),
                         "ranges": [tr.plan.ps_segments(p)[0] for p in range(P)],
                         "hosts": [tr.plan.host_rank(p, world) for p in range(P)],
                         "offsets": list(tr.plan.tensor_offsets), "total": tr.plan.total,
                         "cfg": cfg.to_dict()}
            dist.barrier()
            ex.peer.unmap_peers()
            dist.barrier()
            ex.close()
            dist.barrier()
            del tr, ex
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


def _replay_async(recs, world, order, with_options):
    """The run again in this process in the recorded order: the engine's gradients and
    ops.update_flat, with or without the run's options."""
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.ops import native, rng
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    from ddl_amd.utils.data import batch_indices, synthetic_mnist
    dev = torch.device("cuda", 0)
    cfg = recs[0]["cfg"]
    data = synthetic_mnist(2000, 500, seed=5).to(dev)
    params = torch.zeros(recs[0]["total"], device=dev)
    grads = torch.zeros_like(params)
    eng = HipEngine(params, grads, recs[0]["offsets"], batch=BATCH, graph=False, eval_chunk=BATCH)
    # the service holds lr and the betas as float32 and widens them for Adam's step size; the
    # decay is formed from the doubles (update.h upd_decay)
    h = AdamHyper(lr=f32(cfg["lr"]), beta1=f32(0.9), beta2=f32(0.999))
    adam = cfg["optimizer"] == "adam"
    decay = cfg["lr"] * cfg["weight_decay"] if with_options else 0.0
    nesterov = bool(cfg["nesterov"]) and with_options

    def grad_fn(r, s, params_r):
        params.copy_(params_r)
        lo, hi = batch_indices(s, BATCH, data.total_batch, r, world, cfg["data_sharding"])
        eng.forward_backward(data.x_train[lo:hi], data.y_train[lo:hi], cfg["keep_prob"],
                             rng.step_seed(cfg["seed"], r, s))
        return grads.clone()

    def update_fn(p, st, g, t):
        if adam:
            native.ops().update_flat(ADAM, st.w, g, st.m, st.v, adam_coeffs(h, t), 0.9, 0.999,
                                     1e-8, 0.0, 1.0, decay, False)
        else:
            native.ops().update_flat(MOMENTUM, st.w, g, st.m, None, f32(cfg["lr"]), 0.0, 0.0, 0.0,
                                     cfg["momentum"], 1.0, decay, nesterov)

    out = ar.replay(order, recs[0]["ranges"], recs[0]["init"].to(dev), world, STEPS, grad_fn,
                    update_fn)
    torch.cuda.synchronize()
    return out


@pytest.mark.slow
def test_xgmi_async_service_with_options(tmp_path):
    world = 2
    _spawn(_async_job, world, free_port(), str(tmp_path))
    jobs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    for name, _ in ASYNC_CELLS:
        recs = [j[name] for j in jobs]
        hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
        assert torch.equal(recs[0]["init"], recs[1]["init"])
        log = [e for rec in recs for e in rec["provenance"]]
        assert len(log) == len(hosts) * world * STEPS  # the xGMI service logs every apply
        order = ar.apply_orders(log, world, STEPS)
        print(f"{name}: orders", {p: ar.order_string(o) for p, o in order.items()})
        params, state = _replay_async(recs, world, order, True)
        fails = []
        spans = [(lo, hi, f"range of PS {p}") for p, (lo, hi) in enumerate(ranges)]
        for r in range(world):
            fails += ar.mismatch_report(f"{name} worker {r}", recs[r]["params"], params[r].cpu(),
                                        spans)
            if not torch.equal(bits(recs[r]["params"]), bits(params[r].cpu())):
                fails.append(f"{name} worker {r}: buffer differs from the replay")
        for p in range(len(hosts)):
            got = recs[hosts[p]]["ps"][p]
            w, m, v, t = state[p]
            if got["t"] != t or t != world * STEPS:
                fails.append(f"{name} PS {p}: t {got['t']}, replay {t}")
            for what, a, b in (("params", got["w"], w), ("m", got["m"], m), ("v", got["v"], v)):
                if a is None:
                    assert what == "v" and recs[0]["cfg"]["optimizer"] != "adam"
                elif not torch.equal(bits(a), bits(b.cpu())):
                    fails.append(f"{name} PS {p} {what}: differs from the replay")
        assert not fails, "\n".join(fails[:30])
        plain, _ = _replay_async(recs, world, order, False)
        moved = max(float((a - b).abs().max()) for a, b in zip(plain, params))
        print(f"{name}: replay without the options: max |diff| {moved:.2e}")
        assert moved > 0.0
