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

import pytest
import torch

import async_replay as ar
import onecard as oc
from conftest import free_port
from onecard import PLACEMENTS, f32, rel_err
from onecard import assert_same_run as _assert_same
from oracle_common import bits
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
    """onecard.placement_run at STEPS steps of BATCH."""
    return oc.placement_run(data, opts, shard, STEPS, BATCH, tail, final, setup)


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
JOB_ENV = dict(DDL_ASYNC_INLINE="0")
SYNC_CELLS = [(shard, name, opts) for shard in ("flat", "contiguous")  # contiguous: owner buckets
              for name, opts in (("adamw", ADAMW), ("nesterov-wd", NESTEROV_WD))]
ASYNC_CELLS = [("adamw", ADAMW), ("nesterov-wd", NESTEROV_WD)]


def _sync_job(rank, world, port, outdir):
    with oc.rank_session(rank, world, port, env=JOB_ENV, on_device_0=True) as me:
        from ddl_amd.utils.data import synthetic_mnist
        data = synthetic_mnist(2000, 500, seed=5)
        out = {}
        for shard, name, opts in SYNC_CELLS:
            tr = oc.xgmi_trainer(me.env, "sync", STEPS, BATCH, data, shard=shard, **opts)
            ex = tr.exchange
            owner = shard != "flat"
            assert all((ex.peer.owner(b) >= 0) == owner for b in range(len(ex.peer.nslices())))
            rec = oc.sync_rank_record(tr, STEPS)
            assert ex.peer.error() == 0, ex.peer.error()
            out[(shard, name)] = dict(params=rec["params"], t=rec["t"])
            me.close_one_of_several(ex)
            del tr, ex
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))


def _simulate_sync(world, opts):
    """onecard.simulate_sync with one update_flat with the options per global step."""
    from ddl_amd.models import engine_segments
    from ddl_amd.ops import native
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    from ddl_amd.parallel.sharding import make_plan
    plan = make_plan("flat", world, buckets=engine_segments("hip", torch.device("cuda", 0)))
    h = AdamHyper()
    adam = opts["optimizer"] == "adam"
    decay = h.lr * opts.get("weight_decay", 0.0)

    def update(params, acc, m, v, step):
        if adam:
            native.ops().update_flat(ADAM, params, acc, m, v, adam_coeffs(h, step + 1), h.beta1,
                                     h.beta2, h.eps, 0.0, 1.0, decay, False)
        else:
            native.ops().update_flat(MOMENTUM, params, acc, m, None, h.lr, 0.0, 0.0, 0.0, MU, 1.0,
                                     decay, bool(opts.get("nesterov", False)))

    return oc.simulate_sync(world, STEPS, BATCH, oc.dataset_on_card(2000, 500), plan,
                            update=update)


@pytest.mark.slow
def test_xgmi_sync_exchange_with_options(tmp_path):
    world = 2
    oc.run_ranks(_sync_job, world, free_port(), str(tmp_path), limit_s=JOB_LIMIT_S)
    recs = oc.load_ranks(tmp_path, world)
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
    with oc.rank_session(rank, world, port, env=JOB_ENV, on_device_0=True) as me:
        from ddl_amd.utils.data import synthetic_mnist
        data = synthetic_mnist(2000, 500, seed=5)
        out = {}

        def started(ex):
            assert ex.service_mode == "host", ex.service_mode  # the board service

        for name, opts in ASYNC_CELLS:
            tr = oc.xgmi_trainer(me.env, "async", STEPS, BATCH, data, shard="contiguous", **opts)
            ex = tr.exchange
            assert ex.runner is not None
            out[name] = oc.async_rank_record(tr, world, STEPS, after_start=started)
            me.close_one_of_several(ex)
            del tr, ex
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))


def _replay_async(recs, world, order, with_options):
    """onecard.replay_async with or without the run's options."""
    from ddl_amd.ops import native
    from ddl_amd.ops.adam import adam_coeffs

    def update(st, g, t, h, cfg):
        decay = cfg["lr"] * cfg["weight_decay"] if with_options else 0.0
        if cfg["optimizer"] == "adam":
            native.ops().update_flat(ADAM, st.w, g, st.m, st.v, adam_coeffs(h, t), 0.9, 0.999,
                                     1e-8, 0.0, 1.0, decay, False)
        else:
            native.ops().update_flat(MOMENTUM, st.w, g, st.m, None, f32(cfg["lr"]), 0.0, 0.0, 0.0,
                                     cfg["momentum"], 1.0, decay,
                                     bool(cfg["nesterov"]) and with_options)

    return oc.replay_async(recs, world, order, STEPS, update=update)


@pytest.mark.slow
def test_xgmi_async_service_with_options(tmp_path):
    world = 2
    oc.run_ranks(_async_job, world, free_port(), str(tmp_path), limit_s=JOB_LIMIT_S)
    jobs = oc.load_ranks(tmp_path, world)
    for name, _ in ASYNC_CELLS:
        recs = [j[name] for j in jobs]
        assert torch.equal(recs[0]["init"], recs[1]["init"])
        _, order = oc.recorded_orders(recs, world, STEPS)
        print(f"{name}: orders", {p: ar.order_string(o) for p, o in order.items()})
        params, state = _replay_async(recs, world, order, True)
        spans = [(lo, hi, f"PS {p} / its range") for p, (lo, hi) in enumerate(recs[0]["ranges"])]
        fails = oc.replay_mismatches(recs, world, params, state, spans, tag=f"{name} ")
        fails += [f"{name} PS {p}: t {t}, not {world * STEPS}" for p, (_, _, _, t) in state.items()
                  if t != world * STEPS]
        assert not fails, "\n".join(fails[:30])
        plain, _ = _replay_async(recs, world, order, False)
        moved = max(float((a - b).abs().max()) for a, b in zip(plain, params))
        print(f"{name}: replay without the options: max |diff| {moved:.2e}")
        assert moved > 0.0
