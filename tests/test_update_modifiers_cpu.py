"""Decoupled weight decay (AdamW / SGDW) and Nesterov momentum on the CPU.

1. the fp64 closed form of tests/update_rule_reference.py against torch.optim.AdamW and
   torch.optim.SGD(nesterov=True) in fp64;
2. ParameterServer's pure-torch branches (fp32) against the closed form, one step at a time;
3. the config and the command line;
4. a gloo W = 2 sync job and an asynchronous replay cell with the options on;
5. resume with the options on."""
import argparse
import os

import pytest
import torch

import async_replay as ar
import test_async_replay_cpu as replay_cells
from conftest import free_port
from dist_helpers import spawn, train_rank
from onecard import rel_err
from update_rule_reference import update_closed_form

from ddl_amd.ops.adam import AdamHyper
from ddl_amd.parallel.ps import ParameterServer
from ddl_amd.parallel.sharding import make_plan

N = 1023
WD = 0.1
B1, B2, EPS, MU = 0.9, 0.999, 1e-8, 0.9
# the two option sets the issue names: AdamW, and Nesterov momentum with decay
ADAMW = dict(optimizer="adam", weight_decay=WD)
NESTEROV_WD = dict(optimizer="momentum", nesterov=True, weight_decay=WD)


def _span():
    """w, g, m, v of tests/test_update_rule_gpu.py's span."""
    torch.manual_seed(7)
    return (torch.randn(N), torch.randn(N) * 1e-2, torch.randn(N) * 1e-3, torch.rand(N) * 1e-4)


# ---- 1. the closed form against two independent fp64 implementations ----------------------------
def _grads64(k=4):
    gen = torch.Generator().manual_seed(3)
    return [torch.randn(N, generator=gen, dtype=torch.float64) * 1e-2 for _ in range(k)]


def _run_torch_optim(opt_cls, w0, grads, **kw):
    w = torch.nn.Parameter(w0.clone())
    opt = opt_cls([w], **kw)
    for g in grads:
        w.grad = g.clone()
        opt.step()
    return w.detach()


def test_closed_form_matches_torch_adamw():
    """TF's and PyTorch's Adam differ only in where eps sits, so both run with eps = 0."""
    w0 = _span()[0].double()
    grads = _grads64()
    z = torch.zeros(N, dtype=torch.float64)
    lr = 3e-4
    want = _run_torch_optim(torch.optim.AdamW, w0, grads, lr=lr, betas=(B1, B2), eps=0.0,
                            weight_decay=WD)
    got, _, _ = update_closed_form("adam", w0, z, z, grads, lr, b1=B1, b2=B2, eps=0.0,
                                   weight_decay=WD)
    err = float((got - want).abs().max())
    print(f"closed form vs torch.optim.AdamW: {err:.3e}")
    assert err < 1e-12
    off, _, _ = update_closed_form("adam", w0, z, z, grads, lr, b1=B1, b2=B2, eps=0.0)
    assert float((off - want).abs().max()) > 1e-5  # the decay is visible at this tolerance


def test_closed_form_matches_torch_sgd_nesterov():
    w0 = _span()[0].double()
    grads = _grads64()
    z = torch.zeros(N, dtype=torch.float64)
    lr = 3e-2
    want = _run_torch_optim(torch.optim.SGD, w0, grads, lr=lr, momentum=MU, nesterov=True)
    got, _, _ = update_closed_form("momentum", w0, z, None, grads, lr, mu=MU, nesterov=True)
    err = float((got - want).abs().max())
    print(f"closed form vs torch.optim.SGD(nesterov=True): {err:.3e}")
    assert err < 1e-12
    off, _, _ = update_closed_form("momentum", w0, z, None, grads, lr, mu=MU)
    assert float((off - want).abs().max()) > 1e-5


# ---- 2. ParameterServer's pure-torch branches ------------------------------------------------------
VARIANTS = [
    pytest.param("adam", 3e-4, MU, WD, False, id="adamw"),
    pytest.param("momentum", 3e-2, MU, WD, False, id="momentum-wd"),
    pytest.param("momentum", 3e-2, MU, 0.0, True, id="nesterov"),
    pytest.param("momentum", 3e-2, MU, WD, True, id="nesterov-wd"),
    pytest.param("sgd", 3e-2, 0.0, WD, False, id="sgd-wd"),
]



def check_step(tag, got, before, g, kind, lr, mu, wd, nesterov, scale, t0):
    """One step from the fp32 state `before` = (w, m, v): rel 1e-6 on m and v, abs 1e-6 on w."""
    w, m, v = got
    w_ref, m_ref, v_ref = update_closed_form(kind, *before, [g], lr, b1=B1, b2=B2, eps=EPS, mu=mu,
                                             weight_decay=wd, nesterov=nesterov, scale=scale,
                                             t0=t0)
    err_w = float((w.double() - w_ref).abs().max())
    err_m = rel_err(m, m_ref)
    print(f"{tag}: |w - ref| {err_w:.2e}  m rel {err_m:.2e}")
    assert err_w <= 1e-6, tag
    assert err_m <= 1e-6, tag
    if kind == "adam":
        err_v = rel_err(v, v_ref)
        print(f"{tag}: v rel {err_v:.2e}")
        assert err_v <= 1e-6, tag
    return w_ref


@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("optimizer,lr,mu,wd,nesterov", VARIANTS)
def test_parameter_server_torch_branches(optimizer, lr, mu, wd, nesterov, scale):
    w0, g0, m0, v0 = _span()
    plan = make_plan("none", 1)
    ps = ParameterServer(plan, 0, "cpu", AdamHyper(lr=lr, beta1=B1, beta2=B2, eps=EPS), optimizer,
                         MU, weight_decay=wd, nesterov=nesterov)
    plain = ParameterServer(plan, 0, "cpu", AdamHyper(lr=lr, beta1=B1, beta2=B2, eps=EPS),
                            optimizer, MU)
    kind = "adam" if optimizer == "adam" else "momentum"
    for s in (ps, plain):
        s.m[:N] = m0
        if s.v is not None:
            s.v[:N] = v0
    w, wp = w0.clone(), w0.clone()
    gen = torch.Generator().manual_seed(5)
    for k in range(3):
        g = g0 if k == 0 else torch.randn(N, generator=gen) * 1e-2
        before = (w.clone(), ps.m[:N].clone(), None if ps.v is None else ps.v[:N].clone())
        ps.begin()
        ps.apply(w, g, 0, scale)
        plain.begin()
        plain.apply(wp, g, 0, scale)
        got = (w, ps.m[:N], None if ps.v is None else ps.v[:N])
        if optimizer == "sgd":  # the pure-torch SGD branch keeps no m: the reference's is unused
            before = (before[0], torch.zeros(N), None)
            got = (w, scale * g, None)
        check_step(f"{optimizer} wd {wd} nesterov {nesterov} scale {scale:.3f} step {k}", got,
                   before, g, kind, lr, mu, wd, nesterov, scale, k)
    # the options are visible far above the tolerance
    assert float((w - wp).abs().max()) > 1e-4


# ---- 3. config and command line ------------------------------------------------------------------
def _parse(argv):
    from ddl_amd.config import add_args, from_args
    return from_args(add_args(argparse.ArgumentParser()).parse_args(argv))


def test_flags_parse_and_default_off():
    from ddl_amd.config import TrainConfig
    d = TrainConfig()
    assert d.weight_decay == 0.0 and d.nesterov is False
    cfg = _parse([])
    assert cfg.weight_decay == 0.0 and cfg.nesterov is False and cfg.momentum == d.momentum
    cfg = _parse(["--optimizer", "adam", "--weight-decay", "0.1"])
    assert cfg.weight_decay == 0.1 and not cfg.nesterov
    cfg = _parse(["--optimizer", "momentum", "--nesterov", "--weight-decay", "0.1", "--momentum",
                  "0.8"])
    assert cfg.nesterov and cfg.weight_decay == 0.1 and cfg.momentum == 0.8
    assert _parse(["--optimizer", "sgd", "--weight-decay", "0.5"]).weight_decay == 0.5


@pytest.mark.parametrize("argv,match", [
    (["--nesterov"], "--optimizer momentum"),
    (["--optimizer", "sgd", "--nesterov"], "--optimizer momentum"),
    (["--optimizer", "momentum", "--nesterov", "--momentum", "0"], "momentum above 0"),
    (["--weight-decay", "-0.1"], "negative"),
])
def test_refusals(argv, match):
    with pytest.raises(ValueError, match=match):
        _parse(argv)
    from ddl_amd.parallel import launch
    with pytest.raises(SystemExit):  # the entry point turns it into a usage error
        launch.main(argv)


def test_parameter_server_refuses_too():
    plan = make_plan("none", 1)
    with pytest.raises(ValueError, match="negative"):
        ParameterServer(plan, 0, "cpu", weight_decay=-1.0)
    with pytest.raises(ValueError, match="--optimizer momentum"):
        ParameterServer(plan, 0, "cpu", optimizer="adam", nesterov=True)


def test_momentum_flag_reaches_the_ps():
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    cfg = _parse(["--optimizer", "momentum", "--momentum", "0.7", "--nesterov", "--weight-decay",
                  "0.25", "--engine", "torch", "--steps", "1", "--batch-size", "10", "--quiet",
                  "--eval-every", "0"])
    tr = Trainer(cfg, DistEnv(), dataset=synthetic_mnist(100, 50, seed=7))
    assert tr.servers
    for ps in tr.servers.values():
        assert ps.momentum == 0.7 and ps.nesterov is True and ps.weight_decay == 0.25


# ---- 4. gloo W = 2: a sync job and an async replay cell ---------------------------------------------
SYNC = dict(mode="sync", shard="contiguous", steps=3, batch_size=50, eval_every=0, quiet=True,
            engine="torch", data="synthetic", watchdog_s=120.0)


def _sync_run(tmp, **kw):
    os.makedirs(tmp, exist_ok=True)
    spawn(train_rank, 2, free_port(), dict(SYNC, **kw), str(tmp))
    return [torch.load(os.path.join(tmp, f"rank{r}.pt"), weights_only=False) for r in range(2)]


@pytest.mark.slow
@pytest.mark.parametrize("opts", [ADAMW, NESTEROV_WD], ids=["adamw", "nesterov-wd"])
def test_gloo_sync_replicas_equal_and_options_matter(tmp_path, opts):
    on = _sync_run(tmp_path / "on", **opts)
    off = _sync_run(tmp_path / "off", optimizer=opts["optimizer"])
    assert torch.equal(on[0]["params"], on[1]["params"])
    assert torch.equal(off[0]["params"], off[1]["params"])
    moved = float((on[0]["params"] - off[0]["params"]).abs().max())
    print(f"options on vs off: max |diff| {moved:.2e}")
    assert moved > 0.0
    assert on[0]["ps_t"] == off[0]["ps_t"]


def _update_with(opts, lr):
    """The rule written out in fp32 torch for the replay (the forms of ParameterServer.apply):
    that class is under test, so the replay does not call it."""
    decay = lr * opts.get("weight_decay", 0.0)

    def update(p, st, g, t):
        if decay:
            st.w.sub_(st.w, alpha=decay)
        if opts["optimizer"] == "adam":
            st.m.add_((g - st.m) * (1.0 - B1))
            st.v.add_((g * g - st.v) * (1.0 - B2))
            st.w.sub_(replay_cells.adam_step_size(t, lr) * st.m / (st.v.sqrt() + EPS))
        else:
            st.m.mul_(MU).add_(g, alpha=1.0)
            if opts.get("nesterov"):
                st.w.sub_(lr * (MU * st.m + g * 1.0))
            else:
                st.w.sub_(lr * st.m)
    return update


@pytest.mark.slow
@pytest.mark.parametrize("opts", [ADAMW, NESTEROV_WD], ids=["adamw", "nesterov-wd"])
def test_gloo_async_run_equals_its_replay(tmp_path, opts, monkeypatch):
    world, steps = 2, replay_cells.STEPS
    kw = dict(shard="contiguous", **opts)
    spawn(replay_cells._gloo_rank, world, free_port(), str(tmp_path), kw, ())
    recs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
            for r in range(world)]
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    log = [e for rec in recs for e in rec["provenance"]]
    order = ar.apply_orders(log, world, steps, hosts=hosts)
    lr = recs[0]["cfg"]["lr"]

    def replay(update):
        monkeypatch.setitem(replay_cells.UPDATES, opts["optimizer"], update)
        return replay_cells.replay_gloo(recs, world, order)

    params, state = replay(_update_with(opts, lr))
    for r in range(world):
        assert torch.equal(recs[r]["params"], params[r]), f"worker {r}"
    for p in range(len(hosts)):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        assert got["t"] == t == world * steps
        assert torch.equal(got["w"], w) and torch.equal(got["m"], m)
        if got["v"] is not None:
            assert torch.equal(got["v"], v)
    # the same orders replayed with the options off give another result
    plain, _ = replay(_update_with(dict(optimizer=opts["optimizer"]), lr))
    moved = max(float((a - b).abs().max()) for a, b in zip(plain, params))
    print(f"replay with the options off: max |diff| {moved:.2e}")
    assert moved > 0.0


# ---- 5. resume ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [ADAMW, NESTEROV_WD], ids=["adamw", "nesterov-wd"])
def test_resume_with_options_is_bit_identical(tmp_path, opts):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist

    def train(tmp, **kw):
        cfg = dict(mode="sync", shard="contiguous", num_ps=3, steps=6, batch_size=20,
                   eval_every=0, engine="torch", quiet=True, checkpoint_dir=str(tmp), **opts)
        cfg.update(kw)
        tr = Trainer(TrainConfig(**cfg), DistEnv(), dataset=synthetic_mnist(400, 100, seed=11))
        tr.train()
        return tr

    full = train(tmp_path / "full")
    part = train(tmp_path / "cut", max_steps=3)
    assert part.global_step == 3
    res = train(tmp_path / "cut", resume=True)
    assert res.global_step == 6
    assert torch.equal(res.params, full.params)
    for p, ps in full.servers.items():
        q = res.servers[p]
        assert q.t == ps.t == 6 and torch.equal(q.m, ps.m)
        assert (q.v is None and ps.v is None) or torch.equal(q.v, ps.v)
    off = train(tmp_path / "off", weight_decay=0.0, nesterov=False)
    assert not torch.equal(off.params, full.params)
