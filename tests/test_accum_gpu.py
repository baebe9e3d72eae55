"""Gradient accumulation over K micro-batches on the GPU (csrc/kernels/accum.hip, --accum-steps)
against its CPU twin (ddl_amd/ops/accum.py), bit for bit.

a. the kernel alone: every mode at every size where the code takes another path (one lane, a
   ragged vector, whole passes, one chunk more or less, several chunks), at an aligned and a
   misaligned base, K = 2, 3, 5; the 14-range plan table with poisoned padding in g and in A, at
   every grid size; -0.0, denormals and one inf among the inputs;
b. the W = 1 native sync step: the gradient buffer after a step is the twin's accumulation of
   the three micro-batches' engine gradients, the update is the stand-alone update of that
   buffer, a non-final micro-batch makes no update launch, and K = 1 changes no bit;
c. K = 2 at B = 4 against one B = 8 step on the same 8 images (keep_prob 1), both against the
   fp64 references of tests/op_reference.py under the gradient tolerance of
   tests/test_hip_kernels.py;
d. the clip on top: twin accumulate, then twin clip, {norm, coef} bit-equal;
e. the exchanges on one card: xGMI sync at W = 2 and the forced 1-rank RCCL rehearsal against
   the one-process PS simulation fed each rank's effective gradient; xGMI async in line (W = 1)
   and on the board (W = 2) against the replay of the recorded apply orders.

Every pass is one float32 operation per rounding on both sides, so equality is demanded.
"""
import numpy as np
import pytest
import torch

from ddl_amd.ops import accum as A
from ddl_amd.ops import clip as C
from ddl_amd.ops import native

import onecard as oc
from onecard import f32
from oracle_common import host_bits as bits

pytestmark = pytest.mark.gpu

CH = C.CHUNK
DEV = torch.device("cuda", 0)
KS = [2, 3, 5]


def same_pair(got, want):
    return bits(torch.tensor(got, dtype=torch.float32)).tolist() == \
        bits(torch.tensor(want, dtype=torch.float32)).tolist()


# ---- a. the kernel alone ---------------------------------------------------------------------------
SIZES = [1, 3, 4, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 5]
PAD = 1e30


@pytest.fixture(scope="module")
def noise():
    """Five micro-batch gradients of 3 CH + 16 elements with -0.0, denormals (and sums that land
    among them) and, in the first one only, one inf.  No NaN: inf meets only finite values."""
    g = torch.Generator().manual_seed(21)
    n = 3 * CH + 16
    out = []
    for j in range(5):
        x = torch.randn(n, generator=g) * (10.0 ** (j - 2))
        x[j::97] = -0.0
        x[5 + j::89] = 1e-41 * (j + 1)          # denormals
        x[40 + j::83] = -3e-39 * (j + 1)
        out.append(x)
    for j, x in enumerate(out):
        x[2] = -0.0                               # -0.0 in every micro-batch: stays -0.0
        x[3] = 1e-41 * (j + 1)                    # denormal sums, and their mean
    out[0][1] = float("inf")
    return out


def twin_passes(gs, ranges, total, k):
    """The twin on buffers with PAD outside the ranges: (g, A) after micro-batch j, for every j."""
    buf, acc = torch.full((total,), PAD), torch.full((total,), PAD)
    seen = []
    for j in range(k):
        for lo, n in ranges:
            buf[lo:lo + n] = gs[j][lo:lo + n]
        A.accum_grads_(buf, acc, ranges, A.mode_of(j, k), k)
        seen.append((buf.clone(), acc.clone()))
    return seen


def gpu_passes(gs, ranges, total, k, max_grid=0):
    buf = torch.full((total,), PAD, device=DEV)
    acc = torch.full((total,), PAD, device=DEV)
    seen = []
    for j in range(k):
        for lo, n in ranges:
            buf[lo:lo + n] = gs[j][lo:lo + n].to(DEV)
        native.ops().accum_grads(buf, acc, ranges, A.mode_of(j, k), k, max_grid)
        torch.cuda.synchronize()
        seen.append((buf.cpu(), acc.cpu()))
    return seen


def check_passes(gs, ranges, total, k, max_grid=0):
    want = twin_passes(gs, ranges, total, k)
    got = gpu_passes(gs, ranges, total, k, max_grid)
    for j, ((gb, ga), (wb, wa)) in enumerate(zip(got, want)):
        assert torch.equal(bits(gb), bits(wb)), (k, j, "g")
        assert torch.equal(bits(ga), bits(wa)), (k, j, "A")
    return got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("base", [0, 1])
def test_single_range(noise, n, base):
    """One range of n elements at an aligned and a misaligned base, every K and with it every
    mode: g and A after every pass equal the twin's, the elements around the range included."""
    total = base + n + 3
    neg0 = int(bits(torch.tensor([-0.0]))[0])
    for k in KS:
        got = check_passes(noise, [(base, n)], total, k)
        if base + n > 2 >= base:
            assert int(bits(got[-1][0])[2]) == neg0          # -0.0 + ... + -0.0, times r
        if base + n > 1 >= base:
            assert float(got[-1][0][1]) == float("inf")
        assert not bool(torch.isnan(got[-1][0]).any())


def plan_table():
    from ddl_amd.parallel.sharding import make_plan
    plan = make_plan("none", 1)
    return C.payload_ranges(plan.tensor_offsets), plan.total


@pytest.fixture(scope="module")
def plan_noise():
    _, total = plan_table()
    g = torch.Generator().manual_seed(22)
    out = [torch.randn(total, generator=g) * (0.1 ** j) for j in range(3)]
    for j, x in enumerate(out):
        x[j::1001] = -0.0
        x[7 + j::997] = 2e-42
    return out


def test_plan_table_poisoned_padding_and_grid_sizes(plan_noise):
    """The 14 ranges of the real plan, 1e30 in every padding element of g and of A: found there
    unchanged after every pass, and max_grid 1, 7 and the default give the same bits (K = 3)."""
    ranges, total = plan_table()
    assert len(ranges) == 14
    mask = torch.ones(total, dtype=torch.bool)
    for lo, n in ranges:
        mask[lo:lo + n] = False
    assert bool(mask.any())
    res = [check_passes(plan_noise, ranges, total, 3, mg) for mg in (1, 7, 0)]
    for got in res:
        for gb, ga in got:
            assert bool((gb[mask] == PAD).all()) and bool((ga[mask] == PAD).all())
    for got in res[1:]:
        for (gb, ga), (wb, wa) in zip(got, res[0]):
            assert torch.equal(bits(gb), bits(wb)) and torch.equal(bits(ga), bits(wa))


def test_refusals():
    ops = native.ops()
    g = torch.zeros(64, device=DEV)
    a = torch.zeros(64, device=DEV)
    for bad in (dict(mode=3), dict(mode=-1), dict(k=1), dict(k=0)):
        kw = dict(mode=1, k=2)
        kw.update(bad)
        with pytest.raises((RuntimeError, ValueError)):
            ops.accum_grads(g, a, [(0, 64)], kw["mode"], kw["k"])
    with pytest.raises((RuntimeError, ValueError)):
        ops.accum_grads(g, torch.zeros(63, device=DEV), [(0, 63)], 1, 2)
    with pytest.raises((RuntimeError, ValueError)):
        ops.accum_grads(g, a, [(60, 8)], 1, 2)              # past the end
    with pytest.raises((RuntimeError, ValueError)):
        ops.accum_grads(g, g, [(0, 64)], 1, 2)              # A is g
    with pytest.raises((RuntimeError, ValueError)):
        ops.accum_grads(g[1:33], a[2:34], [(0, 32)], 1, 2)  # other 16-byte alignment
    torch.cuda.synchronize()


# ---- b. the W = 1 native step -------------------------------------------------------------------------
RULES = {
    "adam": dict(optimizer="adam"),
    "nesterov-wd": dict(optimizer="momentum", momentum=0.9, nesterov=True, weight_decay=0.01),
}
LR = 1e-2


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(n_train=400, n_test=100, seed=5)


def make_trainer(data, B, opts, K, steps=2, **kw):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    cfg = TrainConfig(mode="sync", shard="flat", steps=steps, batch_size=B, eval_every=0,
                      engine="hip", quiet=True, lr=LR, seed=0, accum_steps=K, **dict(opts, **kw))
    return Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=data)


def micro_engine_grads(tr, eng2, params2, grads2, step, gstep):
    """The K single-batch engine gradients of step index `step` at global step `gstep`, from the
    trainer's current parameters, on an engine of their own (CPU copies)."""
    from ddl_amd.ops import rng
    cfg = tr.cfg
    K = cfg.accum_steps
    params2.copy_(tr.params)
    out = []
    for j in range(K):
        x, y = tr.batch(step * K + j)
        eng2.forward_backward(x, y, cfg.keep_prob, rng.step_seed(cfg.seed, 0, gstep * K + j))
        torch.cuda.synchronize()
        out.append(grads2.cpu())
    return out


def twin_effective(gs, ranges, total):
    k = len(gs)
    buf, acc = torch.zeros(total), torch.zeros(total)
    for j, g in enumerate(gs):
        buf.copy_(g)
        A.accum_grads_(buf, acc, ranges, A.mode_of(j, k), k)
    return buf


def state_of(tr):
    return [(s.m.clone(), None if s.v is None else s.v.clone())
            for _, s in sorted(tr.servers.items())]


def same_state(a, b):
    ok = True
    for (ma, va), (mb, vb) in zip(a, b):
        ok &= torch.equal(bits(ma), bits(mb))
        if va is not None:
            ok &= torch.equal(bits(va), bits(vb))
    return ok


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("B", [5, 33])
def test_native_step_w1(data, B, rule):
    import step_audit as SA
    from ddl_amd.models import engine_segments
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.ops import rng
    opts = RULES[rule]
    ops = native.ops()
    K = 3
    tr = make_trainer(data, B, opts, K)
    assert tr.accum_buf is not None and tr.exchange.native
    ranges = tr.clip_ranges
    total = tr.plan.total
    params2 = torch.zeros(total, device=DEV)
    grads2 = torch.zeros(total, device=DEV)
    eng2 = HipEngine(params2, grads2, tr.plan.tensor_offsets, batch=B, graph=False, eval_chunk=B)
    segs = [set(s) for s in engine_segments("hip", DEV)]
    merged = SA.segment_pieces(tr.exchange.units, segs, overlap=False)[1]
    adam = opts["optimizer"] == "adam"
    h = next(iter(tr.servers.values())).h
    W = tr.params.clone()
    M = torch.zeros_like(W)
    V = torch.zeros_like(W) if adam else None
    runner = tr.exchange.runner
    for step in range(2):
        gs = micro_engine_grads(tr, eng2, params2, grads2, step, tr.global_step)
        want_g = twin_effective(gs, ranges, total)
        if step == 0:
            # by hand, as Trainer.train_step drives it: no update launch after a non-final one
            for j in range(K):
                x, y = tr.batch(step * K + j)
                seed = rng.step_seed(tr.cfg.seed, 0, tr.global_step * K + j)
                if j < K - 1:
                    tr.exchange.accumulate(x, y, tr.cfg.keep_prob, seed)
                    assert runner.update_launches() == 0
                    assert all(s.t == 0 for s in tr.servers.values())
                else:
                    tr.exchange.step(x, y, tr.cfg.keep_prob, seed)
            tr.global_step += 1
        else:
            tr.train_step(step)
        torch.cuda.synchronize()
        assert runner.update_launches() == len(merged)
        assert all(s.t == step + 1 for s in tr.servers.values())
        got_g = tr.grads.cpu()
        for lo, n in ranges:   # (the padding is outside the contract)
            assert torch.equal(bits(got_g[lo:lo + n]), bits(want_g[lo:lo + n])), (step, lo)
        # ... and the update is the stand-alone update of that buffer, from the same state
        G = tr.grads.clone()
        stepsz = ops.adam_step_size(LR, h.beta1, h.beta2, step + 1) if adam else LR
        ops.update_flat(0 if adam else 1, W, G, M, V, stepsz, h.beta1, h.beta2, h.eps,
                        opts.get("momentum", 0.0), 1.0, LR * opts.get("weight_decay", 0.0),
                        opts.get("nesterov", False))
        torch.cuda.synchronize()
        for u in tr.exchange.units:
            srv = tr.servers[u.ps]
            for (lo, hi), off in zip(u.ranges, u.state_offs or [0] * len(u.ranges)):
                assert torch.equal(bits(tr.params[lo:hi]), bits(W[lo:hi]))
                assert torch.equal(bits(srv.m[off:off + hi - lo]), bits(M[lo:hi]))
                if adam:
                    assert torch.equal(bits(srv.v[off:off + hi - lo]), bits(V[lo:hi]))
    # a micro-batch out of turn is refused
    x, y = tr.batch(0)
    with pytest.raises((RuntimeError, ValueError)):
        tr.exchange.step(x, y, tr.cfg.keep_prob, 1)
    tr.exchange.close()


@pytest.mark.parametrize("rule", sorted(RULES))
def test_k1_changes_no_bit(data, rule):
    """K = 1: the trainer never calls set_accum and runs today's step (the update in the backward
    launches' tails, update_launches() 0); calling set_accum(1, ..) changes nothing either."""
    opts = RULES[rule]
    runs = []
    for explicit in (False, True):
        tr = make_trainer(data, 5, opts, 1)
        assert tr.accum_buf is None
        if explicit:
            tr.exchange.runner.set_accum(1, tr.clip_ranges, None)
        for i in range(2):
            tr.train_step(i)
        torch.cuda.synchronize()
        assert tr.exchange.runner.update_launches() == 0
        with pytest.raises((RuntimeError, ValueError)):
            tr.exchange.accumulate(*tr.batch(0), tr.cfg.keep_prob, 1)
        runs.append((tr.params.clone(), tr.grads.clone(), state_of(tr)))
        tr.exchange.close()
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0]))
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    assert same_state(runs[0][2], runs[1][2])


# ---- c. K = 2 at B = 4 against one step at B = 8 ------------------------------------------------------------
def reference_step_keep1(P, x, labels, dtype=torch.float64):
    """tests/step_audit.py chained_step at keep_prob 1 (that one pins 0.5): the references of
    tests/op_reference.py chained in the engine's op order."""
    import op_reference as R
    Pd = [p.to(dtype) for p in P]
    buf = {"x": x.to(dtype)}
    for op in range(6):
        buf.update(R.run_op(op, Pd, buf, 0, 1.0, True, dtype=dtype))
    hd = R.head(buf["h2"], Pd[12], Pd[13], labels, None, 1.0, dtype=dtype)
    buf.update(loss=hd["loss"], dlog=hd["dlog"], dpre2fc=hd["dpre2fc"], g12=hd["gw"],
               g13=hd["gb"])
    for op in range(6, R.OP_COUNT):
        buf.update(R.run_op(op, Pd, buf, 0, 1.0, True, dtype=dtype))
    return buf


def test_two_micro_batches_are_the_large_batch(data):
    """keep_prob 1, the same 8 images: K = 2 at B = 4 and one B = 8 step differ only by summation
    order.  Each against the fp64 references, under tests/test_hip_kernels.py's gradient bound
    (max |difference| over max |reference| per tensor: 5e-5 for the fc and head tensors, 5e-3
    for the conv ones)."""
    from ddl_amd.models.layout import TENSORS
    grads = {}
    for name, B, K in (("accumulated", 4, 2), ("large", 8, 1)):
        tr = make_trainer(data, B, RULES["adam"], K, steps=1, keep_prob=1.0)
        offs = tr.plan.tensor_offsets
        P = [tr.params[offs[t.index]:offs[t.index] + t.numel].cpu().view(t.shape) for t in TENSORS]
        xs = torch.cat([tr.batch(j)[0] for j in range(K)]).cpu()
        ys = torch.cat([tr.batch(j)[1] for j in range(K)]).cpu()
        tr.train_step(0)
        torch.cuda.synchronize()
        grads[name] = (tr.grads.cpu(), offs, P, xs, ys)
        tr.exchange.close()
    assert torch.equal(grads["accumulated"][3], grads["large"][3])       # the same 8 images
    assert all(torch.equal(a, b) for a, b in zip(grads["accumulated"][2], grads["large"][2]))
    _, _, P, xs, ys = grads["large"]
    ref = reference_step_keep1(P, xs, ys)
    for name, (g, offs, _, _, _) in grads.items():
        for t in TENSORS:
            o = offs[t.index]
            r = ref[f"g{t.index}"].reshape(-1)
            err = float((g[o:o + t.numel].double() - r).abs().max() / (r.abs().max() + 1e-30))
            tol = 5e-5 if t.index > 7 else 5e-3
            print(f"{name} {t.name}: {err:.3g} (bound {tol})")
            assert err < tol, (name, t.name, err)


# ---- d. the clip on top ------------------------------------------------------------------------------------
def test_clip_reads_the_effective_gradient(data):
    """K = 2 with clip_norm at half the effective gradient's norm: the buffer is the twin
    accumulate followed by the twin clip, {norm, coef} bit for bit."""
    from ddl_amd.models.hip_engine import HipEngine
    B, K = 5, 2
    probe = make_trainer(data, B, RULES["adam"], K, steps=1)
    ranges, total = probe.clip_ranges, probe.plan.total
    params2 = torch.zeros(total, device=DEV)
    grads2 = torch.zeros(total, device=DEV)
    eng2 = HipEngine(params2, grads2, probe.plan.tensor_offsets, batch=B, graph=False,
                     eval_chunk=B)
    gs = micro_engine_grads(probe, eng2, params2, grads2, 0, 0)
    probe.exchange.close()
    eff = twin_effective(gs, ranges, total)
    norm, _ = C.grad_norm_coef(eff, ranges, 1.0)
    assert norm > 0 and np.isfinite(norm)
    c = f32(0.5 * norm)
    want = eff.clone()
    pair = C.clip_grads_(want, ranges, c)
    assert pair[1] < 1.0
    tr = make_trainer(data, B, RULES["adam"], K, steps=1, clip_norm=c)
    tr.train_step(0)
    torch.cuda.synchronize()
    got = tr.grads.cpu()
    print("pair", tuple(tr.clip_out.tolist()), "twin", pair)
    assert same_pair(tuple(tr.clip_out.tolist()), pair)
    for lo, n in ranges:
        assert torch.equal(bits(got[lo:lo + n]), bits(want[lo:lo + n]))
    tr.exchange.close()


# ---- e. the exchanges on one card ---------------------------------------------------------------------------
# Worker processes share the one GPU (tests/onecard.py).  At most two workers beside this
# process, each job under one time limit.
LIMIT_S = 150
XB, XK, XSTEPS, ASTEPS = 5, 2, 2, 4


def _sync_rank(rank, world, port, outdir, kw):
    """One rank of an accumulated synchronous run on the xGMI exchange: XSTEPS steps of XK
    micro-batches of XB."""
    import os
    with oc.rank_session(rank, world, port) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "sync", XSTEPS, XB, synthetic_mnist(400, 100, seed=5),
                             accum_steps=XK, **kw)
        rec = oc.sync_rank_record(tr, XSTEPS, per_step=oc.sync_each_step)
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        me.close_single(tr.exchange)


def effective_grad(K, total, ranges):
    """A grad_hook: rank r's effective gradient of step s into the engine's gradient buffer (K
    micro-batches, each on its own batch and dropout seed, through the kernel tested in a)."""
    acc = torch.zeros(total, device=DEV)

    def hook(ge, r, s):
        for j in range(K):
            ge.backward(r, s * K + j, s * K + j)
            if K > 1:
                native.ops().accum_grads(ge.grads, acc, ranges, A.mode_of(j, K), K)
    return hook


_SIM = {}


def simulate_sync(world, K=XK, steps=XSTEPS):
    """The one-process PS simulation (onecard.simulate_sync) fed every rank's effective gradient:
    one native Adam step per step — steps, not micro-batches."""
    if (world, K) not in _SIM:
        from ddl_amd.parallel.sharding import make_plan
        plan = make_plan("none", 1)
        hook = effective_grad(K, plan.total, C.payload_ranges(plan.tensor_offsets))
        _SIM[(world, K)] = oc.simulate_sync(world, steps, XB, oc.dataset_on_card(400, 100), plan,
                                            grad_hook=hook)
    return _SIM[(world, K)]


@pytest.mark.slow
@pytest.mark.parametrize("shard", ["flat", "contiguous"])
def test_xgmi_sync_w2(tmp_path, shard):
    """Sync W = 2 over xGMI on one card, K = 2, 2 steps of B = 5: the replicas agree bit for bit
    and equal the simulation fed each rank's effective gradient; every PS counted 2 steps."""
    from conftest import free_port
    want = simulate_sync(2)
    oc.run_ranks(_sync_rank, 2, free_port(), str(tmp_path), dict(shard=shard), limit_s=LIMIT_S)
    recs = oc.load_ranks(tmp_path, 2)
    assert torch.equal(bits(recs[0]["params"]), bits(recs[1]["params"]))
    for rec in recs:
        assert rec["steps"] == XSTEPS and all(t == XSTEPS for t in rec["t"].values())
    assert torch.equal(bits(recs[0]["params"]), bits(want))
    assert not torch.equal(bits(want), bits(simulate_sync(2, K=1)))


def test_forced_rccl_rehearsal_w1():
    """The forced 1-rank RCCL rehearsal, K = 2: equals the simulation at W = 1."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    want = simulate_sync(1)
    cfg = TrainConfig(mode="sync", shard="flat", steps=XSTEPS, batch_size=XB, eval_every=0,
                      engine="hip", quiet=True, data_sharding="stride", force_collectives=True,
                      accum_steps=XK)
    tr = Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=synthetic_mnist(400, 100, seed=5))
    assert tr.exchange.native and tr.exchange.backend == "rccl"
    for i in range(XSTEPS):
        tr.train_step(i)
        torch.cuda.synchronize()
    got = oc.canon(tr.params, tr.plan.tensor_offsets).cpu()
    assert all(s.t == XSTEPS for s in tr.servers.values())
    tr.exchange.close()
    assert torch.equal(bits(got), bits(want))


def _async_rank(rank, world, port, outdir, kw):
    """One rank of an accumulated asynchronous run on the xGMI data plane, ASTEPS steps (W = 1
    takes the in-line applies)."""
    import os
    with oc.rank_session(rank, world, port) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "async", ASTEPS, XB, synthetic_mnist(2000, 500, seed=5),
                             accum_steps=XK, **kw)
        assert tr.exchange.runner is not None

        def started(ex):
            assert ex.inline == (world == 1)

        rec = oc.async_rank_record(tr, world, ASTEPS, per_step=oc.sync_each_step,
                                   after_start=started)
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        me.close_single(tr.exchange)


@pytest.mark.slow
@pytest.mark.parametrize("world,kw", [
    pytest.param(1, dict(shard="flat", num_ps=3), id="1-inline"),
    pytest.param(2, dict(shard="contiguous"), id="2-board"),
])
def test_xgmi_async_equals_its_replay(tmp_path, world, kw):
    """Async over xGMI, K = 2, 4 steps, W = 1 in-line applies and W = 2 on the arrival board: the
    run equals the replay of its recorded apply orders with a gradient function that accumulates;
    every PS applied W * 4 pushes and logged one provenance row per step, worker and PS."""
    import async_replay as ar
    from conftest import free_port
    oc.run_ranks(_async_rank, world, free_port(), str(tmp_path), kw, limit_s=LIMIT_S)
    recs = oc.load_ranks(tmp_path, world)
    rows, order = oc.recorded_orders(recs, world, ASTEPS)
    assert len(rows) == world * ASTEPS * len(recs[0]["hosts"])
    assert all(rec["steps"] == ASTEPS for rec in recs)
    print("orders", {p: ar.order_string(o) for p, o in order.items()})
    table = C.payload_ranges(recs[0]["offsets"])
    want, state = oc.replay_async(recs, world, order, ASTEPS,
                                  grad_hook=effective_grad(XK, recs[0]["total"], table))
    oc.assert_payload_equals_replay(recs, world, want, state, table)
    assert all(t == world * ASTEPS for (_, _, _, t) in state.values())
