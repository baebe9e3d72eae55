"""Clipping by the global norm on the GPU (csrc/kernels/clip.hip) against its CPU twin
(ddl_amd/ops/clip.py), bit for bit.

a. the two kernels alone: {norm, coef} and the scaled buffer equal the twin's at every size where
   the code takes another path (one lane, a ragged vector, a whole pass, one chunk more or less,
   more partials than the final reduce has lanes), at aligned and misaligned bases, on a table
   shaped like the real plan with poisoned padding, at every grid size, twice on one ticket;
b. the W = 1 native step: the clipped step's gradient buffer is fl(g * coef) of the unclipped
   step's, its update is the stand-alone update of that buffer, a clip norm above the gradient's
   changes no bit, and update_launches() counts the coalesced stand-alone updates;
c. the exchanges on one card: xGMI sync at W = 2 (flat and contiguous plans) and the forced
   1-rank RCCL rehearsal against a one-process PS simulation fed with each rank's own clipped
   gradient, xGMI async in line (W = 1) and on the board (W = 2) against the replay of the
   recorded apply orders.

Both sides widen to float64 and add exact squares in one pinned order, so equality is demanded,
not a tolerance.
"""
import numpy as np
import pytest
import torch

from ddl_amd.ops import clip as C
from ddl_amd.ops import native

import onecard as oc
from onecard import f32
from oracle_common import host_bits as bits

pytestmark = pytest.mark.gpu

CH = C.CHUNK
DEV = torch.device("cuda", 0)


def gpu_clip(buf, ranges, max_norm, max_grid=0):
    """The kernels on a copy of the CPU tensor `buf`: ((norm, coef), the buffer afterwards)."""
    g = buf.to(DEV)
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    native.ops().clip_grads(g, ranges, max_norm, out, max_grid)
    torch.cuda.synchronize()
    o = out.cpu()
    return (float(o[0]), float(o[1])), g.cpu()


def same_pair(got, want):
    return bits(torch.tensor(got, dtype=torch.float32)).tolist() == \
        bits(torch.tensor(want, dtype=torch.float32)).tolist()


def check(buf, ranges, max_norm, max_grid=0):
    want_buf = buf.clone()
    want = C.clip_grads_(want_buf, ranges, max_norm)
    got, got_buf = gpu_clip(buf, ranges, max_norm, max_grid)
    print(f"ranges {ranges[:2]}.. C {max_norm}: gpu {got} cpu {want}")
    assert same_pair(got, want), (got, want)
    assert torch.equal(bits(got_buf), bits(want_buf))
    return got


SIZES = [1, 3, 4, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 5, 257 * CH + 1]


@pytest.fixture(scope="module")
def noise():
    g = torch.Generator().manual_seed(11)
    return torch.randn(257 * CH + 16, generator=g)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("base", [0, 1])
def test_single_range(noise, n, base):
    """One range of n elements at an aligned and a misaligned base: norm above C (scaled) and
    below C (untouched), both bit-equal to the twin; the elements around the range keep their
    bits."""
    buf = noise[:base + n + 3].clone()
    norm, _ = C.grad_norm_coef(buf, [(base, n)], 1.0)
    for c in (0.5 * norm, 2.0 * norm):
        got = check(buf, [(base, n)], f32(c))
        assert (got[1] < 1.0) == (c < norm)


def plan_table():
    """The 14 payload ranges of the contiguous W = 1 plan and its buffer size."""
    from ddl_amd.parallel.sharding import make_plan
    plan = make_plan("none", 1)
    g = torch.Generator().manual_seed(12)
    return C.payload_ranges(plan.tensor_offsets), plan.total, torch.randn(plan.total, generator=g)


def test_plan_table_poisoned_padding():
    """14 ranges shaped like the real plan; 1e30 in every element outside them changes nothing
    and is not scaled."""
    ranges, total, noise = plan_table()
    assert len(ranges) == 14
    buf = torch.full((total,), 1e30)
    clean = torch.zeros(total)
    for lo, n in ranges:
        buf[lo:lo + n] = noise[lo:lo + n]
        clean[lo:lo + n] = noise[lo:lo + n]
    norm, _ = C.grad_norm_coef(clean, ranges, 1.0)
    assert np.isfinite(norm)
    got = check(buf, ranges, f32(0.25 * norm))
    assert same_pair(got, C.grad_norm_coef(clean, ranges, f32(0.25 * norm)))
    mask = torch.ones(total, dtype=torch.bool)
    for lo, n in ranges:
        mask[lo:lo + n] = False
    _, after = gpu_clip(buf, ranges, f32(0.25 * norm))
    assert bool((after[mask] == 1e30).all())


def test_grid_size_does_not_change_bits():
    ranges, total, buf = plan_table()
    norm, _ = C.grad_norm_coef(buf, ranges, 1.0)
    res = [gpu_clip(buf, ranges, f32(0.5 * norm), mg) for mg in (1, 7, 0)]
    for (pair, out) in res[1:]:
        assert same_pair(pair, res[0][0])
        assert torch.equal(bits(out), bits(res[0][1]))
    check(buf, ranges, f32(0.5 * norm), 7)


def test_ticket_is_rearmed(noise):
    """Two calls in a row on the one ticket word: the second is as good as the first."""
    n = 3 * CH + 5
    g = noise[:n].to(DEV)
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    want = noise[:n].clone()
    for _ in range(2):
        norm, _ = C.grad_norm_coef(want, [(0, n)], 1.0)
        c = f32(0.5 * norm)
        pair = C.clip_grads_(want, [(0, n)], c)
        native.ops().clip_grads(g, [(0, n)], c, out)
        torch.cuda.synchronize()
        o = out.cpu()
        assert same_pair((float(o[0]), float(o[1])), pair)
        assert torch.equal(bits(g), bits(want))


def test_semantics_table(noise):
    n = CH + 9
    x = noise[:n].clone() * 1e-3
    x[5] = -0.0
    norm, _ = C.grad_norm_coef(x, [(0, n)], 1.0)
    # norm < C: coef exactly 1, every bit kept (the -0.0 too)
    pair, out = gpu_clip(x, [(0, n)], f32(4.0 * norm))
    assert pair[1] == 1.0 and torch.equal(bits(out), bits(x))
    assert int(bits(out)[5]) == int(bits(torch.tensor([-0.0]))[0])
    # norm > C: the clipped norm is within 1 ulp-level of C (the scale rounds each element once)
    c = f32(0.125 * norm)
    pair, out = gpu_clip(x, [(0, n)], c)
    check(x, [(0, n)], c)
    after, _ = C.grad_norm_coef(out, [(0, n)], 1.0)
    assert abs(after - c) <= 3 * 2.0 ** -24 * c, (after, c)
    # all zero
    z = torch.zeros(n)
    pair, out = gpu_clip(z, [(0, n)], 1.0)
    assert pair == (0.0, 1.0) and torch.equal(bits(out), bits(z))
    # one inf: coef 1, norm inf reported, nothing rewritten
    y = x.clone()
    y[77] = float("inf")
    pair, out = gpu_clip(y, [(0, n)], 1.0)
    assert pair[0] == float("inf") and pair[1] == 1.0 and torch.equal(bits(out), bits(y))
    assert same_pair(pair, C.grad_norm_coef(y, [(0, n)], 1.0))
    # padding of 1e30 around the range
    p = torch.full((n + 8,), 1e30)
    p[4:4 + n] = x
    pair2, _ = gpu_clip(p, [(4, n)], c)
    assert same_pair(pair2, C.grad_norm_coef(x, [(0, n)], c))


# ---- b. the W = 1 native step -------------------------------------------------------------------
RULES = {
    "adam": dict(optimizer="adam"),
    "nesterov-wd": dict(optimizer="momentum", momentum=0.9, nesterov=True, weight_decay=0.01),
}
LR = 1e-2


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(n_train=400, n_test=100, seed=5)


def one_step(data, B, opts, clip_norm=0.0):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    cfg = TrainConfig(mode="sync", shard="flat", steps=1, batch_size=B, eval_every=0,
                      engine="hip", quiet=True, lr=LR, seed=0, clip_norm=clip_norm, **opts)
    tr = Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=data)
    p0 = tr.params.clone()
    tr.train_step(0)
    torch.cuda.synchronize()
    res = dict(tr=tr, p0=p0, params=tr.params.clone(), grads=tr.grads.clone(),
               state=[(s.m.clone(), None if s.v is None else s.v.clone())
                      for _, s in sorted(tr.servers.items())],
               launches=tr.exchange.runner.update_launches(), norm=tr.last_grad_norm())
    return res


def close(*runs):
    for r in runs:
        r["tr"].exchange.close()


def same_run(a, b):
    ok = torch.equal(bits(a["params"]), bits(b["params"]))
    for (ma, va), (mb, vb) in zip(a["state"], b["state"]):
        ok &= torch.equal(bits(ma), bits(mb))
        if va is not None:
            ok &= torch.equal(bits(va), bits(vb))
    return ok


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("B", [5, 33])
def test_native_step_w1(data, B, rule):
    import step_audit as A
    from ddl_amd.models import engine_segments
    opts = RULES[rule]
    ops = native.ops()
    a = one_step(data, B, opts)
    tr = a["tr"]
    assert a["launches"] == 0 and a["norm"] is None
    ranges = tr.clip_ranges
    g = a["grads"].cpu()
    norm, _ = C.grad_norm_coef(g, ranges, 1.0)
    assert norm > 0 and np.isfinite(norm)
    segs = [set(s) for s in engine_segments("hip", DEV)]
    merged = A.segment_pieces(tr.exchange.units, segs, overlap=False)[1]

    # run B: clipped to half the norm
    cb = f32(0.5 * norm)
    b = one_step(data, B, opts, clip_norm=cb)
    want_g = g.clone()
    pair = C.clip_grads_(want_g, ranges, cb)
    print(f"B={B} {rule}: norm {norm}, coef {pair[1]}, launches {b['launches']} "
          f"({len(merged)} coalesced)")
    assert pair[1] < 1.0
    for lo, n in ranges:   # (the padding is outside the contract)
        assert torch.equal(bits(b["grads"][lo:lo + n]), bits(want_g[lo:lo + n]))
    assert same_pair((b["norm"], float(b["tr"].clip_out[1])), pair)
    # ... and its update is the stand-alone update of that buffer, from the same state
    W = a["p0"].clone()
    G = b["grads"].clone()
    M = torch.zeros_like(W)
    adam = opts["optimizer"] == "adam"
    V = torch.zeros_like(W) if adam else None
    h = next(iter(b["tr"].servers.values())).h
    step = ops.adam_step_size(LR, h.beta1, h.beta2, 1) if adam else LR
    ops.update_flat(0 if adam else 1, W, G, M, V, step, h.beta1, h.beta2, h.eps,
                    opts.get("momentum", 0.0), 1.0, LR * opts.get("weight_decay", 0.0),
                    opts.get("nesterov", False))
    torch.cuda.synchronize()
    assert torch.equal(bits(a["p0"]), bits(b["p0"]))
    for u in b["tr"].exchange.units:
        srv = b["tr"].servers[u.ps]
        for (lo, hi), off in zip(u.ranges, u.state_offs or [0] * len(u.ranges)):
            assert torch.equal(bits(b["params"][lo:hi]), bits(W[lo:hi]))
            assert torch.equal(bits(srv.m[off:off + hi - lo]), bits(M[lo:hi]))
            if adam:
                assert torch.equal(bits(srv.v[off:off + hi - lo]), bits(V[lo:hi]))
    assert not same_run(a, b)
    assert b["launches"] == len(merged)

    # run C: a clip norm above the gradient's changes no bit, on the non-tail placement
    c = one_step(data, B, opts, clip_norm=f32(2.0 * norm))
    assert c["launches"] == len(merged)
    assert float(c["tr"].clip_out[1]) == 1.0 and f32(c["norm"]) == f32(norm)
    for lo, n in ranges:
        assert torch.equal(bits(c["grads"][lo:lo + n]), bits(a["grads"][lo:lo + n]))
    assert same_run(a, c)
    close(a, b, c)


# ---- c. the exchanges on one card ---------------------------------------------------------------
# Worker processes share the one GPU (tests/onecard.py).  At most two workers beside this
# process, each job under one time limit.
LIMIT_S = 150
XB, XSTEPS, ASTEPS = 5, 2, 4


def _pairs(tr, i):
    torch.cuda.synchronize()
    return {"pairs": tuple(tr.clip_out.tolist()), "coefs": float(tr.clip_out[1])}


def _sync_rank(rank, world, port, outdir, kw):
    """One rank of a clipped synchronous run on the xGMI exchange: XSTEPS steps of batch XB."""
    import os
    with oc.rank_session(rank, world, port) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "sync", XSTEPS, XB, synthetic_mnist(400, 100, seed=5), **kw)
        rec = oc.sync_rank_record(tr, XSTEPS, per_step=_pairs)
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        me.close_single(tr.exchange)


def _simulate_sync(world, clip_norm, steps=XSTEPS, B=XB):
    """The one-process PS simulation (onecard.simulate_sync) with every rank's gradient clipped
    by the kernel tested above.  Each step is also held against the fp64 rule of
    exchange_reference (rule_step on the rank-order sum, what sync_round applies per region)
    within the exchange tests' bounds: 1e-6 absolute on w, 1e-6 relative on m and v."""
    import exchange_reference as xr
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    from ddl_amd.parallel.sharding import make_plan
    ops = native.ops()
    plan = make_plan("none", 1)
    ranges = C.payload_ranges(plan.tensor_offsets)
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    h = AdamHyper()
    pairs = [[] for _ in range(world)]

    def clipped(ge, r, step):
        oc.plain_grad(ge, r, step)
        if clip_norm > 0:
            ops.clip_grads(ge.grads, ranges, clip_norm, out)
            pairs[r].append(tuple(out.tolist()))

    def fp64_rule(step, params, acc, m, v, before):
        # (sync_round's two ingredients, with the betas as the kernels hold them: float32.  From
        # v = 0 the difference between 1 - 0.999 and 1 - float32(0.999), 4.7e-5 relative, would
        # otherwise be all there is to see)
        w64, m64, v64 = xr.rule_step(xr.ADAM, *before, acc, adam_coeffs(h, step + 1),
                                     b1=f32(h.beta1), b2=f32(h.beta2), eps=f32(h.eps))
        for lo, n in ranges:
            s = slice(lo, lo + n)
            assert float((params[s].double().cpu() - w64[s]).abs().max()) <= 1e-6
            assert float((m[s].double().cpu() - m64[s]).abs().max()) <= \
                1e-6 * float(m64[s].abs().max()) + 1e-30
            assert float((v[s].double().cpu() - v64[s]).abs().max()) <= \
                1e-6 * float(v64[s].abs().max()) + 1e-30

    want = oc.simulate_sync(world, steps, B, oc.dataset_on_card(400, 100), plan,
                            grad_hook=clipped, after_step=fp64_rule)
    return want, pairs


_NORMS = {}


def first_norms(world):
    """Every rank's unclipped first-step norm (computed once per world size)."""
    if world not in _NORMS:
        _, pairs = _simulate_sync(world, 1e30, steps=1)
        _NORMS[world] = [p[0][0] for p in pairs]
    return _NORMS[world]


@pytest.mark.slow
@pytest.mark.parametrize("shard", ["flat", "contiguous"])
def test_xgmi_sync_w2(tmp_path, shard):
    """Sync W = 2 over xGMI on one card (equal-chunk + replicated buckets of the flat plan, owner
    buckets of the contiguous plan): the replicas agree bit for bit and equal the one-process PS
    simulation fed with each rank's own clipped gradient."""
    from conftest import free_port
    c = f32(0.5 * min(first_norms(2)))
    want, pairs = _simulate_sync(2, c)
    assert all(p[0][1] < 1.0 for p in pairs)
    oc.run_ranks(_sync_rank, 2, free_port(), str(tmp_path), dict(shard=shard, clip_norm=c),
                 limit_s=LIMIT_S)
    recs = oc.load_ranks(tmp_path, 2)
    print("pairs", [rec["pairs"] for rec in recs], "simulation", pairs)
    assert torch.equal(bits(recs[0]["params"]), bits(recs[1]["params"]))
    for r, rec in enumerate(recs):
        assert all(same_pair(a, b) for a, b in zip(rec["pairs"], pairs[r]))
        assert all(t == XSTEPS for t in rec["t"].values())
    assert torch.equal(bits(recs[0]["params"]), bits(want))


def test_forced_rccl_rehearsal_w1(data):
    """The forced 1-rank RCCL rehearsal (reduce-scatter / all-gather and all-reduce units as
    RCCL copies): equals the simulation at W = 1."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    c = f32(0.5 * first_norms(1)[0])
    want, pairs = _simulate_sync(1, c)
    cfg = TrainConfig(mode="sync", shard="flat", steps=XSTEPS, batch_size=XB, eval_every=0,
                      engine="hip", quiet=True, data_sharding="stride", force_collectives=True,
                      clip_norm=c)
    tr = Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=synthetic_mnist(400, 100, seed=5))
    assert tr.exchange.native and tr.exchange.backend == "rccl"
    for i in range(XSTEPS):
        tr.train_step(i)
        torch.cuda.synchronize()
        assert same_pair(tuple(tr.clip_out.tolist()), pairs[0][i])
    got = oc.canon(tr.params, tr.plan.tensor_offsets).cpu()
    tr.exchange.close()
    assert torch.equal(bits(got), bits(want))


def _async_rank(rank, world, port, outdir, kw):
    """One rank of a clipped asynchronous run on the xGMI data plane, ASTEPS steps (W = 1 takes
    the in-line applies)."""
    import os
    with oc.rank_session(rank, world, port) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "async", ASTEPS, XB, synthetic_mnist(2000, 500, seed=5), **kw)
        assert tr.exchange.runner is not None

        def started(ex):
            assert ex.inline == (world == 1)

        rec = oc.async_rank_record(tr, world, ASTEPS, per_step=_pairs, after_start=started)
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        me.close_single(tr.exchange)


@pytest.mark.slow
@pytest.mark.parametrize("world,kw", [
    pytest.param(1, dict(shard="flat", num_ps=3), id="1-inline"),
    pytest.param(2, dict(shard="contiguous"), id="2-board"),
])
def test_xgmi_async_equals_its_replay(tmp_path, world, kw):
    """Async over xGMI, W = 1 in-line applies and W = 2 on the arrival board: the run equals the
    replay of its recorded apply orders with a gradient function that clips, bit for bit."""
    import async_replay as ar
    from conftest import free_port
    c = 0.75   # below the first steps' norms at this batch (asserted through the coefficients)
    oc.run_ranks(_async_rank, world, free_port(), str(tmp_path), dict(kw, clip_norm=c),
                 limit_s=LIMIT_S)
    recs = oc.load_ranks(tmp_path, world)
    _, order = oc.recorded_orders(recs, world, ASTEPS)
    print("orders", {p: ar.order_string(o) for p, o in order.items()},
          "coefs", [rec["coefs"] for rec in recs])
    assert all(min(rec["coefs"]) < 1.0 for rec in recs)
    table = C.payload_ranges(recs[0]["offsets"])
    out = torch.zeros(2, dtype=torch.float32, device=DEV)

    def clipped(ge, r, s):
        oc.plain_grad(ge, r, s)
        native.ops().clip_grads(ge.grads, table, c, out)

    want, state = oc.replay_async(recs, world, order, ASTEPS, grad_hook=clipped)
    oc.assert_payload_equals_replay(recs, world, want, state, table)
