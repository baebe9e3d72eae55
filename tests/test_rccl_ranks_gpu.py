"""The RCCL branch of the native sync runner (csrc/kernels/runner.hip) as EACH RANK of a world of
W > 1, in one process on one card, against simulated peers.

Every RCCL call of the runner goes through the table of csrc/kernels/rccl_api.h; here that table
is the fake communicator of csrc/kernels/fake_rccl.hip, whose peers are the one-process PS
simulation (onecard.GradEngine, the loop of onecard.simulate_sync with every rank's gradient row
kept).  No rank is spawned and no communicator exists.  The fake sums in rank order, so this pins
what the runner ASKS of RCCL (which chunk, which root, which state offset, which stream order),
not what RCCL does: real RCCL at W > 1 stays unmeasured.

Per cell: a real NativeSyncExchange(backend="rccl") on DistEnv(world=W, rank=r) with its own
params, grads, engine (batch 8) and ParameterServer objects as roles.py builds them, two steps of
B = 5, keep 0.5, stride sharding.  After each step: no violation; the call log satisfies
rccl_reference.expected(); the live gradient the collectives read is bit-equal to the simulation's
row r; the whole parameter buffer is bit-equal to the simulation's; m, v of every PS the rank
hosts (and the replicated last bucket's) are bit-equal to the simulation's slices, t advanced by
one, no PS object exists for a PS hosted elsewhere; update_launches() is the count of the ranges
the rank owns.

The self-test (SyncRunner::selftest) under the honest fake says ok on every rank of W = 2, 3, 8,
and under each fault knob says no with the reason naming the right half, except where the knob
cannot show (SHOWS below lists that per rank).

The cells are tests/test_rccl_ranks_cpu.py's plans; that file proves on the CPU that the oracle
used here tells a wrong chunk, root, missing gather or state offset from a right one.

Durations on one MI355X, per test in a whole-suite run (648 passed in 315 s): the 29 cells
0.17 - 0.25 s each (two steps, an engine and a runner of their own; the first cell of a world size
also runs its simulation: test_flat[2-0] 0.46 s, test_flat_w2_clipped 0.23 s), the three
self-test tests 0.08 - 0.09 s (every rank of the world, five self-tests each), the file's 33 tests
6.1 s together; 4.2 s as a run of its own.
"""
import contextlib
import gc
import os

import pytest
import torch

import onecard as oc
import rccl_reference as rr
from oracle_common import bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EB, B, STEPS, KEEP = 8, 5, 2, 0.5
NAN = float("nan")


def ops():
    from ddl_amd.ops import native
    return native.ops()


def segs():
    from ddl_amd.models import HIP_SEGMENTS
    return HIP_SEGMENTS


def data():
    return oc.dataset_on_card(400, 100)


def plan_of(shard, P, overlap_buckets=True):
    from ddl_amd.parallel.sharding import make_plan
    return make_plan(shard, P, buckets=segs() if shard == "flat" and overlap_buckets else None)


def clip_ranges(plan):
    from ddl_amd.ops import clip as C
    return C.payload_ranges(plan.tensor_offsets)


# ---- the oracle: the one-process PS simulation with every rank's gradient kept ------------------
_ORACLE = {}


def oracle(shard, W, P, reduce="sum", optimizer="adam", clip=0.0):
    """Per step: peer_grads [W, total], params_next [total], m, v [total] (v None: momentum)."""
    key = (shard, W, P, reduce, optimizer, clip)
    if key in _ORACLE:
        return _ORACLE[key]
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    plan = plan_of(shard, P)
    ge = oc.GradEngine(plan.total, plan.tensor_offsets, EB, data(), W,
                       dict(data_sharding="stride", keep_prob=KEEP, seed=0), init_seed=0)
    ge.batch = B  # (engine batch EB, B rows per rank)
    params, grads = ge.params, ge.grads
    acc, m = torch.zeros_like(params), torch.zeros_like(params)
    v = torch.zeros_like(params) if optimizer == "adam" else None
    h = AdamHyper()
    scale = 1.0 / W if reduce == "mean" else 1.0
    out2 = torch.zeros(2, dtype=torch.float32, device=DEV)
    steps = []
    for s in range(STEPS):
        rows = torch.empty(W, plan.total, device=DEV)
        acc.zero_()
        for r in range(W):
            oc.plain_grad(ge, r, s)
            if clip > 0:
                ops().clip_grads(grads, clip_ranges(plan), clip, out2)
            rows[r].copy_(grads)
            acc.add_(grads)
        if optimizer == "adam":
            ops().adam_flat(params, acc, m, v, adam_coeffs(h, s + 1), h.beta1, h.beta2, h.eps, scale)
        else:
            ops().update_flat(oc.MOMENTUM, params, acc, m, None, h.lr, 0.0, 0.0, 0.0, 0.9, scale)
        steps.append(dict(peer_grads=rows, params_next=params.clone(), m=m.clone(),
                          v=None if v is None else v.clone()))
    torch.cuda.synchronize()
    _ORACLE[key] = steps
    return steps


# ---- the rank under test -------------------------------------------------------------------------
@contextlib.contextmanager
def rank_under_test(shard, W, P, r, reduce="sum", optimizer="adam", clip=0.0):
    """A real NativeSyncExchange on the RCCL backend as rank r of W, its communicator the fake's.
    The override is installed when the exchange asks for its communicator (the shard buffers
    exist by then) and removed when the block ends; yields (exchange, plan, seen)."""
    from ddl_amd.models.hip_engine import HipEngine
    from ddl_amd.models.mnist_cnn import init_params_
    from ddl_amd.ops.adam import AdamHyper
    from ddl_amd.ops.grad_stage import GradStage
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.native_exchange import NativeSyncExchange
    from ddl_amd.parallel.ps import ParameterServer
    plan = plan_of(shard, P)
    params = torch.zeros(plan.total, dtype=torch.float32, device=DEV)
    grads = torch.zeros_like(params)
    seen = torch.full_like(params, NAN)
    init_params_(params, plan.tensor_offsets, 0)
    engine = HipEngine(params, grads, plan.tensor_offsets, batch=EB, graph=False, eval_chunk=EB)
    hyper = AdamHyper()
    servers = {p: ParameterServer(plan, p, DEV, hyper, optimizer, 0.9)
               for p in range(P) if plan.host_rank(p, W) == r}
    stage = GradStage(clip=(clip, clip_ranges(plan),
                            torch.zeros(2, dtype=torch.float32, device=DEV)) if clip > 0 else None)

    class OnFake(NativeSyncExchange):
        def _init_comm_collectively(self, o, env):
            shards = [u.shard_buf for u in self.units if u.shard_buf is not None]
            gc.collect()  # (an earlier test's unreferenced runner may still hold a communicator)
            o.fake_rccl_install(env.world, env.rank, self.params, self.grads, shards, seen)
            self.runner.init_comm(bytes(128))
            o.fake_rccl_set_peers("pattern")
            ok, why = self.runner.selftest()
            o.fake_rccl_set_peers("table")
            assert ok, why

    ex = None
    try:
        ex = OnFake(plan, DistEnv(r, W, 0, DEV), params, grads, segs(), servers, engine, reduce,
                    False, not stage.whole, optimizer, hyper, 0.9, backend="rccl", stage=stage)
        assert ex.backend == "rccl" and ex.runner.has_comm() and ex.peer is None
        assert ops().fake_rccl_violations() == []
        yield ex, plan, seen
    finally:
        torch.cuda.synchronize()
        if ex is not None:
            ex.close()
        del ex
        gc.collect()
        ops().fake_rccl_remove()
        assert not ops().rccl_overridden()


def rank_batch(r, W, s):
    from ddl_amd.ops import rng
    from ddl_amd.utils.data import batch_indices
    d = data()
    lo, hi = batch_indices(s, B, d.total_batch, r, W, "stride")
    return d.x_train[lo:hi], d.y_train[lo:hi], rng.step_seed(0, r, s)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def expected_state(ex, exps, r, sim, which):
    """Every hosted PS's whole m (or v) as the simulation has it: the ranges the rank updates from
    the simulation's slices, everything else untouched zeros; and the replicated bucket's."""
    want = {p: torch.zeros_like(ps.m) for p, ps in ex.servers.items()}
    repl = None
    for e in exps:
        if e.kind == "ar":
            repl = sim[which][e.lo:e.lo + e.n]
        elif e.kind == "rs":
            want[e.ps][e.state_off:e.state_off + e.c] = sim[which][e.lo + r * e.c:e.lo + (r + 1) * e.c]
        elif e.root == r:
            want[e.ps][e.state_off:e.state_off + e.n] = sim[which][e.lo:e.lo + e.n]
    return want, repl


def run_cell(shard, W, P, r, repl_last=True, **opt):
    sims = oracle(shard, W, P, **opt)
    o = ops()
    with rank_under_test(shard, W, P, r, **opt) as (ex, plan, seen):
        overlap = not ex.stage.whole
        exps = rr.expected(plan, segs(), W, r, repl_last=repl_last, overlap=overlap)
        assert (ex.repl is not None) == any(e.kind == "ar" for e in exps)
        hosted = sorted(p for p in range(P) if plan.host_rank(p, W) == r)
        assert sorted(ex.servers) == hosted  # (no state here for a PS hosted elsewhere)
        for s, sim in enumerate(sims):
            o.fake_rccl_set_step(sim["peer_grads"], sim["params_next"])
            o.fake_rccl_clear()
            seen.fill_(NAN)
            torch.cuda.synchronize()
            x, y, seed = rank_batch(r, W, s)
            ex.step(x, y, KEEP, seed)
            torch.cuda.synchronize()
            # 1. and 2.: nothing the fake objects to, and the calls the plan demands
            assert o.fake_rccl_violations() == []
            log = o.fake_rccl_calls()
            assert rr.check_calls(log, exps, r) == [], log
            assert o.fake_rccl_group_depth() == 0
            # 3. what the collectives read of this rank is the rank's own gradient
            assert same(seen, sim["peer_grads"][r]), f"step {s}: live gradient"
            # 4. every replica's parameters
            assert same(ex.params, sim["params_next"]), f"step {s}: parameters"
            # 5. the state of every PS hosted here, and only there
            for which in ("m", "v"):
                if sim[which] is None:
                    assert all(ps.v is None for ps in ex.servers.values())
                    assert ex.repl is None or ex.repl[4] is None
                    continue
                want, repl = expected_state(ex, exps, r, sim, which)
                for p, ps in ex.servers.items():
                    assert same(getattr(ps, which), want[p]), f"step {s}: PS {p} {which}"
                    assert ps.t == s + 1
                if repl is not None:
                    assert same(ex.repl[3 if which == "m" else 4], repl), f"step {s}: repl {which}"
            # 6. one update launch per range this rank owns, none for the others
            assert ex.runner.update_launches() == rr.update_launches(exps, r)
        assert not same(ex.params, sims[0]["params_next"])  # (the second step moved them)
    assert o.SyncRunner.probe() == ""  # the real library's symbols again


RANKS = {2: (0, 1), 3: (0, 1, 2), 8: (0, 3, 7)}


@pytest.mark.parametrize("W,r", [(W, r) for W in (2, 3, 8) for r in RANKS[W]])
def test_flat(W, r):
    """Reduce-scatter / update of chunk r / in-place all-gather per bucket, the last bucket one
    all-reduce on replicated state."""
    run_cell("flat", W, W, r)


@pytest.mark.parametrize("W,r", [(W, r) for W in (2, 3, 8) for r in RANKS[W]])
def test_contiguous(W, r):
    """Reduce to the rank hosting each PS, the update there, broadcast from it."""
    run_cell("contiguous", W, W, r)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_greedy_w3(r):
    run_cell("greedy", 3, 3, r)


@pytest.mark.parametrize("r", [0, 1])
def test_none_w2(r):
    """One PS: rank 1 hosts nothing, updates nothing and takes every parameter by broadcast."""
    run_cell("none", 2, 1, r)


@pytest.mark.parametrize("r", [1, 3])
def test_flat_fewer_ps_than_ranks(r):
    """Flat with P = 2 on W = 4: a hosting rank (1) and one that hosts nothing (3)."""
    run_cell("flat", 4, 2, r)


def test_flat_w3_owner_form_of_the_last_bucket(monkeypatch):
    """DDL_REPL_LAST=0: the last bucket is reduce-scattered like the others (rank 2)."""
    monkeypatch.setenv("DDL_REPL_LAST", "0")
    run_cell("flat", 3, 3, 2, repl_last=False)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_flat_w3_mean(r):
    """--grad-reduce mean: the update's gradient scale 1/3 rounds."""
    run_cell("flat", 3, 3, r, reduce="mean")


def test_contiguous_w3_momentum():
    run_cell("contiguous", 3, 3, 1, optimizer="momentum")


def test_flat_w2_clipped():
    """A clipped step (overlap off, every unit after the last segment): clip_norm at half of
    rank 1's first norm, so the collectives must read the CLIPPED gradient."""
    from ddl_amd.ops import clip as C
    plan = plan_of("flat", 2)
    g = oracle("flat", 2, 2)[0]["peer_grads"][1].cpu()
    norm, _ = C.grad_norm_coef(g, clip_ranges(plan), 1.0)
    c = oc.f32(0.5 * norm)
    clipped = oracle("flat", 2, 2, clip=c)
    assert not same(clipped[0]["peer_grads"][1], oracle("flat", 2, 2)[0]["peer_grads"][1])
    run_cell("flat", 2, 2, 1, clip=c)


# ---- the runner's own self-test must fire --------------------------------------------------------
HALF = {"rs_next_chunk": "reduce_scatter/all_gather", "ag_skip": "reduce_scatter/all_gather",
        "reduce_drop_peer": "reduce/broadcast", "bcast_skip": "reduce/broadcast"}


def SHOWS(fault, W, r):
    """Whether a fault knob can show in the self-test of rank r.  The self-test reduces to
    root = W - 1 and broadcasts from it: only the root sees a wrong Reduce (everyone else takes
    the broadcast, which the knob leaves right), and only a non-root misses a Broadcast."""
    if fault == "reduce_drop_peer":
        return r == W - 1
    if fault == "bcast_skip":
        return r != W - 1
    return True


@pytest.fixture(scope="module")
def small_engine():
    from ddl_amd.models.hip_engine import HipEngine
    plan = plan_of("none", 1)
    params = torch.zeros(plan.total, dtype=torch.float32, device=DEV)
    grads = torch.zeros_like(params)
    return HipEngine(params, grads, plan.tensor_offsets, batch=EB, graph=False, eval_chunk=EB)


@pytest.mark.parametrize("W", [2, 3, 8])
def test_selftest_fires(small_engine, W):
    o = ops()
    e = small_engine
    cannot = []
    gc.collect()
    for r in range(W):
        o.fake_rccl_install(W, r, e.params, e.grads, [], None)
        runner = o.SyncRunner(e.eng, e.params, e.grads, W, r)
        try:
            runner.init_comm(bytes(128))
            with pytest.raises(RuntimeError):  # installing under a live communicator
                o.fake_rccl_install(W, r, e.params, e.grads, [], None)
            o.fake_rccl_set_peers("pattern")
            ok, why = runner.selftest()
            assert ok, (r, why)
            for fault in rr.FAULTS:
                o.fake_rccl_set_fault(fault)
                ok, why = runner.selftest()
                if SHOWS(fault, W, r):
                    assert not ok and HALF[fault] in why, (fault, r, ok, why)
                else:
                    cannot.append((fault, r))
                    assert ok, (fault, r, why)
            o.fake_rccl_set_fault("none")
            ok, why = runner.selftest()
            assert ok, (r, why)
            assert o.fake_rccl_violations() == [] and o.fake_rccl_group_depth() == 0
        finally:
            runner.close()
            o.fake_rccl_remove()
    print(f"W = {W}: cannot show (fault, rank): {cannot}")
    assert len(cannot) == W  # reduce_drop_peer on W - 1 non-roots, bcast_skip on the root


def test_override_is_gone():
    """After the cells above the seam is empty, probe() resolves the real library's symbols
    again, and the fake takes no step data while it is not installed."""
    o = ops()
    assert not o.rccl_overridden()
    assert o.SyncRunner.probe() == ""
    with pytest.raises(RuntimeError):
        o.fake_rccl_set_step(torch.zeros(1, 8, device=DEV), torch.zeros(8, device=DEV))
