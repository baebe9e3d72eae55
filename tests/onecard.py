"""One harness for the multi-process GPU tests that put W ranks on ONE card (helper module, not a
conftest): the rendezvous preamble, the rank launcher with its deadline, the rank wrapper, the
shared xGMI rank bodies, the one-process PS simulation, the replay set-up, the W = 1 placement
runs, the records of the checkpoint / resume tests and the small comparison helpers.

W worker processes share one GPU (default process group over gloo, ``DDL_DIST_BACKEND``): RCCL
refuses two ranks on one device, but the xGMI exchange only needs IPC-mapped memory, so the whole
W > 1 native step runs here exactly as on an 8-GPU node.

torch and the package are imported inside the functions, so that collecting tests and starting a
rank's interpreter stay cheap.
"""
import contextlib
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every job's time limit unless it names another one: the larger of 150 s and three times the
# slowest cell of the test on the commit before this module (3.9 - 5.4 s each, so 150 s for all
# of them; docs/DESIGN.md "One harness for the one-card tests" has the table).  The factor 3
# covers process start and HIP initialisation of several ranks on a card other tenants also use.
LIMIT_S = 150.0
W8_LIMIT_S = 180.0
XGMI_TIMEOUT_S = "20"
GRACE_EXTRA_S = 3.0
ADAM, MOMENTUM = 0, 1  # update.h UpdKind


# ---- small helpers -------------------------------------------------------------------------------
def f32(x):
    """x rounded to float32, as a Python float."""
    import numpy as np
    return float(np.float32(x))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def canon(params, offsets):
    """The 14 tensors of a plan's flat buffer in canonical order, without the plan's padding."""
    import torch
    from ddl_amd.models.layout import TENSORS
    return torch.cat([params[offsets[t.index]:offsets[t.index] + t.numel] for t in TENSORS])


def load_ranks(outdir, world, name="rank{}.pt"):
    import torch
    return [torch.load(os.path.join(outdir, name.format(r)), weights_only=False)
            for r in range(world)]


# ---- 1. the rendezvous preamble ------------------------------------------------------------------
def enter(rank, world, port, env=None, xgmi_timeout_s=XGMI_TIMEOUT_S):
    """The repository root on sys.path and the seven variables of a one-card rank; `env` on top."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), DDL_DIST_BACKEND="gloo",
                      DDL_XGMI_TIMEOUT_S=str(xgmi_timeout_s))
    os.environ.update(env or {})


# ---- 2. the launcher -----------------------------------------------------------------------------
def _grace_s():
    """What a rank needs to end itself once a peer is gone: the xGMI timeout in force plus a few
    seconds (its kernels stop waiting, the runner raises at its next call, the process exits)."""
    return float(os.environ.get("DDL_XGMI_TIMEOUT_S", XGMI_TIMEOUT_S)) + GRACE_EXTRA_S


def _reap(kids, deadline, grace, failed):
    """Wait for every child until `deadline`, or only `grace` more once one rank has failed; kill
    what is still alive then and join everything.  Returns the children that had to be killed."""
    from multiprocessing.connection import wait
    stop = min(deadline, time.monotonic() + grace) if failed else deadline
    while True:
        alive = [k for k in kids if k.is_alive()]
        if not alive:
            break
        if not failed and any(k.exitcode not in (None, 0) for k in kids):
            failed, stop = True, min(stop, time.monotonic() + grace)
        left = stop - time.monotonic()
        if left <= 0:
            break
        wait([k.sentinel for k in alive], timeout=left)
    late = [k for k in kids if k.is_alive()]
    for k in late:
        k.kill()
    for k in kids:
        k.join()
    return late


def run_ranks(fn, world, *args, limit_s, rank0_here=False):
    """fn(rank, world, *args) on every rank, each in a fresh process (the `spawn` context), under
    ONE deadline of `limit_s` for the whole job.  When a rank exits non-zero the others get a
    short grace (`_grace_s`), at the deadline every rank still alive is killed; no child outlives
    the call, nothing is tried twice.  Asserts that no rank had to be killed and that every exit
    code is 0.

    rank0_here: ranks 1..world-1 are spawned and rank 0 runs in the calling process, whose
    os.environ is restored afterwards.  W = 8 on one card must run with EXACTLY eight GPU
    processes: rank 0 is the pytest process (which already holds a GPU context from the earlier
    tests) and ranks 1..7 are spawned.  The round-3 abort (HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION in
    a GEMM dual kernel, profiles/r3_w8_one_gpu_fault.log) happened with eight spawned ranks PLUS
    the pytest process — nine processes with hardware queues, one more than the eight compute
    VMIDs the kernel driver's scheduler keeps resident at once, so the run list was
    over-subscribed and the scheduler time-sliced whole processes by preempting their waves
    (context save / restore) — the regime every W = 8 stall, divergence and abort on one card was
    seen in, and one no 8-GPU node (one process per GPU) ever enters.  docs/DESIGN.md "W = 8 on
    one card: the cause"."""
    import multiprocessing
    ctx = multiprocessing.get_context("spawn")
    first = 1 if rank0_here else 0
    kids = [ctx.Process(target=fn, args=(r, world, *args)) for r in range(first, world)]
    deadline = time.monotonic() + limit_s
    for k in kids:
        k.start()
    saved = dict(os.environ)
    late, here_failed = kids, rank0_here
    try:
        if rank0_here:
            fn(0, world, *args)
            here_failed = False
    finally:
        grace = _grace_s()  # (read before the restore: rank 0's enter() set the timeout in force)
        if rank0_here:
            os.environ.clear()
            os.environ.update(saved)
        late = _reap(kids, deadline, grace, here_failed)
        if rank0_here:
            import gc
            import torch
            gc.collect()
            if torch.cuda.is_initialized():
                torch.cuda.synchronize()
    codes = {first + i: k.exitcode for i, k in enumerate(kids)}
    print(f"run_ranks: exit codes {codes}")
    assert not late and all(c == 0 for c in codes.values()), \
        f"exit codes {codes}; {len(late)} rank(s) killed (limit {limit_s:.0f} s, grace {grace:.0f} s)"


# ---- 3. the rank wrapper -------------------------------------------------------------------------
class _Rank:
    def __init__(self, env, dist, world):
        self.env, self.dist, self.world = env, dist, world
        self._exchange = None

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def close_single(self, ex):
        """The teardown of a process with ONE exchange, run when the `with` block ends: barrier,
        ex.close(), barrier, destroy."""
        self._exchange = ex

    def close_one_of_several(self, ex):
        """The teardown of one exchange in a process that goes on to build the next: HIP leaves
        freeing an exported buffer undefined while a peer still has it mapped, so every rank
        unmaps its peers' buffers (a synchronous exchange closes its runner first), a barrier,
        then every rank frees its own, a barrier: no rank frees a buffer a peer still has mapped.
        (Without them a wait of a later exchange timed out once in two runs: the peer's flag
        stores never showed.)"""
        from ddl_amd.parallel.async_xgmi import AsyncPeerExchange
        self.barrier()
        if isinstance(ex, AsyncPeerExchange):
            ex.peer.unmap_peers()
            self.barrier()
            ex.close()
        else:                              # the synchronous exchange: its runner, then its peer
            ex.runner.close()
            ex.peer.unmap_peers()
            self.barrier()
            ex.peer.close()
        self.barrier()


@contextlib.contextmanager
def rank_session(rank, world, port, env=None, xgmi_timeout_s=XGMI_TIMEOUT_S, on_device_0=False):
    """What every rank body is wrapped in: enter(), init_distributed(), the check that the rank
    sits on the one card, a traceback on any exception (a spawned rank's only voice), and at
    W > 1 the closing barrier / destroy_process_group.  Yields the rank's handle: `.env`,
    `.dist`, `.barrier()`, and the two teardown forms."""
    enter(rank, world, port, env, xgmi_timeout_s)
    try:
        import torch.distributed as dist
        from ddl_amd.parallel.comm import init_distributed
        denv = init_distributed()
        if on_device_0:
            assert denv.device.index == 0
        me = _Rank(denv, dist, world)
        yield me
        if me._exchange is not None:
            me.barrier()
            me._exchange.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:
        traceback.print_exc()
        raise


# ---- 4. the shared rank bodies -------------------------------------------------------------------
def xgmi_trainer(env, mode, steps, batch, dataset, **kw):
    """A Trainer on the xGMI exchange with the constants every one-card job repeats; asserts that
    the xGMI path was taken."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.roles import Trainer
    if mode == "async":
        kw = dict(dict(check_provenance=True, watchdog_s=120.0), **kw)
    cfg = TrainConfig(mode=mode, steps=steps, batch_size=batch, eval_every=0, engine="hip",
                      quiet=True, data_sharding="stride", exchange_backend="xgmi", **kw)
    tr = Trainer(cfg, env, dataset=dataset)
    ex = tr.exchange
    if mode == "async":
        from ddl_amd.parallel.async_xgmi import AsyncPeerExchange
        assert isinstance(ex, AsyncPeerExchange), type(ex)
    else:
        assert getattr(ex, "native", False) and ex.peer is not None, "xgmi path not taken"
    return tr


def _collect(extras, got):
    for k, v in (got or {}).items():
        extras.setdefault(k, []).append(v)


def sync_rank_record(tr, steps, per_step=None):
    """`steps` synchronous steps, then the exchange's own check; the record: canonical params,
    every hosted PS's t, the trainer's step count, and under each key of the dicts that
    per_step(tr, i) returned the list of its values."""
    import torch
    extras = {}
    for i in range(steps):
        tr.train_step(i)
        if per_step is not None:
            _collect(extras, per_step(tr, i))
    torch.cuda.synchronize()
    tr.exchange.check()
    return dict(extras, params=canon(tr.params, tr.plan.tensor_offsets).cpu(),
                t={p: s.t for p, s in tr.servers.items()}, steps=tr.global_step)


def async_rank_record(tr, world, steps, per_step=None, before_step=None, after_start=None):
    """One asynchronous xGMI rank, its steps driven one by one: start, after_start(ex), at W > 1
    a barrier (the ranks start together: their pushes do meet at the PS), before_step(i) /
    train_step / per_step(tr, i), join, verify_provenance.  The record is what a replay needs
    (tests/async_replay.py) plus the lists per_step collected."""
    import torch
    import torch.distributed as dist
    ex = tr.exchange
    init = tr.params.clone()
    ex.steps = steps
    ex.start()
    if after_start is not None:
        after_start(ex)
    if world > 1:
        torch.cuda.synchronize()
        dist.barrier()
    extras = {}
    for i in range(steps):
        if before_step is not None:
            before_step(i)
        tr.train_step(i)
        if per_step is not None:
            _collect(extras, per_step(tr, i))
    ex.join()
    ex.verify_provenance()
    torch.cuda.synchronize()
    assert ex.peer.error() == 0, ex.peer.error()
    P = tr.plan.num_ps
    return dict(extras, init=init.cpu(), params=tr.params.cpu(),
                ps={p: dict(w=s.params.cpu(), m=s.m.cpu(), v=None if s.v is None else s.v.cpu(),
                            t=s.t) for p, s in tr.servers.items()},
                provenance=list(ex.provenance), served=ex.served, steps=tr.global_step,
                ranges=[tr.plan.ps_segments(p)[0] for p in range(P)],
                hosts=[tr.plan.host_rank(p, world) for p in range(P)],
                offsets=list(tr.plan.tensor_offsets), total=tr.plan.total, cfg=tr.cfg.to_dict())


def sync_each_step(tr, i):
    """per_step: a host synchronisation after every step."""
    import torch
    torch.cuda.synchronize()


# ---- the engine both the simulation and the replay draw their gradients from ---------------------
_DATA = {}


def dataset_on_card(n_train, n_test):
    """synthetic_mnist(n_train, n_test, seed=5), the ranks' dataset, on the card: made once."""
    if (n_train, n_test) not in _DATA:
        import torch
        from ddl_amd.utils.data import synthetic_mnist
        _DATA[(n_train, n_test)] = synthetic_mnist(n_train, n_test, seed=5).to(
            torch.device("cuda", 0))
    return _DATA[(n_train, n_test)]


class GradEngine:
    """A HIP engine on buffers of its own, and whose batches and dropout seeds it reads: `cfg`
    holds data_sharding, keep_prob and seed (a TrainConfig's dict does)."""

    def __init__(self, total, offsets, batch, data, world, cfg, init_seed=None):
        import torch
        from ddl_amd.models.hip_engine import HipEngine
        from ddl_amd.models.mnist_cnn import init_params_
        dev = torch.device("cuda", 0)
        self.params = torch.zeros(total, device=dev)
        if init_seed is not None:
            init_params_(self.params, offsets, init_seed)
        self.grads = torch.zeros_like(self.params)
        self.offsets, self.batch, self.data, self.world, self.cfg = offsets, batch, data, world, cfg
        self.eng = HipEngine(self.params, self.grads, offsets, batch=batch, graph=False,
                             eval_chunk=batch)

    def backward(self, r, index, seed_step):
        """Rank r's gradient on its batch number `index` with the dropout seed of `seed_step`,
        into self.grads."""
        from ddl_amd.ops import rng
        from ddl_amd.utils.data import batch_indices
        c, d = self.cfg, self.data
        lo, hi = batch_indices(index, self.batch, d.total_batch, r, self.world, c["data_sharding"])
        self.eng.forward_backward(d.x_train[lo:hi], d.y_train[lo:hi], c["keep_prob"],
                                  rng.step_seed(c["seed"], r, seed_step))


def plain_grad(ge, r, s):
    """The default grad_hook: rank r's gradient of step s, one batch."""
    ge.backward(r, s, s)


# ---- 5. the one-process PS simulation ------------------------------------------------------------
def simulate_sync(world, steps, batch, dataset, plan, grad_hook=None, update=None, coef=None,
                  scale=1.0, after_step=None):
    """Synchronous PS training in one process with the HIP engine: every rank's gradient on its
    own batch and dropout seed (grad_hook(ge, r, step) leaves it in ge.grads; default
    plain_grad), times coef[r], summed in rank order from 0 (the kernels' order), one update per
    global step: update(params, acc, m, v, step), by default one native TF1 Adam step with the
    gradient scale `scale`.  after_step(step, params, acc, m, v, before), if given, is called
    after every update with the (params, m, v) clones from before it.  Returns the canonical
    parameters on the CPU."""
    import torch
    from ddl_amd.ops import native
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    ge = GradEngine(plan.total, plan.tensor_offsets, batch, dataset, world,
                    dict(data_sharding="stride", keep_prob=0.5, seed=0), init_seed=0)
    params, grads = ge.params, ge.grads
    acc, m, v = torch.zeros_like(params), torch.zeros_like(params), torch.zeros_like(params)
    h = AdamHyper()
    grad_hook = grad_hook or plain_grad
    coef = coef or [1.0] * world
    for step in range(steps):
        acc.zero_()
        for r in range(world):
            grad_hook(ge, r, step)
            acc.add_(grads * coef[r] if coef[r] != 1.0 else grads)
        before = (params.clone(), m.clone(), v.clone()) if after_step is not None else None
        if update is not None:
            update(params, acc, m, v, step)
        else:
            native.ops().adam_flat(params, acc, m, v, adam_coeffs(h, step + 1), h.beta1, h.beta2,
                                   h.eps, scale)
        if after_step is not None:
            torch.cuda.synchronize()
            after_step(step, params, acc, m, v, before)
    torch.cuda.synchronize()
    return canon(params, plan.tensor_offsets).cpu()


# ---- 6. the replay of an asynchronous run --------------------------------------------------------
def replay_async(recs, world, order, steps, grad_hook=None, update=None, dataset=None):
    """The run of `recs` (async_rank_record, one per rank) again in this process, in the recorded
    apply `order`: gradients from the HIP engine on the worker's batch and dropout seed
    (grad_hook(ge, r, s), default plain_grad), updates from ops.update_flat on the PS range with
    the step size of the PS's own t (update(st, g, t, h, cfg), default the run's optimizer with
    no further option).  dataset: the ranks' dataset on the card (default
    dataset_on_card(2000, 500)).  Returns async_replay.replay's (worker buffers, PS states)."""
    import torch
    import async_replay as ar
    from ddl_amd.ops import native
    from ddl_amd.ops.adam import AdamHyper, adam_coeffs
    dev = torch.device("cuda", 0)
    cfg = recs[0]["cfg"]
    ge = GradEngine(recs[0]["total"], recs[0]["offsets"], cfg["batch_size"],
                    dataset if dataset is not None else dataset_on_card(2000, 500), world, cfg)
    # the xGMI service holds lr and the betas as float32 and widens them for the step size
    # (update.h adam_step_size; tests/test_numerics_cpu.py pins that to adam_coeffs on the same
    # operands); a decay is formed from the doubles (update.h upd_decay)
    h = AdamHyper(lr=f32(cfg["lr"]), beta1=f32(0.9), beta2=f32(0.999))
    grad_hook = grad_hook or plain_grad
    mu = {"adam": 0.0, "momentum": cfg["momentum"], "sgd": 0.0}[cfg["optimizer"]]

    def grad_fn(r, s, params_r):
        ge.params.copy_(params_r)
        grad_hook(ge, r, s)
        return ge.grads.clone()

    def update_fn(p, st, g, t):
        if update is not None:
            update(st, g, t, h, cfg)
        elif cfg["optimizer"] == "adam":
            native.ops().update_flat(ADAM, st.w, g, st.m, st.v, adam_coeffs(h, t), 0.9, 0.999,
                                     1e-8, 0.0, 1.0)
        else:
            native.ops().update_flat(MOMENTUM, st.w, g, st.m, None, f32(cfg["lr"]), 0.0, 0.0,
                                     0.0, mu, 1.0)

    out = ar.replay(order, recs[0]["ranges"], recs[0]["init"].to(dev), world, steps, grad_fn,
                    update_fn)
    torch.cuda.synchronize()
    return out


def recorded_orders(recs, world, steps):
    """The ranks' provenance logs as one list (the xGMI service logs every apply) and the per-PS
    apply orders they fix."""
    import async_replay as ar
    log = [e for rec in recs for e in rec["provenance"]]
    assert len(log) == len(recs[0]["hosts"]) * world * steps
    return log, ar.apply_orders(log, world, steps)


def assert_payload_equals_replay(recs, world, want, state, table):
    """The bits comparison inside the payload ranges `table` ((lo, n) of the flat buffer; the
    padding is outside the contract): every worker's buffer, every PS's t, m and v."""
    import torch
    from oracle_common import host_bits as bits
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    for r in range(world):
        for lo, n in table:
            assert torch.equal(bits(recs[r]["params"][lo:lo + n]), bits(want[r][lo:lo + n])), r
    for p in range(len(hosts)):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        assert got["t"] == t
        lo0 = ranges[p][0]
        for lo, n in table:
            a, b = max(lo, ranges[p][0]) - lo0, min(lo + n, ranges[p][1]) - lo0
            if a < b:
                assert torch.equal(bits(got["m"][a:b]), bits(m[a:b]))
                assert torch.equal(bits(got["v"][a:b]), bits(v[a:b]))


def replay_mismatches(recs, world, params, state, spans, tag=""):
    """Lines (async_replay.mismatch_report) on where the run differs from its replay: every
    worker's whole buffer, every PS's t, parameters, m and v.  `spans` are (lo, hi, label) of the
    flat buffer, each label starting with 'PS p ' for the PS whose range it lies in; a
    difference outside every span (alignment padding) is reported too.  Empty: equal bits."""
    import torch
    import async_replay as ar
    from oracle_common import host_bits as bits
    hosts, ranges = recs[0]["hosts"], recs[0]["ranges"]
    fails = []
    for r in range(world):
        got, want = recs[r]["params"], params[r].cpu()
        lines = ar.mismatch_report(f"{tag}worker {r}", got, want, spans)
        if not lines and not torch.equal(bits(got), bits(want)):
            lines = [f"{tag}worker {r}: differs outside every span (alignment padding)"]
        fails += lines
    for p in range(len(hosts)):
        got = recs[hosts[p]]["ps"][p]
        w, m, v, t = state[p]
        lo = ranges[p][0]
        inner = [(a - lo, b - lo, label) for (a, b, label) in spans if label.startswith(f"PS {p} ")]
        if got["t"] != t:
            fails.append(f"{tag}PS {p}: t {got['t']}, replay {t}")
        for name, a, b in (("params", got["w"], w), ("m", got["m"], m), ("v", got["v"], v)):
            if a is None:
                assert name == "v" and recs[0]["cfg"]["optimizer"] in ("momentum", "sgd")
                continue
            lines = ar.mismatch_report(f"{tag}PS {p} {name}", a, b.cpu(), inner)
            if not lines and not torch.equal(bits(a), bits(b.cpu())):
                lines = [f"{tag}PS {p} {name}: differs outside every span (alignment padding)"]
            fails += lines
    return fails


# ---- 7. the W = 1 placement runs -----------------------------------------------------------------
PLACEMENTS = ((True, True), (True, False), (False, False))  # (set_use_tail, set_final_in_reduce)


def placement_run(data, opts, shard, steps, batch, tail=None, final=None, setup=None, seed=0):
    """A W = 1 synchronous native run of `steps` steps: the parameters, every server's (m, v) and
    update_launches() of the last step.  tail / final None: the runner's default placement."""
    import torch
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    cfg = TrainConfig(mode="sync", shard=shard, steps=steps, batch_size=batch, eval_every=0,
                      engine="hip", quiet=True, lr=1e-2, seed=seed, **opts)
    tr = Trainer(cfg, env, dataset=data)
    runner = tr.exchange.runner
    if tail is not None:
        runner.set_use_tail(tail)
    if final is not None:
        runner.set_final_in_reduce(final)
    if setup is not None:
        setup(tr)
    p0 = tr.params.clone()
    for i in range(steps):
        tr.train_step(i)
    torch.cuda.synchronize()
    assert not torch.equal(tr.params, p0)  # it trained
    state = [(s.m.clone(), None if s.v is None else s.v.clone())
             for _, s in sorted(tr.servers.items())]
    out = tr.params.clone(), state, runner.update_launches()
    tr.exchange.close()
    return out


def assert_same_run(a, b, has_v=None, t=None):
    """Two placement_run (or run_state) results: the same parameters, m and v (has_v: whether the
    rule keeps one).  t: every server's state is (m, v, t) and both runs' counters equal `t`."""
    import torch
    from oracle_common import bits
    (pa, sa, _), (pb, sb, _) = a, b
    assert torch.isfinite(pa).all()
    assert torch.equal(pa, pb) and torch.equal(bits(pa), bits(pb)), "parameters differ"
    assert len(sa) == len(sb) > 0
    for p, (xa, xb) in enumerate(zip(sa, sb)):
        (ma, va), (mb, vb) = xa[:2], xb[:2]
        if t is not None:
            assert xa[2] == xb[2] == t, f"PS {p}: t {xa[2]} and {xb[2]}, expected {t}"
        assert torch.equal(ma, mb) and torch.equal(bits(ma), bits(mb)), f"PS {p}: m differs"
        assert (va is None) == (vb is None)
        if has_v is not None:
            assert (va is not None) == has_v
        if va is not None:
            assert torch.equal(va, vb) and torch.equal(bits(va), bits(vb)), f"PS {p}: v differs"


# ---- 8. checkpoint and resume --------------------------------------------------------------------
def run_state(tr):
    """A trained Trainer's state in placement_run's form, with the step counters: the parameters
    and every server's (m, v, t), after the exchange has written the optimizer state it holds
    itself back into the PS objects (sync_ps_state)."""
    import torch
    torch.cuda.synchronize()
    tr.exchange.sync_ps_state()
    torch.cuda.synchronize()
    state = [(s.m.clone(), None if s.v is None else s.v.clone(), s.t)
             for _, s in sorted(tr.servers.items())]
    return tr.params.clone(), state, None


def ps_flat(tr, name):
    """The hosted servers' `name` ("m", "v") laid out as the plan's flat buffer: zeros where this
    rank hosts nothing, None where the rule keeps no such slot."""
    import torch
    out = torch.zeros_like(tr.params)
    for ps in tr.servers.values():
        buf = getattr(ps, name)
        if buf is None:
            return None
        for (lo, hi), off in zip(ps.segments, ps.seg_off):
            out[lo:hi] = buf[off:off + hi - lo]
    return out


def canon_state(tr):
    """A one-rank Trainer's parameters, m and v in canonical order on the CPU (canon): what a
    checkpoint must hold whatever the plan.  Reads the PS objects: sync_ps_state() comes first."""
    offs = tr.plan.tensor_offsets
    out = {"w": canon(tr.params, offs).cpu()}
    for name in ("m", "v"):
        flat = ps_flat(tr, name)
        out[name] = None if flat is None else canon(flat, offs).cpu()
    return out


def hosted_ps_record(tr):
    """Every hosted PS's t, m, v and (async) private parameter copy, on the CPU."""
    return {p: dict(t=s.t, m=s.m.cpu(), v=None if s.v is None else s.v.cpu(),
                    w=None if s.params is None else s.params.cpu())
            for p, s in tr.servers.items()}


def async_train_record(tr, world):
    """One asynchronous xGMI rank driven by Trainer.train() (with cfg.resume: checkpoint.load,
    then exchange.start(); join, verify_provenance, the end-of-run save and close inside): the
    record async_rank_record returns.  `init` is taken before train(), so a resumed rank's is its
    fresh initialisation, not the restored buffer; the provenance counts this job's rounds
    from 0."""
    import torch
    ex = tr.exchange
    init = tr.params.clone()
    tr.train()
    torch.cuda.synchronize()
    P = tr.plan.num_ps
    return dict(init=init.cpu(), params=tr.params.cpu(), ps=hosted_ps_record(tr),
                provenance=list(ex.provenance), served=ex.served, steps=tr.global_step,
                pushes=ex.steps, service_mode=ex.service_mode,
                ranges=[tr.plan.ps_segments(p)[0] for p in range(P)],
                hosts=[tr.plan.host_rank(p, world) for p in range(P)],
                offsets=list(tr.plan.tensor_offsets), total=tr.plan.total, cfg=tr.cfg.to_dict())
