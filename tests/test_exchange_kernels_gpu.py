"""The xGMI exchange kernels alone, on small plans, against tests/exchange_reference.py.

`xgmi_ps_kernel`, `xgmi_repl_kernel`, `xgmi_owner_kernel` (csrc/kernels/xgmi.hip) through
`PeerExchange.launch`, and `async_push_kernel` / `async_apply_kernel` (xgmi_async.hip) through
`AsyncPeer.push_all` / `apply` / `wait_done`, with no trainer around them: 3 rounds with a fresh
gradient each, at slice geometries the MNIST plan never produces (docs/DESIGN.md, "The exchange
kernels alone", has the table).  Every buffer holds a finite sentinel pattern outside the spans
the kernels own.  Every round checks, in this order,

1. the exchange's error word is 0 (if not: nothing more is launched);
2. outside the buckets, parameters, m, v and the gradient are unchanged: the state between and
   beyond the runs' state offsets, v under momentum, m under the copy rule, and the whole
   gradient buffer, which is read only;
3. inside, parameters, m and v are BIT-equal to `ops.update_flat` (the vector kernel the update
   rule tests pin) applied to the reference's rank-order sum;
4. the fp64 closed form of one step from the kernel's own previous state: relative 1e-6 on m and
   v, absolute 1e-6 on w (test_adam_kernel's and test_momentum_kernel's bounds, same magnitudes);
5. every rank's parameter replica is bit-equal.

W = 1 runs in this process (the generic `<0>` kernels and `xgmi_owner_kernel<1>`); W = 2 and 3
are one spawned job per world size on one card (gloo for the handle exchange only), which
launches several buckets in index order on one stream, the replicated bucket last, the final wait
on the last launch, with no host barrier between the rounds: the parity-slot and inbox reuse
argument of xgmi.hip's header is what runs.  Measured: see docs/DESIGN.md."""
import os
import time

import pytest
import torch

import onecard as oc
from conftest import free_port
from onecard import rel_err as _rel

import exchange_reference as xr
from exchange_reference import ADAM, MOMENTUM, COPY, B1, B2, EPS

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = xr.N_BUF
ROUNDS = 3
TOL = 1e-6
THIRD = xr.COEF3


def _snap(t):
    """A host copy that shares nothing with the device buffer."""
    return t.detach().cpu().clone()


# ---- plans ---------------------------------------------------------------------------------------
def owner_bucket(runs, owner, base):
    """An owner bucket of `runs` (sizes): the runs out of order and non-adjacent in the plan
    buffer from `base` on, their state offsets shuffled and non-adjacent.  Returns it and the
    plan offset behind it."""
    k = len(runs)
    lo, so = [0] * k, [0] * k
    pos = base
    for i, idx in enumerate(reversed(range(k))):  # plan order: the last run first
        lo[idx] = pos
        pos += runs[idx] + (8 if i % 2 else 4)
    spos = 4
    for i, idx in enumerate(list(range(1, k, 2)) + list(range(0, k, 2))):  # state: odd runs first
        so[idx] = spos
        spos += runs[idx] + (4 if i % 2 else 12)
    return ("owner", [(lo[i], lo[i] + runs[i]) for i in range(k)], so, owner), pos


def equal_cell(c, world, max_slices, plain=True, repl=True):
    """Chunk size c: an equal-chunk bucket of c * world and / or the replicated bucket of c."""
    buckets, pos = [], 8
    if plain:
        buckets.append(("equal", pos, pos + c * world, 8))
        pos += c * world + 12
    if repl:
        buckets.append(("equal", pos, pos + c, 4))
    ns = len(xr.equal_slices(c, max_slices))
    return dict(buckets=buckets, repl=len(buckets) - 1 if repl else -1, max_slices=max_slices,
                nslices=[ns] * len(buckets))


def owner_cell(run_sets, owners, max_slices=128):
    buckets, pos, ns = [], 12, []
    for runs, o in zip(run_sets, owners):
        b, pos = owner_bucket(runs, o, pos)
        buckets.append(b)
        ns.append(len(xr.owner_slices(runs, max_slices)[0]))
    return dict(buckets=buckets, repl=-1, max_slices=max_slices, nslices=ns)


def _spans(bucket):
    return bucket[1] if bucket[0] == "owner" else [(bucket[1], bucket[2])]


def _state_len(bucket, world, repl):
    if bucket[0] == "owner":
        return max(so + hi - lo for (lo, hi), so in zip(bucket[1], bucket[2])) + 8
    n = bucket[2] - bucket[1]
    return bucket[3] + (n if repl else n // world) + 8


class Failures(list):
    """The first failed check of each cell (later checks of a cell whose state already differs
    say nothing new); the rounds go on, so every rank keeps the same sequence of launches."""

    def __init__(self):
        super().__init__()
        self.cell = None
        self.open = True

    def begin(self, cell):
        self.cell, self.open = cell, True

    def check(self, ok, what):
        if self.open and not ok:
            self.append(f"{self.cell}: {what}")
            self.open = False
        return bool(ok)


# ---- one synchronous cell ------------------------------------------------------------------------
def run_sync_cell(ops, rank, world, cell, rule, gather, fails, integer=False):
    """ROUNDS rounds of one PeerExchange.  rule = (kind, mu, scale, coef).  Returns the error
    word any rank saw (non-zero: the job must stop)."""
    kind, mu, scale, coef = rule
    buckets, repl = cell["buckets"], cell["repl"]
    nb = len(buckets)
    regions = [xr.bucket_regions(b, world, i == repl) for i, b in enumerate(buckets)]
    live = torch.zeros(N, dtype=torch.bool)
    for b in buckets:
        for lo, hi in _spans(b):
            assert 0 <= lo < hi <= N and not live[lo:hi].any()
            live[lo:hi] = True
    w_init = torch.where(live, xr.initial_state(N, 1)[0], xr.sentinel(N, 100))
    g_pad = xr.sentinel(N, -50)

    def state_init(b, r):
        sl = _state_len(buckets[b], world, b == repl)
        # (the replicated bucket's state is replicated: the same on every rank)
        _, m0, v0 = xr.initial_state(sl, 100 + 10 * b + (0 if b == repl else r))
        mask = torch.zeros(sl, dtype=torch.bool)
        for _, n, so in regions[b][r]:
            assert not mask[so:so + n].any()
            mask[so:so + n] = True
        return torch.where(mask, m0, xr.sentinel(sl, -7)), torch.where(mask, v0, xr.sentinel(sl, 3)), mask

    init = [[state_init(b, r) for r in range(world)] for b in range(nb)]
    base = [0 if buckets[b][0] == "owner" else buckets[b][3] for b in range(nb)]
    # the bit-exact expectation of every rank's state, advanced with ops.update_flat
    exp_p = [w_init.to(DEV) for _ in range(world)]
    exp_m = [[init[b][r][0].to(DEV) for r in range(world)] for b in range(nb)]
    exp_v = [[init[b][r][1].to(DEV) for r in range(world)] for b in range(nb)]
    P, G = w_init.to(DEV), torch.empty(N, device=DEV)
    M = [init[b][rank][0].to(DEV) for b in range(nb)]
    V = [init[b][rank][1].to(DEV) for b in range(nb)]
    mask = [init[b][rank][2] for b in range(nb)]
    specs = [(b[1], b[2], b[3]) if b[0] == "owner" else (b[1], b[2]) for b in buckets]
    ex = ops.PeerExchange(P, G, world, rank, specs, cell["max_slices"], repl)
    err, snaps = 0, []
    try:
        ex.open(gather(ex.handle()))
        fails.check(list(ex.nslices()) == cell["nslices"],
                    f"slices {list(ex.nslices())}, host arithmetic says {cell['nslices']}")
        for e in range(1, ROUNDS + 1):
            grads = [torch.where(live, g, g_pad)
                     for g in xr.round_gradients(world, e, integer=integer)]
            G.copy_(grads[rank])
            torch.cuda.synchronize()
            prev_p = [_snap(t) for t in exp_p]
            prev_m = [[_snap(t) for t in row] for row in exp_m]
            prev_v = [[_snap(t) for t in row] for row in exp_v]
            prev_p[rank] = _snap(P)  # this rank: the kernel's own previous state
            for b in range(nb):
                prev_m[b][rank], prev_v[b][rank] = _snap(M[b]), _snap(V[b])
            step = xr.step_size(kind, e)
            for b in range(nb):
                ex.launch(b, e, kind, M[b][base[b]:], V[b][base[b]:], step, B1, B2, EPS, mu,
                          scale, coef, b == nb - 1)
            torch.cuda.synchronize()
            err = ex.error()
            if not fails.check(err == 0, f"round {e}: error word {err}"):
                break
            new_p, new_g = _snap(P), _snap(G)
            new_m, new_v = [_snap(t) for t in M], [_snap(t) for t in V]
            snaps.append(new_p)
            # the expectation: update_flat on the rank-order sum, on every rank's spans
            gsum = xr.rank_order_sum(grads, coef)
            gdev = gsum.to(DEV)
            for b in range(nb):
                for r in range(world):
                    for lo, n, so in regions[b][r]:
                        ops.update_flat(kind, exp_p[r][lo:lo + n], gdev[lo:lo + n],
                                        exp_m[b][r][so:so + n],
                                        exp_v[b][r][so:so + n] if kind == ADAM else None,
                                        step, B1, B2, EPS, mu, scale)
                        for q in range(world):
                            if q != r and b != repl:
                                exp_p[q][lo:lo + n].copy_(exp_p[r][lo:lo + n])
            torch.cuda.synchronize()
            tag = f"round {e}: "
            # 2. outside the buckets
            fails.check(torch.equal(new_p[~live], w_init[~live]), tag + "params outside the buckets")
            fails.check(torch.equal(new_g, grads[rank]), tag + "the gradient buffer changed")
            for b in range(nb):
                m0, v0, mk = init[b][rank]
                fails.check(torch.equal(new_m[b][~mk], m0[~mk]), tag + f"m outside bucket {b}'s state")
                fails.check(torch.equal(new_v[b][~mk], v0[~mk]), tag + f"v outside bucket {b}'s state")
                if kind != ADAM:
                    fails.check(torch.equal(new_v[b], v0), tag + f"v of bucket {b} under a rule without v")
                if kind == COPY:
                    fails.check(torch.equal(new_m[b], m0), tag + f"m of bucket {b} under the copy rule")
            # 3. inside: the bits of update_flat on the rank-order sum
            want_p = _snap(exp_p[rank])
            bad = (new_p != want_p) & live
            fails.check(not bad.any(), tag + f"params differ from update_flat(rank-order sum) at "
                        f"{int(bad.sum())} elements, first {int(bad.nonzero()[0]) if bad.any() else -1}")
            for b in range(nb):
                fails.check(torch.equal(new_m[b], _snap(exp_m[b][rank])), tag + f"m of bucket {b}: bits")
                fails.check(torch.equal(new_v[b], _snap(exp_v[b][rank])), tag + f"v of bucket {b}: bits")
            if integer:
                exact = sum(g.double() for g in grads)
                fails.check(torch.equal(new_p.double()[live], exact[live]), tag + "copy of integer sums")
            # 4. one step of the fp64 closed form from the kernel's own previous state
            p64 = prev_p
            for b in range(nb):
                p64, m64, v64 = xr.sync_round(p64, prev_m[b], prev_v[b], grads, regions[b],
                                              b == repl, kind, step, mu, scale, coef)
                if mask[b].any() and kind != COPY:
                    r_m = _rel(new_m[b][mask[b]], m64[rank][mask[b]])
                    fails.check(r_m < TOL, tag + f"m of bucket {b}: relative {r_m:.3e} from the closed form")
                if mask[b].any() and kind == ADAM:
                    r_v = _rel(new_v[b][mask[b]], v64[rank][mask[b]])
                    fails.check(r_v < TOL, tag + f"v of bucket {b}: relative {r_v:.3e} from the closed form")
            d_w = float((new_p.double() - p64[rank])[live].abs().max())
            fails.check(d_w < TOL, tag + f"w: {d_w:.3e} from the closed form")
        # 5. the replicas (gathered after the rounds: no host barrier between them)
        got = gather((err, snaps))
        for e in range(min(len(s) for _, s in got)):
            fails.check(all(torch.equal(s[e], got[0][1][e]) for _, s in got),
                        f"round {e + 1}: the ranks' parameter replicas differ")
        err = max(x for x, _ in got)
        # unmap, barrier, free, barrier: this process goes on to build the next cell's exchange
        # (why: tests/onecard.py, close_one_of_several)
        ex.unmap_peers()
        gather(None)
        ex.close()
        gather(None)
    finally:
        ex.close()
    return err


# ---- one asynchronous cell -----------------------------------------------------------------------
def run_async_cell(ops, rank, world, sizes, hosts, max_slices, rule, elide, gather, fails, name):
    """ROUNDS rounds of one AsyncPeer in the order of parallel/async_xgmi.py _selftest: push_all,
    stream sync, barrier, each host's applies for worker 0..W-1, wait_done, barrier."""
    kind, mu, scale, coef = rule
    os.environ["DDL_ASYNC_ELIDE_LOCAL"] = "1" if elide else "0"
    shards, pos = [], 8
    for i, (n, h) in enumerate(zip(sizes, hosts)):
        shards.append((pos, n, h))
        pos += n + (12 if i % 2 else 4)
    assert pos <= N
    live = torch.zeros(N, dtype=torch.bool)
    for lo, n, _ in shards:
        live[lo:lo + n] = True
    w_init = torch.where(live, xr.initial_state(N, 2)[0], xr.sentinel(N, 100))
    g_pad = xr.sentinel(N, -50)
    PAD = 8

    def ps_init(p):
        lo, n, _ = shards[p]
        _, m0, v0 = xr.initial_state(n + 2 * PAD, 300 + p)
        mk = torch.zeros(n + 2 * PAD, dtype=torch.bool)
        mk[PAD:PAD + n] = True
        w0 = xr.sentinel(n + 2 * PAD, 55)
        w0[PAD:PAD + n] = w_init[lo:lo + n]
        return w0, torch.where(mk, m0, xr.sentinel(n + 2 * PAD, -7)), \
            torch.where(mk, v0, xr.sentinel(n + 2 * PAD, 3)), mk

    init = [ps_init(p) for p in range(len(shards))]
    inner = lambda t, p: t[PAD:PAD + shards[p][1]]  # noqa: E731
    exp = [[inner(t, p).to(DEV).clone() for t in init[p][:3]] for p in range(len(shards))]
    mine = [p for p, (_, _, h) in enumerate(shards) if h == rank]
    ps = {p: [t.to(DEV) for t in init[p][:3]] for p in mine}
    P, G = w_init.to(DEV), torch.empty(N, device=DEV)
    peer = ops.AsyncPeer(P, G, world, rank, [(lo, lo + n) for lo, n, _ in shards], list(hosts),
                         max_slices)
    dead = 0
    try:
        peer.open(gather(peer.handle()))
        if rank == 0:
            peer.attach_done(name, True)
        gather(None)
        if rank != 0:
            peer.attach_done(name, False)
        gather(None)
        for e in range(1, ROUNDS + 1):
            grads = [torch.where(live, g, g_pad) for g in xr.round_gradients(world, e)]
            G.copy_(grads[rank])
            torch.cuda.synchronize()
            t0 = [(e - 1) * world] * len(shards)
            start = {p: [_snap(inner(t, p)) for t in ps[p]] for p in mine}
            exp_start = [[_snap(t) for t in exp[p]] for p in range(len(shards))]
            peer.push_all(e, coef)
            torch.cuda.synchronize()
            gather(None)  # every push has completed before any apply is issued
            hist = {p: [] for p in mine}
            for p in mine:
                for q in range(world):
                    step = xr.step_size(kind, t0[p] + q + 1)
                    peer.apply(p, q, e, kind, inner(ps[p][0], p), inner(ps[p][1], p),
                               inner(ps[p][2], p), step, B1, B2, EPS, step, mu, scale)
                    torch.cuda.synchronize()
                    hist[p].append([_snap(t) for t in ps[p]])
            ok = peer.wait_done(e, 10.0)
            torch.cuda.synchronize()
            err = peer.error()
            fails.check(ok and err == 0, f"round {e}: wait_done {ok}, error word {err}")
            dead = max(int(x) for x in gather(int(err != 0 or not ok)))
            if dead:
                break
            new_p, new_g = _snap(P), _snap(G)
            # the expectation: update_flat per apply, in worker order, on every PS
            chain = []
            for p, (lo, n, _) in enumerate(shards):
                chain.append([])
                for q in range(world):
                    g = xr.scaled(grads[q][lo:lo + n], coef).to(DEV)
                    ops.update_flat(kind, exp[p][0], g, exp[p][1], exp[p][2] if kind == ADAM else None,
                                    xr.step_size(kind, t0[p] + q + 1), B1, B2, EPS, mu, scale)
                    chain[p].append([_snap(t) for t in exp[p]])
            tag = f"round {e}: "
            # 2. outside the shards
            fails.check(torch.equal(new_p[~live], w_init[~live]), tag + "params outside the shards")
            fails.check(torch.equal(new_g, grads[rank]), tag + "the gradient buffer changed")
            for p in mine:
                w0, m0, v0, mk = init[p]
                for q in range(world):
                    w1, m1, v1 = hist[p][q]
                    fails.check(torch.equal(w1[~mk], w0[~mk]) and torch.equal(m1[~mk], m0[~mk]) and
                                torch.equal(v1[~mk], v0[~mk]), tag + f"PS {p}: outside its copy / state")
                    if kind != ADAM:
                        fails.check(torch.equal(v1, v0), tag + f"PS {p}: v under a rule without v")
            # 3. bits: each apply on the PS copy, and the shard every worker got back
            for p in mine:
                for q in range(world):
                    for name_, a, b in zip("wmv", hist[p][q], chain[p][q]):
                        fails.check(torch.equal(inner(a, p), b),
                                    tag + f"PS {p} after worker {q}: {name_} differs from update_flat")
            for p, (lo, n, _) in enumerate(shards):
                fails.check(torch.equal(new_p[lo:lo + n], chain[p][rank][0]),
                            tag + f"worker buffer, shard of PS {p}")
            # 4. closed forms.  Per apply, one step from the PS's own previous state; over the
            # round, async_round from the round's start: W one-step bounds (the errors of
            # successive steps add: each rule maps an error in m, v to a smaller one, factor
            # mu or beta, and carries an error in w over unchanged)
            for p in mine:
                lo, n, _ = shards[p]
                before = start[p]
                for q in range(world):
                    w64, m64, v64 = xr.rule_step(kind, *before, xr.scaled(grads[q][lo:lo + n], coef),
                                                 xr.step_size(kind, t0[p] + q + 1), mu, scale)
                    now = [inner(t, p) for t in hist[p][q]]
                    d_w = float((now[0].double() - w64).abs().max())
                    fails.check(d_w < TOL, tag + f"PS {p} apply {q}: w {d_w:.3e} from the closed form")
                    if kind != COPY:
                        fails.check(_rel(now[1], m64) < TOL, tag + f"PS {p} apply {q}: m")
                    if kind == ADAM:
                        fails.check(_rel(now[2], v64) < TOL, tag + f"PS {p} apply {q}: v")
                    before = now
            ref_start = [start[p] if p in start else exp_start[p] for p in range(len(shards))]
            after, workers = xr.async_round(ref_start, grads, shards, kind, t0, mu, scale, coef)
            for p, (lo, n, _) in enumerate(shards):
                d_w = float((new_p[lo:lo + n].double() - workers[rank][p]).abs().max())
                fails.check(d_w < world * TOL, tag + f"worker shard of PS {p}: {d_w:.3e} from async_round")
            for p in mine:
                w1, m1, v1 = [inner(t, p) for t in hist[p][-1]]
                fails.check(float((w1.double() - after[p][-1][0]).abs().max()) < world * TOL,
                            tag + f"PS {p} copy from async_round")
                if kind != COPY:
                    fails.check(_rel(m1, after[p][-1][1]) < world * TOL, tag + f"PS {p} m from async_round")
                if kind == ADAM:
                    fails.check(_rel(v1, after[p][-1][2]) < world * TOL, tag + f"PS {p} v from async_round")
        gather(None)
        peer.unmap_peers()  # (unmap, barrier, free, barrier: see run_sync_cell)
        gather(None)
        peer.close()
        gather(None)
    finally:
        peer.close()
    return dead


# ---- W = 1, in this process ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from ddl_amd.ops import native
    assert native.available(), native.error()
    saved = os.environ.get("DDL_XGMI_TIMEOUT_S")
    os.environ["DDL_XGMI_TIMEOUT_S"] = "10"
    yield native.ops()
    if saved is None:
        os.environ.pop("DDL_XGMI_TIMEOUT_S", None)
    else:
        os.environ["DDL_XGMI_TIMEOUT_S"] = saved


RULES_W1 = [(kind, mu, scale, coef)
            for kind, mu in [(ADAM, 0.0), (MOMENTUM, 0.9), (MOMENTUM, 0.0), (COPY, 0.0)]
            for coef in (1.0, THIRD) for scale in (1.0, 0.5)]

EQUAL_W1 = [(4, 128, 1), (1020, 128, 1), (1024, 128, 1), (1028, 128, 2), (3076, 128, 4),
            (4100, 1, 1), (4100, 2, 2), (7172, 128, 8)]
OWNER_W1 = [([4], 128, 1), ([4] * 8, 128, 8), ([1028, 4, 2052], 128, 6),
            ([3000, 100, 1500, 8], 128, 8), ([2052, 1028], 2, 3), ([5000, 40], 1, 3)]


def _sweep(ops, cell):
    fails = Failures()
    for rule in RULES_W1:
        fails.begin(f"kind {rule[0]} mu {rule[1]} scale {rule[2]} coef {rule[3]:.4f}")
        err = run_sync_cell(ops, 0, 1, cell, rule, lambda x: [x], fails)
        if err:
            break  # an error word: nothing more is launched
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("repl", [False, True], ids=["plain", "replicated"])
@pytest.mark.parametrize("c,max_slices,nslices", EQUAL_W1)
def test_equal_chunk_geometries_w1(ops, c, max_slices, nslices, repl):
    cell = equal_cell(c, 1, max_slices, plain=not repl, repl=repl)
    assert cell["nslices"] == [nslices]  # the table of docs/DESIGN.md
    _sweep(ops, cell)


@pytest.mark.parametrize("runs,max_slices,nslices", OWNER_W1)
def test_owner_geometries_w1(ops, runs, max_slices, nslices):
    cell = owner_cell([runs], [0], max_slices)
    assert cell["nslices"] == [nslices]
    _sweep(ops, cell)


@pytest.mark.parametrize("elide,coef", [(1, 1.0), (0, THIRD)])
@pytest.mark.parametrize("sizes,max_slices", [([4, 2044, 2052, 4100], 512), ([4100, 4], 1),
                                              ([6148, 2052], 2)])
def test_async_push_apply_w1(ops, sizes, max_slices, elide, coef):
    fails = Failures()
    saved = os.environ.get("DDL_ASYNC_ELIDE_LOCAL")
    try:
        for k, (kind, mu, scale) in enumerate([(ADAM, 0.0, 1.0), (MOMENTUM, 0.9, 0.5),
                                               (MOMENTUM, 0.0, 1.0), (COPY, 0.0, 1.0)]):
            fails.begin(f"kind {kind} mu {mu} scale {scale} coef {coef:.4f} elide {elide}")
            if run_async_cell(ops, 0, 1, sizes, [0] * len(sizes), max_slices,
                              (kind, mu, scale, coef), elide, lambda x: [x], fails,
                              f"/ddl_xk_{os.getpid()}_{k}"):
                break
    finally:
        if saved is None:
            os.environ.pop("DDL_ASYNC_ELIDE_LOCAL", None)
        else:
            os.environ["DDL_ASYNC_ELIDE_LOCAL"] = saved
    assert not fails, "\n".join(fails)


# ---- W = 2 and 3: one spawned job per world size, all on one card -------------------------------
def sync_cells(world):
    """(name, cell, rule, integer) of the multi-process job, each run with DDL_XGMI_CHECK off and on."""
    plans = [(f"equal+repl c={c} max_slices={ms}", equal_cell(c, world, ms))
             for c, ms in [(4, 128), (1028, 128), (3076, 128), (4100, 1)]]
    for o in [(0, world - 1), (world - 1, 0)]:
        plans.append((f"owners {o}", owner_cell([[1028, 4, 2052], [3000, 100, 1500, 8]], o)))
    out = []
    for name, cell in plans:
        out.append((name + " adam", cell, (ADAM, 0.0, 1.0, THIRD), False))
        out.append((name + " momentum", cell, (MOMENTUM, 0.9, 1.0 / world, 1.0), False))
    # one copy-rule round over all three bucket kinds, integer gradients: exact sums
    b0 = ("equal", 8, 8 + 1028 * world, 8)
    b1, pos = owner_bucket([1028, 4, 2052], world - 1, b0[2] + 12)
    mixed = dict(buckets=[b0, b1, ("equal", pos + 4, pos + 4 + 1028, 4)], repl=2, max_slices=128,
                 nslices=[2, 6, 2])
    out.append(("copy, integer gradients", mixed, (COPY, 0.0, 1.0, 1.0), True))
    return out


ASYNC_W3 = dict(sizes=[4, 2052, 4100, 2044], hosts=[0, 2, 2, 1])


def _job(rank, world, port, outdir):
    with oc.rank_session(rank, world, port, xgmi_timeout_s="10", on_device_0=True) as me:
        from ddl_amd.ops import native
        dist = me.dist
        assert native.available(), native.error()
        ops = native.ops()

        def gather(x):
            out = [None] * world
            dist.all_gather_object(out, x)
            return out

        fails, times, stopped = Failures(), {}, 0
        for check in ("0", "1"):
            os.environ["DDL_XGMI_CHECK"] = check
            for name, cell, rule, integer in sync_cells(world):
                if stopped:
                    break
                fails.begin(f"W={world} check={check} {name}")
                t = time.perf_counter()
                stopped = run_sync_cell(ops, rank, world, cell, rule, gather, fails, integer)
                times[fails.cell] = time.perf_counter() - t
        if world == 3:
            k = 0
            for elide, coef in [(1, 1.0), (0, THIRD)]:
                for kind, mu, scale in [(ADAM, 0.0, 1.0), (MOMENTUM, 0.9, 1.0 / world)]:
                    if stopped:
                        break
                    fails.begin(f"W=3 async kind {kind} elide {elide} coef {coef:.4f}")
                    t = time.perf_counter()
                    stopped = run_async_cell(ops, rank, world, ASYNC_W3["sizes"], ASYNC_W3["hosts"],
                                             512, (kind, mu, scale, coef), elide, gather, fails,
                                             f"/ddl_xk_{port}_{k}")
                    times[fails.cell] = time.perf_counter() - t
                    k += 1
        torch.cuda.synchronize()
        torch.save({"fails": list(fails), "times": times, "stopped": stopped},
                   os.path.join(outdir, f"rank{rank}.pt"))


@pytest.mark.slow
@pytest.mark.parametrize("world", [2, 3])
def test_exchange_kernels_multiprocess(tmp_path, world):
    t = time.perf_counter()
    oc.run_ranks(_job, world, free_port(), str(tmp_path), limit_s=oc.LIMIT_S)
    wall = time.perf_counter() - t
    recs = oc.load_ranks(tmp_path, world)
    cells = sum(recs[0]["times"].values())
    print(f"W={world}: job {wall:.1f} s, of which {len(recs[0]['times'])} cells {cells:.2f} s")
    fails = [f"rank {r}: {f}" for r, rec in enumerate(recs) for f in rec["fails"]]
    assert not fails, "\n".join(fails)
    assert not any(rec["stopped"] for rec in recs)
    want = 2 * len(sync_cells(world)) + (4 if world == 3 else 0)
    assert all(len(rec["times"]) == want for rec in recs)
