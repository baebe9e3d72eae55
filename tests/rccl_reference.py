"""What the native sync runner must ask of RCCL as rank r of a world of W, and a plain torch twin
of the fake communicator that answers it (csrc/kernels/fake_rccl.hip).  Helper module, CPU only.

* `expected(plan, segments, world, rank)`: the exchanges of one step, derived from the ShardPlan
  and the engine's backward segments alone (never from the runner's or the exchange's units).
* `check_calls(log, exps)`: the fake's call log against them, as a multiset plus ordering rules.
* `Twin`: the fake's table of semantics on CPU tensors, with the same fault knobs.
* `walk_rank`: one rank's step through the expected exchanges with the twin and a plain per-range
  update: the closed loop of tests/test_rccl_ranks_cpu.py, with the mutations that prove the
  oracle can tell a wrong chunk, root or state offset from a right one.

The sums are in rank order, a left fold from +0, like the fake's, onecard.simulate_sync's and the
xGMI owner kernels'.
"""
from collections import Counter, namedtuple

import torch

# One exchange of one plan range.  kind "rs": ReduceScatter(grads + lo, shard, c), an update of
# chunk `rank`, AllGather in place at params + lo + rank * c.  "ar": one in-place AllReduce of
# [lo, lo + n) and an update on replicated state.  "reduce": Reduce(root) of grads [lo, lo + n),
# an update on the root, Broadcast(root) of params.  ps / state_off: whose optimizer state the
# update reads and where in it (ar: the replicated state, offset 0).  unit: the ranges that must
# share one stream.
Exp = namedtuple("Exp", "kind lo n c root ps state_off unit")

FAULTS = ("rs_next_chunk", "ag_skip", "reduce_drop_peer", "bcast_skip")


def _extent(plan, i):
    from ddl_amd.models.layout import TENSORS
    from ddl_amd.parallel.sharding import TENSOR_ALIGN
    n = -(-TENSORS[i].numel // TENSOR_ALIGN) * TENSOR_ALIGN
    return plan.tensor_offsets[i], plan.tensor_offsets[i] + n


def last_bucket(plan, segments):
    """The flat plan's bucket that holds the last backward segment's tensors."""
    last = set(segments[-1])
    hit = [b for b, ids in enumerate(plan.meta["buckets"]) if last <= set(ids)]
    assert len(hit) == 1, hit
    return hit[0]


def expected(plan, segments, world, rank, repl_last=True, overlap=True):
    """The exchanges of one step on rank `rank`, in no particular order."""
    W, out = world, []
    if plan.bucket_ranges is not None:
        chunks = [(hi - lo) // plan.num_ps for lo, hi in plan.bucket_ranges]
        if plan.num_ps == W:
            rb = last_bucket(plan, segments) if repl_last else -1
            for b, (lo, hi) in enumerate(plan.bucket_ranges):
                if b == rb:
                    out.append(Exp("ar", lo, hi - lo, hi - lo, -1, rank, 0, ("bucket", b)))
                else:
                    out.append(Exp("rs", lo, hi - lo, chunks[b], -1, rank, sum(chunks[:b]),
                                   ("bucket", b)))
            return out
        for b, (lo, hi) in enumerate(plan.bucket_ranges):
            for p in range(plan.num_ps):
                out.append(Exp("reduce", lo + p * chunks[b], chunks[b], chunks[b], p % W, p,
                               sum(chunks[:b]), ("bucket", b, p)))
        return out
    segs = [sorted(s) for s in segments] if overlap else [sorted(i for s in segments for i in s)]
    for p in range(plan.num_ps):
        ps_lo = plan.ps_ranges[p][0]
        for k, seg in enumerate(segs):
            runs = []
            for i in sorted((i for i in seg if plan.owner[i] == p),
                            key=lambda i: plan.tensor_offsets[i]):
                lo, hi = _extent(plan, i)
                if runs and runs[-1][1] == lo:
                    runs[-1][1] = hi
                else:
                    runs.append([lo, hi])
            for lo, hi in runs:
                out.append(Exp("reduce", lo, hi - lo, hi - lo, p % W, p, lo - ps_lo, ("ps", p, k)))
    return out


def update_launches(exps, rank):
    """Stand-alone update launches of one step on `rank`: one per range it updates."""
    return sum(1 for e in exps if e.n > 0 and (e.kind in ("rs", "ar") or e.root == rank))


def calls_of(e, rank):
    """(first, then) of an exchange as (op, buffer, offset, count, root, recv buffer, recv offset);
    a shard receive is ("shard", 0).  `then` is None for an all-reduce."""
    if e.kind == "rs":
        return (("ReduceScatter", "grads", e.lo, e.c, -1, "shard", 0),
                ("AllGather", "params", e.lo + rank * e.c, e.c, -1, "params", e.lo))
    if e.kind == "ar":
        return ("AllReduce", "grads", e.lo, e.n, -1, "grads", e.lo), None
    return (("Reduce", "grads", e.lo, e.n, e.root, "grads", e.lo),
            ("Broadcast", "params", e.lo, e.n, e.root, "params", e.lo))


def _key(entry):
    op, buf, off, count, root, _stream, _depth, rbuf, roff = entry
    if rbuf.startswith("shard"):
        rbuf = "shard"
    return (op, buf, off, count, root, rbuf, roff)


def check_calls(log, exps, rank):
    """The fake's call log of ONE step against the expected exchanges: the collectives as a
    multiset; a range's ReduceScatter / Reduce ahead of its AllGather / Broadcast, on the same
    stream; the collectives of a unit on one stream; group brackets that balance without
    nesting.  Returns a list of complaints (empty: satisfied)."""
    bad = []
    depth = 0
    for e in log:
        if e[0] == "GroupStart":
            depth += 1
            if depth > 1:
                bad.append("nested group")
        elif e[0] == "GroupEnd":
            depth -= 1
            if depth < 0:
                bad.append("GroupEnd without GroupStart")
                depth = 0
    if depth != 0:
        bad.append(f"{depth} group(s) left open")
    coll = [(i, e) for i, e in enumerate(log) if not e[0].startswith("Group")]
    got = Counter(_key(e) for _, e in coll)
    want = Counter()
    for x in exps:
        first, then = calls_of(x, rank)
        want[first] += 1
        if then is not None:
            want[then] += 1
    for k in sorted((got - want).keys(), key=str):
        bad.append(f"unexpected call {k} x{(got - want)[k]}")
    for k in sorted((want - got).keys(), key=str):
        bad.append(f"missing call {k} x{(want - got)[k]}")
    where = {}
    for i, e in coll:
        where.setdefault(_key(e), []).append((i, e[5]))
    streams = {}
    for x in exps:
        first, then = calls_of(x, rank)
        a, b = where.get(first), where.get(then) if then is not None else None
        for hit in (a, b):
            if hit:
                streams.setdefault(x.unit, set()).add(hit[0][1])
        if a and b:
            if not a[0][0] < b[0][0]:
                bad.append(f"{then[0]} of [{x.lo}, {x.lo + x.n}) ahead of its {first[0]}")
            if a[0][1] != b[0][1]:
                bad.append(f"{first[0]} and {then[0]} of [{x.lo}, {x.lo + x.n}) on two streams")
    for unit, ss in streams.items():
        if len(ss) > 1:
            bad.append(f"unit {unit} on {len(ss)} streams")
    return bad


# ---- the fake's semantics on CPU tensors ---------------------------------------------------------
def fold(rows):
    """The rank-order sum of float32 rows as a left fold from +0."""
    acc = torch.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


class Twin:
    """The fake communicator of rank `rank`: peer_grads [W, total] (row `rank` ignored, the live
    buffer is used), params_next [total].  Buffers are addressed as (tensor, offset)."""

    def __init__(self, world, rank, peer_grads, params_next, fault=None):
        assert fault is None or fault in FAULTS
        self.W, self.r, self.pg, self.pn, self.fault = world, rank, peer_grads, params_next, fault

    def _sum(self, own, off, n, skip=-1):
        return fold([own if q == self.r else self.pg[q, off:off + n]
                     for q in range(self.W) if q != skip])

    def reduce_scatter(self, grads, lo, c):
        k = (self.r + 1) % self.W if self.fault == "rs_next_chunk" else self.r
        off = lo + k * c
        return self._sum(grads[off:off + c], off, c)

    def all_gather(self, params, lo, c):
        if self.fault == "ag_skip":
            return
        for q in range(self.W):
            if q != self.r:
                params[lo + q * c:lo + (q + 1) * c] = self.pn[lo + q * c:lo + (q + 1) * c]

    def all_reduce(self, grads, lo, n):
        grads[lo:lo + n] = self._sum(grads[lo:lo + n], lo, n)

    def reduce(self, grads, lo, n, root):
        assert 0 <= root < self.W
        if root != self.r:
            return
        skip = -1
        if self.fault == "reduce_drop_peer":
            skip = self.W - 2 if self.r == self.W - 1 else self.W - 1
        grads[lo:lo + n] = self._sum(grads[lo:lo + n], lo, n, skip)

    def broadcast(self, params, lo, n, root):
        assert 0 <= root < self.W
        if root != self.r and self.fault != "bcast_skip":
            params[lo:lo + n] = self.pn[lo:lo + n]


# ---- the closed loop -------------------------------------------------------------------------------
MUTATIONS = ("next_chunk", "root_plus_1", "no_broadcast", "no_all_gather", "plan_offset_state")


def plain_update(w, g, m):
    """A plain momentum rule, elementwise, in place: the same bits however the buffer is cut."""
    m.mul_(0.5).add_(g)
    w.sub_(m, alpha=0.125)


class RankState:
    """One rank's replica: parameters and, per PS (or "repl"), optimizer state.  Every state
    buffer has the plan buffer's length, so that a wrong offset reads wrong values, not past the
    end."""

    def __init__(self, params0):
        self.params = params0.clone()
        self.total = params0.numel()
        self.m = {}

    def state(self, key):
        if key not in self.m:
            self.m[key] = torch.zeros(self.total)
        return self.m[key]


def walk_rank(st, exps, world, rank, grads_all, params_next, mutation=None):
    """One step of rank `rank`: its own gradient row is its live buffer, the twin answers for the
    peers.  `mutation` makes the walk wrong in one of the ways the GPU test must catch."""
    assert mutation is None or mutation in MUTATIONS
    twin = Twin(world, rank, grads_all, params_next,
                "rs_next_chunk" if mutation == "next_chunk" else None)
    g, w = grads_all[rank].clone(), st.params
    for e in exps:
        if e.kind == "rs":
            shard = twin.reduce_scatter(g, e.lo, e.c)
            mine = e.lo + rank * e.c
            off = mine if mutation == "plan_offset_state" else e.state_off
            plain_update(w[mine:mine + e.c], shard, st.state(e.ps)[off:off + e.c])
            if mutation != "no_all_gather":
                twin.all_gather(w, e.lo, e.c)
        elif e.kind == "ar":
            twin.all_reduce(g, e.lo, e.n)
            plain_update(w[e.lo:e.lo + e.n], g[e.lo:e.lo + e.n], st.state("repl")[0:e.n])
        else:
            root = (e.root + 1) % world if mutation == "root_plus_1" else e.root
            twin.reduce(g, e.lo, e.n, root)
            if rank == e.root:  # (the update stays where the PS lives)
                off = e.lo if mutation == "plan_offset_state" else e.state_off
                plain_update(w[e.lo:e.lo + e.n], g[e.lo:e.lo + e.n],
                             st.state(e.ps)[off:off + e.n])
            if mutation != "no_broadcast":
                twin.broadcast(w, e.lo, e.n, root)


def oracle_step(params, m, grads_all):
    """The PS result of one step on the whole buffer: the rank-order sum, one plain update."""
    plain_update(params, fold(list(grads_all)), m)
