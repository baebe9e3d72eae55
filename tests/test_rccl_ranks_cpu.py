"""The oracle of tests/test_rccl_ranks_gpu.py on the CPU (tests/rccl_reference.py): what the RCCL
branch of the native sync runner must ask of RCCL as rank r of W > 1, and the twin of the fake
communicator that answers it.

a. Closed loop.  Plans flat, contiguous, greedy and none at W = 2, 3, 8 and flat with P = 2 PS on
   W = 4 ranks; random INTEGER gradients per rank (every sum is exact in float32, in any order);
   every rank walks two steps through `expected()` with the twin and a plain per-range update.
   Every rank's parameter buffer, and the state of every PS it hosts, equals the rank-order-sum PS
   result bit for bit.
b. The oracle discriminates.  Each mutation of the walk (chunk (rank + 1) % W, root + 1, no
   Broadcast, no AllGather, m taken at the plan offset where the shard offset is meant) makes at
   least one rank's parameters differ (the state offset: its hosted state), on every plan where
   it can apply; where it cannot (no ReduceScatter in the plan, or a single PS whose range starts
   at 0) the test says so.
c. check_calls() accepts the calls it expects and names a wrong chunk, root, order, stream and an
   unbalanced group.
"""
import pytest
import torch

import rccl_reference as rr
from ddl_amd.models import HIP_SEGMENTS as SEGS
from ddl_amd.parallel.sharding import make_plan

CELLS = [(shard, W, W) for shard in ("flat", "contiguous", "greedy") for W in (2, 3, 8)]
CELLS += [("none", W, 1) for W in (2, 3, 8)] + [("flat", 4, 2)]
STEPS = 2


def plan_of(shard, P):
    return make_plan(shard, P, buckets=SEGS if shard == "flat" else None)


_GRADS = {}


def grads_of(W, total):
    """[STEPS, W, total] small integers, one draw per (W, total)."""
    if (W, total) not in _GRADS:
        g = torch.Generator().manual_seed(100 * W + 7)
        _GRADS[(W, total)] = torch.randint(-8, 9, (STEPS, W, total), generator=g).float()
    return _GRADS[(W, total)]


def closed_loop(shard, W, P, mutation=None):
    """Two steps on every rank.  Returns (ranks whose parameters differ from the PS result, ranks
    whose hosted state differs)."""
    plan = plan_of(shard, P)
    total = plan.total
    grads = grads_of(W, total)
    g0 = torch.Generator().manual_seed(3)
    params0 = torch.randint(-4, 5, (total,), generator=g0).float()
    want, m = params0.clone(), torch.zeros(total)
    nexts = []
    for s in range(STEPS):
        rr.oracle_step(want, m, grads[s])
        nexts.append(want.clone())
    bad_w, bad_m = [], []
    for r in range(W):
        exps = rr.expected(plan, SEGS, W, r)
        st = rr.RankState(params0)
        for s in range(STEPS):
            rr.walk_rank(st, exps, W, r, grads[s], nexts[s], mutation)
        if not torch.equal(st.params.view(torch.int32), want.view(torch.int32)):
            bad_w.append(r)
        for e in exps:
            if e.kind == "ar":
                got, ref = st.state("repl")[:e.n], m[e.lo:e.lo + e.n]
            elif e.kind == "rs":
                got = st.state(e.ps)[e.state_off:e.state_off + e.c]
                ref = m[e.lo + r * e.c:e.lo + (r + 1) * e.c]
            elif e.root == r:
                got, ref = st.state(e.ps)[e.state_off:e.state_off + e.n], m[e.lo:e.lo + e.n]
            else:
                assert e.ps not in st.m  # (a PS hosted elsewhere has no state here)
                continue
            if not torch.equal(got.view(torch.int32), ref.view(torch.int32)):
                bad_m.append(r)
    return bad_w, sorted(set(bad_m))


@pytest.mark.parametrize("shard,W,P", CELLS)
def test_closed_loop(shard, W, P):
    assert closed_loop(shard, W, P) == ([], [])


def applies(mutation, shard, W, P):
    has_rs = shard == "flat" and P == W
    if mutation in ("next_chunk", "no_all_gather"):
        return has_rs                     # only the reduce-scatter form has chunks
    if mutation in ("root_plus_1", "no_broadcast"):
        return not has_rs                 # only the reduce form has roots
    return shard != "none"                # one PS from offset 0: both offsets are the same


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_oracle_discriminates(mutation):
    """Every mutation shows on at least one rank of every cell it applies to, and changes nothing
    where it cannot apply."""
    seen = 0
    for shard, W, P in CELLS:
        if W == 8 and shard in ("greedy", "none"):
            continue                      # (W = 8 once per form: flat and contiguous)
        bad_w, bad_m = closed_loop(shard, W, P, mutation)
        if applies(mutation, shard, W, P):
            # a state offset that is wrong the same way every step is a relabelling as long as no
            # two ranges collide: it shows in WHERE the state lies (the GPU test's check of m and
            # v against the simulation's slice), not in the parameters
            assert bad_m if mutation == "plan_offset_state" else bad_w, (mutation, shard, W, P)
            seen += 1
        else:
            print(f"{mutation}: cannot show on {shard} W={W} P={P}")
            assert (bad_w, bad_m) == ([], [])
    assert seen >= 3


def test_plan_offsets_are_not_shard_offsets():
    """The cells do separate the two offsets: on every plan with P > 1 some range's state offset
    differs from its plan offset (else `plan_offset_state` could never show)."""
    for shard, W, P in CELLS:
        if shard == "none":
            continue
        apart = []
        for r in range(W):
            exps = rr.expected(plan_of(shard, P), SEGS, W, r)
            own = [e for e in exps if e.kind == "rs" or (e.kind == "reduce" and e.root == r)]
            if not own:
                assert shard == "flat" and P < W and r >= P
                continue
            apart.append(any((e.lo + r * e.c if e.kind == "rs" else e.lo) != e.state_off
                             for e in own))
        # (PS 0 of a tensor-granular plan starts at 0: rank 0 alone cannot tell them apart)
        assert all(apart[1:]) and len(apart) > 1, (shard, W, apart)


def test_expected_covers_the_plan_once():
    """Every element of the plan buffer is exchanged exactly once per step, flat buckets split
    into W equal chunks, and the update launches are the rank's own ranges."""
    for shard, W, P in CELLS:
        plan = plan_of(shard, P)
        for r in (0, W - 1):
            exps = rr.expected(plan, SEGS, W, r)
            cover = torch.zeros(plan.total, dtype=torch.int32)
            for e in exps:
                cover[e.lo:e.lo + e.n] += 1
                if e.kind == "rs":
                    assert e.c * W == e.n
            assert bool((cover == 1).all()), (shard, W)
            n = rr.update_launches(exps, r)
            if shard == "flat" and P == W:
                assert n == len(plan.bucket_ranges) and sum(e.kind == "ar" for e in exps) == 1
            elif shard == "none":
                assert n == (len(exps) if r == 0 else 0)
            else:
                assert n == sum(e.root == r for e in exps)


def _log_of(exps, rank, stream_of=lambda e: 1):
    """The call log an honest runner would leave: reductions grouped, then the gathers."""
    log = []
    red = [e for e in exps if e.kind == "reduce"]
    for e in exps:
        if e.kind == "reduce":
            continue
        first, then = rr.calls_of(e, rank)
        for c in (first, then):
            if c is not None:
                rbuf = "shard3" if c[5] == "shard" else c[5]
                log.append((c[0], c[1], c[2], c[3], c[4], stream_of(e), 0, rbuf, c[6]))
    for pick in (0, 1):
        if red:
            log.append(("GroupStart", "", -1, 0, -1, 0, 0, "", -1))
            for e in red:
                c = rr.calls_of(e, rank)[pick]
                log.append((c[0], c[1], c[2], c[3], c[4], stream_of(e), 1, c[5], c[6]))
            log.append(("GroupEnd", "", -1, 0, -1, 0, 1, "", -1))
    return log


@pytest.mark.parametrize("shard,W,P", [("flat", 3, 3), ("contiguous", 3, 3), ("flat", 4, 2)])
def test_check_calls(shard, W, P):
    plan = plan_of(shard, P)
    r = 1
    exps = rr.expected(plan, SEGS, W, r)
    log = _log_of(exps, r)
    assert rr.check_calls(log, exps, r) == []
    # another rank's calls: a wrong chunk (flat) or nothing to tell apart (same roots)
    other = rr.check_calls(_log_of(rr.expected(plan, SEGS, W, 2), 2), exps, r)
    assert bool(other) == (shard == "flat" and P == W)
    # a wrong root, count, order, stream, an open group
    k = next(i for i, e in enumerate(log) if e[0] in ("Reduce", "ReduceScatter"))
    e = log[k]
    for wrong in ((*e[:4], e[4] + 1, *e[5:]), (*e[:3], e[3] - 1, *e[4:]), (*e[:2], e[2] + 64, *e[3:])):
        assert rr.check_calls(log[:k] + [wrong] + log[k + 1:], exps, r), wrong
    assert any("ahead of" in b for b in rr.check_calls(log[::-1], exps, r))
    two = (*e[:5], 2, *e[6:])
    assert any("stream" in b for b in rr.check_calls(log[:k] + [two] + log[k + 1:], exps, r))
    assert rr.check_calls(log + [("GroupStart", "", -1, 0, -1, 0, 0, "", -1)], exps, r)
    assert rr.check_calls(log[:k] + log[k + 1:], exps, r)
