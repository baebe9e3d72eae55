"""The cell table of tests/test_dispatch_oracle_gpu.py (helper module, not a conftest; plain
Python, no GPU): every schedule the test runs, and for each the dispatch branches it must reach.

A schedule is a dict of what differs from the engine's defaults:

* ``cfg`` / ``splits`` / ``wide``: op -> value (`set_cfg` / `set_splits` / `set_wide`);
* ``dual``, ``bfirst`` (ops whose layer dispatches its second problem first), ``direct`` (both
  conv1 switches), ``concurrent``, ``defer`` (`set_fc_wgrad_defer`).

`expected_hits` is the host dispatch of engine.hip `backward_segment`, schedule.h `choose_pair` /
`choose_seg3` / `pair_branch` and engine_impl.h `dual_then_b` written down once more, as
step_audit.expected_update_launches writes down the runners': the GPU test demands that
`dispatch_hits()` after a segment equals it exactly, every other counter 0.
tests/test_dispatch_cells_cpu.py holds the table against BRANCHES and, without a GPU, against
schedule.h itself (csrc/kernels/tests/schedule_check.cpp).
"""
import itertools

# csrc/kernels/schedule.h enum Branch, in its order (the GPU test holds it against dispatch_hits())
BRANCHES = [
    "fc_pack_deferred", "fc_pack_kept", "fc_dual", "fc_back_to_back",
    "conv4_dual_fc_wgrad", "conv4_dual_tail", "conv4_back_to_back_flush", "conv4_back_to_back",
    "conv3_dual", "conv3_back_to_back", "conv2_dual", "conv2_back_to_back",
    "seg3_direct_reduce", "seg3_direct", "seg3_reduce_gemm", "seg3_reduce_refused",
    "seg3_unfused", "tail_standalone", "tail_consumed", "concurrent",
]

# csrc/kernels/schedule.h enum Op and the engine's defaults (Schedule::defaults)
FC2_DGRAD, FC2_WGRAD, FC1_DGRAD, FC1_WGRAD = 6, 7, 8, 9
CONV4_DGRAD, CONV4_WGRAD, CONV3_DGRAD, CONV3_WGRAD = 10, 11, 12, 13
CONV2_DGRAD, CONV2_WGRAD, CONV1_WGRAD = 14, 15, 16
KWAVE, MF16 = 13, 14
DEF_CFG = [3, 3, 3, 3, 15, 15, 13, 5, 13, 5, 3, 14, 3, 14, 14, 3, 3]
DEF_SPLITS = [1, 3, 3, 5, 8, 8, 4, 1, 4, 1, 5, 6, 5, 12, 4, 48, 1024]
DEF_INLAUNCH = [0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0]
WIDE_INLAUNCH, WIDE_SEPARATE = 1 << 20, 1
DEF_WIDE = [WIDE_INLAUNCH if i else WIDE_SEPARATE for i in DEF_INLAUNCH]
DEF_BFIRST = (CONV2_DGRAD, CONV3_DGRAD)
ONE_WAVE = (3, 5, MF16)
# ops with an instantiation of the K-wave launch (13), the 16x16x4 tile (14) and the 16-row K-wave
# launch (15): csrc/kernels/schedule.h op_has_cfg (tests/test_dispatch_cells_cpu.py holds them
# against it); every other op falls back to config 3
KWAVE_OPS = (4, 5, 6, 8)
MF16_OPS = (1, 2, 3, 10, 11, 12, 13, 14, 15)
KW16_OPS = (4, 5)
# segment -> (data-gradient op, weight-gradient op) of its conv layer
PAIR = {1: (CONV4_DGRAD, CONV4_WGRAD), 2: (CONV3_DGRAD, CONV3_WGRAD), 3: (CONV2_DGRAD, CONV2_WGRAD)}
LAYER = {1: "conv4", 2: "conv3", 3: "conv2"}


def resolved(sched):
    """The whole schedule: cfg, splits, wide as lists of 17 and the flags."""
    out = {"cfg": list(DEF_CFG), "splits": list(DEF_SPLITS), "wide": list(DEF_WIDE),
           "dual": sched.get("dual", True), "bfirst": tuple(sched.get("bfirst", DEF_BFIRST)),
           "direct": sched.get("direct", True), "concurrent": sched.get("concurrent", False),
           "defer": sched.get("defer", True)}
    for k in ("cfg", "splits", "wide"):
        for op, v in sched.get(k, {}).items():
            out[k][op] = v
    return out


def bk_of(cfg):
    """K tile of the one-wave tile a dual launch runs for run-time config `cfg`."""
    return 16 if cfg == 5 else 32


def splitk_z(K, splits, bk):
    """gemm.h splitk_kchunk / splitk_z: the number of K chunks a launch really runs."""
    if splits <= 1:
        return 1
    per = -(-K // splits)
    kc = max(bk, -(-per // bk) * bk)
    return max(1, -(-K // kc))


def mode_of(K, splits, wide, bk):
    """gemm.h plan_gemm: 0 unsplit, 1 in-launch last arriver, 2 separate wide reduce (no launch of
    these tests has more tiles than arrival tickets)."""
    z = splitk_z(K, splits, bk)
    return 0 if z == 1 else (2 if z > wide else 1)


def _add(h, name, n=1):
    h[name] = h.get(name, 0) + n


def _pair(h, s, sc, tail, fc_pending):
    """run_dual_inst of segment s's conv pair; returns (tail still pending, fc wgrads pending)."""
    a, b = PAIR[s]
    if sc["dual"] and sc["cfg"][a] in ONE_WAVE and sc["cfg"][b] in ONE_WAVE:
        if s == 1:
            _add(h, "conv4_dual_fc_wgrad" if fc_pending else "conv4_dual_tail")
        else:
            _add(h, LAYER[s] + "_dual")
        if tail:
            _add(h, "tail_consumed")
        return False, False
    if s == 1:
        _add(h, "conv4_back_to_back_flush" if fc_pending else "conv4_back_to_back")
    else:
        _add(h, LAYER[s] + "_back_to_back")
    if tail:
        _add(h, "tail_standalone")
    return False, False   # (backward_segment(1) flushes the fc weight gradients itself)


def _fc_pair(h, sc, a, b, tail, fc_pending):
    first = a == FC2_DGRAD    # fc2's launches carry fc3's weight gradient: the tail is flushed
    if sc["dual"] and sc["cfg"][a] == KWAVE and sc["cfg"][b] in (3, 5):
        _add(h, "fc_pack_deferred" if sc["defer"] else "fc_pack_kept")
        fc_pending = fc_pending or sc["defer"]
        took = not first
    elif not sc["dual"] or sc["cfg"][a] not in ONE_WAVE or sc["cfg"][b] not in ONE_WAVE:
        _add(h, "fc_back_to_back")
        took = False
    else:
        _add(h, "fc_dual")
        took = not first
    if tail:
        _add(h, "tail_consumed" if took else "tail_standalone")
    return False, fc_pending


def expected_hits(s, sched, K15=None, tail=False, fc_pending=False):
    """dispatch_hits() after backward_segment(s) under `sched` (every other counter 0), and
    whether fc weight gradients are pending afterwards.  K15: K of conv2's weight gradient at the
    batch (segment 3 only: it decides the reduce mode); tail: an update tail is pending before;
    fc_pending: deferred fc weight gradients are."""
    sc = resolved(sched)
    h = {}
    if sc["concurrent"]:
        _add(h, "concurrent")
        if tail:
            _add(h, "tail_standalone")
        return h, fc_pending
    if s == 0:
        tail, fc_pending = _fc_pair(h, sc, FC2_DGRAD, FC2_WGRAD, tail, fc_pending)
        tail, fc_pending = _fc_pair(h, sc, FC1_DGRAD, FC1_WGRAD, tail, fc_pending)
        return h, fc_pending
    if s in (1, 2):
        _pair(h, s, sc, tail, fc_pending)
        return h, False
    ca, cb, cn = (sc["cfg"][op] for op in (CONV2_DGRAD, CONV2_WGRAD, CONV1_WGRAD))
    if not sc["dual"] or ca not in (3, MF16) or cb not in ONE_WAVE or cn != 3:
        _add(h, "seg3_unfused")
        _pair(h, 3, sc, tail, False)
        return h, fc_pending
    if tail:
        _add(h, "tail_consumed")
    mode = mode_of(K15, sc["splits"][CONV2_WGRAD], sc["wide"][CONV2_WGRAD], bk_of(cb))
    if sc["direct"]:
        _add(h, "seg3_direct_reduce" if mode == 2 else "seg3_direct")
    else:
        _add(h, "seg3_reduce_gemm" if mode == 2 else "seg3_reduce_refused")
    return h, fc_pending


# ---- the schedules ---------------------------------------------------------------------------------
# split-K mode of one problem -> (split, wide threshold)
MODES = {0: (1, WIDE_INLAUNCH), 1: (3, WIDE_INLAUNCH), 2: (3, WIDE_SEPARATE)}


def pairing_cells(s):
    """Segment s's pair over {3, 5, 14}^2 with both block orders at default splits, then each op
    in turn on a config with no dual launch (0 and 13): back to back."""
    a, b = PAIR[s]
    out = []
    for ca, cb in itertools.product(ONE_WAVE, ONE_WAVE):
        for bf in (0, 1):
            out.append((f"{LAYER[s]} pair ({ca}, {cb}) bfirst={bf}",
                        dict(cfg={a: ca, b: cb}, bfirst=(a,) if bf else ())))
    for op, c in itertools.product((a, b), (0, KWAVE)):
        out.append((f"{LAYER[s]} op {op} on config {c}", dict(cfg={op: c})))
    return out


MODE_PAIRINGS = ((3, 3), (MF16, 5), (5, MF16))


def mode_cells(s, pairings=MODE_PAIRINGS):
    """Both problems of segment s's launch in each split-K mode (3 x 3), on `pairings`, in both
    block orders."""
    a, b = PAIR[s]
    out = []
    for (ca, cb), ma, mb, bf in itertools.product(pairings, MODES, MODES, (0, 1)):
        out.append((f"{LAYER[s]} modes ({ma}, {mb}) on ({ca}, {cb}) bfirst={bf}",
                    dict(cfg={a: ca, b: cb}, splits={a: MODES[ma][0], b: MODES[mb][0]},
                         wide={a: MODES[ma][1], b: MODES[mb][1]}, bfirst=(a,) if bf else ())))
    return out


# conv2's weight gradient in the fused segment 3: (name, split, wide, lanes per float4 of the
# reduce).  launch_reduce / conv1_wgrad_kernel / reduce_gemm_kernel take 4, 16 or 64 lanes for
# z <= 4, <= 32, > 32.
FUSED_MODES = (("mode 0", 1, WIDE_INLAUNCH, None), ("mode 1", 3, WIDE_INLAUNCH, None),
               ("mode 2 split 3", 3, WIDE_SEPARATE, 4), ("mode 2 split 12", 12, WIDE_SEPARATE, 16),
               ("mode 2 split 48", 48, WIDE_SEPARATE, 64))


def fused_cells():
    """Segment 3 on dual_then_b: conv2's data gradient on {3, 14} x its weight gradient on
    {3, 5, 14} x conv1's direct kernel on / off x the weight gradient's reduce mode."""
    out = []
    for ca, cb, direct, (mname, spl, wide, _) in itertools.product(
            (3, MF16), ONE_WAVE, (True, False), FUSED_MODES):
        out.append((f"segment 3 fused ({ca}, {cb}) direct={direct} {mname}",
                    dict(cfg={CONV2_DGRAD: ca, CONV2_WGRAD: cb}, splits={CONV2_WGRAD: spl},
                         wide={CONV2_WGRAD: wide}, direct=direct)))
    return out


def unfused_cells():
    """Segment 3 off dual_then_b by each of its three conditions (conv1's weight gradient on
    config 5 on its direct kernel and on the GEMM)."""
    return [("segment 3 unfused: conv2 dgrad on 5", dict(cfg={CONV2_DGRAD: 5})),
            ("segment 3 unfused: conv1 wgrad on 5", dict(cfg={CONV1_WGRAD: 5})),
            ("segment 3 unfused: conv1 wgrad on 5, GEMM", dict(cfg={CONV1_WGRAD: 5}, direct=False)),
            ("segment 3 unfused: dual off", dict(dual=False))]


def segment_cells(s, reduced=False):
    """Every exact cell of segment s (reduced: the set of the 136-row engine)."""
    out = pairing_cells(s)[:18] if reduced else pairing_cells(s)
    out += mode_cells(s, MODE_PAIRINGS[:1] if reduced else MODE_PAIRINGS)
    if s == 3:
        out += fused_cells()
        if not reduced:
            out += unfused_cells()
    if not reduced:
        out.append((f"segment {s} two streams", dict(concurrent=True)))
    return out


# One schedule per branch for the pending-tail cells: (segment, name, schedule).  Segment 3's K at
# every batch of the test gives mode 2 under the default schedule (split 48, separate reduce).
TAIL_CELLS = [
    (1, "conv4 dual", {}),
    (1, "conv4 back to back", dict(cfg={CONV4_DGRAD: 0})),
    (2, "conv3 dual", {}),
    (2, "conv3 back to back", dict(cfg={CONV3_WGRAD: 0})),
    (3, "direct, reduce pending", {}),
    (3, "direct, no reduce", dict(wide={CONV2_WGRAD: WIDE_INLAUNCH})),
    (3, "reduce with the GEMM", dict(direct=False)),
    (3, "reduce refused", dict(direct=False, splits={CONV2_WGRAD: 1})),
    (3, "unfused, conv2 dual", dict(cfg={CONV2_DGRAD: 5})),
    (3, "unfused, conv2 back to back", dict(dual=False)),
    (1, "two streams", dict(concurrent=True)),
]

# The chained segments 0 -> 1 on real values: name -> schedule.  `big`: also at B = 129.
CHAIN_CELLS = {
    "default": dict(sched={}, big=True),
    "defer-off": dict(sched=dict(defer=False), big=True),
    "conv4-dgrad-0": dict(sched=dict(cfg={CONV4_DGRAD: 0}), big=True),
    "conv4-dgrad-13": dict(sched=dict(cfg={CONV4_DGRAD: KWAVE}), big=True),
    "fc-dgrad-3": dict(sched=dict(cfg={FC2_DGRAD: 3, FC1_DGRAD: 3}), big=False),
    "fc-dgrad-5": dict(sched=dict(cfg={FC2_DGRAD: 5, FC1_DGRAD: 5}), big=False),
    "dual-off": dict(sched=dict(dual=False), big=False),
}


def chain_expected(sched, tail0=False, tail1=False):
    """Counters after backward_segment(0) then (1); tail0 / tail1: a tail queued before each."""
    h0, pend = expected_hits(0, sched, tail=tail0)
    h1, _ = expected_hits(1, sched, tail=tail1, fc_pending=pend)
    for k, v in h1.items():
        _add(h0, k, v)
    return h0


def all_expectations(K15=6272):
    """(cell name, expected counters) of every cell of the table (K15: conv2's weight-gradient K
    at a batch of at most 32)."""
    out = []
    for s in (1, 2, 3):
        for name, sched in segment_cells(s):
            out.append((name, expected_hits(s, sched, K15)[0]))
    for s, name, sched in TAIL_CELLS:
        out.append(("tail: " + name, expected_hits(s, sched, K15, tail=True)[0]))
    for name, c in CHAIN_CELLS.items():
        out.append(("chain: " + name, chain_expected(c["sched"])))
        out.append(("chain + tails: " + name, chain_expected(c["sched"], True, True)))
    return out
