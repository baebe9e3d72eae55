"""The audit of one native training step (helper module, not a conftest), plain torch on the CPU.

tests/test_step_audit_gpu.py reads every buffer of the engine after one `SyncRunner::step` and
hands them to `audit_step`, which checks each launch's outputs against the fp64 reference of that
op on the GPU's own inputs ("teacher-forced": an error does not travel to the next op's check).
tests/test_step_audit_cpu.py runs the same functions without a GPU: that they notice a weight
updated too early, that the pool-code rule holds for the data used, and that the update yardstick
is the parameter server's.

`coalesced` is the planner of csrc/kernels/update_plan.h written down once more (the CPU test runs
the real one beside it), and `expected_update_launches` the host logic of `SyncRunner::step`,
`AsyncRunner::step_inline` and their shared `run_riding_backward` (csrc/kernels/runner.hip) and of
the engine's last launch (engine_impl.h dual_then_b); the GPU test's table of `update_launches()`
is derived from them.
"""
import torch

import op_reference as R
from oracle_common import HEAD_MARGIN

KEEP = 0.5
LR = 0.01          # the first Adam step moves every weight with a gradient by lr: > 10 % of a weight
DATA_SEED = 3
STEP_SEEDS = (20240, 20241)   # dropout seeds of the two audited steps
CODE_CAP = 1e-3    # share of a code buffer's windows that may differ from the reference's code
TAIL_PIECES = 4    # csrc/kernels/tail.h kTailPieces
PAD = 256          # engine_impl.h final_split_conv12 kPad


def batch(B, step=0):
    """Images uniform in [0, 1) and labels (all ten classes from B = 10 on) of audited step
    `step` at batch B: rows of one fixed 40-row draw per step."""
    g = torch.Generator().manual_seed(DATA_SEED + 100 * step)
    x = torch.rand(40, 784, generator=g)
    y = torch.randperm(40, generator=g) % 10
    return x[:B].contiguous(), y[:B].contiguous()


# ---- the ops ---------------------------------------------------------------------------------------
def op_inputs(op, bufs):
    return {n: bufs[n] for n in R.OP_IO[op][0]}


def code_failures(op, P64, inputs, got_code, tag, lines):
    """The forward's pool codes against the reference's.  With ceiling = (K + 8) 2^-24 times the
    window's abs-sum: a window whose fp64 winner leads the runner-up and lies away from 0 by at
    least the ceiling must carry exactly the reference's code.  In the other windows (which fp32
    arithmetic may decide either way) the code must still name a candidate: a position within the
    ceiling of the winner, or 0xFF if the winner is within the ceiling of 0.  And over the whole
    buffer at most CODE_CAP of the windows may differ from the reference's code at all."""
    B = next(iter(inputs.values())).shape[0]
    name = f"p{op}" if op else "x"
    src = inputs["x"].reshape(B, 28, 28, 1) if op == 0 else inputs[name]
    pre = R.conv_pre(src, P64[2 * op], P64[2 * op + 1])
    win = R._windows(pre, float("-inf"))
    _, ref = R.pool_relu_code(pre)
    got = got_code.reshape(ref.shape).long()
    s = R.abs_sum(op, P64, inputs, KEEP)[f"p{op + 1}"].reshape(ref.shape)
    tol = (R.k_terms(op, B) + 8) * R.U32 * s
    top = win.topk(2, dim=-1).values
    best = top[..., 0]
    open_ = ((best - top[..., 1]) < tol) | (best.abs() < tol)
    differ = got != ref.long()
    q = got.clamp(max=3)
    cand = torch.where(got == R.NO_GRAD_CODE, best <= tol,
                       (got < 4) & (win.gather(-1, q.unsqueeze(-1)).squeeze(-1) >= best - tol) &
                       (best > -tol))
    n = ref.numel()
    lines.append(f"AUDIT-CODES {tag} c{op + 1}: {int(differ.sum())} of {n} windows differ from the "
                 f"reference ({int(open_.sum())} within the ceiling of a tie)")
    fails = []
    if bool((differ & ~open_).any()):
        fails.append(f"{tag}: c{op + 1} differs in {int((differ & ~open_).sum())} decided windows")
    if bool((~cand).any()):
        fails.append(f"{tag}: c{op + 1} names no candidate in {int((~cand).sum())} windows")
    if int(differ.sum()) > CODE_CAP * n:
        fails.append(f"{tag}: c{op + 1} differs in {int(differ.sum())} windows > {CODE_CAP * n:.1f}")
    return fails


def audit_op(op, P, P64, bufs, seed, tag, lines, stats):
    """Op `op`'s outputs in `bufs` against the references on `bufs`' own inputs, as
    test_ops_real_valued_precision compares them."""
    B = bufs["x"].shape[0]
    inputs = op_inputs(op, bufs)
    ref = R.run_op(op, P64, inputs, seed, KEEP, True)
    f32 = R.run_op(op, P, inputs, seed, KEEP, True, dtype=torch.float32)
    asum = R.abs_sum(op, P64, inputs, KEEP)
    K = R.k_terms(op, B)
    fails = []
    for name, r64 in ref.items():
        if name.startswith("c"):
            fails += code_failures(op, P64, inputs, bufs[name], tag, lines)
            continue
        s = asum[name].reshape(r64.shape)
        got = bufs[name].reshape(r64.shape)
        base = R.rms(R.rel_err(f32[name].reshape(r64.shape), r64, s)[0], s)
        f, (emax, erms) = R.precision_failures(got, r64, s, K, base)
        ratio = erms / max(base, 1e-300) if erms > 0 else 0.0
        lines.append(f"AUDIT-RATIO {tag} {R.OP_NAMES[op]} {name}: K={K} max err {emax:.3g} "
                     f"(ceiling {(K + 8) * R.U32:.3g}) rms {erms:.3g} fp32 CPU rms {base:.3g} "
                     f"ratio {ratio:.3f}")
        key = (R.OP_NAMES[op], name)
        old = stats.get(key, (0.0, 0.0))
        stats[key] = (max(old[0], ratio), max(old[1], emax))
        fails += [f"{tag}: {R.OP_NAMES[op]} {name}: {m}" for m in f]
    return fails


def audit_head(P, bufs, labels, seed, tag, lines, stats):
    """loss, dlog, dpre2fc, fc3's dW / db against the head reference on the GPU's h2, with the
    margin rule of test_head_matches_reference; and the two dropout masks."""
    B = bufs["x"].shape[0]
    mask1 = R.keep_mask(seed, 1, B, 1024, KEEP)
    mask2 = R.keep_mask(seed, 2, B, 512, KEEP)
    ref = R.head(bufs["h2"], P[12], P[13], labels, mask2, 1.0 / KEEP)
    cpu = R.head(bufs["h2"], P[12], P[13], labels, mask2, 1.0 / KEEP, dtype=torch.float32)
    got = {"loss": bufs["loss"], "dlog": bufs["dlog"], "dpre2fc": bufs["dpre2fc"],
           "gw": bufs["g12"], "gb": bufs["g13"]}
    fails = []
    for name, g in got.items():
        r = ref[name]
        g = g.double().reshape(r.shape)
        e_gpu = float((g - r).abs().max())
        e_cpu = float((cpu[name].double() - r).abs().max())
        floor = R.U32 * float(r.abs().max())
        ratio = e_gpu / max(e_cpu, floor, 1e-300)
        lines.append(f"AUDIT-HEAD {tag} {name}: gpu {e_gpu:.3g} fp32 CPU {e_cpu:.3g} floor "
                     f"{floor:.3g} ratio {ratio:.3f}")
        old = stats.get(("head", name), (0.0, 0.0))
        stats[("head", name)] = (max(old[0], ratio), max(old[1], e_gpu))
        if not (e_gpu <= HEAD_MARGIN * max(e_cpu, floor)):
            fails.append(f"{tag}: head {name}: gpu err {e_gpu:.3g} > {HEAD_MARGIN} x "
                         f"max(fp32 CPU err {e_cpu:.3g}, {floor:.3g})")
    if bool(((bufs["dpre2fc"] != 0) & ~mask2).any()):
        fails.append(f"{tag}: dpre2fc non-zero where the mask of layer 2 drops")
    if bool(((bufs["h1"] != 0) & ~mask1).any()):
        fails.append(f"{tag}: h1 non-zero where the mask of layer 1 drops")
    if not bool(((bufs["h2"] != 0) & mask2).any()) or not bool(((bufs["h1"] != 0) & mask1).any()):
        fails.append(f"{tag}: h1 / h2 zero everywhere the masks keep")
    return fails


def audit_step(P, bufs, labels, seed, tag, lines, stats, ops=range(R.OP_COUNT)):
    """Every GEMM op and the head of one step.  P: the 14 fp32 parameter tensors from before the
    step; bufs: name -> fp32 / uint8 CPU tensor of rows < B ("x", the activations, the codes,
    "g0".."g13")."""
    P64 = [p.double() for p in P]
    fails = []
    for op in ops:
        fails += audit_op(op, P, P64, bufs, seed, tag, lines, stats)
    fails += audit_head(P, bufs, labels, seed, tag, lines, stats)
    return fails


def chained_step(P, x, labels, seed, dtype=torch.float64):
    """The references chained in the engine's op order (as tests/test_op_reference_cpu.py
    reference_step), in `dtype`: name -> tensor, "x" and "g0".."g13" included."""
    B = x.shape[0]
    Pd = [p.to(dtype) for p in P]
    buf = {"x": x.to(dtype)}
    for op in range(6):
        buf.update(R.run_op(op, Pd, buf, seed, KEEP, True, dtype=dtype))
    m2 = R.keep_mask(seed, 2, B, 512, KEEP)
    hd = R.head(buf["h2"], Pd[12], Pd[13], labels, m2, 1.0 / KEEP, dtype=dtype)
    buf.update(loss=hd["loss"], dlog=hd["dlog"], dpre2fc=hd["dpre2fc"], g12=hd["gw"], g13=hd["gb"])
    for op in range(6, R.OP_COUNT):
        buf.update(R.run_op(op, Pd, buf, seed, KEEP, True, dtype=dtype))
    return buf


# ---- which launch carries which update ---------------------------------------------------------
def unit_pieces(units, seg_sets, overlap=True):
    """What SyncRunner::set_units hands the planner at W = 1: per backward segment the
    (lo, hi, ps, state_off) ranges of its units, in unit order."""
    segs = [[] for _ in seg_sets]
    for u in units:
        s = len(seg_sets) - 1 if not overlap else max(
            next(i for i, ss in enumerate(seg_sets) if t in ss) for t in u.tensors)
        offs = u.state_offs or [0] * len(u.ranges)
        segs[s] += [(lo, hi, u.ps, off) for (lo, hi), off in zip(u.ranges, offs)]
    return segs


def inline_pieces(plan, seg_sets):
    """What AsyncRunner::set_inline hands the planner: each PS's one range with that PS's own
    state, in the last backward segment any of its tensors completes in (async_xgmi.py
    attach_runner)."""
    from ddl_amd.models.layout import TENSORS
    off = plan.tensor_offsets
    segs = [[] for _ in seg_sets]
    for p in range(plan.num_ps):
        (lo, hi), = plan.ps_segments(p)
        ts = [t.index for t in TENSORS if off[t.index] < hi and off[t.index] + t.numel > lo]
        s = max(next(i for i, ss in enumerate(seg_sets) if t in ss) for t in ts)
        segs[s].append((lo, hi, p, 0))
    return segs


def segment_pieces(units, seg_sets, overlap=True):
    """SyncRunner::set_units at W = 1: the coalesced pieces of the units' ranges."""
    return coalesced(unit_pieces(units, seg_sets, overlap))


def coalesced(segs):
    """UpdatePlan::finish (csrc/kernels/update_plan.h): each segment's pieces coalesced where
    adjacent in the buffer and in one PS's state; and all of them coalesced (`merged`)."""
    def coalesce(v):
        out = []
        for lo, hi, ps, off in sorted(v):
            if out and out[-1][1] == lo and out[-1][2] == ps and \
                    out[-1][3] + (out[-1][1] - out[-1][0]) == off:
                out[-1] = (out[-1][0], hi, ps, out[-1][3])
            else:
                out.append((lo, hi, ps, off))
        return out

    return [coalesce(s) for s in segs], coalesce([p for s in segs for p in s])


def final_split_conv12_ok(pieces, offsets):
    """engine_impl.h final_split_conv12: the last segment's pieces are exactly conv1's and conv2's
    weights and biases (and padding below PAD elements), every piece starts on a tensor and every
    tensor lies inside one piece."""
    spans = [(offsets[i], offsets[i] + n) for i, n in zip(range(4), (800, 32, 51200, 64))]
    for lo, hi, _, _ in pieces:
        pos, first = lo, True
        while pos < hi:
            inside = [s for s in spans if s[0] >= pos and s[1] <= hi]
            if not inside:
                break
            a, b = min(inside)
            if a - pos >= PAD or (first and a != pos):
                return False
            pos, first = b, False
        if first or hi - pos >= PAD:
            return False
    return all(any(lo <= a and b <= hi for lo, hi, _, _ in pieces) for a, b in spans)


def expected_update_launches(seg_pieces, merged, offsets, use_tail=True, final_in_reduce=True,
                             dual=True, conv1_direct=True, per_segment=False,
                             pair_takes=(True, True, True), conv2_reduce_separate=True):
    """Stand-alone optimizer launches of one W = 1 step (update_launches() of either runner), by
    reading SyncRunner::step, AsyncRunner::step_inline and run_riding_backward (runner.hip).  Every
    plan buffer keeps tensors and PS chunks on 64-element boundaries, so the alignment and length
    conditions of tail_ok always hold here; what decides is the piece count.  per_segment: the
    in-line runner's policy, a segment with more than TAIL_PIECES pieces is launched piece by
    piece and the others still ride; otherwise one such segment sends every update after the
    backward (SyncRunner).  pair_takes: whether the launches of conv4's / conv3's / conv2's pair
    carry a tail (a pair with an op on a config without a dual launch runs back to back and
    flushes it: engine_impl.h run_dual_inst); conv2_reduce_separate: conv2's weight gradient leaves
    a separate reduce (mode 2) for conv1's launch, whose epilogue is what applies the last
    segment's update (dual_then_b)."""
    rides = [len(sp) <= TAIL_PIECES for sp in seg_pieces]
    if not per_segment and not (use_tail and all(rides)):
        return len(merged)           # the coalesced launches after the backward
    # (without dual launches run_back_to_back flushes the pending tail, a launch per piece)
    n = sum(len(sp) for sp, r, takes in zip(seg_pieces[:-1], rides, pair_takes)
            if not (r and dual and takes))
    last = seg_pieces[-1]
    taken = rides[-1] and final_in_reduce and dual and pair_takes[-1] and conv2_reduce_separate
    if conv1_direct:                 # (else final_split + launch_reduce_tail: conv1's spans cut out)
        taken = taken and final_split_conv12_ok(last, offsets)
    return n + (0 if taken else len(last))
