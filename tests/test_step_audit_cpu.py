"""The step audit's own yardsticks (tests/step_audit.py, tests/test_step_audit_gpu.py), checked
without a GPU on the audit's parameters, learning rate and data:

* the op comparison notices a weight tensor that was updated before the op read it, and even one
  updated float4 of it;
* the pool-code rule passes on the fp32 CPU chain, which differs from the fp64 codes nowhere;
* the update yardstick (exchange_reference.rule_step) is parallel/ps.py's pure-torch branch at
  this learning rate and these gradients;
* the tables of `update_launches()` agree with the runners' host logic on every plan, and that
  logic's planner half with the real planner (update_plan.h) run as a host program.
"""
import pytest
import torch

import exchange_reference as xr
import op_reference as R
import step_audit as A
import test_step_audit_gpu as G
from ddl_amd.models import HIP_SEGMENTS
from ddl_amd.models.mnist_cnn import param_views
from ddl_amd.ops.adam import AdamHyper, adam_coeffs
from ddl_amd.parallel.comm import DistEnv, SyncExchange
from ddl_amd.parallel.ps import ParameterServer
from ddl_amd.parallel.roles import resolve_num_ps
from ddl_amd.config import TrainConfig
from ddl_amd.parallel.sharding import async_groups, make_plan
from oracle_common import BATCHES, make_real_params

EPS32 = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def P():
    return make_real_params()


@pytest.fixture(scope="module")
def chain33(P):
    """The fp32 CPU chain of step 0 at B = 33: stands in for the GPU's buffers."""
    x, y = A.batch(33)
    return A.chained_step(P, x, y, A.STEP_SEEDS[0], dtype=torch.float32), y


def adam_first_step(w, g):
    step = adam_coeffs(AdamHyper(lr=A.LR), 1)
    return xr.rule_step(xr.ADAM, w, torch.zeros_like(w), torch.zeros_like(w), g, step)[0]


def test_labels_cover_every_class():
    for step in (0, 1):
        assert len(torch.unique(A.batch(33, step)[1])) == 10
        x = A.batch(33, step)[0]
        assert 0.0 <= float(x.min()) and float(x.max()) < 1.0
        assert torch.equal(A.batch(5, step)[0], x[:5])


def test_audit_passes_on_the_fp32_chain(P):
    """The plumbing: the fp32 CPU chain's own buffers pass every check of audit_step."""
    for B in (1, 5):
        x, y = A.batch(B)
        bufs = A.chained_step(P, x, y, A.STEP_SEEDS[0], dtype=torch.float32)
        lines, stats = [], {}
        fails = A.audit_step(P, bufs, y, A.STEP_SEEDS[0], f"B={B}", lines, stats)
        assert not fails, "\n".join(fails)
        assert len(stats) == 23 + 5 and sum("AUDIT-CODES" in ln for ln in lines) == 4


@pytest.mark.parametrize("op", sorted(R.OP_WEIGHT))
def test_audit_notices_an_early_update(P, chain33, op):
    """The hazard of the tail design: a tail block updates a weight that a GEMM block of the same
    or a later launch still reads.  Op `op` on the chain's inputs with one Adam step (lr 0.01,
    from zero state, the chain's own gradient) already applied to its weight tensor fails
    `precision_failures` against the reference on the weights from before the step; so it does
    with only ONE float4 of the weights updated (the first group past the middle of the tensor
    whose four gradients are non-zero), the least a stray tail lane can do.

    Outcome (B = 33; largest error over the ceiling, RMS error over the fp32 CPU's, whole tensor /
    one float4): conv1 fwd 1.4e5, 4.1e6 / 1.4e4, 1.6e5; conv2 fwd 8447, 9.3e6 / 30, 7646; conv3
    fwd 6177, 1.4e7 / 7.7, 823; conv4 fwd 4293, 1.6e7 / 6.0, 3936; fc1 fwd 6281, 2.0e7 / 15,
    5272; fc2 fwd 5830, 1.5e7 / 15, 4060; fc2 dgrad 10459, 6.6e6 / 105, 5215; fc1 dgrad 6202,
    6.8e6 / 93, 5894; conv4 dgrad 2121, 4.4e6 / 17, 5639; conv3 dgrad 2333, 2.0e6 / 37, 3698;
    conv2 dgrad 2323, 1.6e6 / 154, 20126.  One float4 is noticed for every op, K = 6400 included:
    the update moves a weight by lr = 0.01, a fifth to a half of a typical weight, so the one
    changed term is ~1e5 ulps of its product against a ceiling of K + 8 ulps of the abs-sum."""
    bufs, _ = chain33
    B, seed = 33, A.STEP_SEEDS[0]
    P64 = [p.double() for p in P]
    wi = R.OP_WEIGHT[op]
    w, g = P[wi], bufs[f"g{wi}"].reshape(P[wi].shape)
    inputs = A.op_inputs(op, bufs)
    ref = R.run_op(op, P64, inputs, seed, A.KEEP)
    f32 = R.run_op(op, P, inputs, seed, A.KEEP, dtype=torch.float32)
    asum = R.abs_sum(op, P64, inputs, A.KEEP)
    K = R.k_terms(op, B)
    w_all = adam_first_step(w, g)
    has = g != 0
    move = float((w_all - w.double()).abs()[has].median() / w.abs().median())
    print(f"{R.OP_NAMES[op]}: a weight with a gradient moves by {move:.2f} of the median |w| "
          f"({float(has.float().mean()):.2f} of them have one)")
    assert move > 0.1
    i = (g.numel() // 2) & ~3
    while not bool((g.reshape(-1)[i:i + 4] != 0).all()):
        i += 4
    w_one = w.double().clone()
    w_one.view(-1)[i:i + 4] = w_all.reshape(-1)[i:i + 4]
    for what, wm in (("whole tensor", w_all), ("one float4", w_one)):
        Pm = list(P64)
        Pm[wi] = wm
        got = R.run_op(op, Pm, inputs, seed, A.KEEP)
        for name, r64 in ref.items():
            if name.startswith("c"):
                continue
            s = asum[name].reshape(r64.shape)
            base = R.rms(R.rel_err(f32[name].reshape(r64.shape), r64, s)[0], s)
            clean, _ = R.precision_failures(f32[name].reshape(r64.shape), r64, s, K, base)
            assert not clean
            fails, (emax, erms) = R.precision_failures(got[name].float().reshape(r64.shape), r64, s,
                                                       K, base)
            print(f"{R.OP_NAMES[op]} {what}: max err / ceiling {emax / ((K + 8) * R.U32):.3g}, "
                  f"rms / fp32 CPU rms {erms / base:.3g}")
            assert fails, (R.OP_NAMES[op], what)


@pytest.mark.parametrize("B", BATCHES)
def test_code_rule_on_the_reference(P, B):
    """From the references alone, both audited steps' data: the codes of the fp32 CPU chain pass
    the audit's code rule, differing from the fp64 codes in at most CODE_CAP of a buffer's windows
    (measured: in none).  The printed lines also count the windows inside the ceiling of a tie,
    which is why the rule leaves none out (tests/test_step_audit_gpu.py)."""
    P64 = [p.double() for p in P]
    for step in (0, 1):
        x, y = A.batch(B, step)
        bufs = A.chained_step(P, x, y, A.STEP_SEEDS[step], dtype=torch.float32)
        lines = []
        for op in range(4):
            fails = A.code_failures(op, P64, A.op_inputs(op, bufs), bufs[f"c{op + 1}"],
                                    f"B={B} step {step}", lines)
            assert not fails, fails
        print("\n".join(lines))


@pytest.mark.parametrize("optimizer,kind,mu", [("adam", xr.ADAM, 0.0), ("momentum", xr.MOMENTUM, 0.9),
                                               ("sgd", xr.MOMENTUM, 0.0)])
def test_update_yardstick_matches_parameter_server(P, chain33, optimizer, kind, mu):
    """One step of parallel/ps.py's pure-torch branch at lr 0.01 on the audit's parameters and the
    chain's gradients against exchange_reference.rule_step: within one fp32 rounding of the
    largest element, as tests/test_exchange_reference_cpu.py argues it."""
    bufs, _ = chain33
    plan = make_plan("flat", 3, buckets=HIP_SEGMENTS)
    w = torch.zeros(plan.total)
    g = torch.zeros(plan.total)
    for i, (wv, gv) in enumerate(zip(param_views(w, plan.tensor_offsets),
                                     param_views(g, plan.tensor_offsets))):
        wv.copy_(P[i])
        gv.copy_(bufs[f"g{i}"].reshape(gv.shape))
    w0 = w.clone()
    for p in range(plan.num_ps):
        ps = ParameterServer(plan, p, "cpu", AdamHyper(lr=A.LR), optimizer, 0.9)
        ps.update_flat(w, g)
        step = adam_coeffs(ps.h, 1) if kind == xr.ADAM else ps.h.lr
        for (lo, hi), off in zip(ps.segments, ps.seg_off):
            n = hi - lo
            z = torch.zeros(n)
            w2, m2, v2 = xr.rule_step(kind, w0[lo:hi], z, z if kind == xr.ADAM else None, g[lo:hi],
                                      step, mu)
            pairs = [("w", w[lo:hi], w2)]
            if optimizer != "sgd":   # (the pure-torch SGD branch keeps no m)
                pairs.append(("m", ps.m[off:off + n], m2))
            if optimizer == "adam":
                pairs.append(("v", ps.v[off:off + n], v2))
            for what, got, ref in pairs:
                err = float((got.double() - ref).abs().max())
                assert err <= EPS32 * float(ref.abs().max()), (optimizer, p, what, err)
    assert not torch.equal(w, w0)


SEG_SETS = [set(s) for s in HIP_SEGMENTS]


def cell_units(kw):
    cfg = TrainConfig(mode="sync", **kw)
    n = resolve_num_ps(cfg, 1)
    plan = make_plan(cfg.shard, n, buckets=HIP_SEGMENTS if cfg.shard == "flat" else None)
    z = torch.zeros(plan.total)
    servers = {p: ParameterServer(plan, p, "cpu", optimizer=cfg.optimizer) for p in range(n)}
    ex = SyncExchange(plan, DistEnv(0, 1, 0, torch.device("cpu")), z, z.clone(), HIP_SEGMENTS,
                      servers)
    assert all(u.kind == "local" for u in ex.units)
    return plan, ex.units


def cell_pieces(kw):
    plan, units = cell_units(kw)
    return plan, A.segment_pieces(units, SEG_SETS)


def inline_plan(num_ps):
    """The in-line audit's plan (parallel/roles.py, async mode, flat)."""
    return make_plan("flat", num_ps, buckets=async_groups(HIP_SEGMENTS), segment_aligned=True)


def test_planner_agrees_with_its_python_twin(tmp_path):
    """csrc/kernels/update_plan.h, the planner both runners build their pieces through, as a
    stand-alone host program (csrc/kernels/tests/update_plan_check.cpp) built with AddressSanitizer
    + UndefinedBehaviorSanitizer (hipcc's host compiler, else g++): on every plan of CELLS and the
    in-line audit's segment-aligned plans with 3 and 8 PS its coalesced pieces per segment, the
    merged list and tail_ok are exactly step_audit's."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "distributed-deep-learning_amd", "csrc", "kernels", "tests",
                       "update_plan_check.cpp")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "update_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if os.path.exists(hipcc):
        cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
               *[a for f in san for a in ("-Xarch_host", f)], src, "-o", exe]
    elif shutil.which("g++"):
        cmd = ["g++", "-std=c++17", "-O1", "-g", *san, src, "-o", exe]
    else:
        pytest.skip("needs hipcc or g++")
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    plans = {name: A.unit_pieces(cell_units(G.CELLS[name][0])[1], SEG_SETS) for name in G.CELLS}
    for n in G.INLINE_LAUNCHES:
        plans[f"inline-ps{n}"] = A.inline_pieces(inline_plan(n), SEG_SETS)
    fmt = lambda v: "".join(f" {lo} {hi} {ps} {off};" for lo, hi, ps, off in v)  # noqa: E731
    text, want = "", ""
    for name, segs in plans.items():
        text += f"plan {name}\n" + "".join(f"{s} {lo} {hi} {ps} {off}\n" for s, sp in enumerate(segs)
                                           for lo, hi, ps, off in sp) + "end\n"
        pieces, merged = A.coalesced(segs)   # (what segment_pieces returns for the units)
        want += f"plan {name}\n" + "".join(f"seg {s}:{fmt(sp)}\n" for s, sp in enumerate(pieces))
        want += f"merged:{fmt(merged)}\n"
        ok = int(all(len(sp) <= A.TAIL_PIECES for sp in pieces))
        want += f"tail_ok {ok} tail_v_ok 1\n"   # (every PS here has an aligned v)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == want
    assert "tail_ok 0" in want and "tail_ok 1" in want   # both outcomes occur


@pytest.mark.parametrize("num_ps", sorted(G.INLINE_LAUNCHES))
def test_inline_launch_table_follows_the_runner_logic(num_ps):
    """INLINE_LAUNCHES is what AsyncRunner::set_inline / step_inline give on the in-line audit's
    plans: a segment rides when it has at most kTailPieces PS, whatever the others do."""
    plan = inline_plan(num_ps)
    pieces, merged = A.coalesced(A.inline_pieces(plan, SEG_SETS))
    assert len(merged) == num_ps        # one PS, one piece: nothing coalesces across PS
    n = A.expected_update_launches(pieces, merged, plan.tensor_offsets, per_segment=True)
    print(f"inline {num_ps} PS: pieces per segment {[len(s) for s in pieces]}, {n} launches")
    assert G.INLINE_LAUNCHES[num_ps] == n
    if num_ps == 8:   # the per-segment fallback: six PS complete in segment 1
        assert [len(s) for s in pieces] == [0, 6, 1, 1]


@pytest.mark.parametrize("name", sorted(G.CELLS))
def test_launch_table_follows_the_runner_logic(name):
    """LAUNCHES[name] is what UpdatePlan / SyncRunner::step give on the cell's plan, planned by the
    exchange's own planner; and the flagship plans ride everything."""
    kw, _, _, _, flags = G.CELLS[name]
    plan, (pieces, merged) = cell_pieces(kw)
    for sp in pieces:   # what tail_ok_ also asks: 16-byte aligned ranges of whole float4
        assert all(lo % 4 == 0 and hi % 4 == 0 and off % 4 == 0 for lo, hi, _, off in sp)
    n = A.expected_update_launches(pieces, merged, plan.tensor_offsets, **flags)
    print(f"{name}: pieces per segment {[len(s) for s in pieces]}, {len(merged)} coalesced, "
          f"{n} stand-alone launches")
    assert G.LAUNCHES[name] == n
    if name in ("flat", "none", "contiguous"):
        assert n == 0


def test_cells_reach_every_piece_count():
    """1 .. kTailPieces pieces in a segment ride, more fall back; a PS boundary inside conv2's
    weight keeps the last segment out of conv1's launch."""
    counts = {name: [len(s) for s in cell_pieces(G.CELLS[name][0])[1][0]] for name in G.CELLS}
    seen = {c for v in counts.values() for c in v}
    assert {1, 2, 3, 4} <= seen and max(seen) > A.TAIL_PIECES
    assert counts["lpt-ps4"][1] == A.TAIL_PIECES and counts["greedy-ps3"][1] > A.TAIL_PIECES
    plan, (pieces, _) = cell_pieces(G.CELLS["flat-ps3"][0])
    assert not A.final_split_conv12_ok(pieces[-1], plan.tensor_offsets)
    plan, (pieces, _) = cell_pieces(G.CELLS["contiguous-ps8"][0])
    assert len(pieces[-1]) == 4 and A.final_split_conv12_ok(pieces[-1], plan.tensor_offsets)
