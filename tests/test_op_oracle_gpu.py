"""Every GEMM-shaped op of the engine alone against the references of tests/op_reference.py.

Exact tests: FP32 MFMA is an exact fmaf chain and with integer operands in [-3, 3] every product
and partial sum is an fp32 integer (tests/test_op_reference_cpu.py test_exactness_condition), so
every summation order, split-K factor and tile gives the same bits and the comparison is
``torch.equal``.  Each case runs on a small engine (40 rows) whose float buffers are poisoned
with NaN in every row (halos stay 0), writes the inputs of rows < B, runs one op and checks the
rows < B of its outputs bit for bit, that the rows >= B and every other buffer are bit-unchanged
and that the halos are still zero.  The poison is data only: no index or address is derived from it.

Cells run (op x B x config): all 17 ops at B = 1, 5, 33 on the default config with the direct
conv1 kernels on and off; at B = 5 and 33 every tile config 0-8, 13 and 15 (4 / 8 / 16 waves) and 14
with splits 1 / 3 / default and the in-launch or the separate reduce; backward_segment 1-3 with
and without dual launches; the eval forward (default eval configs, 9-12 on conv2-4, and
DDL_EVAL_KMAP2=0); eval_count over three chunks; then the real-valued precision check of every
op and the classifier head.

Past 128 rows, on a second engine of 136 rows (the fc ops have M = batch: below 64 rows no 32-row
tile is followed by another full one and the 64- and 128-row tiles are never filled; the conv
weight gradients have K = H*H*max(batch, 32), and split counts are not monotonic in the batch):
all 17 ops at B = 128 and 129 on the default config with the direct conv1 kernels on and off; the
whole tile-config sweep at B = 129; backward_segment 1-3 at B = 128 and 129 and the head's
segment 0 at B = 129; the eval forward at B = 129, with fc1 / fc2 on eval configs 0-8.  The
exactness condition holds there too (test_op_reference_cpu.py test_exactness_condition).

Measured on one MI355X (per-test durations of a whole-suite run): the 27 tests on the 136-row
engine 3.3 s together (slowest test_ops_exact_default_config_past_128_rows[128-True], 0.52 s: it
builds the engine and the first fp64 references), so the whole tile-config sweep stays; the 75
tests on the 40-row engine, which the file had before, 4.1 s.
"""
import pytest
import torch

import op_reference as R
from ddl_amd.models.layout import CANON_OFFSETS, TOTAL_NUMEL
from ddl_amd.models.mnist_cnn import init_params_, param_views
from oracle_common import (BATCHES, BMAX, DEV, HEAD_MARGIN, KEEP, ROWS_BIG, SEED, WIDE_INLAUNCH,
                           WIDE_SEPARATE, Ctx, bits, check, head_inputs, make_real_params, prepare,
                           run_case, segment_case)

pytestmark = pytest.mark.gpu


# (Ctx, run_case, segment_case and head_inputs: tests/oracle_common.py, shared with
# tests/test_dispatch_oracle_gpu.py)
@pytest.fixture(scope="module")
def ctx():
    return Ctx(R.make_params(11))


# 128: a whole number of 16-, 32-, 64- and 128-row tiles (no partial tile, NB = 128); 129: one row
# more than each (a full interior tile followed by a partial one; NB = 129 gives ragged K tiles in
# every weight gradient)
BATCHES_BIG = (128, 129)


@pytest.fixture(scope="module")
def ctx136():
    """A 136-row engine on the same integer parameters: the fc ops have M = batch, so only past
    128 rows is every row tile (32, 64 and 128 rows) filled and followed by another one."""
    return Ctx(R.make_params(11), rows=ROWS_BIG)


@pytest.fixture(scope="module")
def rctx():
    """The same engine on real-valued, glorot-sized parameters with noisy biases."""
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=5)
    gen = torch.Generator().manual_seed(6)
    P = [p.clone() + (0.05 * torch.randn(p.shape, generator=gen) if p.dim() == 1 else 0)
         for p in param_views(flat, CANON_OFFSETS)]
    return Ctx(P)


# ---- exact: default config ------------------------------------------------------------------------
def default_config_cases(ctx, B, direct):
    e = ctx.e()
    prev = e.conv1_direct(), e.conv1_wgrad_direct()
    fails = []
    try:
        e.set_conv1_direct(direct)
        e.set_conv1_wgrad_direct(direct)
        for op in range(R.OP_COUNT):
            fails += run_case(ctx, op, B, f"default direct={direct}")
    finally:
        e.set_conv1_direct(prev[0])
        e.set_conv1_wgrad_direct(prev[1])
    return fails


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("B", BATCHES)
def test_ops_exact_default_config(ctx, B, direct):
    """All 17 ops through run_op(train=True) on the default config, the direct conv1 kernels on
    and off."""
    fails = default_config_cases(ctx, B, direct)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("B", BATCHES_BIG)
def test_ops_exact_default_config_past_128_rows(ctx136, B, direct):
    """The same on the 136-row engine at B = 128 and 129."""
    fails = default_config_cases(ctx136, B, direct)
    assert not fails, "\n".join(fails)


# ---- exact: every tile config, split and reduce mode ---------------------------------------------------
# (config, waves): 13 / 15 take their wave count from the op's split factor
TILE_CFGS = [(c, None) for c in range(9)] + [(13, w) for w in (4, 8, 16)] + [(14, None)] + \
            [(15, w) for w in (4, 8, 16)]


def tile_config_cases(ctx, B, cfg, waves):
    e = ctx.e()
    eng = ctx.eng
    base = eng.get_cfg(), eng.get_splits(), eng.get_wide()
    prev = e.conv1_direct(), e.conv1_wgrad_direct()
    n = len(base[0])
    if waves is not None:
        variants = [([waves] * n, WIDE_INLAUNCH)]
    else:
        variants = [([1] * n, WIDE_INLAUNCH)]
        for spl in ([3] * n, list(base[1])):
            variants += [(spl, WIDE_INLAUNCH), (spl, WIDE_SEPARATE)]
    fails = []
    try:
        e.set_conv1_direct(False)
        e.set_conv1_wgrad_direct(False)
        eng.set_cfg([cfg] * n)
        for spl, wide in variants:
            eng.set_splits(spl)
            eng.set_wide([wide] * n)
            for op in range(R.OP_COUNT):
                fails += run_case(ctx, op, B, f"cfg={cfg} splits={spl[op]} wide={wide}")
    finally:
        e.set_conv1_direct(prev[0])
        e.set_conv1_wgrad_direct(prev[1])
        eng.set_cfg(base[0])
        eng.set_splits(base[1])
        eng.set_wide(base[2])
    return fails


@pytest.mark.parametrize("cfg,waves", TILE_CFGS)
@pytest.mark.parametrize("B", [5, 33])
def test_ops_exact_tile_configs(ctx, B, cfg, waves):
    """Every op on tile config `cfg` (ops without an instantiation of it fall back to the
    one-wave 32x32 tile with the same split factor), splits 1 / 3 / default, in-launch and
    separate split-K reduce; conv1 on the GEMM path so that its configs run too."""
    fails = tile_config_cases(ctx, B, cfg, waves)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("cfg,waves", TILE_CFGS)
def test_ops_exact_tile_configs_129_rows(ctx136, cfg, waves):
    """The same sweep (every config, splits 1 / 3 / default, both reduce modes) at B = 129 on the
    136-row engine: the 64-row tiles of configs 0, 2, 6, 7 are filled twice and the 128-row tile
    of config 1 once, each followed by a one-row tile."""
    fails = tile_config_cases(ctx136, 129, cfg, waves)
    assert not fails, "\n".join(fails[:40])


# ---- exact: the default launches of backward_segment --------------------------------------------------
def backward_segment_cases(ctx, B, dual):
    fails = []
    ctx.eng.set_dual(dual)
    try:
        for s in (1, 2, 3):
            inputs, ref = segment_case(ctx, s, B)
            x, snap = prepare(ctx, B, inputs)
            ctx.e().backward_segment(s, x, ctx.labels[:B], ctx.seed_t)
            torch.cuda.synchronize()
            fails += check(ctx, B, snap, ref, f"segment {s} B={B} dual={dual}")
    finally:
        ctx.eng.set_dual(True)
    return fails


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("B", BATCHES)
def test_backward_segments_exact(ctx, B, dual):
    """backward_segment(1..3): the dual launches, run_dual_then with the direct conv1 weight
    gradient and conv2's reduce inside it; then the same back to back (set_dual(False))."""
    fails = backward_segment_cases(ctx, B, dual)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("B", BATCHES_BIG)
def test_backward_segments_exact_past_128_rows(ctx136, B, dual):
    """The same on the 136-row engine at B = 128 and 129."""
    fails = backward_segment_cases(ctx136, B, dual)
    assert not fails, "\n".join(fails)


# ---- exact: the eval forward ------------------------------------------------------------------------
def eval_cases(c, B, tag):
    e = c.e()
    base = list(e.get_eval_cfg())
    fails = []
    try:
        for big in (None, 9, 10, 11, 12):
            cfg = list(base)
            if big is not None:
                cfg[1] = cfg[2] = cfg[3] = big
            e.set_eval_cfg(cfg)
            for op in (range(6) if big is None else (1, 2, 3)):
                fails += run_case(c, op, B, f"{tag} eval_cfg={cfg[op]}", train=False)
    finally:
        e.set_eval_cfg(base)
    return fails


@pytest.mark.parametrize("B", BATCHES)
def test_eval_forward_exact(ctx, B):
    """run_op(train=False) of the conv and fc forwards: the default eval configs (conv2 on its
    eval K map), then the eval-only tiles 9-12 on conv2-4, conv1 on both of its kernels.  No
    dropout, and the code buffers (the sentinel in rows < B) stay bit-unchanged."""
    e = ctx.e()
    prev = e.conv1_direct()
    fails = eval_cases(ctx, B, "direct")
    try:
        e.set_conv1_direct(not prev)
        fails += run_case(ctx, 0, B, f"eval conv1_direct={not prev}", train=False)
    finally:
        e.set_conv1_direct(prev)
    assert not fails, "\n".join(fails)


def test_eval_forward_exact_129_rows(ctx136):
    """The eval forward cells of test_eval_forward_exact at B = 129 on the 136-row engine, then
    fc1 and fc2 (run_op(train=False), M = 129) on each of the tile configs 0-8 as eval config."""
    c = ctx136
    e = c.e()
    B = 129
    fails = eval_cases(c, B, "rows=136")
    prev = e.conv1_direct()
    base = list(e.get_eval_cfg())
    try:
        e.set_conv1_direct(not prev)
        fails += run_case(c, 0, B, f"eval conv1_direct={not prev}", train=False)
        e.set_conv1_direct(prev)
        for cfg in range(9):
            ec = list(base)
            ec[4] = ec[5] = cfg
            e.set_eval_cfg(ec)
            for op in (4, 5):
                fails += run_case(c, op, B, f"rows=136 eval_cfg={cfg}", train=False)
    finally:
        e.set_conv1_direct(prev)
        e.set_eval_cfg(base)
    assert not fails, "\n".join(fails)


def test_eval_forward_exact_image_major_conv2(monkeypatch):
    """The same on an engine built with DDL_EVAL_KMAP2=0 (conv2's eval forward on the image-major
    GEMM)."""
    monkeypatch.setenv("DDL_EVAL_KMAP2", "0")
    c = Ctx(R.make_params(11))
    fails = []
    for B in BATCHES:
        fails += eval_cases(c, B, "kmap2=0")
    assert not fails, "\n".join(fails)


def test_eval_count_last_chunk_small(rctx):
    """eval_count over 3 chunks (40, 40 and 5 rows: the last one runs on buffers that hold the
    previous chunk's rows) equals the count from the GPU's own logits() argmax, row by row
    without ties."""
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2 * BMAX + 5, 784, generator=gen).to(DEV)
    y = torch.randint(0, 10, (2 * BMAX + 5,), generator=gen).to(DEV)
    want = 0
    for i in range(0, x.shape[0], BMAX):
        lg = rctx.eng.logits(x[i:i + BMAX]).clone()
        top = lg.max(dim=1, keepdim=True).values
        assert int((lg == top).sum()) == lg.shape[0]   # no duplicated maximum
        want += int((lg.argmax(1) == y[i:i + BMAX]).sum())
    assert rctx.eng.correct(x, y) == want
    assert 0 < want < x.shape[0]


# ---- real-valued precision ------------------------------------------------------------------------------
@pytest.mark.parametrize("op", range(R.OP_COUNT))
def test_ops_real_valued_precision(rctx, op):
    """B = 33, default config (conv1 on the direct kernels and on the GEMM path), asymmetric real
    inputs, codes and masks given.  Per element err = |gpu - ref64| / sum |a_i||b_i| must stay
    within the fp32 dot-product ceiling (K + 8) 2^-24, and the tensor's RMS err within
    op_reference.MARGIN (2) times the RMS err of the fp32 CPU computation of the same op.

    The margin is 2 rather than 4 because 4 would not notice one extra term at K = 6400
    (op_reference.MARGIN).  Measured RMS err ratio GPU / fp32 CPU on one MI355X (dW / db for the
    weight gradients; the printed lines give the current figures):
    conv1 fwd 1.01 (direct) 0.80 (GEMM), conv2 fwd 0.40, conv3 fwd 0.39, conv4 fwd 0.30,
    fc1 fwd 0.84, fc2 fwd 0.85, fc2 dgrad 0.64, fc2 wgrad 0.68 / 0.89, fc1 dgrad 0.85,
    fc1 wgrad 0.68 / 0.91, conv4 dgrad 0.52, conv4 wgrad 0.84 / 1.23, conv3 dgrad 0.33,
    conv3 wgrad 0.96 / 1.48, conv2 dgrad 0.52, conv2 wgrad 0.50 / 0.87,
    conv1 wgrad 0.024 / 1.31 (direct) 0.016 / 0.61 (GEMM).  Largest per-element err 2.1e-7
    (conv1 fwd, ceiling 2.0e-6).  The ratios above 1 are bias gradients, which the CPU sums with
    torch's cascaded sum and the GPU as one more GEMM row in K-tile order.
    """
    B = 33
    c = rctx
    inputs, ref = c.case(op, B, True, real=True)
    f32 = R.run_op(op, c.P, inputs, SEED, KEEP, True, dtype=torch.float32)
    asum = R.abs_sum(op, c.P64, inputs, KEEP)
    K = R.k_terms(op, B)
    e = c.e()
    prev = e.conv1_direct(), e.conv1_wgrad_direct()
    fails = []
    try:
        for direct in ((True, False) if op in (0, 16) else (True,)):
            e.set_conv1_direct(direct)
            e.set_conv1_wgrad_direct(direct)

            def compare(name, got, r64):
                s = asum[name].reshape(r64.shape)
                base = R.rms(R.rel_err(f32[name].reshape(r64.shape), r64, s)[0], s)
                f, (emax, erms) = R.precision_failures(got, r64, s, K, base)
                print(f"ORACLE-RATIO {R.OP_NAMES[op]} direct={direct} {name}: K={K} "
                      f"max err {emax:.3g} (ceiling {(K + 8) * R.U32:.3g}) rms {erms:.3g} "
                      f"fp32 CPU rms {base:.3g} ratio {erms / max(base, 1e-300):.3f}")
                return [f"{R.OP_NAMES[op]} {name} direct={direct}: {m}" for m in f]

            x, snap = prepare(c, B, inputs)
            e.run_op(op, x, c.seed_t, True)
            torch.cuda.synchronize()
            vals = {k: v for k, v in ref.items() if not k.startswith("c")}
            fails += check(c, B, snap, vals, f"{R.OP_NAMES[op]} real", compare,
                           ignore=[k for k in ref if k.startswith("c")])
    finally:
        e.set_conv1_direct(prev[0])
        e.set_conv1_wgrad_direct(prev[1])
    assert not fails, "\n".join(fails)


# ---- classifier head -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["fused", "fwd_bwd"])
@pytest.mark.parametrize("keep", [0.5, 1.0])
@pytest.mark.parametrize("B", [1, 33])
def test_head_matches_reference(B, keep, kernel):
    """head_fused (the default) and head_fwd + head_bwd (set_concurrent(True)) through
    backward_segment(0), h2 written directly: per-row loss, dlog, dpre2fc, fc3's dW / db against
    the fp64 reference.  Each tensor's max abs error must stay within 8x that of the fp32 torch CPU
    computation on the same inputs (not counted below half an ulp of the tensor's largest value,
    the error of merely storing the fp64 result in fp32): the kernels use the hardware exp / log
    approximations and a 4-wave partial-sum order.  dpre2fc is exactly 0 where ops.rng drops, and
    non-zero where it keeps on the ordinary rows.

    Measured max-error ratio GPU / max(fp32 CPU, half-ulp floor) on one MI355X, the largest over
    B, keep and labels, the same for both kernel pairs: loss 1.39, dlog 0.35, dpre2fc 1.33,
    fc3 dW 0.63, db 0.35.
    """
    fails = head_cases(Ctx(make_real_params()), B, keep, kernel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kernel", ["fused", "fwd_bwd"])
def test_head_matches_reference_129_rows(kernel):
    """backward_segment(0) by the same rule at B = 129 and keep 0.5 on a 136-row engine:
    head_fused's row tiles (bx = row >> 5) past the fourth, and the fc backward of the segment
    at M = 129."""
    fails = head_cases(Ctx(make_real_params(), rows=ROWS_BIG), 129, 0.5, kernel)
    assert not fails, "\n".join(fails)


def head_cases(c, B, keep, kernel):
    gen = torch.Generator().manual_seed(100 + B)
    if B > 1:
        h2, labels, extreme = head_inputs(c.P, B, gen, range(0, B, 3))
        assert len(torch.unique(labels)) == 10
        cases = [(h2, labels, extreme)]
    else:   # every class as the label, on an ordinary and on an extreme row in turn
        rows = [head_inputs(c.P, 1, gen, ()), head_inputs(c.P, 1, gen, (0,))]
        cases = [(rows[k % 2][0], torch.tensor([k]), rows[k % 2][2]) for k in range(10)]
    c.eng._set_keep(keep)
    c.eng.set_concurrent(kernel == "fwd_bwd")
    fails = []
    try:
        for h2, lab, extreme in cases:
            mask = R.keep_mask(SEED, 2, B, 512, keep) if keep < 1.0 else None
            ref = R.head(h2, c.P[12], c.P[13], lab, mask, 1.0 / keep)
            cpu = R.head(h2, c.P[12], c.P[13], lab, mask, 1.0 / keep, dtype=torch.float32)
            # finite, ordinary data in everything the rest of the segment (the fc backward) reads
            inputs = {"h2": h2, "h1": R.make_inputs(5, B, 2, real=True)["h1"],
                      "p4": R.make_inputs(4, B, 2, real=True)["p4"],
                      "c4": torch.zeros(B, 1024, dtype=torch.uint8)}
            x, snap = prepare(c, B, inputs)
            c.e().backward_segment(0, x, lab.to(DEV), c.seed_t)
            torch.cuda.synchronize()
            got = {"loss": c.whole("loss")[:B], "dlog": c.whole("dlog")[:B],
                   "dpre2fc": c.whole("dpre2fc")[:B], "gw": c.gview(12), "gb": c.gview(13)}
            for name, g in got.items():
                g = g.cpu().double()
                r = ref[name].reshape(g.shape)
                e_gpu = float((g - r).abs().max())
                e_cpu = float((cpu[name].reshape(g.shape).double() - r).abs().max())
                floor = R.U32 * float(r.abs().max())
                ratio = e_gpu / max(e_cpu, floor, 1e-300)
                print(f"HEAD-RATIO {kernel} B={B} keep={keep} lab={lab[0].item()} {name}: gpu "
                      f"{e_gpu:.3g} fp32 CPU {e_cpu:.3g} floor {floor:.3g} ratio {ratio:.3f}")
                if not (e_gpu <= HEAD_MARGIN * max(e_cpu, floor)):
                    fails.append(f"{name} B={B} keep={keep} {kernel}: gpu err {e_gpu:.3g} > 8 x "
                                 f"max(fp32 CPU err {e_cpu:.3g}, {floor:.3g})")
            nz = got["dpre2fc"].cpu() != 0
            keepm = mask if mask is not None else torch.ones(B, 512, dtype=torch.bool)
            if bool((nz & ~keepm).any()):
                fails.append(f"dpre2fc non-zero where the mask drops (B={B} keep={keep} {kernel})")
            if not torch.equal(nz[~extreme], keepm[~extreme]):
                fails.append(f"dpre2fc zero pattern differs from the mask (B={B} keep={keep})")
            ordinary = ~extreme
            if bool(ordinary.any()):
                ml = float(got["loss"].cpu().double()[ordinary].mean())
                if abs(ml - float(ref["loss"][ordinary].mean())) >= 1e-5:
                    fails.append(f"mean loss off by more than 1e-5 (B={B} keep={keep} {kernel})")
            for n in ("loss", "dlog", "dpre2fc"):
                if not torch.equal(bits(c.whole(n)[B:]), snap[n][B:]):
                    fails.append(f"{n} rows >= {B} changed")
    finally:
        c.eng.set_concurrent(False)
    return fails


def test_slab_sized_for_every_smaller_batch():
    """The split-K slab holds the partials of every batch up to the engine's.  A split count is K
    over a chunk rounded to whole K tiles, so it is not monotonic in the batch: conv4's weight
    gradient (split 6) stores 5 partial sets at batch 40 and 6 at batch 33 and at every batch
    <= 32.  Sized at its own batch alone, a 40-row engine let the conv4 dual launch of
    backward_segment(1) at B = 1 write 3.3 MB past the second slab, beyond the workspace
    (found by test_backward_segments_exact[1-True])."""
    from ddl_amd.models.hip_engine import HipEngine
    params = torch.zeros(TOTAL_NUMEL, device=DEV)
    grads = torch.zeros_like(params)
    size = {}
    for small, big in ((33, BMAX), (129, ROWS_BIG)):
        for b in (small, big):
            eng = HipEngine(params, grads, CANON_OFFSETS, batch=b, graph=False, eval_chunk=big)
            size[b] = eng.eng.workspace_bytes()
        assert size[big] >= size[small]
