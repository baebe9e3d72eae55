"""Numerics of the gfx950 HIP kernels vs a plain PyTorch fp32 CPU reference of the same ops.

Every activation (pooled conv outputs, fc outputs with dropout), every one of the 14
gradients, the fused Adam update and the eval count are checked.  Inputs are asymmetric
random data (guide rule: never a symmetric / identity operand).
"""
import pytest
import torch
import torch.nn.functional as F

from ddl_amd.models.layout import TENSORS, CANON_OFFSETS, TOTAL_NUMEL
from ddl_amd.models.mnist_cnn import (init_params_, param_views, torch_forward, xent_loss,
                                      dropout_apply, _pool_same)
from ddl_amd.ops import rng
from onecard import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"



def ref_intermediates(p, x, keep, seed):
    """CPU fp32 forward returning NHWC pooled maps and fc activations."""
    n = x.shape[0]
    h = x.view(n, 1, 28, 28)
    pooled = []
    for li in range(4):
        h = F.conv2d(h, p[2 * li].permute(3, 2, 0, 1), p[2 * li + 1], padding=2)
        h = _pool_same(F.relu(h))
        pooled.append(h.permute(0, 2, 3, 1).contiguous())
    f = pooled[-1].reshape(n, -1)
    h1 = dropout_apply(F.relu(f @ p[8] + p[9]), seed, 1, keep)
    h2 = dropout_apply(h1 @ p[10] + p[11], seed, 2, keep)
    return pooled, h1, h2


@pytest.fixture(scope="module")
def setup():
    from ddl_amd.models.hip_engine import HipEngine
    torch.manual_seed(0)
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=3)
    # make biases non-trivial so bias paths are exercised
    pv = param_views(flat, CANON_OFFSETS)
    for t, v in zip(TENSORS, pv):
        if t.kind == "bias":
            v.add_(torch.randn_like(v) * 0.05)
    params = flat.to(DEV)
    grads = torch.zeros_like(params)
    B = 100
    eng = HipEngine(params, grads, CANON_OFFSETS, batch=B, graph=False, eval_chunk=500,
                    keep_prob=0.5)
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,))
    return eng, flat, params, grads, x, y


def test_forward_activations(setup):
    eng, flat, params, grads, x, y = setup
    seed = 12345
    pv = param_views(flat, CANON_OFFSETS)
    pooled, h1, h2 = ref_intermediates(pv, x, 0.5, seed)
    seed_t = torch.tensor([seed], dtype=torch.int32, device=DEV)
    eng.eng.forward(x.to(DEV), seed_t, True)
    torch.cuda.synchronize()
    B = x.shape[0]
    for name, ref in zip(["p1", "p2", "p3", "p4"], pooled):
        got = eng.eng.buffer(name, B)
        assert rel_err(got.reshape(ref.shape), ref) < 2e-5, name
    assert rel_err(eng.eng.buffer("h1", B), h1) < 2e-5
    assert rel_err(eng.eng.buffer("h2", B), h2) < 2e-5
    # dropout masks identical: zero pattern of h1 (relu & mask) matches
    assert torch.equal(eng.eng.buffer("h1", B).cpu() > 0, h1 > 0)


def test_halo_borders_stay_zero(setup):
    """Conv inputs and conv data-gradient inputs are stored with a 2-pixel zero halo that no
    kernel writes (csrc/kernels/layers.h kHalo): after training steps and a full-batch eval
    every border element is still exactly 0 and the interior is not."""
    eng, flat, params, grads, x, y = setup
    for i in range(3):
        eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 100 + i)
    eng.correct(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    B = eng.eng.max_batch()
    for name in ["p1", "p2", "p3", "d4", "d3", "d2"]:
        whole = eng.eng.buffer(name + "+halo", B).cpu()
        inner = whole[:, 2:-2, 2:-2, :].clone()
        whole[:, 2:-2, 2:-2, :] = 0
        assert torch.count_nonzero(whole) == 0, name
        assert torch.count_nonzero(inner[: x.shape[0]]) > 0, name


def ref_grads(flat, x, y, keep, seed, dtype):
    pv = [v.detach().to(dtype).clone().requires_grad_(True) for v in param_views(flat, CANON_OFFSETS)]
    loss = xent_loss(torch_forward(pv, x.to(dtype), keep, seed), y)
    return loss, torch.autograd.grad(loss, pv)


def check_grads(grads, flat, x, y, keep, seed):
    """HIP grads vs the fp32 torch reference; where fp32 summation order itself matters
    (conv1 dW sums 78,400 cancelling terms) the HIP error vs an fp64 reference must be no
    worse than 2x the fp32 reference's own error."""
    loss32, r32 = ref_grads(flat, x, y, keep, seed, torch.float32)
    _, r64 = ref_grads(flat, x, y, keep, seed, torch.float64)
    for t, g, a, b in zip(TENSORS, param_views(grads, CANON_OFFSETS), r32, r64):
        e_hip, e_ref = rel_err(g, b), rel_err(a, b)
        assert rel_err(g, a) < 5e-5 or e_hip <= 2 * e_ref + 1e-6, \
            f"{t.name} {t.layer} {t.kind} hip-vs-f64={e_hip:.3g} torch32-vs-f64={e_ref:.3g}"
    return loss32


@pytest.mark.parametrize("B", [100, 37])
def test_gradients_match_autograd(setup, B):
    eng, flat, params, grads, x, y = setup
    seed = 777
    x, y = x[:B], y[:B]
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, seed)
    torch.cuda.synchronize()
    loss = check_grads(grads, flat, x, y, 0.5, seed)
    assert abs(float(eng.eng.buffer("loss", B).mean()) - float(loss.detach())) < 1e-5


@pytest.mark.parametrize("B", [100, 37])
def test_conv1_direct_matches_gemm_path(setup, B):
    """conv1 forward on the direct LDS-staged kernel (csrc/kernels/conv1.hip) against the GEMM
    engine's ConvFwd<28, 1, 32> launch: pooled p1 to fp32 summation-order noise (the two
    accumulate the 25 taps in different MFMA pairings) and the pool / ReLU codes equal except
    on exact near-ties."""
    eng, flat, params, grads, x, y = setup
    xb = x[:B].to(DEV)
    seed_t = torch.tensor([5], dtype=torch.int32, device=DEV)
    out = []
    prev = eng.eng.conv1_direct()
    try:
        for on in (True, False):
            eng.eng.set_conv1_direct(on)
            eng.eng.forward(xb, seed_t, True)
            torch.cuda.synchronize()
            out.append((eng.eng.buffer("p1", B).clone(), eng.eng.buffer("c1", B).clone()))
    finally:
        eng.eng.set_conv1_direct(prev)
    assert rel_err(out[0][0], out[1][0]) < 1e-6
    assert (out[0][1] == out[1][1]).float().mean().item() > 0.9999


@pytest.mark.parametrize("B", [100, 37])
def test_conv1_wgrad_direct_matches_gemm_path(setup, B):
    """conv1's weight / bias gradient on the direct kernel with its two-level in-launch reduce
    (csrc/kernels/conv1.h, sharing the launch with conv2's weight-gradient reduce) against the
    split-K GEMM + wide reduce: conv1's dW / db to fp32 summation-order noise, every other
    gradient bit-identical."""
    eng, flat, params, grads, x, y = setup
    xb, yb = x[:B].to(DEV), y[:B].to(DEV)
    out = []
    prev = eng.eng.conv1_wgrad_direct()
    try:
        for on in (True, False, True):
            eng.eng.set_conv1_wgrad_direct(on)
            grads.zero_()
            eng.forward_backward(xb, yb, 0.5, 4242)
            torch.cuda.synchronize()
            out.append(grads.clone())
    finally:
        eng.eng.set_conv1_wgrad_direct(prev)
    # deterministic: the same launch twice gives the same bits
    assert torch.equal(out[0], out[2])
    va, vb = param_views(out[0], CANON_OFFSETS), param_views(out[1], CANON_OFFSETS)
    for t, a, b in zip(TENSORS, va, vb):
        if t.index < 2:
            assert rel_err(a, b) < 2e-6, t.name
        else:
            assert torch.equal(a, b), t.name


@pytest.mark.parametrize("B", [8, 13, 130])
def test_conv1_direct_kernels_odd_batches(B):
    """The direct conv1 kernels at batch sizes that exercise their edges: two full reduce groups
    of 8 blocks (B = 8), a partial last group (B = 13: 26 blocks), and more than 32 groups
    (B = 130: the final reduce level loops over two chunks) — against the GEMM path, and conv1's
    dW / db against the fp64 autograd reference."""
    from ddl_amd.models.hip_engine import HipEngine
    torch.manual_seed(B)
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=11)
    params = flat.to(DEV)
    grads = torch.zeros_like(params)
    eng = HipEngine(params, grads, CANON_OFFSETS, batch=B, graph=False, eval_chunk=500,
                    keep_prob=1.0)
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,))
    out = []
    for on in (True, False):
        eng.eng.set_conv1_direct(on)
        eng.eng.set_conv1_wgrad_direct(on)
        grads.zero_()
        eng.forward_backward(x.to(DEV), y.to(DEV), 1.0, 0)
        torch.cuda.synchronize()
        out.append((grads.clone(), eng.eng.buffer("p1", B).clone()))
    va, vb = param_views(out[0][0], CANON_OFFSETS), param_views(out[1][0], CANON_OFFSETS)
    for t, a, b in zip(TENSORS, va, vb):
        assert rel_err(a, b) < 1e-5, t.name
    assert rel_err(out[0][1], out[1][1]) < 1e-6
    _, r64 = ref_grads(flat, x, y, 1.0, 0, torch.float64)
    for t in TENSORS[:2]:
        o = CANON_OFFSETS[t.index]
        assert rel_err(out[0][0][o:o + t.numel], r64[t.index].reshape(-1)) < 5e-3, t.name


def test_gradients_no_dropout(setup):
    eng, flat, params, grads, x, y = setup
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 1.0, 0)
    torch.cuda.synchronize()
    check_grads(grads, flat, x, y, 1.0, 0)
    eng._set_keep(0.5)


def test_split_k_variants_agree(setup):
    """Every op with split-K 1 vs its default split gives the same gradients."""
    eng, flat, params, grads, x, y = setup
    base = eng.get_splits()
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 99)
    g0 = grads.clone()
    eng.set_splits([1] * len(base))
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 99)
    g1 = grads.clone()
    eng.set_splits([max(2, s * 2) for s in base])
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 99)
    g2 = grads.clone()
    eng.set_splits(base)
    _, r64 = ref_grads(flat, x, y, 0.5, 99, torch.float64)
    _, r32 = ref_grads(flat, x, y, 0.5, 99, torch.float32)
    for t in TENSORS:
        o = CANON_OFFSETS[t.index]
        ref = r64[t.index].reshape(-1)
        # conv dW/db reduce 1,600-78,400 cancelling terms over the batch; and an fp32 forward
        # can take a different pool/ReLU branch than fp64 on near-ties (at this seed the CPU
        # fp32 reference itself is 6.4e-3 off fp64 on conv2 dW): bound by the fp32
        # reference's own error as well
        e32 = rel_err(r32[t.index].reshape(-1), ref)
        for name, g in (("default", g0), ("split1", g1), ("split2x", g2)):
            tol = 5e-5 if t.index > 7 else max(5e-3, 2 * e32 + 1e-6)
            err = rel_err(g[o:o + t.numel], ref)
            assert err < tol, (t.name, name, err, e32)


@pytest.mark.parametrize("cfg", [None, 0, 1, 2, 4, 5, 6, 7, 8])
def test_split_factors_match_reference(setup, cfg):
    """Split-K schedules (several split factors, every tile config) give the fp64-reference
    gradients, and a given schedule is bit-deterministic across runs (the stream-K schedules
    this test covered until round 5 were removed: docs/DESIGN.md round 6)."""
    eng, flat, params, grads, x, y = setup
    base_cfg, base_s = eng.get_cfg(), eng.get_splits()
    if cfg is not None:
        eng.set_cfg([cfg] * len(base_cfg))
    _, r64 = ref_grads(flat, x, y, 0.5, 31, torch.float64)
    try:
        for f in (1, 3, 8):
            eng.set_splits([max(1, s * f // 4) for s in base_s])
            outs = []
            for _ in range(2):
                grads.zero_()
                eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 31)
                torch.cuda.synchronize()
                outs.append(grads.clone())
            assert torch.equal(outs[0], outs[1]), f"split x{f}/4 not deterministic"
            for t in TENSORS:
                o = CANON_OFFSETS[t.index]
                tol = 5e-5 if t.index > 7 else 5e-3
                err = rel_err(outs[0][o:o + t.numel], r64[t.index].reshape(-1))
                assert err < tol, (t.name, f, err)
    finally:
        eng.set_cfg(base_cfg)
        eng.set_splits(base_s)


@pytest.mark.parametrize("cfg", [None, 6, 7, 8])
@pytest.mark.parametrize("wide", [1 << 20, 1])
def test_inlaunch_splitk_reduce_matches_reference(setup, cfg, wide):
    """Split-K with the in-launch last-arriver reduce (sc1 hand-off; wide = 1: the separate
    wide-reduce kernel) for every op, default and multi-wave tile configs: fp64 reference
    gradients, bit-deterministic across runs."""
    eng, flat, params, grads, x, y = setup
    base_s, base_wide = eng.get_splits(), eng.get_wide()
    base_cfg = eng.get_cfg()
    _, r64 = ref_grads(flat, x, y, 0.5, 77, torch.float64)
    try:
        if cfg is not None:
            eng.set_cfg([cfg] * len(base_cfg))
        eng.set_splits([max(2, min(s, 64)) for s in base_s])
        eng.set_wide([wide] * len(base_s))
        outs = []
        for _ in range(2):
            grads.zero_()
            eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 77)
            torch.cuda.synchronize()
            outs.append(grads.clone())
        assert torch.equal(outs[0], outs[1])
        for t in TENSORS:
            o = CANON_OFFSETS[t.index]
            tol = 5e-5 if t.index > 7 else 5e-3
            assert rel_err(outs[0][o:o + t.numel], r64[t.index].reshape(-1)) < tol, t.name
    finally:
        eng.set_cfg(base_cfg)
        eng.set_splits(base_s)
        eng.set_wide(base_wide)


@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("packed", [False, True])
def test_kwave_config_matches_reference(setup, waves, packed):
    """The GEMMs on the K-wave launch (CFG_KWAVE = 13: K split over the waves of one
    workgroup, LDS reduction, fused epilogue): fp64-reference gradients, bit-deterministic
    across runs.  packed=False: every op set to 13 (the forward convs fall back to one-wave
    32x32 and so do the conv GEMMs, which have no K-wave instantiation; the fc backward pairs
    run back to back as K-wave launches); packed=True: only the fc data gradients on 13, so
    each fc backward is one packed launch with its weight gradient and the fc3 aux blocks."""
    eng, flat, params, grads, x, y = setup
    base_cfg, base_s = eng.get_cfg(), eng.get_splits()
    try:
        if packed:
            cfg, spl = list(base_cfg), list(base_s)
            for op in (6, 8):  # the fc data gradients
                cfg[op], spl[op] = 13, waves
            eng.set_cfg(cfg)
            eng.set_splits(spl)
        else:
            eng.set_cfg([13] * len(base_cfg))
            eng.set_splits([waves] * len(base_s))
        outs = []
        for _ in range(2):
            grads.zero_()
            eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 55)
            torch.cuda.synchronize()
            outs.append(grads.clone())
        assert torch.equal(outs[0], outs[1])
        # fc tensors within 5e-5 of fp64; the cancelling conv sums no worse than 2x the fp32
        # reference's own error (check_grads)
        check_grads(outs[0], flat, x, y, 0.5, 55)
    finally:
        eng.set_cfg(base_cfg)
        eng.set_splits(base_s)


# conv2-4 forward, conv4..conv2 data / weight gradient (csrc/kernels/schedule.h op order)
MF16_OPS = (1, 2, 3, 10, 11, 12, 13, 14, 15)
KWAVE_OPS = (4, 5, 6, 8)   # fc forwards and data gradients (test_kwave_config_matches_reference)
KW16_OPS = (4, 5)          # fc forwards (test_kw16_fc_matches_reference)


def test_special_config_op_sets_are_the_engines(setup):
    """The op sets these tests put on configs 13 / 14 / 15 are the ops the engine has those
    instantiations for (Engine.op_has_cfg, csrc/kernels/schedule.h): a config anywhere else falls
    back to config 3, silently, and such a test would pass without running its kernel."""
    eng = setup[0].eng
    for cfg, ops in ((13, KWAVE_OPS), (14, MF16_OPS), (15, KW16_OPS)):
        for train in (True, False):
            assert tuple(op for op in range(17) if eng.op_has_cfg(op, cfg, train)) == ops
    cfg = list(eng.get_cfg())
    assert eng.effective_cfg() == [c if eng.op_has_cfg(op, c, True) else 3
                                   for op, c in enumerate(cfg)]


@pytest.mark.parametrize("mode", ["default", "split1", "wide", "nodual", "mixed"])
def test_mf16_config_matches_reference(setup, mode):
    """CFG_MF16 = 14 (gemm.h mainloop_dma16: one-wave 32x32x32 tile on v_mfma_f32_16x16x4_f32,
    LDS-DMA staging with the 16x16 image swizzles, accumulators re-laid out through LDS into the
    32x32 layout) on every conv GEMM: the fp32 / fp64 autograd gradients (check_grads) under
    every schedule that consumes its accumulators — fused epilogue (split 1), in-launch
    last-arriver reduce, separate wide reduce, dual and back-to-back
    launches, and mixed with the 32x32x2 tiles in one dual launch — bit-deterministic across
    reruns, and the forward activations within fp32 noise of the reference."""
    eng, flat, params, grads, x, y = setup
    base = (eng.get_cfg(), eng.get_splits(), eng.get_wide())
    cfg, spl, wide = (list(v) for v in base)
    ops = MF16_OPS if mode != "mixed" else (1, 3, 10, 13, 14)  # the others stay on 32x32x2
    for op in ops:
        cfg[op] = 14
        if mode == "split1":
            spl[op] = 1
        elif mode == "wide":
            spl[op], wide[op] = max(2, spl[op]), 1
    try:
        eng.set_cfg(cfg)
        eng.set_splits(spl)
        eng.set_wide(wide)
        eng.set_dual(mode != "nodual")
        outs = []
        for _ in range(2):
            grads.zero_()
            eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 66)
            torch.cuda.synchronize()
            outs.append(grads.clone())
        assert torch.equal(outs[0], outs[1])
        check_grads(outs[0], flat, x, y, 0.5, 66)
        pv = param_views(flat, CANON_OFFSETS)
        pooled, _, _ = ref_intermediates(pv, x, 0.5, 66)
        for name, ref in zip(["p1", "p2", "p3", "p4"], pooled):
            got = eng.eng.buffer(name, x.shape[0])
            assert rel_err(got.reshape(ref.shape), ref) < 2e-5, name
    finally:
        eng.set_dual(True)
        eng.set_cfg(base[0])
        eng.set_splits(base[1])
        eng.set_wide(base[2])


@pytest.mark.parametrize("op,waves", [(4, 4), (4, 8), (4, 16), (5, 4), (5, 8), (5, 16)])
def test_kw16_fc_matches_reference(setup, op, waves):
    """CFG_KW16 = 15 (kwave16.h gemm_kw16_kernel: the K-wave launch on 16-row v_mfma_f32_16x16x4
    tiles, N-contiguous B staged through each wave's swizzled LDS image) on fc1's or fc2's
    forward (fc2: the head then reads h2 instead of fc2's split-K partials; both are the
    default), at 4 / 8 / 16 waves: h1 / h2 (ReLU, dropout) within fp32 noise of the CPU reference, the 14 gradients against the fp32 /
    fp64 autograd reference, bit-deterministic across runs."""
    eng, flat, params, grads, x, y = setup
    base_cfg, base_s = eng.get_cfg(), eng.get_splits()
    cfg, spl = list(base_cfg), list(base_s)
    cfg[op], spl[op] = 15, waves  # OP_FC1_FWD / OP_FC2_FWD (api.h op order)
    try:
        eng.set_cfg(cfg)
        eng.set_splits(spl)
        outs = []
        for _ in range(2):
            grads.zero_()
            eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 88)
            torch.cuda.synchronize()
            outs.append(grads.clone())
        assert torch.equal(outs[0], outs[1])
        check_grads(outs[0], flat, x, y, 0.5, 88)
        pv = param_views(flat, CANON_OFFSETS)
        _, h1, h2 = ref_intermediates(pv, x, 0.5, 88)
        got = eng.eng.buffer("h1", x.shape[0])
        assert rel_err(got, h1) < 2e-5
        assert torch.equal(got.cpu() > 0, h1 > 0)
        assert rel_err(eng.eng.buffer("h2", x.shape[0]), h2) < 2e-5
    finally:
        eng.set_cfg(base_cfg)
        eng.set_splits(base_s)


@pytest.mark.parametrize("conc,dual", [(False, True), (False, False), (True, False)])
def test_backward_modes_match(setup, conc, dual):
    """Single-stream dual launches, single-stream back-to-back and the two-stream backward
    compute the same (bitwise: same schedules, same reduction orders) gradients."""
    eng, flat, params, grads, x, y = setup
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 55)
    torch.cuda.synchronize()
    ref = grads.clone()
    eng.set_concurrent(conc)
    eng.set_dual(dual)
    try:
        grads.zero_()
        eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 55)
        torch.cuda.synchronize()
        assert torch.equal(grads, ref)
    finally:
        eng.set_concurrent(False)
        eng.set_dual(True)


def test_graph_replay_matches_eager(setup):
    from ddl_amd.models.hip_engine import HipEngine
    eng, flat, params, grads, x, y = setup
    geng = HipEngine(params, grads, CANON_OFFSETS, batch=100, graph=True, keep_prob=0.5)
    grads.zero_()
    eng.forward_backward(x.to(DEV), y.to(DEV), 0.5, 4242)
    ge = grads.clone()
    for seed in (1, 4242):  # second replay with the real seed
        grads.zero_()
        geng.forward_backward(x.to(DEV), y.to(DEV), 0.5, seed)
    torch.cuda.synchronize()
    assert torch.equal(grads, ge)


def test_eval_count(setup):
    """These inputs get one prediction for every row (the bias noise decides the argmax), so the
    count here does not depend on the per-row forward: tests/test_eval_audit_gpu.py checks it row
    by row on inputs whose predictions are known."""
    eng, flat, params, grads, x, y = setup
    xe = torch.rand(1200, 784)
    ye = torch.randint(0, 10, (1200,))
    pv = param_views(flat, CANON_OFFSETS)
    ref = int((torch_forward(pv, xe, 1.0, 0).argmax(1) == ye).sum())
    got = eng.correct(xe.to(DEV), ye.to(DEV))
    assert abs(got - ref) <= 1  # argmax ties at fp32 rounding
    lg = eng.logits(xe[:64].to(DEV))
    assert rel_err(lg, torch_forward(pv, xe[:64], 1.0, 0)) < 2e-5


@pytest.mark.parametrize("n,off", [(4096, 0), (1000, 3), (4098, 4), (2656010, 0)])
def test_adam_kernel(n, off):
    from ddl_amd.ops import native
    torch.manual_seed(1)
    w = torch.randn(n + off)
    g = torch.randn(n + off) * 1e-2
    m = torch.randn(n + off) * 1e-3
    v = torch.rand(n + off) * 1e-4
    lr_t, b1, b2, eps, scale = 3e-4, 0.9, 0.999, 1e-8, 0.5
    W, G, M, V = (t.to(DEV) for t in (w, g, m, v))
    native.ops().adam_flat(W[off:], G[off:], M[off:], V[off:], lr_t, b1, b2, eps, scale)
    gs = g[off:] * scale
    m2 = m[off:] + (gs - m[off:]) * (1 - b1)
    v2 = v[off:] + (gs * gs - v[off:]) * (1 - b2)
    w2 = w[off:] - lr_t * m2 / (v2.sqrt() + eps)
    assert rel_err(M[off:], m2) < 1e-6
    assert rel_err(V[off:], v2) < 1e-6
    assert (W[off:].cpu() - w2).abs().max() < 1e-6


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("mu", [0.9, 0.0])
@pytest.mark.parametrize("n,off", [(4096, 0), (1000, 3), (4098, 4), (2656010, 0)])
def test_momentum_kernel(n, off, mu, scale):
    """momentum_flat (momentum / plain-SGD optimizers, mu = 0: plain SGD) against the fp64 closed
    form of common.h momentum1, m' = mu m + scale g, w' = w - lr m' (what parallel/ps.py
    expects), at the sizes, misalignments and bounds of test_adam_kernel."""
    from ddl_amd.ops import native
    torch.manual_seed(2)
    w = torch.randn(n + off)
    g = torch.randn(n + off) * 1e-2
    m = torch.randn(n + off) * 1e-3
    lr = 3e-2
    W, G, M = (t.to(DEV) for t in (w, g, m))
    native.ops().momentum_flat(W[off:], G[off:], M[off:], lr, mu, scale)
    m2 = m[off:].double() * mu + g[off:].double() * scale
    w2 = w[off:].double() - lr * m2
    assert rel_err(M[off:], m2) < 1e-6
    assert (W[off:].cpu().double() - w2).abs().max() < 1e-6
    # the gradient is read only, and nothing in front of the shard is touched
    assert torch.equal(G.cpu(), g)
    assert torch.equal(W[:off].cpu(), w[:off]) and torch.equal(M[:off].cpu(), m[:off])


def test_training_tracks_torch_engine():
    """20 Adam steps: HIP engine vs stock-torch engine on the same GPU stay close and
    both reduce the loss."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    from ddl_amd.utils.data import synthetic_mnist
    data = synthetic_mnist(2000, 500)
    res = {}
    for engine in ("hip", "torch"):
        cfg = TrainConfig(mode="single", shard="none", steps=20, eval_every=0, engine=engine,
                          quiet=True)
        tr = Trainer(cfg, DistEnv(device=torch.device(DEV)), dataset=data)
        tr.train()
        res[engine] = tr.params.detach().cpu()
    # Adam moves every weight by ~lr per step whatever the gradient's size, so compare the
    # mean drift against the mean update, not the max (sign flips of ~0 gradients).
    from ddl_amd.models.mnist_cnn import init_params_ as _init
    p0 = torch.zeros_like(res["hip"])
    _init(p0, CANON_OFFSETS, 0)
    upd = (res["torch"] - p0).abs().mean()
    drift = (res["hip"] - res["torch"]).abs().mean()
    assert drift < 0.2 * upd, (float(drift), float(upd))
