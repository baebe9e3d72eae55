"""Plain references of the engine's ops, one function per op (helper module, not a conftest).

Every function is written from the op's definition (``csrc/kernels/layers.h``, ``head.hip``,
``conv1.hip``) on the buffers that ``make_policy<OP>`` (``engine_impl.h``) binds: NHWC maps
without the halo, HWIO weights, fc weights ``[K_in, N_out]``.  They run in plain torch on the CPU,
in fp64 by default; ``dtype=torch.float32`` gives the fp32 CPU computation of the same op (torch
conv / matmul) that the precision checks use as their yardstick.  Nothing here copies the
kernels' index arithmetic (no im2col, no row enumerations, no K maps).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ddl_amd.ops import rng

F64 = torch.float64
NO_GRAD_CODE = 0xFF

# (H, CIN, COUT) of conv1..conv4 and the op numbering of csrc/kernels/api.h `enum Op`
CONV_GEO = [(28, 1, 32), (14, 32, 64), (7, 64, 128), (4, 128, 256)]
OP_NAMES = ["conv1_fwd", "conv2_fwd", "conv3_fwd", "conv4_fwd", "fc1_fwd", "fc2_fwd",
            "fc2_dgrad", "fc2_wgrad", "fc1_dgrad", "fc1_wgrad", "conv4_dgrad", "conv4_wgrad",
            "conv3_dgrad", "conv3_wgrad", "conv2_dgrad", "conv2_wgrad", "conv1_wgrad"]
OP_COUNT = len(OP_NAMES)


def k_terms(op: int, B: int) -> int:
    """Products summed into one output element of op `op` at batch B (bias included)."""
    name = OP_NAMES[op]
    layer = int(name[4]) - 1 if name.startswith("conv") else None
    if name.endswith("_fwd") and layer is not None:
        return 25 * CONV_GEO[layer][1] + 1
    if name in ("fc1_fwd", "fc2_fwd"):
        return 1024 + 1
    if name == "fc2_dgrad":
        return 512
    if name == "fc1_dgrad":
        return 1024
    if name in ("fc1_wgrad", "fc2_wgrad"):
        return B
    if name.endswith("_dgrad"):
        return 25 * CONV_GEO[layer][2]
    h = CONV_GEO[layer][0]          # conv weight gradients: every position of every image
    return B * h * h


# ---- pooling codes --------------------------------------------------------------------------
def _windows(pre: torch.Tensor, fill: float) -> torch.Tensor:
    """[B,H,H,C] -> [B,HP,HP,C,4]: the 2x2/2 SAME windows (pad bottom / right), q = dy*2+dx."""
    B, H, _, C = pre.shape
    HP = (H + 1) // 2
    if H % 2:
        pre = F.pad(pre, (0, 0, 0, 1, 0, 1), value=fill)
    return pre.reshape(B, HP, 2, HP, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, HP, HP, C, 4)


def pool_relu_code(pre: torch.Tensor):
    """max-pool 2x2/2 SAME + ReLU of the pre-activation map `pre` [B,H,H,C] and the 1-byte code:
    the lowest q = dy*2+dx among the window's maxima, or 0xFF when the max is <= 0."""
    win = _windows(pre, float("-inf"))
    best = win.max(dim=-1).values
    q = torch.arange(4).expand_as(win)
    arg = torch.where(win == best.unsqueeze(-1), q, torch.full_like(q, 4)).min(dim=-1).values
    code = torch.where(best > 0, arg, torch.full_like(arg, NO_GRAD_CODE)).to(torch.uint8)
    return best.clamp_min(0), code


def pool_scatter(g: torch.Tensor, code: torch.Tensor, hprev: int) -> torch.Tensor:
    """Pooled-output gradient g [B,HP,HP,C] through the codes into the pre-pool gradient map
    [B,hprev,hprev,C]: every window position is written, g where code == q, else 0."""
    B, HP, _, C = g.shape
    q = torch.arange(4).view(1, 1, 1, 1, 4)
    win = torch.where(code.long().unsqueeze(-1) == q, g.unsqueeze(-1), torch.zeros((), dtype=g.dtype))
    full = win.reshape(B, HP, HP, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * HP, 2 * HP, C)
    return full[:, :hprev, :hprev, :].contiguous()


def draw_codes(gen: torch.Generator, B: int, HP: int, C: int, H: int) -> torch.Tensor:
    """Random codes a forward can emit on an H x H map: a window position inside the map, or
    0xFF (about one in five)."""
    r = torch.rand(B, HP, HP, C, 4, generator=gen)
    py = torch.arange(HP).view(1, HP, 1, 1, 1)
    px = torch.arange(HP).view(1, 1, HP, 1, 1)
    q = torch.arange(4).view(1, 1, 1, 1, 4)
    ok = (2 * py + q // 2 < H) & (2 * px + q % 2 < H)
    code = torch.where(ok, r, torch.full_like(r, -1.0)).argmax(dim=-1)
    dead = torch.rand(B, HP, HP, C, generator=gen) < 0.2
    return torch.where(dead, torch.full_like(code, NO_GRAD_CODE), code).to(torch.uint8)


# ---- convolutions -----------------------------------------------------------------------------
def conv_pre(x, w, b, dtype=F64):
    """5x5 SAME conv + bias: x [B,H,H,CIN], w [5,5,CIN,COUT], b [COUT] -> [B,H,H,COUT]."""
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(3, 2, 0, 1), b.to(dtype),
                 padding=2)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_fwd(x, w, b, dtype=F64):
    """conv forward op: pooled map [B,HP,HP,COUT] and codes."""
    return pool_relu_code(conv_pre(x, w, b, dtype))


def conv_dx(dpre, w, dtype=F64):
    """dX[b,y,x,ci] = sum dpre[b,y-ky+2,x-kx+2,co] W[ky,kx,ci,co]: [B,H,H,COUT] -> [B,H,H,CIN]."""
    y = F.conv_transpose2d(dpre.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(3, 2, 0, 1),
                           padding=2)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_dgrad(dpre, w, code_prev, hprev, dtype=F64):
    """conv data-gradient op: dX scattered through the previous layer's codes."""
    return pool_scatter(conv_dx(dpre, w, dtype), code_prev, hprev)


def conv_wgrad(x, dpre, dtype=F64):
    """dW[ky,kx,ci,co] = sum_{b,y,x} x[b,y+ky-2,x+kx-2,ci] dpre[b,y,x,co] and db = sum dpre."""
    x, dpre = x.to(dtype), dpre.to(dtype)
    B, H, _, CIN = x.shape
    xp = F.pad(x, (0, 0, 2, 2, 2, 2))
    d2 = dpre.reshape(B * H * H, -1)
    dw = torch.stack([torch.stack([xp[:, ky:ky + H, kx:kx + H, :].reshape(B * H * H, CIN).t() @ d2
                                   for kx in range(5)]) for ky in range(5)])
    return dw, d2.sum(0)


# ---- fully connected ---------------------------------------------------------------------------
def keep_mask(seed: int, layer: int, B: int, N: int, keep: float) -> torch.Tensor:
    return rng.keep_mask(seed, layer, B * N, keep).view(B, N)


def fc_fwd(x, w, b, relu: bool, mask, inv_keep: float, dtype=F64):
    """x W + b, ReLU (fc1 only), dropout (mask [B,N] bool or None) as dropout_apply does."""
    y = x.to(dtype) @ w.to(dtype) + b.to(dtype)
    if relu:
        y = y.clamp_min(0)
    if mask is not None:
        y = torch.where(mask, y * inv_keep, torch.zeros((), dtype=dtype))
    return y


def fc_dx(dy, w, dtype=F64):
    return dy.to(dtype) @ w.to(dtype).t()


def fc_dgrad_act(dy, w, hpost, inv_keep: float, dtype=F64):
    """fc2's data gradient through fc1's dropout + ReLU: masked by h1 > 0, times 1/keep."""
    return torch.where(hpost > 0, fc_dx(dy, w, dtype) * inv_keep, torch.zeros((), dtype=dtype))


def fc_dgrad_pool(dy, w, c4, dtype=F64):
    """fc1's data gradient scattered through c4 [B,2,2,256] into d4 [B,4,4,256]."""
    B = dy.shape[0]
    return pool_scatter(fc_dx(dy, w, dtype).reshape(B, 2, 2, 256), c4.reshape(B, 2, 2, 256), 4)


def fc_wgrad(x, dy, dtype=F64):
    return x.to(dtype).t() @ dy.to(dtype), dy.to(dtype).sum(0)


# ---- classifier head ---------------------------------------------------------------------------
def head(h2, w3, b3, labels, mask2, inv_keep: float, dtype=F64):
    """Per-row loss, dlog = (softmax - onehot) / B, dpre2fc (fc2's dropout backward), fc3 dW/db."""
    h2, w3, b3 = h2.to(dtype), w3.to(dtype), b3.to(dtype)
    B = h2.shape[0]
    logits = h2 @ w3 + b3
    loss = torch.logsumexp(logits, 1) - logits.gather(1, labels.view(-1, 1)).squeeze(1)
    dlog = (torch.softmax(logits, 1) - F.one_hot(labels, 10).to(dtype)) / B
    dh2 = dlog @ w3.t()
    if mask2 is not None:
        dh2 = torch.where(mask2, dh2 * inv_keep, torch.zeros((), dtype=dtype))
    return {"loss": loss, "dlog": dlog, "dpre2fc": dh2, "gw": h2.t() @ dlog, "gb": dlog.sum(0)}


# ---- one op on named buffers ----------------------------------------------------------------
# buffers an op reads / writes (Engine.buffer names; "x" is the image argument, "gN" gradient
# tensor N); its parameters come from the list P
OP_IO = {
    0: (("x",), ("p1", "c1")), 1: (("p1",), ("p2", "c2")), 2: (("p2",), ("p3", "c3")),
    3: (("p3",), ("p4", "c4")), 4: (("p4",), ("h1",)), 5: (("h1",), ("h2",)),
    6: (("dpre2fc", "h1"), ("dpre1fc",)), 7: (("h1", "dpre2fc"), ("g10", "g11")),
    8: (("dpre1fc", "c4"), ("d4",)), 9: (("p4", "dpre1fc"), ("g8", "g9")),
    10: (("d4", "c3"), ("d3",)), 11: (("p3", "d4"), ("g6", "g7")),
    12: (("d3", "c2"), ("d2",)), 13: (("p2", "d3"), ("g4", "g5")),
    14: (("d2", "c1"), ("d1",)), 15: (("p1", "d2"), ("g2", "g3")),
    16: (("x", "d1"), ("g0", "g1")),
}
BUF_SHAPE = {
    "x": (28, 28, 1), "p1": (14, 14, 32), "p2": (7, 7, 64), "p3": (4, 4, 128), "p4": (1024,),
    "h1": (1024,), "h2": (512,), "dpre2fc": (512,), "dpre1fc": (1024,), "dlog": (10,),
    "d4": (4, 4, 256), "d3": (7, 7, 128), "d2": (14, 14, 64), "d1": (28, 28, 32),
    "c1": (14, 14, 32), "c2": (7, 7, 64), "c3": (4, 4, 128), "c4": (1024,),
}
# pre-pool map size of the layer whose forward emits the codes
CODE_H = {"c1": 28, "c2": 14, "c3": 7, "c4": 4}


def run_op(op: int, P, buf, seed: int, keep: float, train: bool = True, dtype=F64):
    """Op `op` on CPU buffers `buf` (name -> tensor, maps without halo) and parameters P (the 14
    shaped tensors): dict of the op's outputs.  train=False: no dropout, no codes."""
    B = next(iter(buf.values())).shape[0]
    inv_keep = 1.0 / keep if train else 1.0
    drop = train and keep < 1.0
    if op < 4:
        H, CIN, COUT = CONV_GEO[op]
        src = buf["x"].reshape(B, 28, 28, 1) if op == 0 else buf[f"p{op}"]
        out, code = conv_fwd(src, P[2 * op], P[2 * op + 1], dtype)
        if op == 3:
            out, code = out.reshape(B, 1024), code.reshape(B, 1024)
        res = {f"p{op + 1}": out}
        if train:
            res[f"c{op + 1}"] = code
        return res
    if op == 4:
        m = keep_mask(seed, 1, B, 1024, keep) if drop else None
        return {"h1": fc_fwd(buf["p4"], P[8], P[9], True, m, inv_keep, dtype)}
    if op == 5:
        m = keep_mask(seed, 2, B, 512, keep) if drop else None
        return {"h2": fc_fwd(buf["h1"], P[10], P[11], False, m, inv_keep, dtype)}
    if op == 6:
        return {"dpre1fc": fc_dgrad_act(buf["dpre2fc"], P[10], buf["h1"], inv_keep, dtype)}
    if op == 7:
        gw, gb = fc_wgrad(buf["h1"], buf["dpre2fc"], dtype)
        return {"g10": gw, "g11": gb}
    if op == 8:
        return {"d4": fc_dgrad_pool(buf["dpre1fc"], P[8], buf["c4"], dtype)}
    if op == 9:
        gw, gb = fc_wgrad(buf["p4"], buf["dpre1fc"], dtype)
        return {"g8": gw, "g9": gb}
    layer = {10: 3, 11: 3, 12: 2, 13: 2, 14: 1, 15: 1, 16: 0}[op]
    H = CONV_GEO[layer][0]
    if op in (10, 12, 14):  # data gradients of conv4 / conv3 / conv2
        hprev = CONV_GEO[layer - 1][0]
        return {f"d{layer}": conv_dgrad(buf[f"d{layer + 1}"], P[2 * layer], buf[f"c{layer}"],
                                        hprev, dtype)}
    src = buf["x"].reshape(B, 28, 28, 1) if layer == 0 else buf[f"p{layer}"]
    gw, gb = conv_wgrad(src, buf[f"d{layer + 1}"], dtype)
    return {f"g{2 * layer}": gw, f"g{2 * layer + 1}": gb}


def abs_sum(op: int, P, buf, keep: float):
    """sum_i |a_i| |b_i| of every output element of op `op`: the same reference on |inputs|
    (codes and masks pass through).  For a conv forward the window's largest abs-sum stands for
    the pooled element (max-pool and ReLU are 1-Lipschitz in the max norm, so the error of the
    pooled value is at most the largest error in its window)."""
    Pa = [p.abs() for p in P]
    ba = {k: (v if v.dtype == torch.uint8 else v.abs()) for k, v in buf.items()}
    if op < 4:
        B = next(iter(buf.values())).shape[0]
        src = ba["x"].reshape(B, 28, 28, 1) if op == 0 else ba[f"p{op}"]
        s = _windows(conv_pre(src, Pa[2 * op], Pa[2 * op + 1]), 0.0).max(dim=-1).values
        return {f"p{op + 1}": s.reshape(B, 1024) if op == 3 else s}
    if op in (4, 5):
        # dropout / ReLU only scale or zero an element: the abs-sum of the kept value
        name = "h1" if op == 4 else "h2"
        src, w, b = (ba["p4"], Pa[8], Pa[9]) if op == 4 else (ba["h1"], Pa[10], Pa[11])
        return {name: (src.double() @ w.double() + b.double()) / keep}
    if op == 6:
        # the mask comes from the sign of the real h1, not of |h1|
        return {"dpre1fc": torch.where(buf["h1"] > 0, fc_dx(ba["dpre2fc"], Pa[10]) / keep,
                                       torch.zeros((), dtype=F64))}
    return run_op(op, Pa, ba, 0, keep, True)


# ---- the real-valued metric ---------------------------------------------------------------------
U32 = 2.0 ** -24   # fp32 unit roundoff
# RMS margin over the fp32 CPU computation.  Both sum in O(sqrt(K) u), in different orders.  4
# would be too loose: at K = 6400 (conv4's data gradient) one extra typical term in the element
# with the largest abs-sum raises the tensor's RMS error to 2.4x the fp32 CPU's own
# (tests/test_op_reference_cpu.py test_metric_notices_one_term), so the margin has to stay below
# that for the check to notice a single term.
MARGIN = 2.0


def rel_err(got, ref64, asum):
    """Per element |got - ref| / sum|a_i||b_i| (0 where the abs-sum is 0: the element is an exact
    zero and must be one)."""
    d = (got.double() - ref64).abs()
    e = torch.where(asum > 0, d / asum.clamp_min(1e-300), torch.zeros((), dtype=F64))
    return e, bool(((asum == 0) & (d != 0)).any())


def rms(e, asum=None):
    """RMS of the per-element errors; with `asum`, over the elements that sum at least one
    non-zero term (an element whose terms are all zero is an exact zero: it carries no rounding
    error and is checked for exactness instead)."""
    if asum is not None:
        e = e[asum > 0]
    return float(e.pow(2).mean().sqrt()) if e.numel() else 0.0


def precision_failures(got, ref64, asum, K: int, base_rms: float, margin: float = MARGIN):
    """The two conditions of the real-valued check: every element within the fp32 dot-product
    ceiling (K + 8) u of its abs-sum, and the tensor's RMS error within `margin` times the RMS
    error `base_rms` of the fp32 CPU computation of the same op.  Returns the list of failures
    (empty: pass) and the measured (max err, rms err)."""
    e, nonzero = rel_err(got, ref64, asum)
    fails = []
    if not bool(torch.isfinite(got).all()):
        fails.append("non-finite output")
    if nonzero:
        fails.append("non-zero where every term is zero")
    emax, erms = float(e.max()), rms(e, asum)
    if emax > (K + 8) * U32:
        fails.append(f"max err {emax:.3g} > (K+8)u = {(K + 8) * U32:.3g}")
    if erms > margin * base_rms:
        fails.append(f"rms err {erms:.3g} > {margin} x fp32 CPU rms {base_rms:.3g}")
    return fails, (emax, erms)


# ---- test data ------------------------------------------------------------------------------------
INT_AMAX = 3   # integer operands lie in [-INT_AMAX, INT_AMAX]
# the weight tensor an op multiplies its input with (ops with two activation operands: none)
OP_WEIGHT = {0: 0, 1: 2, 2: 4, 3: 6, 4: 8, 5: 10, 6: 10, 8: 8, 10: 6, 12: 4, 14: 2}
PARAM_SHAPES = [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (5, 5, 64, 128), (128,),
                (5, 5, 128, 256), (256,), (1024, 1024), (1024,), (1024, 512), (512,),
                (512, 10), (10,)]


def _ints(gen, shape, sparse: bool):
    """Asymmetric integers in [-2, 3]; sparse: about half of them zero."""
    v = torch.randint(-2, INT_AMAX + 1, shape, generator=gen)
    if sparse:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v.to(torch.float32)


def _reals(gen, shape):
    """Asymmetric reals in [-0.5, 1)."""
    return (torch.rand(shape, generator=gen) * 1.5 - 0.5).to(torch.float32)


def make_params(seed: int, real: bool = False):
    """The 14 parameter tensors: integers in [-2, 3] with non-zero biases, or asymmetric reals."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for s in PARAM_SHAPES:
        if real:
            out.append(_reals(gen, s) * 0.25)
            continue
        v = _ints(gen, s, sparse=False)
        if len(s) == 1:
            v = torch.where(v == 0, torch.full_like(v, 3.0), v)
        out.append(v)
    return out


def make_inputs(op: int, B: int, seed: int, real: bool = False):
    """Input buffers of op `op` for rows < B (fp32 values, uint8 codes), by buffer name."""
    gen = torch.Generator().manual_seed(seed * 1000 + op * 64 + B)
    buf = {}
    for name in OP_IO[op][0]:
        shape = (B,) + BUF_SHAPE[name]
        if name.startswith("c"):
            hp = BUF_SHAPE[name][0] if len(BUF_SHAPE[name]) == 3 else 2
            c = 256 if name == "c4" else BUF_SHAPE[name][2]
            buf[name] = draw_codes(gen, B, hp, c, CODE_H[name]).reshape(shape)
        elif name == "x":
            v = _reals(gen, (B, 784)) if real else _ints(gen, (B, 784), True)
            buf[name] = v
        else:
            buf[name] = _reals(gen, shape) if real else _ints(gen, shape, True)
    return buf
