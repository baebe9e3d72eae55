"""The exchange-kernel tests' yardstick (tests/exchange_reference.py) pinned on the CPU:

* its synchronous round, chained over 3 steps at W = 3, against ParameterServer's pure-torch
  branches (parallel/ps.py apply(), no native ops) fed the same rank-order sum, for Adam,
  momentum and SGD;
* its asynchronous round against the same servers applying one worker's gradient at a time;
* the fixed test gradients can tell the kernels' summation order from the two orders a wrong
  kernel (or a compiler that fused the scale into the adds) would produce;
* its slice arithmetic gives the geometries docs/DESIGN.md tabulates."""
import pytest
import torch

from ddl_amd.ops.adam import AdamHyper, adam_coeffs
from ddl_amd.parallel.ps import ParameterServer
from ddl_amd.parallel.sharding import make_plan

import exchange_reference as xr
from exchange_reference import ADAM, MOMENTUM

STEPS, WORLD = 3, 3
EPS32 = float(torch.finfo(torch.float32).eps)  # 2^-23: the spacing of fp32 relative to 1
RULES = [("adam", ADAM, 0.0), ("momentum", MOMENTUM, 0.9), ("sgd", MOMENTUM, 0.0)]


def _servers(plan, optimizer, w0=None):
    lr = xr.LR[ADAM if optimizer == "adam" else MOMENTUM]
    return [ParameterServer(plan, p, "cpu", AdamHyper(lr=lr, beta1=xr.B1, beta2=xr.B2, eps=xr.EPS),
                            optimizer, 0.9, own_params=w0) for p in range(plan.num_ps)]


def _close(x, ref, steps, what):
    """One fp32 rounding per step, as test_momentum_reference_cpu.py argues it: the pure-torch
    branch stores w, m and v in fp32 once per step (at most EPS32 relative to the largest
    element); the roundings of its intermediates are half-spacings of quantities no larger than
    the stored ones and reach w only through a step size <= 3e-2.  Adam's quotient m / (sqrt(v) +
    eps) is O(1) here and enters w times lr_t <= 3.2e-4, far below w's own spacing."""
    err = (x.double() - ref).abs().max().item()
    tol = steps * EPS32 * ref.abs().max().item()
    print(f"{what}: max |x - ref| {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, what


@pytest.mark.parametrize("coef,scale", [(1.0, 1.0), (xr.COEF3, 1.0), (1.0, 0.5)])
@pytest.mark.parametrize("optimizer,kind,mu", RULES)
def test_sync_round_matches_parameter_server(optimizer, kind, mu, coef, scale):
    plan = make_plan("contiguous", 4)
    n = plan.total
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(11))
    servers = _servers(plan, optimizer)
    w = w0.clone()
    # every PS an owner bucket on "rank" p % WORLD, its state at offset 0 of its own buffers
    regions = [[[] for _ in range(WORLD)] for _ in servers]
    for s in servers:
        regions[s.id][s.id % WORLD] = [(lo, hi - lo, off) for (lo, hi), off in
                                       zip(s.segments, s.seg_off)]
    P = [w0.clone() for _ in range(WORLD)]
    M = [[torch.zeros(s.numel) if r == s.id % WORLD else None for r in range(WORLD)]
         for s in servers]
    V = [[torch.zeros(s.numel) if r == s.id % WORLD else None for r in range(WORLD)]
         for s in servers]
    for t in range(1, STEPS + 1):
        grads = xr.round_gradients(WORLD, t, n)
        gsum = xr.rank_order_sum(grads, coef)
        for s in servers:
            s.update_flat(w, gsum, scale)
            assert xr.step_size(kind, s.t) == (adam_coeffs(s.h, s.t) if kind == ADAM else s.h.lr)
            P, M[s.id], V[s.id] = xr.sync_round(P, M[s.id], V[s.id], grads, regions[s.id], False,
                                                kind, xr.step_size(kind, t), mu, scale, coef)
    owned = torch.zeros(n, dtype=torch.bool)
    for s in servers:
        for lo, hi in s.segments:
            owned[lo:hi] = True
    assert owned.any() and torch.equal(w[~owned], w0[~owned])
    for r in range(WORLD):  # every replica received every owner's result, and nothing else
        assert torch.equal(P[r], P[0]) and torch.equal(P[r][~owned], w0.double()[~owned])
    _close(w[owned], P[0][owned], STEPS, f"{optimizer} w")
    for s in servers:
        r = s.id % WORLD
        if optimizer != "sgd":  # (the pure-torch SGD branch keeps no m)
            _close(s.m, M[s.id][r], STEPS, f"{optimizer} m of PS {s.id}")
        if optimizer == "adam":
            _close(s.v, V[s.id][r], STEPS, f"{optimizer} v of PS {s.id}")


@pytest.mark.parametrize("optimizer,kind,mu", RULES)
def test_async_round_matches_parameter_server(optimizer, kind, mu):
    """Every PS applies worker 0..W-1 in order, one step of its own counter each; worker q ends
    the round with the copy as it stood after its own apply."""
    plan = make_plan("contiguous", 4)
    n = plan.total
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(12))
    servers = _servers(plan, optimizer, w0)
    shards = [(s.segments[0][0], s.numel, 0) for s in servers]
    assert all(len(s.segments) == 1 for s in servers)
    ps = [(s.params.clone(), torch.zeros(s.numel), torch.zeros(s.numel)) for s in servers]
    for t in range(STEPS):
        grads = xr.round_gradients(WORLD, t + 1, n)
        seen = [[None] * len(servers) for _ in range(WORLD)]
        for s in servers:
            lo, hi = s.segments[0]
            for q in range(WORLD):
                s.update_own(xr.scaled(grads[q][lo:hi], xr.COEF3), 0.5)
                seen[q][s.id] = s.params.clone()
        after, workers = xr.async_round(ps, grads, shards, kind, [t * WORLD] * len(servers), mu,
                                        0.5, xr.COEF3)
        ps = [after[p][-1] for p in range(len(servers))]
        k = (t + 1) * WORLD
        for s in servers:
            assert s.t == k
            for q in range(WORLD):
                _close(seen[q][s.id], workers[q][s.id], k, f"{optimizer} worker {q} PS {s.id}")
            _close(s.params, ps[s.id][0], k, f"{optimizer} PS {s.id} copy")
            if optimizer != "sgd":
                _close(s.m, ps[s.id][1], k, f"{optimizer} PS {s.id} m")
            if optimizer == "adam":
                _close(s.v, ps[s.id][2], k, f"{optimizer} PS {s.id} v")


@pytest.mark.parametrize("epoch", [1, 2, 3])
def test_gradients_tell_the_summation_orders_apart(epoch):
    """If the rank-order sum of the GPU tests' own gradients equalled the reversed-order sum, or
    the sum scaled once at the end, everywhere, those tests could not see a kernel that summed in
    another order or folded the scale into the adds.  Seed, magnitude (randn * 1e-2) and
    coef = 1/3 are fixed in exchange_reference.py, so this holds by construction."""
    grads = xr.round_gradients(WORLD, epoch)
    assert len(grads) == WORLD and grads[0].numel() == xr.N_BUF
    want = xr.rank_order_sum(grads, xr.COEF3)
    rev = xr.rank_order_sum(grads[::-1], xr.COEF3)
    late = xr.scaled(xr.rank_order_sum(grads, 1.0), xr.COEF3)
    plain_rev = xr.rank_order_sum(grads[::-1], 1.0)
    assert int((want != rev).sum()) >= 1
    assert int((want != late).sum()) >= 1
    assert int((xr.rank_order_sum(grads, 1.0) != plain_rev).sum()) >= 1
    # (a fused multiply-add keeps the product unrounded: the same sum in fp64 products)
    c = float(torch.tensor(xr.COEF3, dtype=torch.float32))
    fused = torch.zeros_like(want)
    for g in grads:
        fused = (fused.double() + g.double() * c).float()
    assert int((want != fused).sum()) >= 1
    # (and within the first 4096 floats, where the smallest cells' buckets lie)
    assert int((want[:4096] != rev[:4096]).sum()) >= 1
    assert int((want[:4096] != fused[:4096]).sum()) >= 1


def test_integer_gradients_sum_exactly():
    grads = xr.round_gradients(WORLD, 1, integer=True)
    want = xr.rank_order_sum(grads)
    assert torch.equal(want, xr.rank_order_sum(grads[::-1]))
    assert torch.equal(want.double(), sum(g.double() for g in grads))
    assert want.abs().max() > 0


def test_slice_arithmetic():
    """The geometries of the GPU cells (docs/DESIGN.md, "The exchange kernels alone")."""
    f4 = xr.equal_slices
    assert f4(4) == [1] and f4(1020) == [255] and f4(1024) == [256]
    assert f4(1028) == [129, 128]
    assert f4(3076) == [193, 193, 193, 190]
    assert f4(4100, 1) == [1025] and f4(4100, 2) == [513, 512]
    assert f4(7172) == [225] * 7 + [218]
    own = xr.owner_slices
    assert own([4]) == ([1], [0, 1])
    assert own([4] * 8) == ([1] * 8, list(range(9)))  # ns raised to the run count
    assert own([1028, 4, 2052])[1] == [0, 2, 3, 6]
    assert own([1028, 4, 2052])[0] == [193, 64, 1, 193, 193, 127]
    assert own([3000, 100, 1500, 8])[1] == [0, 4, 5, 7, 8]
    assert own([3000, 100, 1500, 8])[0] == [231, 231, 231, 57, 25, 231, 144, 2]
    assert own([2052, 1028], 2) == ([385, 128, 257], [0, 2, 3])
    assert own([5000, 40], 1) == ([630, 620, 10], [0, 2, 3])
    a = xr.async_slices
    assert a(4) == [1] and a(2044) == [511] and a(2052) == [257, 256]
    assert a(4100) == [342, 342, 341] and a(4100, 1) == [1025] and a(6148, 2) == [769, 768]
