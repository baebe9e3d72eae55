"""The GPU momentum tests' yardstick pinned on the CPU: the fp64 closed form of
tests/momentum_reference.py against ParameterServer's pure-torch momentum and SGD branches
(parallel/ps.py apply(), no native ops) over 3 steps."""
import pytest
import torch

from ddl_amd.ops.adam import AdamHyper
from ddl_amd.parallel.ps import ParameterServer
from ddl_amd.parallel.sharding import make_plan

from momentum_reference import momentum_closed_form

STEPS = 3
EPS32 = float(torch.finfo(torch.float32).eps)  # 2^-23: the spacing of fp32 relative to 1


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("optimizer,mu", [("momentum", 0.9), ("sgd", 0.0)])
def test_closed_form_matches_parameter_server(optimizer, mu, scale):
    """Tolerance: one fp32 rounding per step.  The pure-torch branch stores w and m in fp32
    once per step, an error of at most EPS32 relative to the largest element; the roundings of
    its intermediates (mu * m, scale * g, lr * m) are half-spacings of quantities no larger
    than m, which reach w only through lr = 3e-2.  So after k steps
    |x - ref| <= k * EPS32 * max|ref| for x in (w, m)."""
    plan = make_plan("contiguous", 4)  # the smallest shard is conv1 + conv2, the largest fc1
    gen = torch.Generator().manual_seed(11)
    w0 = torch.randn(plan.total, generator=gen)
    grads = [torch.randn(plan.total, generator=gen) * 1e-2 for _ in range(STEPS)]
    lr = 3e-2
    w = w0.clone()
    servers = [ParameterServer(plan, p, "cpu", AdamHyper(lr=lr), optimizer, 0.9)
               for p in range(plan.num_ps)]
    assert all(s.v is None for s in servers)
    for g in grads:
        for s in servers:
            s.update_flat(w, g, scale)
    w_ref, m_ref = momentum_closed_form(w0, torch.zeros_like(w0), grads, lr, mu, scale)
    # every element of the plan buffer that some PS owns (the rest is alignment padding)
    owned = torch.zeros(plan.total, dtype=torch.bool)
    for s in servers:
        for lo, hi in s.segments:
            owned[lo:hi] = True
    assert owned.any() and torch.equal(w[~owned], w0[~owned])
    err_w = (w.double() - w_ref)[owned].abs().max().item()
    tol_w = STEPS * EPS32 * w_ref[owned].abs().max().item()
    print(f"{optimizer} scale {scale}: |w - ref| max {err_w:.3e} (tolerance {tol_w:.3e})")
    assert err_w <= tol_w
    if optimizer == "momentum":  # (the pure-torch SGD branch keeps no m)
        for s in servers:
            for (lo, hi), off in zip(s.segments, s.seg_off):
                ref = m_ref[lo:hi]
                err_m = (s.m[off:off + hi - lo].double() - ref).abs().max().item()
                assert err_m <= STEPS * EPS32 * ref.abs().max().item()
