"""The update rule (csrc/kernels/update.h) through its three stand-alone shapes on one span: the
16-byte vector kernel, the scalar kernel and Engine::flush_tail's fall-back launch must give the
same bits for Adam and momentum; the copy rule writes w := g and leaves the state alone.

The buffers hold 1023 + 4 + 1 elements: the span of 1023 starts at element 4 (16-byte aligned:
255 float4 of vector body plus the n % 4 = 3 remainder lanes) or at element 5 (4 bytes past
alignment: the scalar kernel).  These are the smallest sizes that cross the float4 body, the
remainder and the misaligned path; everything outside the span must stay as it was.

(Adam's cases failed on m's last bit while adam1 left its roundings to the compiler: the scalar
kernel alone kept a separate product and sum.  common.h pins them now, as momentum1's, with
the gradient scale inside the pinned form.)"""
import pytest
import torch

from ddl_amd.models.hip_engine import HipEngine
from ddl_amd.models.layout import CANON_OFFSETS, TOTAL_NUMEL

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, ALIGNED, SHIFTED = 1023, 4, 5
ADAM, MOMENTUM, COPY = 0, 1, 2  # update.h UpdKind
B1, B2, EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def engine():
    params = torch.zeros(TOTAL_NUMEL, device=DEV)
    return HipEngine(params, torch.zeros_like(params), CANON_OFFSETS, batch=8, graph=False,
                     eval_chunk=8).eng


@pytest.fixture(scope="module")
def span():
    """w, g, m, v of the span (CPU), the same for every case."""
    torch.manual_seed(7)
    return (torch.randn(N), torch.randn(N) * 1e-2, torch.randn(N) * 1e-3, torch.rand(N) * 1e-4)


def _placed(x, lo):
    """x at [lo, lo + N) of a NaN-filled buffer of N + 4 + 1 elements on the GPU."""
    buf = torch.full((N + 4 + 1,), float("nan"), device=DEV)
    buf[lo:lo + N] = x.to(DEV)
    assert buf[lo:].data_ptr() % 16 == (4 * lo) % 16
    return buf


def _outside_intact(buf, lo):
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + N:]).all())


def _apply(launch, span, lo, kind, step, mu, scale):
    """One update of the span placed at `lo` by `launch`; (w, m, v) afterwards, on the CPU."""
    w, g, m, v = span
    W, G, M, V = (_placed(t, lo) for t in (w, g, m, v))
    view = lambda b: b[lo:lo + N]
    launch(kind, view(W), view(G), view(M), view(V) if kind == ADAM else None, step, B1, B2, EPS,
           mu, scale)
    torch.cuda.synchronize()
    assert all(_outside_intact(b, lo) for b in (W, G, M, V))
    assert torch.equal(view(G).cpu(), g)  # the gradient is read only
    if kind != ADAM:
        assert torch.equal(view(V).cpu(), v)  # no v stream under momentum
    return view(W).cpu(), view(M).cpu(), view(V).cpu()


# 1/3: not a power of two, so g * scale rounds, and a site that fused the product into g - m
# where another did not would show
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize("kind,step,mu", [(ADAM, 3e-4, 0.0), (MOMENTUM, 3e-2, 0.9),
                                          (MOMENTUM, 3e-2, 0.0)])
def test_vector_scalar_and_flushed_tail_same_bits(engine, span, kind, step, mu, scale):
    from ddl_amd.ops import native
    vec = _apply(native.ops().update_flat, span, ALIGNED, kind, step, mu, scale)
    sca = _apply(native.ops().update_flat, span, SHIFTED, kind, step, mu, scale)
    tail = _apply(engine.flush_update_tail, span, ALIGNED, kind, step, mu, scale)
    assert not torch.equal(vec[0], span[0]) and not torch.equal(vec[1], span[2])  # it updated
    for name, a, b, c in zip("wmv", vec, sca, tail):
        assert torch.equal(a, b), f"{name}: vector vs scalar kernel"
        assert torch.equal(a, c), f"{name}: vector kernel vs flushed tail"


@pytest.mark.parametrize("lo", [ALIGNED, SHIFTED])
def test_copy_rule_writes_w_only(span, lo):
    """w == g after the copy rule, on both kernel shapes; m and v are not touched (and need not
    exist)."""
    from ddl_amd.ops import native
    w, g, m, v = span
    W, G, M, V = (_placed(t, lo) for t in (w, g, m, v))
    view = lambda b: b[lo:lo + N]
    native.ops().update_flat(COPY, view(W), view(G), view(M), view(V), 0.0)
    native.ops().update_flat(COPY, view(W), view(G), None, None, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(view(W).cpu(), g)
    assert torch.equal(view(G).cpu(), g)
    assert torch.equal(view(M).cpu(), m) and torch.equal(view(V).cpu(), v)
    assert all(_outside_intact(b, lo) for b in (W, G, M, V))
