"""Momentum / plain-SGD updates at one worker: the 16-byte vector kernel (optim.hip), the update
riding in the backward launches (tail.h: tail blocks, the weight-gradient reduce epilogues, the
stand-alone flush), and SyncRunner.update_launches(), which tells which of them a step took.
momentum1 (common.h) pins the roundings, so every placement must give the same bits."""
import pytest
import torch

from ddl_amd.utils.data import synthetic_mnist

from momentum_reference import momentum_closed_form
from onecard import PLACEMENTS, placement_run, rel_err
from onecard import assert_same_run as _assert_same

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8  # NaN elements on either side of a shard (a multiple of 4: keeps the shard 16-B aligned)


def _guarded(x, shift):
    """x on the GPU between NaN guards, `shift` elements past a 16-byte boundary."""
    buf = torch.full((GUARD + shift + x.numel() + GUARD,), float("nan"), device=DEV)
    lo = GUARD + shift
    buf[lo:lo + x.numel()] = x.to(DEV)
    return buf, buf[lo:lo + x.numel()]


def _guards_intact(buf, shift, n):
    lo = GUARD + shift
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())


# 1 .. 7: remainder only, body + remainder; 2,100,000: n / 4 exceeds 2048 blocks x 256 threads, so
# the vector kernel's grid-stride loop takes a second trip
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("mu", [0.9, 0.0])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 7, 1023, 1024, 2_100_000])
def test_momentum_vector_kernel(n, mu, scale):
    """momentum_flat on a 16-byte aligned shard (the vector kernel) against the fp64 closed form
    with test_hip_kernels.py::test_momentum_kernel's inputs and tolerances, and bit for bit
    against the same data one element off alignment (the scalar kernel); NaN guards around
    w, g and m stay untouched and g is read only."""
    from ddl_amd.ops import native
    torch.manual_seed(2)
    w = torch.randn(n)
    g = torch.randn(n) * 1e-2
    m = torch.randn(n) * 1e-3
    lr = 3e-2
    out = []
    for shift in (0, 1):
        (Wb, W), (Gb, G), (Mb, M) = (_guarded(t, shift) for t in (w, g, m))
        assert n == 0 or all(t.data_ptr() % 16 == 4 * shift for t in (W, G, M))
        native.ops().momentum_flat(W, G, M, lr, mu, scale)
        torch.cuda.synchronize()
        assert all(_guards_intact(b, shift, n) for b in (Wb, Gb, Mb))
        assert torch.equal(G.cpu(), g)
        out.append((W.cpu(), M.cpu()))
    (w_vec, m_vec), (w_sca, m_sca) = out
    assert torch.equal(w_vec, w_sca) and torch.equal(m_vec, m_sca)
    if n == 0:
        return
    w2, m2 = momentum_closed_form(w, m, [g], lr, mu, scale)
    err_m, err_w = rel_err(m_vec, m2), float((w_vec.double() - w2).abs().max())
    print(f"n {n} mu {mu} scale {scale}: rel_err(m) {err_m:.3e}  |w - ref| {err_w:.3e}")
    assert err_m < 1e-6
    assert err_w < 1e-6


@pytest.fixture(scope="module")
def data():
    return synthetic_mnist(n_train=2000, n_test=500, seed=5)


STEPS = 5


def _run(data, optimizer, shard, tail=None, final=None, setup=None, seed=0):
    """onecard.placement_run at STEPS steps of batch 100."""
    return placement_run(data, dict(optimizer=optimizer), shard, STEPS, 100, tail, final, setup,
                         seed)


@pytest.mark.parametrize("shard", ["flat", "contiguous"])
@pytest.mark.parametrize("optimizer", ["momentum", "sgd"])
def test_momentum_placements_bit_identical(data, optimizer, shard):
    """The update as tail blocks + conv1's / conv2's weight-gradient reduce epilogues, as tail
    blocks + a launch for the last segment, and as launches after the backward: the same
    parameters and m, no v anywhere."""
    runs = [_run(data, optimizer, shard, t, f) for t, f in PLACEMENTS]
    for r in runs[:2]:
        _assert_same(r, runs[2], has_v=False)
    if optimizer == "sgd":
        assert runs[0][1][0][0].abs().sum() > 0  # m holds the last scaled gradient


@pytest.mark.parametrize("setting", ["set_dual", "set_conv1_wgrad_direct"])
def test_momentum_tail_other_engine_paths(data, setting):
    """set_dual(False): no dual launch takes a tail, each leaves through Engine::flush_tail.
    set_conv1_wgrad_direct(False): the last segment's update goes through final_split and
    splitk_wide_reduce_tail instead of final_split_conv12.  Each against the launches after the
    backward under the same engine setting."""
    def setup(tr):
        getattr(tr.engine.eng, setting)(False)
    on = _run(data, "momentum", "flat", True, True, setup)
    off = _run(data, "momentum", "flat", False, False, setup)
    _assert_same(on, off, has_v=False)
    if setting == "set_dual":
        assert on[2] > 0  # flushed tails are stand-alone launches, and counted as such


def test_momentum_step_takes_the_tail_path(data):
    """With default settings a momentum step issues as many stand-alone optimizer launches as an
    Adam step (every update rides in a backward launch), strictly fewer than with the tails
    off."""
    adam = _run(data, "adam", "flat")[2]
    mom = _run(data, "momentum", "flat")[2]
    mom_off = _run(data, "momentum", "flat", tail=False)[2]
    print(f"update_launches: adam {adam}, momentum {mom}, momentum tails off {mom_off}")
    assert mom == adam
    assert mom < mom_off and adam < mom_off


def test_adam_default_path_unchanged(data):
    """The shared tail code still gives Adam the bits of its end-of-step launch."""
    on = _run(data, "adam", "flat", seed=3)
    off = _run(data, "adam", "flat", tail=False, seed=3)
    _assert_same(on, off, has_v=True)
