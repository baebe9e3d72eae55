"""The inputs of the row-by-row eval audit (tests/eval_reference.py), checked on the CPU.

Every condition comes from the fp64 and fp32 CPU references alone, never from the code under
test: all ten classes are predicted, every row's top-two gap is at least 1024 times the largest
fp32 rounding error of any logit of the case (a condition on the inputs, not a tolerance on the
kernels: the measured GPU / fp32-CPU error ratios of this project are all below 2.1), and no row
is left out of any comparison.  Then why the file exists (both older eval-count set-ups predict
one class for every row) and that the label-set reader names a row whose prediction is altered.
"""
import pytest
import torch

import eval_reference as E
from ddl_amd.models.layout import CANON_OFFSETS, TENSORS, TOTAL_NUMEL
from ddl_amd.models.mnist_cnn import init_params_, param_views, torch_forward


@pytest.fixture(scope="module")
def case():
    return E.eval_case()


@pytest.mark.parametrize("which", ["A", "B"])
def test_predictions_known_with_wide_margins(case, which):
    P, T, lg64 = (case.P, case.T, case.logits64) if which == "A" else \
                 (case.P_B, case.T_B, case.logits64_B)
    n = case.n
    assert n == E.N_ROWS and T.shape == (n,)
    assert torch.equal(lg64.argmax(1), T)
    per_class = torch.bincount(T, minlength=10)
    assert int(per_class.min()) >= 10, per_class.tolist()
    lg32 = E.logits32(P, case.x)
    assert lg32.dtype == torch.float32
    err = float((lg32.double() - lg64).abs().max())
    gap = E.top_two_gap(lg64)
    print(f"EVAL-CASE {which}: rows per class {per_class.tolist()}, smallest top-two gap "
          f"{float(gap.min()):.4f}, max |W3| {float(P[12].abs().max()):.2f}, largest |fp32 CPU - "
          f"fp64| logit {err:.3g}, gap / error {float(gap.min()) / err:.3g}")
    assert err > 0
    # every row, no exclusions
    assert bool((gap >= E.GAP_FACTOR * err).all()), (float(gap.min()), err)
    assert torch.equal(lg32.argmax(1), T)
    # the maximum is not duplicated in fp32 either
    top = lg32.max(dim=1, keepdim=True).values
    assert int((lg32 == top).sum()) == n


def test_second_targets_differ(case):
    assert int((case.T_B != case.T).sum()) >= case.n // 2
    # the two parameter sets differ in fc3 alone
    for i in range(12):
        assert torch.equal(case.P[i], case.P_B[i])
    assert not torch.equal(case.P[12], case.P_B[12])


def test_case_is_deterministic(case):
    E._CACHE.clear()
    again = E.eval_case()
    assert torch.equal(again.x, case.x) and torch.equal(again.T, case.T)
    assert torch.equal(again.P[12], case.P[12]) and torch.equal(again.P_B[13], case.P_B[13])


def test_old_setups_predict_one_class():
    """Regression note: the inputs of test_hip_kernels.py::test_eval_count (1200 rows) and of
    test_op_oracle_gpu.py::test_eval_count_last_chunk_small (85 rows) get one prediction for
    every row, so neither count depends on what the eval forward computes per row."""
    # test_hip_kernels.py `setup` followed by test_eval_count's draws
    torch.manual_seed(0)
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=3)
    pv = param_views(flat, CANON_OFFSETS)
    for t, v in zip(TENSORS, pv):
        if t.kind == "bias":
            v.add_(torch.randn_like(v) * 0.05)
    torch.rand(100, 784)
    torch.randint(0, 10, (100,))
    xe = torch.rand(1200, 784)
    assert len(torch.unique(torch_forward(pv, xe, 1.0, 0).argmax(1))) == 1
    # test_op_oracle_gpu.py `rctx` and its test's images
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=5)
    gen = torch.Generator().manual_seed(6)
    P = [p.clone() + (0.05 * torch.randn(p.shape, generator=gen) if p.dim() == 1 else 0)
         for p in param_views(flat, CANON_OFFSETS)]
    x = torch.rand(85, 784, generator=torch.Generator().manual_seed(9))
    assert len(torch.unique(torch_forward(P, x, 1.0, 0).argmax(1))) == 1


# ---- the reader -------------------------------------------------------------------------------
def test_label_sets_pass_on_the_targets(case):
    sets = E.label_sets(case.T)
    assert len(sets) == 2 + 10 + 2 * E.ROW_BITS + 1
    assert not E.read_failures(E.host_counter(case.T), sets, case.n)
    # the questions differ: no two label vectors are equal
    ys = [y for _, y, _ in sets]
    assert all(not torch.equal(a, b) for i, a in enumerate(ys) for b in ys[:i])
    name, y, want = sets[-1]
    assert 0 < want < case.n


@pytest.mark.parametrize("row", [0, 7, 63, 64, 127, 128, 167])
def test_reader_names_one_altered_row(case, row):
    """Sensitivity of the audit, without touching the package: a prediction vector with one row
    altered on the host fails the label sets, and the message names that row and no other."""
    pred = case.T.clone()
    pred[row] = (pred[row] + 3) % 10
    fails = E.read_failures(E.host_counter(pred), E.label_sets(case.T), case.n)
    assert fails
    assert fails[-1].endswith(f"single out rows [{row}]"), fails[-1]
    assert any(f.startswith("y=T:") for f in fails)


def test_reader_notices_broken_evals(case):
    """The broken eval paths the older tests would pass: a constant prediction, row r given the
    prediction of row r + 1, a counter that counts label == constant."""
    n, sets = case.n, E.label_sets(case.T)
    assert E.read_failures(E.host_counter(torch.full((n,), 3)), sets, n)
    assert E.read_failures(E.host_counter(case.T.roll(-1)), sets, n)
    assert E.read_failures(lambda y: int((y == 3).sum()), sets, n)
    # the last rows of a chunk left with the previous chunk's predictions (chunks of 64)
    stale = case.T.clone()
    stale[128:] = case.T[64:104]
    assert E.read_failures(E.host_counter(stale), sets, n)
