"""The eval count, audited row by row on inputs whose predictions are known.

bench.py's headline is the time to a target accuracy, and that accuracy is the count of
``HipEngine.correct`` / ``correct_async`` (Engine::eval_count: the eval forward, then head_fwd's
``correct`` counter).  The inputs of tests/eval_reference.py give every row a prediction T[r] of its
own, all ten classes, with a top-two gap 4e4 times the fp32 rounding error of a logit
(tests/test_eval_reference_cpu.py), so every count below is known exactly and every comparison is
an equality of integers or of bits.  An eval returns a count only: each row's prediction is read
through label vectors (eval_reference.label_sets: y = T, y = T + 1, y = c, y = T on the rows whose
index has bit k set or clear, a random y).  The same reader applied to a host prediction vector
with one row altered names that row (test_eval_reference_cpu.py test_reader_names_one_altered_row).

Cells (engine batch, eval chunk) over the 168 rows: (8, 168) one chunk on a small engine as in
production; (8, 64) chunks of 64, 64, 40; (8, 17) nine chunks of 17 and one of 15; (168, 168);
(40, 200) a chunk larger than the set.  On (8, 64) also conv1 on the GEMM path, eval tiles 9-12
on conv2-4, DDL_EVAL_KMAP2=0, and fc1 / fc2 on tile configs 1 (128 rows) and 3.  Then the
counter's semantics, the tie rule, the engine's neighbouring state, eval between training steps
of a native sync Trainer, and the snapshot semantics of parallel/async_eval.py.

Measured on one MI355X (per-test durations of a whole-suite run): this file's 18 tests 0.8 s
together, the slowest test_count_row_by_row[8-168] at 0.39 s (0.38 s of it the first fixture:
the fp64 fit); tests/test_op_oracle_gpu.py 7.4 s, of which the 27 tests on the 136-row engine
take 3.3 s (slowest test_ops_exact_default_config_past_128_rows[128-True], 0.52 s) and the 75
tests the file had before 4.1 s; both files alone in one run, 120 tests: 11.8 s with start-up.
"""
import pytest
import torch

import eval_reference as E
from ddl_amd.models.layout import CANON_OFFSETS
from ddl_amd.models.mnist_cnn import param_views
from oracle_common import CODE_BUFS, CODE_SENTINEL, DEV, HALO_BUFS, bits

pytestmark = pytest.mark.gpu

CELLS = [(8, 168), (8, 64), (8, 17), (168, 168), (40, 200)]


@pytest.fixture(scope="module")
def case():
    return E.eval_case()


def flat_params(P):
    return torch.cat([p.reshape(-1) for p in P]).to(DEV)


def make_engine(P, b, c):
    from ddl_amd.models.hip_engine import HipEngine
    params = flat_params(P)
    return HipEngine(params, torch.zeros_like(params), CANON_OFFSETS, batch=b, graph=False,
                     eval_chunk=c)


def counter(eng, x):
    return lambda y: eng.correct(x, y.to(DEV))


@pytest.fixture(scope="module")
def eng64(case):
    """The (8, 64) cell's engine, shared by the variants that only switch a setting."""
    return make_engine(case.P, 8, 64)


# ---- the cells ---------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", CELLS)
def test_count_row_by_row(case, b, c):
    """Every label set of eval_reference.label_sets gives exactly its known count."""
    eng = make_engine(case.P, b, c)
    fails = E.read_failures(counter(eng, case.x.to(DEV)), E.label_sets(case.T), case.n)
    assert not fails, "\n".join(fails)


def t_and_bit_sets(case):
    return [("y=T", case.T, case.n)] + E.bit_sets(case.T)


def test_count_conv1_gemm_path(case, eng64):
    e = eng64.eng
    prev = e.conv1_direct()
    try:
        e.set_conv1_direct(False)
        fails = E.read_failures(counter(eng64, case.x.to(DEV)), t_and_bit_sets(case), case.n)
    finally:
        e.set_conv1_direct(prev)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("big", [9, 10, 11, 12])
def test_count_eval_only_conv_tiles(case, eng64, big):
    e = eng64.eng
    base = list(e.get_eval_cfg())
    cfg = list(base)
    cfg[1] = cfg[2] = cfg[3] = big
    try:
        e.set_eval_cfg(cfg)
        fails = E.read_failures(counter(eng64, case.x.to(DEV)), t_and_bit_sets(case), case.n)
    finally:
        e.set_eval_cfg(base)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fc", [1, 3])
def test_count_fc_eval_tiles(case, eng64, fc):
    """fc1 / fc2 eval on the 128-row tile (config 1: the 64-row chunks fill half of one tile,
    the 40-row chunk less) and on config 3."""
    e = eng64.eng
    base = list(e.get_eval_cfg())
    cfg = list(base)
    cfg[4] = cfg[5] = fc
    try:
        e.set_eval_cfg(cfg)
        fails = E.read_failures(counter(eng64, case.x.to(DEV)), t_and_bit_sets(case), case.n)
    finally:
        e.set_eval_cfg(base)
    assert not fails, "\n".join(fails)


def test_count_image_major_conv2(case, monkeypatch):
    monkeypatch.setenv("DDL_EVAL_KMAP2", "0")
    eng = make_engine(case.P, 8, 64)
    fails = E.read_failures(counter(eng, case.x.to(DEV)), t_and_bit_sets(case), case.n)
    assert not fails, "\n".join(fails)


# ---- the counter -------------------------------------------------------------------------------
def test_counter_semantics(case, eng64):
    x = case.x.to(DEV)
    name, y, want = E.label_sets(case.T)[-1]
    assert name == "y=random"
    yd = y.to(DEV)
    # correct() starts from zero every time
    assert eng64.correct(x, yd) == want
    assert eng64.correct(x, yd) == want
    # correct_async accumulates over its chunks: the sum of the chunks counted alone
    parts = [eng64.correct(x[i:i + 64], yd[i:i + 64]) for i in (0, 64, 128)]
    assert parts == [int((case.T[i:i + 64] == y[i:i + 64]).sum()) for i in (0, 64, 128)]
    assert all(p > 0 for p in parts)
    cnt = eng64.correct_async(x, yd)
    assert int(cnt.item()) == sum(parts) == want
    eng64.eng.zero_correct()
    torch.cuda.synchronize()
    assert int(eng64.eng.buffer("correct", 1).item()) == 0


def test_ties_take_the_first_maximum(case):
    """W3 = 0 and b3 = [0, 1, 0, 1, ...]: the logits are exactly the bias in every row and the
    maximum occurs five times.  The model's argmax (torch.argmax documents the same) takes the
    first maximum, class 1."""
    P = [p.clone() for p in case.P]
    P[12] = torch.zeros_like(P[12])
    P[13] = torch.tensor([0.0, 1.0] * 5)
    eng = make_engine(P, 8, 64)
    x = case.x.to(DEV)
    full = lambda c: torch.full((case.n,), c, dtype=torch.int64, device=DEV)  # noqa: E731
    got = [eng.correct(x, full(c)) for c in range(10)]
    assert got == [0, case.n] + [0] * 8, got


def test_eval_leaves_halos_and_codes(case):
    """After a count over 168 rows on a 168-row engine every halo is still zero and the code
    buffers are bit-unchanged (the eval forward passes code = nullptr)."""
    eng = make_engine(case.P, 168, 168)
    e = eng.eng
    n = case.n
    for name in CODE_BUFS:
        e.buffer(name, n).fill_(CODE_SENTINEL)
    snap = {name: e.buffer(name, n).clone() for name in CODE_BUFS}
    assert eng.correct(case.x.to(DEV), case.T.to(DEV)) == n
    for name in CODE_BUFS:
        assert torch.equal(e.buffer(name, n), snap[name]), name
    for name in HALO_BUFS:
        border = e.buffer(name + "+halo", n).clone()
        border[:, 2:-2, 2:-2, :] = 0
        assert int(torch.count_nonzero(border)) == 0, name
    # the maps the eval forward wrote are not all zero: the check above looked at live buffers
    assert int(torch.count_nonzero(e.buffer("p3", n))) > 0


# ---- on a Trainer ------------------------------------------------------------------------------
def _trainer(dataset, **kw):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    base = dict(mode="sync", shard="contiguous", batch_size=100, eval_every=0, engine="hip",
                quiet=True)
    base.update(kw)
    return Trainer(TrainConfig(**base), DistEnv(0, 1, 0, torch.device("cuda", 0)), dataset=dataset)


@pytest.fixture(scope="module")
def dataset(case):
    """400 synthetic training rows; the test set is the case's images labelled with T."""
    from ddl_amd.utils.data import Dataset, synthetic_mnist
    d = synthetic_mnist(n_train=400, n_test=10, seed=11)
    return Dataset(d.x_train, d.y_train, case.x, case.T, "eval-case")


def test_eval_between_steps_changes_no_bit(dataset):
    """4 steps of the native sync Trainer with evaluate() after steps 1 and 2 end on the
    parameters and optimizer state of 4 steps without it: the eval forward on the training
    engine leaves nothing behind (a deferred fc2 reduce, pending weight gradients, a tail) that
    the next step would pick up."""
    runs = []
    for with_eval in (False, True):
        tr = _trainer(dataset, steps=4)
        start = tr.params.clone()
        accs = []
        for i in range(4):
            tr.train_step(i)
            if with_eval and i < 2:
                accs.append(tr.evaluate())
        torch.cuda.synchronize()
        runs.append(tr)
        if with_eval:
            assert all(0.0 <= a <= 1.0 for a in accs) and len(accs) == 2
    ref, got = runs
    assert torch.equal(bits(got.params), bits(ref.params))
    assert sorted(got.servers) == sorted(ref.servers)
    for p in ref.servers:
        assert got.servers[p].t == ref.servers[p].t == 4
        assert torch.equal(bits(got.servers[p].m), bits(ref.servers[p].m))
        assert torch.equal(bits(got.servers[p].v), bits(ref.servers[p].v))
    # the steps moved the parameters
    assert not torch.equal(ref.params, start)


def test_async_eval_scores_the_submitted_snapshot(case, dataset, monkeypatch):
    """parallel/async_eval.py: eval i scores exactly the parameters at its submit.  Parameter
    sets A (fc3 fitted to T), B (fitted to T_B) and A again are written into the trainer's
    parameters on the training stream, each followed at once by submit(); no sleep and no
    synchronisation besides submit / drain.  The three accuracies are exactly 1,
    (T_B == T).sum() / 168 and 1, in order."""
    from ddl_amd.parallel.async_eval import AsyncEvaluator
    monkeypatch.setenv("DDL_EVAL_CHUNK", "64")
    tr = _trainer(dataset, steps=4)
    results = []
    aeval = AsyncEvaluator(tr, on_result=lambda meta, acc, secs: results.append((meta["i"], acc)))
    assert aeval.engine.eval_chunk == 64
    A = [p.to(DEV) for p in case.P]
    B = [p.to(DEV) for p in case.P_B]
    views = param_views(tr.params, tr.plan.tensor_offsets)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(aeval.train_stream):
            aeval.start()
            for i, src in enumerate((A, B, A)):
                for v, p in zip(views, src):
                    v.copy_(p)
                aeval.submit({"i": i})
            aeval.drain()
    finally:
        aeval.close()
    same = int((case.T_B == case.T).sum())
    assert 0 < same < case.n // 2 + 1
    assert results == [(0, 1.0), (1, same / case.n), (2, 1.0)]
