"""tests/onecard.py without a GPU: the launcher's deadline, grace and clean-up on trivial ranks,
the rendezvous preamble, and canon against the expression it replaced."""
import os
import sys
import time

import pytest

import onecard as oc

ENV_KEYS = ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK", "DDL_DIST_BACKEND",
            "DDL_XGMI_TIMEOUT_S")
START_S = 10.0   # allowance for starting two interpreters on a busy machine


def _ok(rank, world):
    pass


def _exit3_or_sleep(rank, world):
    """Rank 0 fails at once; rank 1 would sleep for a minute."""
    if rank == 0:
        sys.exit(3)
    time.sleep(60)


def _sleep(rank, world):
    time.sleep(60)


def _rank0_sets_env(rank, world, outdir, fail):
    """Rank 0 changes os.environ and may raise; the other rank sleeps when rank 0 is to raise."""
    if rank == 0:
        oc.enter(rank, world, 12345, env=dict(ONECARD_TEST_VAR="1"), xgmi_timeout_s="0")
        with open(os.path.join(outdir, "rank0_pid"), "w") as f:
            f.write(str(os.getpid()))
        if fail:
            raise RuntimeError("rank 0 fails")
    elif fail:
        time.sleep(60)


@pytest.fixture
def env_restored():
    saved = dict(os.environ)
    yield
    os.environ.clear()
    os.environ.update(saved)


@pytest.fixture
def grace(env_restored):
    """No xGMI timeout in force: the grace is onecard.GRACE_EXTRA_S alone."""
    os.environ["DDL_XGMI_TIMEOUT_S"] = "0"
    return oc.GRACE_EXTRA_S


@pytest.fixture
def made(monkeypatch):
    """Every Process run_ranks creates."""
    import multiprocessing
    out = []
    ctx = multiprocessing.get_context("spawn")

    class Recording:
        def Process(self, *a, **kw):
            out.append(ctx.Process(*a, **kw))
            return out[-1]

    def get_context(kind):
        assert kind == "spawn"   # fresh processes, never a fork of one that holds a GPU context
        return Recording()

    monkeypatch.setattr(multiprocessing, "get_context", get_context)
    return out


def test_two_ranks_that_exit_0(made):
    oc.run_ranks(_ok, 2, limit_s=60)
    assert [k.exitcode for k in made] == [0, 0]


def test_a_failed_rank_ends_the_job(made, grace):
    t = time.monotonic()
    with pytest.raises(AssertionError) as e:
        oc.run_ranks(_exit3_or_sleep, 2, limit_s=60)
    took = time.monotonic() - t
    assert "0: 3" in str(e.value) and "1: -9" in str(e.value), str(e.value)  # both exit codes
    assert took < grace + START_S, took   # far from the sibling's 60 s
    assert len(made) == 2 and not any(k.is_alive() for k in made)


def test_the_deadline_kills_what_is_left(made, grace):
    t = time.monotonic()
    with pytest.raises(AssertionError, match="2 rank.s. killed"):
        oc.run_ranks(_sleep, 2, limit_s=2)
    took = time.monotonic() - t
    assert 2.0 <= took < 2.0 + grace, took
    assert len(made) == 2 and not any(k.is_alive() for k in made)
    assert [k.exitcode for k in made] == [-9, -9]


@pytest.mark.parametrize("fail", [False, True])
def test_rank0_here_restores_the_environment(tmp_path, made, grace, fail):
    before = dict(os.environ)
    t = time.monotonic()
    if fail:
        with pytest.raises(RuntimeError, match="rank 0 fails"):
            oc.run_ranks(_rank0_sets_env, 2, str(tmp_path), True, limit_s=60, rank0_here=True)
        assert time.monotonic() - t < grace + START_S   # the sleeping rank 1: reaped in the grace
    else:
        oc.run_ranks(_rank0_sets_env, 2, str(tmp_path), False, limit_s=60, rank0_here=True)
    assert dict(os.environ) == before and "ONECARD_TEST_VAR" not in os.environ
    assert int(open(tmp_path / "rank0_pid").read()) == os.getpid()   # rank 0 ran here
    assert len(made) == 1 and not made[0].is_alive()                 # ... and only rank 1 apart
    assert made[0].exitcode == (-9 if fail else 0)


def test_enter_sets_the_seven_variables(env_restored):
    for k in ENV_KEYS + ("DDL_XGMI_CHECK",):
        os.environ.pop(k, None)
    oc.enter(1, 3, 23456)
    assert {k: os.environ[k] for k in ENV_KEYS} == dict(
        MASTER_ADDR="127.0.0.1", MASTER_PORT="23456", RANK="1", WORLD_SIZE="3", LOCAL_RANK="1",
        DDL_DIST_BACKEND="gloo", DDL_XGMI_TIMEOUT_S="20")
    assert oc.ROOT in sys.path
    oc.enter(0, 2, 23457, xgmi_timeout_s="10")
    assert os.environ["DDL_XGMI_TIMEOUT_S"] == "10" and os.environ["RANK"] == "0"
    oc.enter(0, 8, 23458, env=dict(DDL_XGMI_TIMEOUT_S="60", DDL_XGMI_CHECK="1"))
    assert os.environ["DDL_XGMI_TIMEOUT_S"] == "60" and os.environ["DDL_XGMI_CHECK"] == "1"
    assert os.environ["WORLD_SIZE"] == "8"


def test_canon_is_the_layouts_tensors_in_order():
    import torch
    from ddl_amd.models.layout import TENSORS
    from ddl_amd.parallel.sharding import make_plan
    for plan in (make_plan("none", 1), make_plan("contiguous", 3)):
        offsets = plan.tensor_offsets
        params = torch.arange(plan.total, dtype=torch.float32)
        want = torch.cat([params[offsets[t.index]:offsets[t.index] + t.numel] for t in TENSORS])
        got = oc.canon(params, offsets)
        assert torch.equal(got, want) and got.numel() == sum(t.numel for t in TENSORS)
