"""Shuffled passes and shifted images on the GPU (csrc/kernels/batch.hip, --shuffle,
--augment-shift) against the CPU twin (ddl_amd/ops/shuffle.py), bit for bit.

a. the kernel alone, on the ramp set of tests/shuffle_reference.py and into a poisoned
   destination: N = 1, 17, 257 at B = 1, 5, 33, the copy path (S = 0) and the shifted one
   (S = 1, 3, with a draw in a corner of the range), shuffled and not, at the first and the last
   batch of the set; N = 4097, just above a power of four, where the cycle walk loops; the
   launcher's refusals;
b. the W = 1 native sync step on the HIP engine at B = 5: three --shuffle --augment-shift 2 steps
   equal three plain steps fed the twin's batches, and the update tails keep riding;
c. one cell on one card: sync xGMI at W = 2 under `stride`, three shuffled steps against the same
   job unshuffled on the set pre-permuted by the twin.

Data movement only: equality is demanded everywhere.
"""
import pytest
import torch

from ddl_amd.ops import native
from ddl_amd.ops import shuffle as S

import onecard as oc
from oracle_common import host_bits as bits
from shuffle_reference import (ROW, bases, corner_key, expected_batch, keeps_poison, poisoned,
                               pre_permuted, ramp_set)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


# ---- a. the kernel alone ---------------------------------------------------------------------------
_RAMPS = {}


def ramp_on_card(n):
    if n not in _RAMPS:
        x, y = ramp_set(n)
        _RAMPS[n] = (x.to(DEV), y.to(DEV))
    return _RAMPS[n]


def check_kernel(n, b, s, shuffle, base, key, ks):
    """One launch into a poisoned destination against the rule written out element by element
    (tests/test_shuffle_cpu.py holds the twin to the same rule)."""
    x, y = ramp_on_card(n)
    xb, yb = poisoned(b, DEV)
    native.ops().assemble_batch(x, y, xb, yb, b, base, key, ks, s, shuffle)
    torch.cuda.synchronize()
    wx, wy, draws = expected_batch(n, b, base, key, ks, s, shuffle)
    assert torch.equal(bits(xb[:b]), bits(wx)), (n, b, s, shuffle, base)
    assert torch.equal(yb[:b].cpu(), wy), (n, b, s, shuffle, base)
    assert keeps_poison(xb, yb, b), (n, b, s, shuffle, base)
    return draws


GRID = [(n, b) for n in (1, 17, 257) for b in (1, 5, 33) if b <= n]


@pytest.mark.parametrize("s", [0, 1, 3])
@pytest.mark.parametrize("n,b", GRID)
def test_kernel_is_the_twin(n, b, s):
    for shuffle in (False, True):
        for base in bases(n, b):
            ks = corner_key(base, b, s, start=n) if s else 99
            draws = check_kernel(n, b, s, shuffle, base, 0x1234 + n, ks)
            if s:
                assert any(abs(dx) == s and abs(dy) == s for dx, dy in draws)


@pytest.mark.parametrize("s", [0, 2])
def test_kernel_walks_the_cycle(s):
    """N = 4097: the network's domain is 16384, so three applications in four land outside the set
    and the walk goes on (some position of these batches needs at least eight)."""
    n, b, key = 4097, 5, 77

    def walks(i):
        h = S.half_bits(n)
        ks, x, w = S.round_keys(key), i, 0
        while True:
            left, right = x >> h, x & ((1 << h) - 1)
            for k in ks:
                left, right = right, left ^ (S.mix_scalar(right ^ k) & ((1 << h) - 1))
            x, w = (left << h) | right, w + 1
            if x < n:
                return w
    long_base = max(range(0, n - b + 1, b), key=lambda q: max(walks(q + j) for j in range(b)))
    assert max(walks(long_base + j) for j in range(b)) >= 8
    for base in (0, long_base, n - b):
        check_kernel(n, b, s, True, base, key, 5)


def test_kernel_matches_the_twin_on_images():
    """On real-valued images (the synthetic set), every shift up to the largest: the twin's bits."""
    from ddl_amd.utils.data import synthetic_mnist
    d = synthetic_mnist(100, 100, seed=3)
    x, y = d.x_train.to(DEV), d.y_train.to(DEV)
    for s in (0, 8):
        xb, yb = poisoned(33, DEV)
        wx, wy = poisoned(33)
        native.ops().assemble_batch(x, y, xb, yb, 33, 66, 11, 12, s, True)
        S.assemble_batch(d.x_train, d.y_train, wx, wy, 33, 66, 11, 12, s, True)
        torch.cuda.synchronize()
        assert torch.equal(bits(xb), bits(wx)) and torch.equal(yb.cpu(), wy)


def test_refusals():
    ops = native.ops()
    x, y = ramp_on_card(17)
    xb, yb = poisoned(5, DEV)
    ok = (x, y, xb, yb, 5, 0, 1, 2, 0, True)

    def bad(**kw):
        names = ("x_train", "y_train", "xb", "yb", "b", "base", "key", "key_shift", "s", "shuffle")
        args = dict(zip(names, ok))
        args.update(kw)
        with pytest.raises((RuntimeError, ValueError)):
            ops.assemble_batch(*[args[k] for k in names])
    bad(base=13)                      # the batch would end past the set
    bad(base=-1)
    bad(b=0)
    bad(b=8)                          # xb holds 7 rows
    bad(s=9)
    bad(s=-1)
    bad(key=1 << 32)
    bad(xb=x[:7])                     # the destination inside the training set
    bad(xb=xb.cpu())
    bad(xb=xb[:, :783])
    bad(yb=yb.to(torch.int32))
    bad(xb=torch.zeros(7 * ROW + 1, device=DEV)[1:].view(7, ROW))   # not 16-byte aligned
    ops.assemble_batch(*ok)
    torch.cuda.synchronize()
    assert keeps_poison(xb, yb, 5)


# ---- b. the W = 1 native step ----------------------------------------------------------------------
B, STEPS, SEED = 5, 3, 2


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(n_train=400, n_test=100, seed=5)


def make_trainer(data, k, **kw):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    cfg = TrainConfig(mode="sync", shard="flat", steps=STEPS, batch_size=B, eval_every=0,
                      engine="hip", quiet=True, lr=1e-2, seed=SEED, accum_steps=k, **kw)
    return Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=data)


def state_of(tr):
    return [t.clone() for _, s in sorted(tr.servers.items()) for t in (s.m, s.v) if t is not None]


@pytest.mark.parametrize("k", [1, 2])
def test_native_step_w1(data, k):
    """Three steps of K micro-batches: the shuffled, shifted trainer against a plain trainer whose
    native runner is handed the twin's batches, parameters and optimizer state bit for bit.  The
    assembly is no update launch: K = 1 keeps every update in the backward launches' tails
    (update_launches() 0), K = 2 makes the plain run's count."""
    from ddl_amd.ops import rng
    got = make_trainer(data, k, shuffle=True, augment_shift=2)
    assert got.exchange.native
    for i in range(STEPS):
        got.train_step(i)
    torch.cuda.synchronize()
    assert got.batch_x is not None and got.batch_x.shape == (B, ROW)

    want = make_trainer(data, k)
    cpu = data   # (the module's dataset lives on the host; the trainers hold device copies)
    for i in range(STEPS):
        for j in range(k):
            base, key, ks = S.batch_rule(SEED, 0, i * k + j, B, cpu.total_batch)
            wx, wy = torch.zeros(B, ROW), torch.zeros(B, dtype=torch.int64)
            S.assemble_batch(cpu.x_train, cpu.y_train, wx, wy, B, base, key, ks, 2, True)
            seed = rng.step_seed(SEED, 0, want.global_step * k + j)
            x, y = wx.to(DEV), wy.to(DEV)
            if j < k - 1:
                want.exchange.accumulate(x, y, want.cfg.keep_prob, seed)
            else:
                want.exchange.step(x, y, want.cfg.keep_prob, seed)
            torch.cuda.synchronize()   # (x and y die here: the step has read them)
        want.global_step += 1
    assert want.batch_x is None
    assert torch.equal(bits(got.params), bits(want.params))
    for a, b in zip(state_of(got), state_of(want)):
        assert torch.equal(bits(a), bits(b))
    launches = got.exchange.runner.update_launches()
    assert launches == want.exchange.runner.update_launches()
    if k == 1:
        assert launches == 0
    # ... and it is not the unshuffled run
    plain = make_trainer(data, k)
    for i in range(STEPS):
        plain.train_step(i)
    torch.cuda.synchronize()
    assert not torch.equal(bits(plain.params), bits(got.params))
    for tr in (got, want, plain):
        tr.exchange.close()


# ---- c. one cell on one card ---------------------------------------------------------------------------
XSTEPS = 3


def _sync_rank(rank, world, port, outdir):
    """One rank of two synchronous xGMI jobs of XSTEPS steps of B, one after the other: shuffled,
    then unshuffled on the set pre-permuted by the twin."""
    import os
    with oc.rank_session(rank, world, port) as me:
        from ddl_amd.utils.data import synthetic_mnist
        d = synthetic_mnist(400, 100, seed=5)
        tr = oc.xgmi_trainer(me.env, "sync", XSTEPS, B, d, shard="flat", seed=SEED, shuffle=True)
        rec = oc.sync_rank_record(tr, XSTEPS, per_step=oc.sync_each_step)
        torch.save(rec, os.path.join(outdir, f"shuffled{rank}.pt"))
        me.close_one_of_several(tr.exchange)
        tr = oc.xgmi_trainer(me.env, "sync", XSTEPS, B, pre_permuted(d, SEED), shard="flat",
                             seed=SEED)
        rec = oc.sync_rank_record(tr, XSTEPS, per_step=oc.sync_each_step)
        torch.save(rec, os.path.join(outdir, f"permuted{rank}.pt"))
        me.close_single(tr.exchange)


@pytest.mark.slow
def test_xgmi_sync_w2(tmp_path):
    """Sync W = 2 over xGMI on one card under `stride`, three steps of B = 5 (raw batches 0..5,
    one wrap): the replicas agree bit for bit on both ranks and equal the same job unshuffled on
    the pre-permuted set; every PS counted three steps."""
    from conftest import free_port
    oc.run_ranks(_sync_rank, 2, free_port(), str(tmp_path), limit_s=oc.LIMIT_S)
    got = oc.load_ranks(tmp_path, 2, name="shuffled{}.pt")
    want = oc.load_ranks(tmp_path, 2, name="permuted{}.pt")
    for rec in got + want:
        assert rec["steps"] == XSTEPS and all(t == XSTEPS for t in rec["t"].values())
    assert torch.equal(bits(got[0]["params"]), bits(got[1]["params"]))
    assert torch.equal(bits(want[0]["params"]), bits(want[1]["params"]))
    assert torch.equal(bits(got[0]["params"]), bits(want[0]["params"]))
