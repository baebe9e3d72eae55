"""The host-driven step body on the device: accumulation and clip through the native ops, composed
by ``Trainer.train_step``, against a hand loop written here from the building blocks.

Three cells at W = 1, B = 5, K = 2, clip on, 3 steps, each an exchange whose step the host drives:
the Python sync exchange on the HIP engine, the xGMI async plane without its native runner
(``DDL_ASYNC_NATIVE=0``: ``push_pull``), and the RCCL-session async plane.  The hand loop is
``begin_step`` (sync only) / ``engine.forward_backward`` / ``ops.accum_grads`` / ``ops.clip_grads``
/ ``finish_step`` or ``push_pull``.  Same kernels in the same order from the same state, so the
parameters and every hosted PS's ``m``, ``v`` and ``t`` are equal bit for bit; the recorded
coefficient is below 1 in at least one step, so the clip is known to bite.

The clip norm and the data are those of tests/test_clip_gpu.py (0.75; synthetic_mnist(400, 100,
seed=5)).  The CPU twin of the same body is pinned by tests/test_accum_cpu.py and
tests/test_clip_cpu.py.
"""
import pytest
import torch

from ddl_amd.ops import accum as A
from ddl_amd.ops import native, rng

from oracle_common import host_bits as bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B, K, STEPS, CLIP = 5, 2, 3, 0.75

CELLS = {
    "sync-python": (dict(mode="sync", shard="flat", native_exchange=False), {}),
    "async-xgmi-push-pull": (dict(mode="async", shard="contiguous", exchange_backend="xgmi"),
                             dict(DDL_ASYNC_NATIVE="0")),
    "async-rccl": (dict(mode="async", shard="contiguous", exchange_backend="rccl"), {}),
}


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(n_train=400, n_test=100, seed=5)


def hand_step(tr, step):
    """One step of the reference loop: K micro-batches, the accumulate pass after each, the clip
    after the last, then the exchange's own step end."""
    cfg, ex, ops = tr.cfg, tr.exchange, native.ops()
    if cfg.mode == "sync":
        ex.begin_step()
    for j in range(K):
        x, y = tr.batch(step * K + j)
        seed = rng.step_seed(cfg.seed, tr.env.rank, tr.global_step * K + j)
        tr.engine.forward_backward(x, y, cfg.keep_prob, seed)
        ops.accum_grads(tr.grads, tr.accum_buf, tr.clip_ranges, A.mode_of(j, K), K)
    ops.clip_grads(tr.grads, tr.clip_ranges, cfg.clip_norm, tr.clip_out)
    if cfg.mode == "sync":
        ex.finish_step()
    else:
        ex.push_pull()
    tr.global_step += 1


def run(data, kw, one_step):
    """A fresh trainer, STEPS steps through `one_step`, its state afterwards."""
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    cfg = TrainConfig(steps=STEPS, batch_size=B, eval_every=0, engine="hip", quiet=True, seed=0,
                      accum_steps=K, clip_norm=CLIP, **kw)
    tr = Trainer(cfg, DistEnv(0, 1, 0, DEV), dataset=data)
    ex = tr.exchange
    asyncm = cfg.mode == "async"
    if asyncm:
        ex.steps = STEPS
        ex.start()
    coefs = []
    try:
        for i in range(STEPS):
            one_step(tr, i)
            torch.cuda.synchronize()
            coefs.append(float(tr.clip_out[1]))
    finally:
        if asyncm:
            ex.join()
    torch.cuda.synchronize()
    state = dict(type=type(ex).__name__, runner=getattr(ex, "runner", None), coefs=coefs,
                 params=tr.params.clone(), global_step=tr.global_step,
                 ps={p: (s.m.clone(), None if s.v is None else s.v.clone(), s.t)
                     for p, s in sorted(tr.servers.items())})
    if asyncm:
        ex.close()
    return state


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_train_step_is_the_hand_loop(data, monkeypatch, cell):
    kw, env = CELLS[cell]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    want = run(data, kw, hand_step)
    got = run(data, kw, lambda tr, i: tr.train_step(i))
    print(f"{cell}: {got['type']}, coefs {got['coefs']} (hand loop {want['coefs']})")
    assert got["type"] == want["type"] == {"sync-python": "SyncExchange",
                                           "async-xgmi-push-pull": "AsyncPeerExchange",
                                           "async-rccl": "RcclAsyncExchange"}[cell]
    assert got["runner"] is None   # the host drives the step
    assert min(want["coefs"]) < 1.0 and got["coefs"] == want["coefs"]
    assert got["global_step"] == want["global_step"] == STEPS
    assert torch.equal(bits(got["params"]), bits(want["params"]))
    assert sorted(got["ps"]) == sorted(want["ps"]) and got["ps"]
    for p, (m, v, t) in got["ps"].items():
        wm, wv, wt = want["ps"][p]
        assert t == wt == STEPS
        assert torch.equal(bits(m), bits(wm))
        assert torch.equal(bits(v), bits(wv))
