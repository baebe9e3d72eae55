"""Checkpoint and resume on the GPU for every native runtime: a job cut after CUT updates and
resumed by a NEW Trainer through ``Trainer.train()`` (``resume=True``: ``checkpoint.load``, then
``exchange.start()``) must be, bit for bit, the uninterrupted job.

The state that has to survive lives where the CPU tests (torch engine, Python exchange) never
reach: the ParameterServer objects' m / v / t, the replicated optimizer state of the step's last
bucket (``NativeSyncExchange.repl``, written back by ``sync_ps_state`` before a save and rebuilt by
``load_ps_state`` after a load, with an ``all_gather_object`` at W > 1), the in-line step counters
of the async runner, the hosted-PS bank of the xGMI and RCCL services, each async worker's own
stale buffer and the private PS copies.  A resumed run that silently restarts Adam's moments for
conv1 and conv2 still trains; only a comparison on bits sees it.

The reference is exact and already in the tree: the uninterrupted run of the same job; at W > 1
also the one-process simulation (``onecard.simulate_sync``) and the replay in recorded apply order
(``tests/async_replay.py``).  Every comparison is ``torch.equal`` on values and on bit patterns.

Every run is STEPS = 6 updates cut at CUT = 3, batch 20, on ``synthetic_mnist(400, 100, seed=5)``
(the epoch-boundary row: two epochs of three steps cut at 4): the smallest runs with a non-trivial
t, m and v on both sides of the cut.  The cut run stops with ``max_steps`` and saves through the
end-of-run ``checkpoint.save`` in ``train()``; the resumed trainer is built after the cut one's
exchange was closed.

1. ``test_sync_resume_matrix``: W = 1, the native sync runner, the option matrix (update
   modifiers, the forced RCCL / xGMI rehearsals with and without a replicated bucket, clip +
   accumulation, shuffle + shift across an epoch boundary, another update placement after the
   resume).
2. ``test_async_resume_matrix``: W = 1, the async data planes (in-line applies, the host service,
   momentum, RCCL self sessions).
3. ``test_checkpoint_holds_live_state`` / ``test_checkpoint_reshards``: the files hold what was
   live, and load under another plan.
4. ``test_sync_xgmi_w2_resume``: two ranks on one card, sync over xGMI.
5. ``test_async_xgmi_w2_resume_is_one_run``: two ranks, async over xGMI: cut + resume replayed as
   ONE run in its recorded apply order.

docs/DESIGN.md "Checkpoint and resume on the GPU" has the matrix, the step numbering of a
restarted service and the four one-line breaks each of these tests was seen to catch.
"""
import json
import os

import pytest
import torch

import async_replay as ar
import onecard as oc
from conftest import free_port
from oracle_common import bits

pytestmark = pytest.mark.gpu

STEPS, CUT, BATCH = 6, 3, 20
N_TRAIN, N_TEST = 400, 100
LR = 1e-2          # the W = 1 runs (onecard.placement_run's); the W = 2 jobs keep the default
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data():
    from ddl_amd.utils.data import synthetic_mnist
    return synthetic_mnist(N_TRAIN, N_TEST, seed=5)


def _same(a, b, what):
    assert torch.equal(a, b) and torch.equal(bits(a), bits(b)), f"{what} differs"


def _trainer(data, setup=None, **kw):
    from ddl_amd.config import TrainConfig
    from ddl_amd.parallel.comm import DistEnv
    from ddl_amd.parallel.roles import Trainer
    base = dict(mode="sync", steps=STEPS, batch_size=BATCH, eval_every=0, engine="hip",
                quiet=True, lr=LR)
    base.update(kw)
    tr = Trainer(TrainConfig(**base), DistEnv(0, 1, 0, DEV), dataset=data)
    if setup is not None:
        setup(tr)
    return tr


def _train(data, setup=None, **kw):
    """A W = 1 job through Trainer.train(): the trainer (its exchange closed) and its state."""
    tr = _trainer(data, setup, **kw)
    tr.train()
    state = oc.run_state(tr)
    if not tr.asyncx:       # (an asynchronous run closes its data plane at the end of train())
        tr.exchange.close()
    return tr, state


def _full_cut_resume(data, ck, row, cut=CUT, setups=None):
    """The three jobs of a row, one after the other (each trainer is built after the last one's
    exchange was closed): uninterrupted, cut at `cut` and saved by train(), resumed by a new
    trainer.  setups: {"full" | "part" | "res": hook on the trainer before its train()}."""
    setups = setups or {}
    full = _train(data, setups.get("full"), **row)
    part = _train(data, setups.get("part"), checkpoint_dir=ck, max_steps=cut, **row)
    assert part[0].global_step == cut
    assert all(s.t == cut for s in part[0].servers.values())
    res = _train(data, setups.get("res"), checkpoint_dir=ck, resume=True, **row)
    assert res[0].global_step == full[0].global_step == STEPS
    return full, part, res


# ---- 1. W = 1, sync, the native runner ------------------------------------------------------------
def _no_tail(tr):
    tr.exchange.runner.set_use_tail(False)


FORCED = dict(shard="flat", force_collectives=True)
SYNC_ROWS = [
    pytest.param(dict(optimizer="momentum", nesterov=True, weight_decay=0.01, shard="lpt",
                      num_ps=4), {}, id="nesterov-wd-lpt4"),
    pytest.param(dict(optimizer="sgd", shard="greedy", num_ps=3), {}, id="sgd-greedy3"),
    pytest.param(dict(FORCED, exchange_backend="rccl"), dict(repl=True), id="rccl-ar"),
    pytest.param(dict(FORCED, exchange_backend="xgmi"), dict(repl=True), id="xgmi-repl"),
    pytest.param(dict(FORCED, exchange_backend="xgmi", optimizer="momentum"), dict(repl=True),
                 id="xgmi-repl-momentum"),
    pytest.param(dict(shard="contiguous", force_collectives=True, exchange_backend="xgmi"),
                 dict(repl=False), id="xgmi-owner"),
    pytest.param(dict(accum_steps=2), dict(clip=True), id="clip-accum2"),
    pytest.param(dict(shuffle=True, augment_shift=3, epochs=2, steps=3), dict(cut=4),
                 id="shuffle-shift-epoch2"),
    pytest.param({}, dict(resume_setup=_no_tail), id="resumed-without-tail"),
]


def _clip_value(data, row):
    """A clip norm inside the largest gap between the six pre-clip norms of the row's run with
    the clip out of reach (1e30): below some steps' norms and above others'.  (Adam's step hardly
    depends on the gradient's scale, so the clipped run's norms stay close to these; the test
    asserts from the clipped run itself that both kinds of step occurred.)"""
    pairs = []
    _train(data, _watch_clip(pairs), clip_norm=1e30, **row)
    norms = sorted(p[0] for p in pairs)
    assert len(norms) == STEPS and all(p[1] == 1.0 for p in pairs), pairs
    gap, i = max((norms[i + 1] / norms[i], i) for i in range(STEPS - 1))
    c = oc.f32((norms[i] * norms[i + 1]) ** 0.5)
    print(f"clip: unclipped norms {norms}; largest gap x{gap:.3f} after {i}; clip_norm {c}")
    assert norms[i] < c < norms[i + 1]
    return c


def _watch_clip(pairs):
    """A set-up hook: every train_step of train() appends the step's (norm, coefficient)."""
    def setup(tr):
        step = tr.train_step

        def watched(i):
            step(i)
            torch.cuda.synchronize()
            pairs.append(tuple(tr.clip_out.tolist()))
        tr.train_step = watched
    return setup


def _path_taken(row, how):
    """A set-up hook (the exchange is still open): the row runs on the path it names."""
    def setup(tr):
        ex = tr.exchange
        assert ex.native and not tr.asyncx
        if "repl" not in how:
            assert ex.backend == "local" and ex.repl is None
            return
        assert (ex.repl is not None) == how["repl"], "the replicated last bucket"
        assert any(u.kind != "local" for u in ex.units)
        if row["exchange_backend"] == "xgmi":
            assert ex.peer is not None
            owner = [ex.peer.owner(b) >= 0 for b in range(len(ex.peer.nslices()))]
            assert all(owner) if row["shard"] != "flat" else not any(owner)
        else:
            assert ex.peer is None and ex.runner.has_comm()
        if how["repl"]:
            assert (ex.repl[4] is None) == (row.get("optimizer", "adam") != "adam")
    return setup


@pytest.mark.parametrize("row,how", SYNC_ROWS)
def test_sync_resume_matrix(tmp_path, data, row, how):
    """W = 1, synchronous, the native runner: full run against cut + resume, on bits: the
    parameters, every server's m, its v where the rule keeps one, and t == STEPS on every PS.
    The rows that name a path prove they took it."""
    row, ck, cut = dict(row), str(tmp_path / "ck"), how.get("cut", CUT)
    hooks, pairs = {k: [_path_taken(row, how)] for k in ("full", "part", "res")}, {}
    if how.get("clip"):
        row["clip_norm"] = _clip_value(data, row)
        pairs = {k: [] for k in hooks}
        for k in hooks:
            hooks[k].append(_watch_clip(pairs[k]))
    if "resume_setup" in how:
        hooks["res"].append(how["resume_setup"])
    setups = {k: (lambda tr, fs=fs: [f(tr) for f in fs]) for k, fs in hooks.items()}
    full, part, res = _full_cut_resume(data, ck, row, cut, setups)
    has_v = row.get("optimizer", "adam") == "adam"
    oc.assert_same_run(res[1], full[1], has_v=has_v, t=STEPS)
    # the resumed half did something: the parameters at the cut are not the final ones
    assert not torch.equal(part[1][0], res[1][0])
    assert all(s[2] == cut for s in part[1][1])
    if pairs:
        print("clip: (norm, coefficient) per step", pairs)
        assert pairs["part"] + pairs["res"] == pairs["full"]   # floats off the device: exact
        coefs = [c for _, c in pairs["full"]]
        assert len(coefs) == STEPS
        assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
        # ... and on both sides of the cut something other than a fresh run's first steps
        assert pairs["res"] != pairs["full"][:CUT]


# ---- 2. W = 1, async -------------------------------------------------------------------------------
ASYNC_ROWS = [
    pytest.param(dict(exchange_backend="xgmi", shard="flat"), {}, "inline", id="xgmi-inline"),
    pytest.param(dict(exchange_backend="xgmi", shard="flat"), dict(DDL_ASYNC_INLINE="0"), "host",
                 id="xgmi-service"),
    pytest.param(dict(exchange_backend="xgmi", shard="flat", optimizer="momentum"), {}, "host",
                 id="xgmi-momentum"),
    pytest.param(dict(exchange_backend="rccl", optimizer="momentum"), {}, None,
                 id="rccl-momentum"),
]


@pytest.mark.parametrize("row,env,mode", ASYNC_ROWS)
def test_async_resume_matrix(tmp_path, data, monkeypatch, row, env, mode):
    """W = 1, asynchronous, over the xGMI data plane (3 segment-aligned PS: the runner's in-line
    applies with their own step counters, or the host service, board and gate that W > 1 uses)
    and over RCCL self sessions (a bank without v): full run against cut + resume, on bits, with
    every PS's t and private parameter copy."""
    from ddl_amd.parallel.async_rccl import RcclAsyncExchange
    from ddl_amd.parallel.async_xgmi import AsyncPeerExchange
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    row = dict(row, mode="async", check_provenance=True)
    full, part, res = _full_cut_resume(data, str(tmp_path / "ck"), row)
    xgmi = row["exchange_backend"] == "xgmi"
    for tr, _ in (full, part, res):
        assert tr.asyncx
        assert isinstance(tr.exchange, AsyncPeerExchange if xgmi else RcclAsyncExchange)
        assert tr.exchange.service_mode == mode, tr.exchange.service_mode
        assert len(tr.servers) == (3 if xgmi else 1)
    if xgmi:  # (the board serves the worker's own pushes too; a self session is not "served")
        assert res[0].exchange.served == len(res[0].servers) * (STEPS - CUT)
    oc.assert_same_run(res[1], full[1], has_v=row.get("optimizer", "adam") == "adam", t=STEPS)
    assert not torch.equal(part[1][0], res[1][0])
    for p, f in full[0].servers.items():
        r = res[0].servers[p]
        assert r.t == f.t == STEPS, (p, r.t, f.t)
        _same(r.params, f.params, f"PS {p}'s private copy")
        lo, hi = res[0].plan.ps_segments(p)[0]
        _same(r.params, res[0].params[lo:hi], f"PS {p}'s copy and the worker's range")


# ---- 3. the checkpoint holds what was live, and reshards -------------------------------------------
SAVER = dict(shard="flat", force_collectives=True, exchange_backend="xgmi")


def _assert_repl_is_ps_state(tr, what):
    """The exchange's replicated buffers equal the matching slice of the PS objects' m / v."""
    _, lo, hi, m, v = tr.exchange.repl
    _same(m, oc.ps_flat(tr, "m")[lo:hi], f"{what}: replicated m and the PS's")
    if v is not None:
        _same(v, oc.ps_flat(tr, "v")[lo:hi], f"{what}: replicated v and the PS's")
    assert bool((m != 0).any()), f"{what}: replicated m is all zeros"


@pytest.fixture(scope="module")
def saved(tmp_path_factory, data):
    """CUT steps of the forced xGMI rehearsal (a replicated last bucket), sync_ps_state(), the
    canonical live parameters, m and v, then the save: (directory, live state)."""
    from ddl_amd.utils import checkpoint as ckpt
    ck = str(tmp_path_factory.mktemp("resume") / "ck")
    a = _trainer(data, **SAVER)
    assert a.exchange.repl is not None and a.exchange.peer is not None
    for i in range(CUT):
        a.train_step(i)
    torch.cuda.synchronize()
    a.exchange.sync_ps_state()
    live = oc.canon_state(a)
    _assert_repl_is_ps_state(a, "the saving trainer")
    ckpt.save(a, ck)
    a.exchange.close()
    return ck, live


def test_checkpoint_holds_live_state(saved):
    """The files of a checkpoint taken with a replicated last bucket: the stitched PS files give
    back the live m, v and w of all 14 tensors, the worker file the parameters, the manifest
    t = CUT."""
    from safetensors.torch import load_file
    from ddl_amd.models.layout import TENSORS
    from ddl_amd.utils import checkpoint as ckpt
    ck, live = saved
    man = json.load(open(os.path.join(ck, "manifest.json")))
    assert man["ps_t"] == {"0": CUT} and man["global_step"] == CUT and man["num_ps"] == 1
    full, _ = ckpt._stitch(ck, man["num_ps"])
    assert sorted(full) == [t.index for t in TENSORS]
    worker = load_file(os.path.join(ck, "worker0.safetensors"))
    off = 0
    for t in TENSORS:
        for slot in ("w", "m", "v"):
            _same(full[t.index][slot], live[slot][off:off + t.numel], f"{t.name} {slot}")
        assert bool((live["m"][off:off + t.numel] != 0).any()), f"{t.name}: m is all zeros"
        _same(worker[f"mnist/v{t.index}"].reshape(-1), live["w"][off:off + t.numel],
              f"worker file {t.name}")
        off += t.numel
    assert off == live["w"].numel()


@pytest.mark.parametrize("plan,repl", [
    pytest.param(dict(shard="contiguous", num_ps=3), False, id="contiguous3-local"),
    pytest.param(dict(shard="flat"), False, id="flat-local"),
    pytest.param(dict(shard="greedy", num_ps=3, force_collectives=True, exchange_backend="xgmi"),
                 False, id="greedy3-xgmi"),
    # (the plans that rebuild a replicated bucket from the loaded PS chunks: load_ps_state)
    pytest.param(dict(SAVER), True, id="flat-xgmi-repl"),
    pytest.param(dict(SAVER, exchange_backend="rccl"), True, id="flat-rccl-ar"),
])
def test_checkpoint_reshards(saved, data, plan, repl):
    """The checkpoint loaded into a fresh trainer under another plan: canonical parameters, m and
    v bit-equal to the saved ones, every PS at t = CUT (t_resume where the plan changed), a
    replicated bucket rebuilt from the loaded chunks, and a further step that trains."""
    from ddl_amd.utils import checkpoint as ckpt
    ck, live = saved
    b = _trainer(data, **plan)
    ckpt.load(b, ck)
    torch.cuda.synchronize()
    got = oc.canon_state(b)
    for slot in ("w", "m", "v"):
        _same(got[slot], live[slot], f"loaded {slot}")
    assert b.global_step == CUT and len(b.servers) == plan.get("num_ps", 1)
    assert all(ps.t == CUT for ps in b.servers.values()), {p: s.t for p, s in b.servers.items()}
    assert (b.exchange.repl is not None) == repl
    if b.exchange.repl is not None:
        _assert_repl_is_ps_state(b, "the loaded trainer")
    loaded = b.params.clone()
    b.train_step(CUT)
    torch.cuda.synchronize()
    b.exchange.check()
    assert torch.isfinite(b.params).all()
    assert not torch.equal(b.params, loaded)
    assert all(ps.t == CUT + 1 for ps in b.servers.values())
    b.exchange.close()


# ---- 4. W = 2 on one card, sync over xGMI ----------------------------------------------------------
def _job_kw(phase, ck):
    return {"full": dict(checkpoint_dir=ck), "cut": dict(checkpoint_dir=ck, max_steps=CUT),
            "resume": dict(checkpoint_dir=ck, resume=True)}[phase]


def _sync_rank(rank, world, port, outdir, ck, phase, kw):
    kw = dict(kw)
    env = kw.pop("_env", {})
    with oc.rank_session(rank, world, port, env=env, on_device_0=True) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "sync", STEPS, BATCH, synthetic_mnist(N_TRAIN, N_TEST, seed=5),
                             **dict(dict(shard="flat"), **kw), **_job_kw(phase, ck))
        tr.train()
        torch.cuda.synchronize()
        tr.exchange.check()
        tr.exchange.sync_ps_state()
        rec = dict(params=oc.canon(tr.params, tr.plan.tensor_offsets).cpu(),
                   ps=oc.hosted_ps_record(tr), steps=tr.global_step,
                   repl=tr.exchange.repl is not None)
        torch.save(rec, os.path.join(outdir, f"{phase}{rank}.pt"))
        me.close_single(tr.exchange)


_SIM = {}


def _simulation():
    """simulate_sync of the flat W = 2 Adam job on the ranks' dataset: computed once."""
    if not _SIM:
        from ddl_amd.models import engine_segments
        from ddl_amd.parallel.sharding import make_plan
        plan = make_plan("flat", 2, buckets=engine_segments("hip", DEV))
        _SIM["ref"] = oc.simulate_sync(2, STEPS, BATCH, oc.dataset_on_card(N_TRAIN, N_TEST), plan)
    return _SIM["ref"]


@pytest.mark.slow
@pytest.mark.parametrize("kw,repl,simulated", [
    pytest.param({}, True, True, id="flat-repl"),
    pytest.param(dict(optimizer="momentum"), True, False, id="momentum"),
    pytest.param(dict(shard="contiguous"), False, False, id="contiguous"),
    pytest.param(dict(_env=dict(DDL_REPL_LAST="0")), False, True, id="flat-owner"),
])
def test_sync_xgmi_w2_resume(tmp_path, kw, repl, simulated):
    """Two ranks on one card, synchronous over xGMI, three jobs (full, cut, resume): the resumed
    ranks agree with each other and with the full job's ranks in the parameters, every PS's m / v
    and t == STEPS; the flat Adam cases also equal the one-process simulation, which pins the
    full run itself.  With the replicated last bucket, each rank's checkpoint holds only its own
    chunk of that state and load_ps_state gathers the other's."""
    world = 2
    cks = {"full": str(tmp_path / "ck_full"), "cut": str(tmp_path / "ck"),
           "resume": str(tmp_path / "ck")}
    recs = {}
    for phase in ("full", "cut", "resume"):
        oc.run_ranks(_sync_rank, world, free_port(), str(tmp_path), cks[phase], phase, kw,
                     limit_s=oc.LIMIT_S)
        recs[phase] = oc.load_ranks(tmp_path, world, name=phase + "{}.pt")
    full, cut, res = recs["full"], recs["cut"], recs["resume"]
    assert all(rec["repl"] == repl for rs in recs.values() for rec in rs)
    assert [r["steps"] for r in full + cut + res] == [STEPS] * 2 + [CUT] * 2 + [STEPS] * 2
    _same(res[0]["params"], res[1]["params"], "the resumed ranks' parameters")
    hosted = sorted(p for rec in res for p in rec["ps"])
    assert hosted == [0, 1]
    for r in range(world):
        _same(res[r]["params"], full[r]["params"], f"rank {r}: parameters")
        assert not torch.equal(cut[r]["params"], res[r]["params"])
        assert res[r]["ps"].keys() == full[r]["ps"].keys()
        for p, got in res[r]["ps"].items():
            want = full[r]["ps"][p]
            assert got["t"] == want["t"] == STEPS and cut[r]["ps"][p]["t"] == CUT, (p, got["t"])
            _same(got["m"], want["m"], f"PS {p} m")
            assert (got["v"] is None) == (want["v"] is None) == (kw.get("optimizer") == "momentum")
            if got["v"] is not None:
                _same(got["v"], want["v"], f"PS {p} v")
    if simulated:
        ref = _simulation()
        diff = float((res[0]["params"] - ref).abs().max())
        assert torch.equal(res[0]["params"], ref) and torch.equal(bits(res[0]["params"]),
                                                                 bits(ref)), f"max |diff| {diff}"


# ---- 5. W = 2 on one card, async over xGMI ---------------------------------------------------------
def _async_rank(rank, world, port, outdir, ck, phase, kw):
    with oc.rank_session(rank, world, port, on_device_0=True) as me:
        from ddl_amd.utils.data import synthetic_mnist
        tr = oc.xgmi_trainer(me.env, "async", STEPS, BATCH,
                             synthetic_mnist(N_TRAIN, N_TEST, seed=5), **kw, **_job_kw(phase, ck))
        assert tr.exchange.runner is not None, "native async step not taken"
        rec = oc.async_train_record(tr, world)   # (train() closes the data plane itself)
        assert rec["service_mode"] == "host" or not tr.servers
        torch.save(rec, os.path.join(outdir, f"{phase}{rank}.pt"))


@pytest.mark.slow
@pytest.mark.parametrize("kw,num_ps", [
    pytest.param(dict(shard="flat"), 4, id="adam-flat"),
    pytest.param(dict(optimizer="momentum"), 2, id="momentum"),
])
def test_async_xgmi_w2_resume_is_one_run(tmp_path, kw, num_ps):
    """Two ranks on one card, asynchronous over xGMI: the cut job and the resumed job together
    are ONE realisable run.  An asynchronous run is not reproducible, but the two phases have a
    recorded apply order, and the replay gives every bit that follows from it: from the cut job's
    initial parameters, through CUT + (STEPS - CUT) steps in that order, to every resumed
    worker's stale buffer and every PS's parameters, m, v and t.  The replay's gradients use the
    GLOBAL step for the batch index and the dropout seed, as the uninterrupted run would.

    How a restarted service numbers things (ps_bank.h ``PsBank::record``, xgmi_async.hip
    ``AsyncService::serve``, async_xgmi.py): the logged round is the service's own count of that
    worker's pushes at that PS, which every new service starts from the exchange's round base
    (the set-up self-test is round 1, so ``round_base`` = 2 and ``_collect`` reports rounds from
    0): the resumed job logs steps 0 .. STEPS - CUT - 1 again, not CUT .. STEPS - 1, and
    ``verify_provenance`` checks them against this run's own window.  The PS counter t is the
    one thing that carries over: ``start()`` hands each restored ``ps.t`` to the new service's
    bank, so the resumed job's first apply at a PS is t = 2 * CUT + 1.  One log of the whole run
    is therefore the cut job's entries as they are plus the resumed job's with the step shifted
    by CUT; its t must run 1 .. 2 * STEPS per PS with no gap and no repeat at the cut."""
    from test_async_replay_gpu import _spans
    world, ck = 2, str(tmp_path / "ck")
    recs = {}
    for phase in ("cut", "resume"):
        oc.run_ranks(_async_rank, world, free_port(), str(tmp_path), ck, phase, kw,
                     limit_s=oc.LIMIT_S)
        recs[phase] = oc.load_ranks(tmp_path, world, name=phase + "{}.pt")
    cut, res = recs["cut"], recs["resume"]
    hosts, ranges, offsets = cut[0]["hosts"], cut[0]["ranges"], cut[0]["offsets"]
    assert len(hosts) == num_ps
    for rec in cut + res:
        assert rec["ranges"] == ranges and rec["offsets"] == offsets and rec["hosts"] == hosts
    assert torch.equal(cut[0]["init"], cut[1]["init"])
    assert [r["steps"] for r in cut + res] == [CUT] * 2 + [STEPS] * 2
    assert [r["pushes"] for r in cut + res] == [CUT] * 2 + [STEPS - CUT] * 2
    log_cut = [e for rec in cut for e in rec["provenance"]]
    log_res = [e for rec in res for e in rec["provenance"]]
    assert len(log_cut) == num_ps * world * CUT and len(log_res) == num_ps * world * (STEPS - CUT)
    # the restarted services count their rounds from 0 again ...
    assert sorted({s for (_, _, s, _) in log_res}) == list(range(STEPS - CUT))
    # ... and their t from the restored counters
    assert all(t <= world * CUT for (_, _, _, t) in log_cut)
    assert all(t > world * CUT for (_, _, _, t) in log_res), sorted(t for *_, t in log_res)[:4]
    log = log_cut + [(w, p, s + CUT, t) for (w, p, s, t) in log_res]
    order = ar.apply_orders(log, world, STEPS)
    for p in range(num_ps):
        ts = sorted(t for (_, pp, _, t) in log if pp == p)
        assert ts == list(range(1, world * STEPS + 1)), (p, ts)
    orders = {p: ar.order_string(o) for p, o in order.items()}
    print(f"orders (cut | resumed): "
          f"{ {p: s[:world * CUT] + '|' + s[world * CUT:] for p, s in orders.items()} }")
    spans = _spans(ranges, offsets)
    dataset = oc.dataset_on_card(N_TRAIN, N_TEST)
    # the cut job alone (a mismatch here is not the resume's)
    order_cut = ar.apply_orders(log_cut, world, CUT)
    params, state = oc.replay_async(cut, world, order_cut, CUT, dataset=dataset)
    fails = oc.replay_mismatches(cut, world, params, state, spans, tag="cut job: ")
    assert not fails, f"orders {orders}\n" + "\n".join(fails[:40])
    # the whole run, from the cut job's init, against what the resumed job left
    whole = [dict(res[r], init=cut[r]["init"]) for r in range(world)]
    params, state = oc.replay_async(whole, world, order, STEPS, dataset=dataset)
    fails = oc.replay_mismatches(whole, world, params, state, spans, tag="cut + resume: ")
    assert not fails, f"orders {orders}\n" + "\n".join(fails[:40])
    for rec in res:
        assert all(ps["t"] == world * STEPS for ps in rec["ps"].values())
