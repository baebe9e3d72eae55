"""The native W = 1 step (`SyncRunner::step`, the one bench.py times) audited launch by launch.

Each cell builds a Trainer as tests/test_native_runner.py::_run does (native exchange, HIP engine,
sync, one worker, batch_size 40) on the real-valued parameters of the oracle test, lr 0.01,
keep probability 0.5, and drives two consecutive steps with `tr.exchange.step` at B = 1, 5, 33.
Before a step the parameters and every PS's m / v / t are copied and the first 40 rows of every
engine buffer are poisoned as tests/test_op_oracle_gpu.py does (NaN in the interiors, the code
sentinel in rows < B, 0 in code rows >= B) and every gradient tensor is filled with NaN (the
padding between tensors of the plan buffer stays 0: the engine never writes it and the runner's
last launch relies on its update being a no-op).  After the step and one synchronize:

* each of the 17 GEMM ops: its outputs against `op_reference.run_op` on the GPU's OWN input
  buffers and the parameters from BEFORE the step, with `precision_failures` exactly as
  test_ops_real_valued_precision (per element within (K + 8) 2^-24 of the abs-sum, tensor RMS
  within MARGIN = 2 of the fp32 CPU computation);
* the head (loss, dlog, dpre2fc, fc3's dW / db) on the GPU's h2 with the HEAD_MARGIN rule; h1 and
  dpre2fc exactly 0 where `keep_mask(seed, layer)` drops (the `seed_value` path draws the mask of
  the seed-word path);
* pool codes c1..c4, see `step_audit.code_failures`;
* rows >= B of every buffer bit-unchanged, halos zero, every gradient finite, padding still 0;
* the update: for every range of every unit, parameters, m and v bit-equal to `ops.update_flat` on
  copies of the state before the step with the GPU's final gradient and the step size the
  exchange used, and within the fp64 closed form of tests/exchange_reference.py (relative 1e-6 on
  m and v, absolute 1e-6 on w); every PS's t advanced by one; nothing else of the parameter
  buffer changed;
* `runner.update_launches()` against LAUNCHES below.

The references of one (engine variant, B, step) are computed for the first cell that gets there;
every other cell with the same engine launches must reproduce that cell's buffers and gradients
bit for bit (a tail block that updates a weight some GEMM block still reads shows up here), then
passes its own update check.

The pool-code rule.  Leaving out every window whose fp64 winner is within the op's ceiling
(K + 8) 2^-24 x abs-sum of the runner-up or of 0 cannot stay under 0.1 % of a buffer: the
reference alone puts 0.4 - 1.8 % of c2..c4's windows there for every data seed tried (B = 33:
c1 3-5 of 206976, c2 426-431 of 103488, c3 447-476 of 67584, c4 499-595 of 33792; B = 1: c2 9-12
of 3136, c3 11-15 of 2048, c4 8-15 of 1024), because the ceiling is K u while the pre-activations
spread over only about abs-sum / sqrt(K).  So no window is left out: a window outside the ceiling
must carry the reference's code, a window inside it must still name a position (or 0xFF) that is
within the ceiling of the winner, and the 0.1 % cap applies to the windows whose code differs from
the reference's at all (tests/test_step_audit_cpu.py: the fp32 CPU chain differs in none).

The closed form's hyper-parameters.  The rule (update.h UpdRule) holds 1 - beta formed in fp32, as
TF1's ApplyAdam does.  From zero state v' = (1 - beta2) g^2, and fp32(0.999) is 1.29e-8 above
0.999, so every fp32 implementation is 1.29e-5 (relative) away from the closed form on the decimal
0.999 (measured: exactly that in every range; the exchange-kernel tests start from v = 1e-4 and do
not see it).  `stored_hyper` feeds exchange_reference.rule_step the values as the rule stores them;
the tolerances stay.

One more cell: the asynchronous W = 1 step over the xGMI plane with the in-line applies
(async_runner.hip step_inline), flat plan with 3 PS, batch_size = B, and with 8 PS at B = 5 (six
shards in one segment: the stand-alone launches of the shared run_riding_backward): the same op
audit, the update with each PS's own t, update_launches() against INLINE_LAUNCHES.

Measured on one MI355X (docs/DESIGN.md "The native step, audited launch by launch" has the whole
table): the file's 56 tests in 9.7 s, the slowest 0.83 s, a full audit at B = 33 0.7 s.  RMS-error
ratio GPU / fp32 CPU, the largest over every cell, batch and step (dW / db for the weight
gradients): conv1 fwd 0.98, conv2 fwd 0.44, conv3 fwd 0.47, conv4 fwd 0.34, fc1 fwd 0.86, fc2 fwd
0.94, fc2 dgrad 0.79, fc2 wgrad 1.06 / 1.09, fc1 dgrad 0.86, fc1 wgrad 1.09 / 1.10, conv4 dgrad
0.62, conv4 wgrad 1.44 / 1.52, conv3 dgrad 0.41, conv3 wgrad 1.25 / 1.86, conv2 dgrad 0.59, conv2
wgrad 0.98 / 1.25, conv1 wgrad 0.46 / 1.16.  Largest per-element error 5.2e-7 of the abs-sum
(conv4 wgrad, B = 33, ceiling 3.2e-5).  Head, error ratio under the HEAD_MARGIN rule: loss 2.01,
dlog 1.83, dpre2fc 1.86, fc3 dW 1.50, db 1.43.  Pool codes: 0 windows differ from the reference in
all 128 audited buffers; inside the ceiling of a tie (flat, step 0, B = 1 / 5 / 33): c1 0 / 1 / 5,
c2 9 / 52 / 427, c3 15 / 65 / 448, c4 15 / 89 / 539.  Update: |w - closed form| <= 3.0e-8, m
within 8.8e-8, v within 9.6e-8.  update_launches() equalled LAUNCHES in every cell: 0 everywhere
except greedy-ps3 3, flat-ps3 3, flat-ps7 28, flat-last-alone 1, flat-no-tail 1, flat-no-dual 4.
(Three cells added later, off the default schedule: flat-conv4-b2b 1, flat-conv2-inlaunch 1,
flat-fc-dual 0, as read from the code and as the GPU gave them; 0.23-0.36 s each, the file's 59
tests 8.9 s.)
"""
import time

import pytest
import torch

import exchange_reference as xr
import op_reference as R
import step_audit as A
from ddl_amd.config import TrainConfig
from ddl_amd.models.mnist_cnn import param_views
from ddl_amd.ops.adam import adam_coeffs
from ddl_amd.parallel.comm import DistEnv
from ddl_amd.parallel.roles import Trainer
from ddl_amd.utils.data import synthetic_mnist
from onecard import f32, rel_err
from oracle_common import (BATCHES, BMAX, CODE_BUFS, DEV, FLOAT_BUFS, HALO_BUFS, bits, interior,
                           make_real_params, prepare, untouched_failures)

pytestmark = pytest.mark.gpu

KEEP, LR = A.KEEP, A.LR
BUF_NAMES = FLOAT_BUFS + CODE_BUFS


# ---- cells ---------------------------------------------------------------------------------------------
def _engine(name, on):
    def setup(tr):
        getattr(tr.engine.eng, name)(on)
    return setup


def _runner(**calls):
    def setup(tr):
        for name, args in calls.items():
            getattr(tr.exchange.runner, name)(*args)
    return setup


def _fc2_split(tr):
    """fc2's forward on the split-K 32x32 tile (config 3, split 16), as
    test_fc2_reduce_in_head_is_bit_identical: the native step leaves its reduce to the head."""
    e = tr.engine.eng
    cf, sp = e.get_cfg(), e.get_splits()
    cf[5], sp[5] = 3, 16
    e.set_cfg(cf)
    e.set_splits(sp)


def _schedule(cfg=None, wide=None):
    """Tile configs / wide thresholds by op (csrc/kernels/schedule.h enum Op) over the defaults."""
    def setup(tr):
        e = tr.engine.eng
        if cfg:
            cf = e.get_cfg()
            for op, c in cfg.items():
                cf[op] = c
            e.set_cfg(cf)
        if wide:
            wd = e.get_wide()
            for op, w in wide.items():
                wd[op] = w
            e.set_wide(wd)
    return setup


def cell(shard, batches=BATCHES, setup=None, variant="default", flags=None, **kw):
    return dict(shard=shard, **kw), setup, batches, variant, flags or {}


# name: (TrainConfig arguments, setup, batches, engine variant, the setting as arguments of
# step_audit.expected_update_launches).  Cells of one variant issue the same engine launches apart
# from where the update rides, so their buffers must agree bit for bit.
CELLS = {
    "flat": cell("flat"),
    "none": cell("none"),
    "contiguous": cell("contiguous"),
    "flat-momentum": cell("flat", optimizer="momentum"),
    "none-momentum": cell("none", optimizer="momentum"),
    "contiguous-momentum": cell("contiguous", optimizer="momentum"),
    "flat-sgd": cell("flat", optimizer="sgd"),
    "none-sgd": cell("none", optimizer="sgd"),
    "contiguous-sgd": cell("contiguous", optimizer="sgd"),
    "contiguous-ps2": cell("contiguous", (5, 33), num_ps=2),
    "contiguous-ps8": cell("contiguous", (5, 33), num_ps=8),
    "greedy-ps3": cell("greedy", (5, 33), num_ps=3),
    "lpt-ps4": cell("lpt", (5, 33), num_ps=4),
    "flat-ps3": cell("flat", (5, 33), num_ps=3),
    "flat-ps7": cell("flat", (5, 33), num_ps=7),
    "flat-last-alone": cell("flat", (5,), _runner(set_final_in_reduce=(False,)),
                            flags=dict(final_in_reduce=False)),
    "flat-no-tail": cell("flat", (5,), _runner(set_final_in_reduce=(False,), set_use_tail=(False,)),
                         flags=dict(final_in_reduce=False, use_tail=False)),
    "flat-conv1-gemm": cell("flat", BATCHES, _engine("set_conv1_wgrad_direct", False), "conv1-gemm",
                            flags=dict(conv1_direct=False)),
    "flat-no-dual": cell("flat", (5,), _engine("set_dual", False), "no-dual", flags=dict(dual=False)),
    "flat-tail-0-128": cell("flat", (5,), _runner(set_tail_cfg=(0, 128))),
    "flat-tail-0-1024": cell("flat", (5,), _runner(set_tail_cfg=(0, 1024))),
    "flat-tail-1-128": cell("flat", (5,), _runner(set_tail_cfg=(1, 128))),
    "flat-tail-1-1024": cell("flat", (5,), _runner(set_tail_cfg=(1, 1024))),
    "flat-fc2-split": cell("flat", BATCHES, _fc2_split, "fc2-split"),
    # dispatch branches off the default schedule (tests/test_dispatch_oracle_gpu.py runs them
    # segment by segment): conv4's data gradient (op 10) on config 0, conv2's weight gradient
    # (op 15) reduced in its launch, the fc data gradients (ops 6, 8) on the one-wave 32x32 tile
    "flat-conv4-b2b": cell("flat", (5,), _schedule(cfg={10: 0}), "conv4-b2b",
                           flags=dict(pair_takes=(False, True, True))),
    "flat-conv2-inlaunch": cell("flat", (5,), _schedule(wide={15: 1 << 20}), "conv2-inlaunch",
                                flags=dict(conv2_reduce_separate=False)),
    "flat-fc-dual": cell("flat", (5,), _schedule(cfg={6: 3, 8: 3}), "fc-dual"),
}

# runner.update_launches() of a step: the stand-alone optimizer launches.  Read off UpdatePlan
# (update_plan.h), SyncRunner::step / run_riding_backward (runner.hip) and dual_then_b
# (engine_impl.h); the same
# reading as code is step_audit.expected_update_launches, and tests/test_step_audit_cpu.py holds
# this table against it on every plan.  Segments: 0 fc3, 1 conv4 + fc1 + fc2, 2 conv3, 3 conv2 + conv1;
# segment s's update rides in segment s + 1's dual launch, segment 3's in conv1's weight-gradient
# launch.
LAUNCHES = {
    # one PS, one piece per segment: all ride; segment 3 is one piece of exactly conv1 + conv2
    "flat": 0, "none": 0, "contiguous": 0,
    # the same pieces with a null v
    "flat-momentum": 0, "none-momentum": 0, "contiguous-momentum": 0,
    "flat-sgd": 0, "none-sgd": 0, "contiguous-sgd": 0,
    # pieces per segment 1 / 2 / 1 / 1 (conv4's weight on PS 0, the rest of segment 1 on PS 1): ride
    "contiguous-ps2": 0,
    # 1 / 2 / 2 / 4: segment 3 is one piece per tensor, each on its own PS with the same t: all ride
    "contiguous-ps8": 0,
    # 2 / 6 / 1 / 4: segment 1 has more than kTailPieces pieces (the zig-zag order separates its
    # tensors), tail_ok_ is false: one coalesced launch per PS after the backward
    "greedy-ps3": 3,
    # 1 / 4 / 1 / 1: exactly kTailPieces in segment 1, still rides
    "lpt-ps4": 0,
    # 3 chunks per bucket ride in segments 1-3; segment 3's chunk boundaries lie inside conv2's
    # weight, final_split_conv12 refuses (a piece starts off a tensor): one launch per chunk
    "flat-ps3": 3,
    # 7 chunks per segment > kTailPieces: the fallback, 4 buckets x 7 chunks, no two adjacent
    # chunks on one PS
    "flat-ps7": 28,
    # the tails ride, segment 3's one piece is a launch of its own
    "flat-last-alone": 1,
    # no tails: merged_, the four buckets of the one PS coalesce into one range
    "flat-no-tail": 1,
    # final_split cuts conv1's spans out, the rest rides in launch_reduce_tail
    "flat-conv1-gemm": 0,
    # every pair runs back to back: flush_tail launches segments 0-2's piece each, conv1's
    # stand-alone kernel takes no update, so segment 3's piece follows the backward
    "flat-no-dual": 4,
    # placement and block length of the tail blocks change no launch
    "flat-tail-0-128": 0, "flat-tail-0-1024": 0, "flat-tail-1-128": 0, "flat-tail-1-1024": 0,
    # the head takes fc2's reduce; the updates ride as in "flat"
    "flat-fc2-split": 0,
    # the conv4 pair runs back to back and its flush_tail launches segment 0's piece; the fc weight
    # gradients go through flush_fc_wgrad; the other segments ride
    "flat-conv4-b2b": 1,
    # conv2's weight gradient is final when its dual launch ends (gb.mode == 1): conv1's direct
    # kernel has no reduce epilogue to apply conv2's update in, so dual_then_b leaves final_upd and
    # the runner launches segment 3's piece
    "flat-conv2-inlaunch": 1,
    # no tail is pending at segment 0; the fc pairs run as one-wave dual launches that keep their
    # weight gradients, and the conv4 dual carries segment 0's piece as a plain TailAux
    "flat-fc-dual": 0,
}
assert LAUNCHES.keys() == CELLS.keys()


# ---- a trainer and its buffers -------------------------------------------------------------------------
class StepCtx:
    """The oracle's view (oracle_common) of a Trainer's engine: its first 40 rows."""

    def __init__(self, tr):
        self.tr = tr
        self.grads = tr.grads
        self.offsets = tr.plan.tensor_offsets

    def whole(self, name):
        return self.tr.engine.eng.buffer(name + "+halo" if name in HALO_BUFS else name, BMAX)

    def gview(self, i):
        return param_views(self.grads, self.offsets)[i]

    def poison_grads(self):
        for v in param_views(self.grads, self.offsets):
            v.fill_(float("nan"))


@pytest.fixture(scope="module")
def data():
    return synthetic_mnist(n_train=200, n_test=100, seed=5)


@pytest.fixture(scope="module")
def store():
    """(engine variant, B, step[, optimizer]) -> the audited buffers; "stats": the largest ratios."""
    return {"stats": {}, "t0": time.time()}


def make_trainer(data, **kw):
    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    cfg = TrainConfig(mode="sync", steps=2, batch_size=BMAX, eval_every=0, engine="hip",
                      quiet=True, native_exchange=True, lr=LR, keep_prob=KEEP, **kw)
    tr = Trainer(cfg, env, dataset=data)
    assert getattr(tr.exchange, "native", False) and tr.exchange.backend == "local"
    for view, p in zip(param_views(tr.params, tr.plan.tensor_offsets), make_real_params()):
        view.copy_(p)   # in place: the engine holds pointers into the flat tensor
    return tr


def state_of(tr):
    return {"params": tr.params.clone(),
            "ps": {p: (s.m.clone(), None if s.v is None else s.v.clone(), s.t)
                   for p, s in tr.servers.items()}}


def read_buffers(ctx, B, x):
    bufs = {n: interior(n, ctx.whole(n))[:B].cpu().contiguous() for n in BUF_NAMES}
    bufs["x"] = x.cpu()
    for i in range(14):
        bufs[f"g{i}"] = ctx.gview(i).cpu().contiguous()
    return bufs


def tensor_mask(ctx):
    m = torch.zeros(ctx.grads.numel(), dtype=torch.bool, device=DEV)
    for i in range(14):
        m[ctx.offsets[i]:ctx.offsets[i] + ctx.gview(i).numel()] = True
    return m


def untouched(ctx, B, snap, bufs, tag):
    fails = []
    for n in BUF_NAMES:
        fails += untouched_failures(n, ctx.whole(n), B, snap, tag)
        if n in FLOAT_BUFS and not bool(torch.isfinite(bufs[n]).all()):
            fails.append(f"{tag}: {n} rows < {B} not all written")
        if n in CODE_BUFS and bool((bufs[n] == 0x77).any()):
            fails.append(f"{tag}: {n} rows < {B} keep the sentinel")
    for i in range(14):
        if not bool(torch.isfinite(bufs[f"g{i}"]).all()):
            fails.append(f"{tag}: gradient tensor {i} not all written")
    if int(torch.count_nonzero(ctx.grads[~tensor_mask(ctx)])) != 0:
        fails.append(f"{tag}: gradient padding written")
    return fails



def stored_hyper(h):
    """Adam's hyper-parameters as the rule holds them (update.h UpdRule): 1 - beta formed in fp32,
    as TF1's ApplyAdam forms it.  From zero state v' = (1 - beta2) g^2, so the fp64 closed form on
    the decimal 0.999 is 1.29e-5 (relative) away from any fp32 implementation: fp32(0.999) is
    1.29e-8 above 0.999."""
    one = torch.tensor(1.0)
    c1 = float(one - torch.tensor(h.beta1, dtype=torch.float32))
    c2 = float(one - torch.tensor(h.beta2, dtype=torch.float32))
    return dict(b1=1.0 - c1, b2=1.0 - c2, eps=f32(h.eps))


def range_failures(tr, before, ranges, optimizer, tag, lines):
    """Every (PS, lo, hi, state offset, step size) of `ranges` after the step against
    ops.update_flat (bit for bit) and the fp64 closed form, from the state before the step and
    the GPU's final gradient; nothing outside the ranges moved."""
    from ddl_amd.ops import native
    adam = optimizer == "adam"
    kind = xr.ADAM if adam else xr.MOMENTUM
    mu = tr.cfg.momentum if optimizer == "momentum" else 0.0
    fails = []
    covered = torch.zeros(tr.params.numel(), dtype=torch.bool, device=DEV)
    worst = [0.0, 0.0, 0.0]
    for p, lo, hi, off, step in ranges:
        ps = tr.servers[p]
        m0, v0, _ = before["ps"][p]
        n = hi - lo
        covered[lo:hi] = True
        w = before["params"][lo:hi].clone()
        m = m0[off:off + n].clone()
        v = v0[off:off + n].clone() if adam else None
        g = tr.grads[lo:hi]
        native.ops().update_flat(kind, w, g, m, v, step, ps.h.beta1, ps.h.beta2, ps.h.eps, mu, 1.0)
        where = f"{tag}: PS {p} range [{lo}, {hi})"
        if not torch.equal(bits(w), bits(tr.params[lo:hi])):
            fails.append(f"{where}: parameters differ from update_flat's")
        if not torch.equal(bits(m), bits(ps.m[off:off + n])):
            fails.append(f"{where}: m differs from update_flat's")
        if adam and not torch.equal(bits(v), bits(ps.v[off:off + n])):
            fails.append(f"{where}: v differs from update_flat's")
        if not adam and ps.v is not None:
            fails.append(f"{where}: a v under {optimizer}")
        w2, m2, v2 = xr.rule_step(kind, before["params"][lo:hi], m0[off:off + n],
                                  v0[off:off + n] if adam else None, g, f32(step), mu, 1.0,
                                  **stored_hyper(ps.h))
        ew = float((tr.params[lo:hi].double().cpu() - w2).abs().max())
        em = rel_err(ps.m[off:off + n], m2)
        ev = rel_err(ps.v[off:off + n], v2) if adam else 0.0
        worst = [max(a, b) for a, b in zip(worst, (ew, em, ev))]
        if not (ew < 1e-6 and em < 1e-6 and ev < 1e-6):
            fails.append(f"{where}: |w - closed form| {ew:.3g}, rel m {em:.3g}, rel v {ev:.3g}")
    if not torch.equal(bits(tr.params[~covered]), bits(before["params"][~covered])):
        fails.append(f"{tag}: parameters outside every unit's ranges changed")
    lines.append(f"AUDIT-UPDATE {tag}: |w - closed form| {worst[0]:.3g} rel m {worst[1]:.3g} "
                 f"rel v {worst[2]:.3g}")
    return fails


def update_failures(tr, before, tag, lines):
    """The ranges of every unit of the synchronous exchange, each with the step size the exchange
    used: adam_coeffs(ps.h, ps.t), or lr under momentum / SGD."""
    adam = tr.cfg.optimizer == "adam"
    fails, ranges = [], []
    for u in tr.exchange.units:
        ps = tr.servers[u.ps]
        t0 = before["ps"][u.ps][2]
        if ps.t != t0 + 1:
            fails.append(f"{tag}: PS {u.ps} at t = {ps.t} after the step from t = {t0}")
        step = adam_coeffs(ps.h, t0 + 1) if adam else ps.h.lr
        ranges += [(u.ps, lo, hi, off, step)
                   for (lo, hi), off in zip(u.ranges, u.state_offs or [0] * len(u.ranges))]
    return fails + range_failures(tr, before, ranges, tr.cfg.optimizer, tag, lines)


def typical_move(before, tr):
    """Median |dw| over the elements with a gradient / median |w|, for each weight tensor that a
    GEMM multiplies by (an element without one does not move: in conv4's and fc1's weights more
    than half have none at B = 33, their inputs being sparse)."""
    off = tr.plan.tensor_offsets
    out = {}
    for i in sorted(set(R.OP_WEIGHT.values()) | {12}):
        n = param_views(tr.grads, off)[i].numel()
        w0 = before["params"][off[i]:off[i] + n]
        has = tr.grads[off[i]:off[i] + n] != 0
        dw = (tr.params[off[i]:off[i] + n] - w0).abs()
        out[i] = float(dw[has].median() / w0.abs().median())
    return out


def run_cell(store, data, name, B):
    kw, setup, _, variant, _ = CELLS[name]
    tr = make_trainer(data, **kw)
    if setup is not None:
        setup(tr)
    ctx = StepCtx(tr)
    optimizer = kw.get("optimizer", "adam")
    fails, lines = [], []
    for step in (0, 1):
        tag = f"{name} B={B} step {step}"
        x, y = A.batch(B, step)
        seed = A.STEP_SEEDS[step]
        before = state_of(tr)
        xg, snap = prepare(ctx, B, {"x": x})
        tr.exchange.step(xg, y.to(DEV), KEEP, seed)
        torch.cuda.synchronize()
        launches = tr.exchange.runner.update_launches()
        bufs = read_buffers(ctx, B, xg)
        fails += untouched(ctx, B, snap, bufs, tag)
        # the first step starts from the same parameters under every rule
        key = (variant, B, step) + ((optimizer,) if step else ())
        if key in store:
            ref_name, ref = store[key]
            for n, t in bufs.items():
                if not torch.equal(t, ref[n]):
                    fails.append(f"{tag}: {n} differs from cell {ref_name}'s "
                                 f"({int((t != ref[n]).sum())} elements)")
        else:
            P = [p.cpu().clone() for p in param_views(before["params"], ctx.offsets)]
            fails += A.audit_step(P, bufs, y, seed, tag, lines, store["stats"])
            store[key] = (name, bufs)
        fails += update_failures(tr, before, tag, lines)
        if launches != LAUNCHES[name]:
            fails.append(f"{tag}: update_launches() {launches}, the table says {LAUNCHES[name]}")
        lines.append(f"AUDIT-LAUNCHES {tag}: {launches}")
        if step == 0 and optimizer == "adam" and B == 33:
            move = typical_move(before, tr)
            lines.append(f"AUDIT-MOVE {tag}: " + " ".join(f"{i}:{v:.2f}" for i, v in move.items()))
            if not all(v > 0.1 for v in move.values()):
                fails.append(f"{tag}: the first Adam step moves a typical weight by {move}")
    tr.exchange.close()
    print("\n".join(lines))
    print(f"AUDIT-WALL {name} B={B}: {time.time() - store['t0']:.1f} s since the module began")
    return fails


@pytest.mark.parametrize("name,B", [(n, B) for n, c in CELLS.items() for B in c[2]])
def test_step_audit(store, data, name, B):
    fails = run_cell(store, data, name, B)
    assert not fails, "\n".join(fails[:40])


# update_launches() of an in-line step by the number of PS, read off AsyncRunner::set_inline /
# step_inline and run_riding_backward (runner.hip); tests/test_step_audit_cpu.py derives the same
# numbers from step_audit.expected_update_launches(per_segment=True).
# 3 PS, one per group of segments: the pieces ride in segments 2 and 3, and PS 0 = [0, 52160) is
# exactly conv1 + conv2, so conv1's launch takes it.  8 PS, 1 / 1 / 6 per group: six PS complete in
# segment 1, more than kTailPieces, so those six shards are launched stand-alone and the rest ride.
INLINE_LAUNCHES = {3: 0, 8: 6}


@pytest.mark.parametrize("num_ps,B", [pytest.param(3, B, id=str(B)) for B in BATCHES] +
                         [pytest.param(8, 5, id="ps8-5")])
def test_step_audit_async_inline(store, data, monkeypatch, num_ps, B):
    """The asynchronous W = 1 step over the xGMI plane with the in-line applies (async_runner.hip
    step_inline, the default at one worker): segment-aligned flat plan, each PS's Adam as tail
    blocks of the next segment's launch (tail blocks after the GEMM blocks) and the last segment's
    in conv1's weight-gradient launch.  batch_size = B.  The same op audit; the update with each
    PS's own step counter and the step size the runner forms (ops.adam_step_size).  With 3 PS
    every segment rides; with 8 PS (1 / 1 / 6 per group of segments) segment 1 holds six shards,
    more than one tail takes, and run_riding_backward launches those stand-alone while the other
    segments still ride.  update_launches() after each step against INLINE_LAUNCHES."""
    from ddl_amd.ops import native
    monkeypatch.delenv("DDL_ASYNC_INLINE", raising=False)
    env = DistEnv(0, 1, 0, torch.device("cuda", 0))
    cfg = TrainConfig(mode="async", shard="flat", steps=2, batch_size=B, eval_every=0,
                      engine="hip", quiet=True, exchange_backend="xgmi", lr=LR, keep_prob=KEEP,
                      num_ps=None if num_ps == 3 else num_ps)   # (3: the plan's own choice)
    tr = Trainer(cfg, env, dataset=data)
    ex = tr.exchange
    assert tr.num_ps == num_ps and ex.runner is not None
    for view, p in zip(param_views(tr.params, tr.plan.tensor_offsets), make_real_params()):
        view.copy_(p)
    for p, ps in tr.servers.items():   # the PS's private copies start from the worker's
        lo, hi = ex.ranges[p]
        ps.params.copy_(tr.params[lo:hi])
    ex.steps = 2
    ex.start()
    fails, lines = [], []
    try:
        assert ex.inline and ex.service_mode == "inline"
        ctx = StepCtx(tr)
        for step in (0, 1):
            tag = f"async-inline ps={num_ps} B={B} step {step}"
            x, y = A.batch(B, step)
            seed = A.STEP_SEEDS[step]
            before = state_of(tr)
            t0 = {p: ex.runner.inline_t(p) for p in tr.servers}
            xg, snap = prepare(ctx, B, {"x": x})
            ex.step(xg, y.to(DEV), KEEP, seed)
            ex.drain_round()
            torch.cuda.synchronize()
            launches = ex.runner.update_launches()
            if launches != INLINE_LAUNCHES[num_ps]:
                fails.append(f"{tag}: update_launches() {launches}, the table says "
                             f"{INLINE_LAUNCHES[num_ps]}")
            lines.append(f"AUDIT-LAUNCHES {tag}: {launches}")
            bufs = read_buffers(ctx, B, xg)
            fails += untouched(ctx, B, snap, bufs, tag)
            P = [p.cpu().clone() for p in param_views(before["params"], ctx.offsets)]
            fails += A.audit_step(P, bufs, y, seed, tag, lines, store["stats"])
            ranges = []
            for p, ps in tr.servers.items():
                lo, hi = ex.ranges[p]
                if ex.runner.inline_t(p) != t0[p] + 1:
                    fails.append(f"{tag}: PS {p} at t = {ex.runner.inline_t(p)} from {t0[p]}")
                # (the in-line runner's convention: float32 hyper-parameters widened to double,
                # tests/test_numerics_cpu.py test_native_adam_step_size_matches_python_bitwise)
                step_size = native.ops().adam_step_size(f32(ps.h.lr), f32(ps.h.beta1),
                                                        f32(ps.h.beta2), t0[p] + 1)
                ranges.append((p, lo, hi, 0, step_size))
                if not torch.equal(ps.params, tr.params[lo:hi]):
                    fails.append(f"{tag}: PS {p}'s private copy differs from the worker's")
            fails += range_failures(tr, before, ranges, "adam", tag, lines)
    finally:
        ex.join()
        ex.close()
    assert all(ps.t == 2 for ps in tr.servers.values())
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:40])


def test_audit_summary(store):
    """The largest RMS ratio and per-element error of every tensor over the cells that ran."""
    for (op, name), (ratio, emax) in sorted(store["stats"].items()):
        print(f"AUDIT-MAX {op} {name}: ratio {ratio:.3f} max err {emax:.3g}")
    print(f"AUDIT-WALL module: {time.time() - store['t0']:.1f} s")
    if store["stats"]:   # (empty when this test is selected alone)
        assert len(store["stats"]) == 23 + 5   # every float output of the 17 ops, and the head's
