"""Every dispatch branch of the backward segments, through `backward_segment` itself.

engine.hip `backward_segment` and engine_impl.h `run_dual_inst` / `run_dual_then_inst` /
`dual_then_b` pick a segment's launches at run time from the tile configs, `dual`, the split
counts, the wide thresholds, `dual_bfirst`, the conv1 switches and what is pending (fc weight
gradients, an optimizer tail).  tests/test_op_oracle_gpu.py sweeps the configs one op per launch
and runs the segments on the default schedule only; here the segments run under every schedule of
tests/dispatch_cells.py, and after each run the engine's host counters (`dispatch_hits()`) must
equal `dispatch_cells.expected_hits` exactly, so a cell that fell back to another branch fails.

a. Segments 1-3 on the integer operands of `segment_case`: bit-equal to the fp64 reference
   through `oracle_common.check` (rows >= B and every other buffer bit-unchanged, halos zero, no
   other gradient touched).  Per conv layer: both ops over {3, 5, 14}^2 x both block orders; each
   op on a config with no dual launch (0, 13); both problems in each split-K mode (unsplit, last
   arriver, separate reduce: z > 1 asserted) on pairings (3, 3), (14, 5), (5, 14) x both orders;
   segment 3's fused launches (conv2's data gradient on {3, 14} x its weight gradient on
   {3, 5, 14} x conv1's direct kernel on / off x the reduce unsplit, in-launch, and separate at
   splits 3 / 12 / 48: 4, 16 and 64 reduce lanes, asserted) and the unfused sequence by each of
   its three conditions; the two-stream mode.  40-row engine at B = 1, 5, 33; on the 136-row
   engine at B = 129 the pairings, the mode grid on (3, 3) and the fused cells.
b. One Adam piece queued with `queue_update_tail` on tensors outside every engine buffer before
   one schedule per branch (dispatch_cells.TAIL_CELLS, and before each segment of the chain
   cells): the segment stays exact, w / m / v equal `update_flat` on copies bit for bit, the
   NaN around the span stays, and exactly one of tail_consumed / tail_standalone counts once.
c. Segments 0 -> 1 chained on real values (`make_real_params`, the rows of `head_inputs`): fc2 /
   fc1 data and weight gradients and conv4's pair by `step_audit.audit_op` on the GPU's own inputs
   (per element within (K + 8) 2^-24 of the abs-sum, RMS within MARGIN of the fp32 CPU's), every
   gradient NaN beforehand.  Cells: the default (packs that defer, `FcWgradAux` in the conv4
   dual); `set_fc_wgrad_defer(False)` (the packs keep them); conv4's data gradient on config 0
   and on 13 (back to back, then `flush_fc_wgrad`); the fc data gradients on 3 and on 5 (one-wave
   dual with `head_aux`, the conv4 dual with `TailAux`); `dual` off.  G[8..11] are bit-equal to
   the default cell's in every one of them, at every batch: engine_impl.h's "the same bits" holds
   for the packs, and the flush path (config 5: the 32x32 tile with BK 16) and the one-wave fc
   dual do not differ either, because each of these tiles sums its element's K = batch products
   in index order, unsplit.  All of it is asserted.
d. `test_every_branch_was_hit` sums the counters of every run above: no branch with zero hits.

Measured on one MI355X (per-test durations of a whole-suite run; docs/DESIGN.md "Every dispatch
branch of the backward segments" has the tables): the file's 68 tests 3.6 s together, 6.8 s as a
run of its own; slowest test_segment_schedules_exact_129_rows[3] 0.36 s (96 schedules at B = 129),
test_segment_schedules_exact[1-1] 0.30 s (77 schedules and the module's first references),
segment 3 at B = 33 0.26 s (141 schedules): 2-4 ms per schedule; a chain cell 0.07-0.13 s.  No
cell failed on its first run: every schedule gave the reference's bits and the branch it names.
"""
import collections
import contextlib

import pytest
import torch

import dispatch_cells as D
import op_reference as R
import step_audit as A
from oracle_common import (BATCHES, DEV, KEEP, ROWS_BIG, SEED, Ctx, bits, check, head_inputs,
                           interior, make_real_params, prepare, segment_case, untouched_failures)

pytestmark = pytest.mark.gpu

B_BIG = 129
TOTAL = collections.Counter()   # every run's counters, for test_every_branch_was_hit
GBITS = {}                      # (rows, B) -> bits of G[8..11] after the default chain cell


@pytest.fixture(scope="module")
def ctx():
    return Ctx(R.make_params(11))


@pytest.fixture(scope="module")
def ctx136():
    return Ctx(R.make_params(11), rows=ROWS_BIG)


@pytest.fixture(scope="module")
def rctx():
    return Ctx(make_real_params())


@pytest.fixture(scope="module")
def rctx136():
    return Ctx(make_real_params(), rows=ROWS_BIG)


@contextlib.contextmanager
def scheduled(c, sched):
    """The engine under `sched` (dispatch_cells.resolved), the defaults put back afterwards."""
    e, eng = c.e(), c.eng
    sc = D.resolved(sched)
    base = dict(cfg=eng.get_cfg(), splits=eng.get_splits(), wide=eng.get_wide(),
                bfirst=e.get_dual_bfirst(), direct=(e.conv1_direct(), e.conv1_wgrad_direct()),
                defer=e.fc_wgrad_defer())
    try:
        if sc["cfg"] != base["cfg"]:
            eng.set_cfg(sc["cfg"])
        if sc["splits"] != base["splits"]:
            eng.set_splits(sc["splits"])
        eng.set_wide(sc["wide"])
        e.set_dual_bfirst(sum(1 << op for op in sc["bfirst"]))
        e.set_conv1_direct(sc["direct"])
        e.set_conv1_wgrad_direct(sc["direct"])
        e.set_fc_wgrad_defer(sc["defer"])
        eng.set_dual(sc["dual"])
        eng.set_concurrent(sc["concurrent"])
        yield sc
    finally:
        eng.set_concurrent(False)
        eng.set_dual(True)
        e.set_fc_wgrad_defer(base["defer"])
        e.set_conv1_direct(base["direct"][0])
        e.set_conv1_wgrad_direct(base["direct"][1])
        e.set_dual_bfirst(base["bfirst"])
        eng.set_wide(base["wide"])
        if eng.get_splits() != base["splits"]:
            eng.set_splits(base["splits"])
        if eng.get_cfg() != base["cfg"]:
            eng.set_cfg(base["cfg"])


def counted(e, want, tag):
    """The counters since the last reset against `want` (every other one 0); adds them to TOTAL."""
    hits = {k: v for k, v in e.dispatch_hits().items() if v}
    TOTAL.update(hits)
    return [] if hits == want else [f"{tag}: dispatch_hits() {hits}, the cell expects {want}"]


# ---- b: a pending tail -------------------------------------------------------------------------------
ADAM, B1, B2, EPS, STEP = 0, 0.9, 0.999, 1e-8, 3e-4   # update.h UpdKind; test_update_rule_gpu.py


class Tail:
    """One Adam piece of N elements at [LO, LO + N) of NaN-filled buffers of the test's own: 16-byte
    aligned, N a multiple of 4, 385 float4 = 4 tail blocks of kTailF4PerBlock = 128."""
    N, LO = 1540, 4

    def __init__(self):
        gen = torch.Generator().manual_seed(21)
        n = self.N
        self.host = (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2,
                     torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-4)
        self.want = None
        self.bufs = None

    def _placed(self):
        out = []
        for t in self.host:
            buf = torch.full((self.N + 8,), float("nan"), device=DEV)
            buf[self.LO:self.LO + self.N] = t.to(DEV)
            assert buf[self.LO:].data_ptr() % 16 == 0
            out.append(buf)
        return out

    def _view(self, buf):
        return buf[self.LO:self.LO + self.N]

    def queue(self, e):
        self.bufs = self._placed()
        e.queue_update_tail(ADAM, *(self._view(b) for b in self.bufs), STEP, B1, B2, EPS, 0.0, 1.0)

    def failures(self, tag):
        """After the launch that took the piece (synchronized): w, m, v against update_flat on
        copies, g and everything around the span unchanged."""
        from ddl_amd.ops import native
        if self.want is None:
            ref = self._placed()
            native.ops().update_flat(ADAM, *(self._view(b) for b in ref), STEP, B1, B2, EPS, 0.0,
                                     1.0)
            torch.cuda.synchronize()
            self.want = [bits(b).clone() for b in ref]
            assert not torch.equal(self.want[0], bits(self._placed()[0]))   # it updates
        return [f"{tag}: the tail's {n} differs from update_flat's (applied twice, dropped or "
                f"written outside the span)"
                for n, b, w in zip("wgmv", self.bufs, self.want) if not torch.equal(bits(b), w)]


@pytest.fixture(scope="module")
def tail():
    return Tail()


# ---- a: segments 1-3, exact ----------------------------------------------------------------------------
def dev_case(c, s, B):
    """segment_case with inputs and fp32 references already on the device."""
    key = ("seg-dev", s, B)
    if key not in c.cases:
        inputs, ref = segment_case(c, s, B)
        c.cases[key] = ({k: v.to(DEV) for k, v in inputs.items()},
                        {k: v.to(torch.float32).to(DEV) for k, v in ref.items()})
    return c.cases[key]


def run_segment(c, s, B, name, sched, tail=None):
    e = c.e()
    tag = f"{name} B={B}"
    with scheduled(c, sched):
        inputs, ref = dev_case(c, s, B)
        x, snap = prepare(c, B, inputs)
        e.reset_dispatch_hits()
        if tail is not None:
            tail.queue(e)
        e.backward_segment(s, x, c.labels[:B], c.seed_t)
        torch.cuda.synchronize()
        fails = check(c, B, snap, ref, tag)
        K15 = e.op_shape(D.CONV2_WGRAD, B)[2]
        want, _ = D.expected_hits(s, sched, K15, tail=tail is not None)
        fails += counted(e, want, tag)
        if tail is not None:
            fails += tail.failures(tag)
    return fails


def assert_split_counts(c, s, B, cells):
    """Every problem a mode cell splits really runs more than one K chunk (z = 3 by gemm.h
    splitk_z on op_shape's K), and the fused cells' separate reduces 4, 16 and 64 lanes."""
    e = c.e()
    for name, sched in cells:
        sc = D.resolved(sched)
        if " modes " in name:
            for op in D.PAIR[s]:
                if sc["splits"][op] > 1:
                    z = D.splitk_z(e.op_shape(op, B)[2], sc["splits"][op], D.bk_of(sc["cfg"][op]))
                    assert z > 1, (name, op, z)
    if s == 3:
        K = e.op_shape(D.CONV2_WGRAD, B)[2]
        for _, spl, _, lanes in D.FUSED_MODES:
            for bk in (16, 32):
                z = D.splitk_z(K, spl, bk)
                assert (z > 1) == (spl > 1), (spl, bk, z)
                if lanes is not None:
                    assert {4: z <= 4, 16: 4 < z <= 32, 64: z > 32}[lanes], (spl, bk, z)


def segment_cases(c, s, B, reduced=False):
    cells = D.segment_cells(s, reduced)
    assert_split_counts(c, s, B, cells)
    fails = []
    for name, sched in cells:
        fails += run_segment(c, s, B, name, sched)
    return fails


def test_tables_match_the_engine(ctx):
    """dispatch_cells' copy of the defaults and of the branch names is the engine's."""
    e = ctx.e()
    assert list(e.dispatch_hits().keys()) == D.BRANCHES
    assert ctx.eng.get_cfg() == D.DEF_CFG and ctx.eng.get_splits() == D.DEF_SPLITS
    assert ctx.eng.get_wide() == D.DEF_WIDE
    assert e.get_dual_bfirst() == sum(1 << op for op in D.DEF_BFIRST)
    assert e.fc_wgrad_defer() and e.conv1_wgrad_direct()
    e.set_fc_wgrad_defer(False)
    assert not e.fc_wgrad_defer()
    e.set_fc_wgrad_defer(True)
    # (K, split, K tile) -> chunks: conv4's weight gradient at B <= 32; conv2's at B <= 32, at 129
    for k, z in {(512, 3, 32): 3, (6272, 48, 32): 40, (6272, 48, 16): 44, (25284, 12, 32): 12}.items():
        assert D.splitk_z(*k) == z


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("s", [1, 2, 3])
def test_segment_schedules_exact(ctx, s, B):
    """Every schedule of dispatch_cells.segment_cells(s) on the 40-row engine: same bits as the
    reference, and the branch the cell names."""
    fails = segment_cases(ctx, s, B)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("s", [1, 2, 3])
def test_segment_schedules_exact_129_rows(ctx136, s):
    """The reduced set (pairings, the mode grid on (3, 3), the fused segment 3) at B = 129."""
    fails = segment_cases(ctx136, s, B_BIG, reduced=True)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("s,name,sched", D.TAIL_CELLS, ids=[c[1] for c in D.TAIL_CELLS])
@pytest.mark.parametrize("B", [5, 33])
def test_pending_tail_in_every_branch(ctx, tail, B, s, name, sched):
    """One schedule per branch with an Adam piece pending before the segment."""
    fails = run_segment(ctx, s, B, "tail: " + name, sched, tail)
    assert not fails, "\n".join(fails)


# ---- c: segments 0 -> 1 chained, real values -----------------------------------------------------------
CHAIN_OPS = (6, 7, 8, 9, 10, 11)
CHAIN_OUT = ("dpre1fc", "d4", "d3") + tuple(f"g{i}" for i in range(6, 14))
HEAD_OUT = ("loss", "dlog", "dpre2fc")   # (audited by test_head_matches_reference)


def chain_inputs(c, B):
    key = ("chain", B)
    if key not in c.cases:
        gen = torch.Generator().manual_seed(100 + B)
        h2, labels, _ = head_inputs(c.P, B, gen, range(0, B, 3) if B > 1 else ())
        inputs = {"h2": h2, "h1": R.make_inputs(5, B, 2, real=True)["h1"],
                  "p4": R.make_inputs(4, B, 2, real=True)["p4"],
                  "c4": R.make_inputs(8, B, 2, real=True)["c4"],
                  "p3": R.make_inputs(11, B, 2, real=True)["p3"],
                  "c3": R.make_inputs(10, B, 2, real=True)["c3"]}
        c.cases[key] = (inputs, labels.to(DEV))
    return c.cases[key]


def run_chain(c, B, name, tail=None):
    """backward_segment(0) then (1) under CHAIN_CELLS[name]; returns the failures and the bits of
    G[8..11].  tail: an Adam piece queued before each of the two segments."""
    sched = D.CHAIN_CELLS[name]["sched"]
    e = c.e()
    tag = f"chain {name} B={B}"
    inputs, labels = chain_inputs(c, B)
    fails, lines = [], []
    with scheduled(c, sched):
        x, snap = prepare(c, B, inputs)
        pend = False
        for s in (0, 1):
            e.reset_dispatch_hits()
            if tail is not None:
                tail.queue(e)
            e.backward_segment(s, x, labels, c.seed_t)
            torch.cuda.synchronize()
            want, pend = D.expected_hits(s, sched, tail=tail is not None, fc_pending=pend)
            fails += counted(e, want, f"{tag} segment {s}")
            if tail is not None:
                fails += tail.failures(f"{tag} segment {s}")
        bufs = {n: interior(n, c.whole(n))[:B].cpu().contiguous()
                for n in ("h1", "p4", "c4", "p3", "c3", "dpre2fc", "dpre1fc", "d4", "d3")}
        bufs["x"] = x.cpu()
        for i in range(6, 14):
            bufs[f"g{i}"] = c.gview(i).cpu().contiguous()
        for op in CHAIN_OPS:
            fails += A.audit_op(op, c.P, c.P64, bufs, SEED, tag, lines, {})
        for i in (12, 13):
            if not bool(torch.isfinite(bufs[f"g{i}"]).all()):
                fails.append(f"{tag}: g{i} not all written")
        # rows >= B, halos, every buffer and gradient that is no output: bit-unchanged
        fails += check(c, B, snap, {n: bufs[n] for n in CHAIN_OUT}, tag, lambda *a: [], HEAD_OUT)
        for n in HEAD_OUT:
            fails += untouched_failures(n, c.whole(n), B, snap, tag)
        lo, hi = c.offsets[8], c.offsets[11] + c.gview(11).numel()
        gbits = bits(c.grads[lo:hi]).clone()
    print("\n".join(lines))
    return fails, gbits


def default_gbits(c, B):
    key = (c.rows, B)
    if key not in GBITS:
        fails, GBITS[key] = run_chain(c, B, "default")
        assert not fails, "\n".join(fails)
    return GBITS[key]


def chain_cell(c, B, name):
    want = default_gbits(c, B)
    if name == "default":
        return
    fails, got = run_chain(c, B, name)
    same = torch.equal(got, want)
    print(f"CHAIN-BITS {name} B={B}: G[8..11] {'equal' if same else 'differ from'} the default "
          f"cell's bits")
    if not same:
        fails.append(f"chain {name} B={B}: G[8..11] differ from the default cell's bits")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("name", list(D.CHAIN_CELLS))
@pytest.mark.parametrize("B", BATCHES)
def test_chained_fc_and_conv4_segments(rctx, B, name):
    """Segments 0 -> 1 under each chain cell: the audit of ops 6-11, the counters of each segment,
    and G[8..11] bit-equal to the default cell's (the packs that keep the weight gradient, the
    flush after a back-to-back conv4 pair, the one-wave fc dual, the fc pairs back to back: all
    sum K = batch in index order, unsplit)."""
    chain_cell(rctx, B, name)


@pytest.mark.parametrize("name", [n for n, c in D.CHAIN_CELLS.items() if c["big"]])
def test_chained_fc_and_conv4_segments_129_rows(rctx136, name):
    """The first three cells (conv4's data gradient on 0 and on 13) at B = 129."""
    chain_cell(rctx136, B_BIG, name)


@pytest.mark.parametrize("name", list(D.CHAIN_CELLS))
def test_chained_segments_with_pending_tails(rctx, tail, name):
    """B = 5, an Adam piece pending before segment 0 (every fc2 launch flushes it: fc3's weight
    gradient takes its aux slot) and another before segment 1 (FcWgradAux / TailAux of the conv4
    dual take it, a back-to-back pair flushes it)."""
    fails, got = run_chain(rctx, 5, name, tail)
    if not torch.equal(got, default_gbits(rctx, 5)):
        fails.append(f"chain {name} with tails: G[8..11] differ from the default cell's bits")
    assert not fails, "\n".join(fails[:40])


# ---- d: coverage -----------------------------------------------------------------------------------------
def test_every_branch_was_hit():
    """Resets nothing: over every run of this module, no branch of dispatch_hits() with zero hits
    (nothing to sum when this test is selected alone)."""
    print("DISPATCH-TOTAL " + " ".join(f"{k}={TOTAL[k]}" for k in D.BRANCHES))
    if TOTAL:
        assert [k for k in D.BRANCHES if TOTAL[k] == 0] == []
