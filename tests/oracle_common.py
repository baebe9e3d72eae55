"""Shared by the GPU oracle tests (helper module, not a conftest): the poison / snapshot / check
cycle around one engine call, on any object `ctx` that offers

* ``ctx.whole(name)``: the stored buffer, every row the context covers, halo included;
* ``ctx.grads`` and ``ctx.offsets``: the flat gradient buffer and its 14 tensor offsets;
* ``ctx.gview(i)``: gradient tensor i, shaped;
* ``ctx.poison_grads()``: NaN into every gradient element a kernel may write.

tests/test_op_oracle_gpu.py runs it around one op on a 40-row and on a 136-row engine,
tests/test_dispatch_oracle_gpu.py around one backward segment under every schedule,
tests/test_step_audit_gpu.py around a whole training step of a Trainer's engine.  The engine
context of the first two (`Ctx`), `run_case`, `segment_case` and `head_inputs` live here too.
"""
import torch

import op_reference as R
from ddl_amd.models.layout import CANON_OFFSETS, TOTAL_NUMEL
from ddl_amd.models.mnist_cnn import init_params_, param_views

DEV = "cuda"
BMAX = 40
KEEP = 0.5
SEED = 20240
BATCHES = (1, 5, 33)
FLOAT_BUFS = ["p1", "p2", "p3", "p4", "h1", "h2", "dlog", "loss", "dpre2fc", "dpre1fc", "d4", "d3",
              "d2", "d1"]
HALO_BUFS = ("p1", "p2", "p3", "d4", "d3", "d2")
CODE_BUFS = ["c1", "c2", "c3", "c4"]
CODE_SENTINEL = 0x77   # not a code any kernel writes
HEAD_MARGIN = 8.0


def interior(name, t):
    return t[:, 2:-2, 2:-2, :] if name in HALO_BUFS else t


def bits(t, host=False):
    """t's bit pattern (float32 as int32) on t's device, or with host=True on the CPU."""
    t = t.detach().cpu() if host else t.detach()
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def host_bits(t):
    return bits(t, host=True)


def prepare(ctx, B, inputs):
    """Poison every float buffer and the gradients with NaN (every row, interiors only), put the
    code sentinel in rows < B and 0 in rows >= B, write the inputs of rows < B; returns the image
    argument and a snapshot of everything."""
    nan = float("nan")
    for n in FLOAT_BUFS:
        interior(n, ctx.whole(n)).fill_(nan)
    ctx.poison_grads()
    for n in CODE_BUFS:
        c = ctx.whole(n)
        c[:B] = CODE_SENTINEL
        c[B:] = 0
    x = torch.full((B, 784), nan, device=DEV)
    for name, v in inputs.items():
        if name == "x":
            x = v.to(DEV).reshape(B, 784).contiguous()
        else:
            dst = interior(name, ctx.whole(name))[:B]
            dst.copy_(v.to(DEV).reshape(dst.shape))
    snap = {n: bits(ctx.whole(n)).clone() for n in FLOAT_BUFS + CODE_BUFS}
    snap["grads"] = bits(ctx.grads).clone()
    return x, snap


def untouched_failures(name, whole, B, snap, tag):
    """What an op may not do to an output buffer: change a row >= B, write the halo of a row < B."""
    fails = []
    if not torch.equal(bits(whole[B:]), snap[name][B:]):
        fails.append(f"{tag}: {name} rows >= {B} changed")
    if name in HALO_BUFS:
        border = whole[:B].clone()
        border[:, 2:-2, 2:-2, :] = 0
        if int(torch.count_nonzero(border)) != 0:
            fails.append(f"{tag}: halo of {name} written")
    return fails


def check(ctx, B, snap, ref, tag, compare=None, ignore=()):
    """Outputs `ref` (name -> fp64 / uint8 reference of rows < B) against the engine's buffers;
    everything else against the snapshot.  `compare(name, got, ref64)` replaces torch.equal
    for the real-valued checks; buffers in `ignore` are outputs that are not compared.  Returns
    the list of failures."""
    fails = []
    touched = torch.zeros(ctx.grads.numel(), dtype=torch.bool, device=DEV)
    for name, want in ref.items():
        if name.startswith("g"):
            i = int(name[1:])
            got = ctx.gview(i)
            o = ctx.offsets[i]
            touched[o:o + got.numel()] = True
            if compare is not None:
                fails += compare(name, got.cpu(), want.reshape(got.shape))
            elif not torch.equal(got, want.to(torch.float32).to(DEV).reshape(got.shape)):
                fails.append(f"{tag}: {name} differs from the reference")
            continue
        whole = ctx.whole(name)
        fails += untouched_failures(name, whole, B, snap, tag)
        got = interior(name, whole)[:B]
        if name.startswith("c"):
            if not torch.equal(got, want.to(DEV).reshape(got.shape)):
                fails.append(f"{tag}: codes {name} differ from the reference")
        elif compare is not None:
            fails += compare(name, got.cpu(), want.reshape(got.shape))
        elif not torch.equal(got, want.to(torch.float32).to(DEV).reshape(got.shape)):
            fails.append(f"{tag}: {name} differs from the reference")
    for n in FLOAT_BUFS + CODE_BUFS:
        if n not in ref and n not in ignore and not torch.equal(bits(ctx.whole(n)), snap[n]):
            fails.append(f"{tag}: {n} is not an output and changed")
    g = bits(ctx.grads)
    if not torch.equal(g[~touched], snap["grads"][~touched]):
        fails.append(f"{tag}: a gradient that is not an output changed")
    return fails


def make_real_params():
    """Real-valued parameters: glorot-sized weights, biases with noise of 0.05."""
    flat = torch.zeros(TOTAL_NUMEL)
    init_params_(flat, CANON_OFFSETS, seed=8)
    gen = torch.Generator().manual_seed(12)
    return [p.clone() + (0.05 * torch.randn(p.shape, generator=gen) if p.dim() == 1 else 0)
            for p in param_views(flat, CANON_OFFSETS)]


# ---- an engine of its own, and the cases it runs (tests/test_op_oracle_gpu.py,
# tests/test_dispatch_oracle_gpu.py) -----------------------------------------------------------------
WIDE_INLAUNCH, WIDE_SEPARATE = 1 << 20, 1
ROWS_BIG = 136


class Ctx:
    """An engine of `rows` rows (40 by default) on the parameters `P` (CPU fp32 tensors), and a
    cache of cases."""

    def __init__(self, P, rows=BMAX):
        from ddl_amd.models.hip_engine import HipEngine
        self.P = P
        self.rows = rows
        self.P64 = [p.double() for p in P]
        self.params = torch.zeros(TOTAL_NUMEL, device=DEV)
        self.grads = torch.zeros_like(self.params)
        self.offsets = CANON_OFFSETS
        self.eng = HipEngine(self.params, self.grads, CANON_OFFSETS, batch=rows, graph=False,
                             eval_chunk=rows, keep_prob=KEEP)
        # in place: the engine holds pointers into the flat tensor
        self.params.copy_(torch.cat([p.reshape(-1) for p in P]))
        self.seed_t = torch.tensor([SEED], dtype=torch.int32, device=DEV)
        self.labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
        self.cases = {}

    def e(self):
        return self.eng.eng

    def whole(self, name):
        """The stored buffer, every row of the engine, halo included (re-fetched: set_cfg /
        set_splits reallocate the workspace)."""
        return self.e().buffer(name + "+halo" if name in HALO_BUFS else name, self.rows)

    def gview(self, i):
        return param_views(self.grads, CANON_OFFSETS)[i]

    def poison_grads(self):
        self.grads.fill_(float("nan"))

    def case(self, op, B, train=True, real=False):
        """(inputs, fp64 reference outputs) of op at batch B, computed once: the reference is
        exact, so every config shares it."""
        key = (op, B, train, real)
        if key not in self.cases:
            inp = R.make_inputs(op, B, 1, real)
            self.cases[key] = (inp, R.run_op(op, self.P64, inp, SEED, KEEP, train))
        return self.cases[key]


def run_case(ctx, op, B, tag, train=True):
    inputs, ref = ctx.case(op, B, train)
    x, snap = prepare(ctx, B, inputs)
    ctx.e().run_op(op, x, ctx.seed_t, train)
    torch.cuda.synchronize()
    return check(ctx, B, snap, ref, f"{R.OP_NAMES[op]} B={B} {tag}")


SEGMENT_OPS = {1: (10, 11), 2: (12, 13), 3: (14, 15, 16)}


def segment_case(ctx, s, B):
    """Hand-written integer inputs of segment s and the references of its ops; conv1's weight
    gradient (segment 3) reads the d1 that conv2's data gradient writes."""
    key = ("seg", s, B)
    if key not in ctx.cases:
        inputs, ref = {}, {}
        for op in SEGMENT_OPS[s]:
            if op == 16:
                inp = {"x": R.make_inputs(16, B, 1)["x"], "d1": ref["d1"].to(torch.float32)}
                # exactness of the chained op: its abs-sums (an upper bound of every partial sum)
                # are fp32 integers
                asum = R.abs_sum(16, ctx.P64, inp, KEEP)
                assert max(float(v.max()) for v in asum.values()) < 2 ** 24
                inputs["x"] = inp["x"]
            else:
                inp = R.make_inputs(op, B, 1)
                for k, v in inp.items():
                    inputs.setdefault(k, v)
                inp = {k: inputs[k] for k in inp}
            ref.update(R.run_op(op, ctx.P64, inp, SEED, KEEP, True))
        ctx.cases[key] = (inputs, ref)
    return ctx.cases[key]


def head_inputs(P, B, gen, extreme_rows):
    """h2 rows: ordinary ones, and the rows `extreme_rows` along W3[:, a] - W3[:, b] scaled so
    that their largest |logit| is about 60, labelled with their largest or smallest logit in
    turn."""
    w3, b3 = P[12].double(), P[13].double()
    h2 = (torch.rand(B, 512, generator=gen) * 1.5 - 0.5)
    labels = torch.randperm(max(B, 10), generator=gen)[:B] % 10
    extreme = torch.zeros(B, dtype=torch.bool)
    for i, r in enumerate(extreme_rows):
        a, b = r % 10, (r + 3) % 10
        d = w3[:, a] - w3[:, b]
        h2[r] = (d * (60.0 / float((d @ w3).abs().max()))).float()
        extreme[r] = True
        lg = h2[r].double() @ w3 + b3
        assert 50 < float(lg.abs().max()) < 70
        if i % 3 == 0:
            labels[r] = int(lg.argmax())
        elif i % 3 == 1:
            labels[r] = int(lg.argmin())
    return h2, labels, extreme
