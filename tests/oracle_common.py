"""Shared by the GPU oracle tests (helper module, not a conftest): the poison / snapshot / check
cycle around one engine call, on any object `ctx` that offers

* ``ctx.whole(name)``: the stored buffer, every row the context covers, halo included;
* ``ctx.grads`` and ``ctx.offsets``: the flat gradient buffer and its 14 tensor offsets;
* ``ctx.gview(i)``: gradient tensor i, shaped;
* ``ctx.poison_grads()``: NaN into every gradient element a kernel may write.

tests/test_op_oracle_gpu.py runs it around one op on a 40-row and on a 136-row engine,
tests/test_step_audit_gpu.py
around a whole training step of a Trainer's engine.
"""
import torch

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
