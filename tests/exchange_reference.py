"""The yardstick of the exchange-kernel tests (tests/test_exchange_kernels_gpu.py), plain torch on
the CPU: what one round of the xGMI exchange kernels (csrc/kernels/xgmi.hip, xgmi_async.hip) must
compute, and the gradients, geometries and sentinels those tests use.

* ``rank_order_sum``: the fp32 sum the three synchronous kernels document: from 0, add rank q's
  contribution for q = 0..W-1, each first multiplied by ``coef`` in a separate fp32 multiply
  (``coef == 1``: the raw value).
* ``rule_step``: one step of an update rule (update.h) in fp64: TF1 Adam as test_adam_kernel
  writes it, momentum / SGD from tests/momentum_reference.py, copy ``w := g``.
* ``sync_round`` / ``async_round``: one round over every rank's parameters and optimizer state.

tests/test_exchange_reference_cpu.py pins this file against parallel/ps.py's pure-torch branch
and checks that the fixed gradients can tell the summation orders apart."""
import math

import torch

from momentum_reference import momentum_closed_form

ADAM, MOMENTUM, COPY = 0, 1, 2  # update.h UpdKind
B1, B2, EPS = 0.9, 0.999, 1e-8
LR = {ADAM: 1e-3, MOMENTUM: 3e-2, COPY: 0.0}
# fixed for the sensitivity argument of test_exchange_reference_cpu.py
GRAD_SEED, GRAD_MAG, COEF3 = 20240, 1e-2, 1.0 / 3.0
N_BUF = 20480  # floats in every params / grads buffer of the GPU tests


def step_size(kind, t):
    """The kernels' `step` at the PS's step t (1-based): TF1 Adam's lr_t, or the learning rate."""
    if kind == ADAM:
        return LR[ADAM] * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
    return LR[kind]


def round_gradients(world, epoch, n=N_BUF, integer=False):
    """Every rank's gradient buffer of round `epoch` (fp32, [n] each), the same on every caller.
    integer: small whole numbers, whose sums and copies are exact."""
    gen = torch.Generator().manual_seed(GRAD_SEED + 1000 * epoch + world)
    if integer:
        return [torch.randint(-64, 65, (n,), generator=gen).float() for _ in range(world)]
    return [torch.randn(n, generator=gen) * GRAD_MAG for _ in range(world)]



def initial_state(n, seed):
    """(w, m, v) of test_adam_kernel's magnitudes; non-zero m and v, so a wrong state offset shows."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-3,
            torch.rand(n, generator=gen) * 1e-4)


def sentinel(n, base):
    """A finite pattern for everything a kernel must not touch (a stray update of NaN would stay
    NaN and hide itself)."""
    return (torch.arange(n) % 97).float() * 0.25 + float(base)


def scaled(g, coef):
    """g * coef as the push kernels form it: one fp32 multiply, skipped when coef == 1."""
    c = torch.tensor(coef, dtype=torch.float32)
    return g if float(c) == 1.0 else g * c


def rank_order_sum(grads_by_rank, coef=1.0):
    acc = torch.zeros_like(grads_by_rank[0])
    for g in grads_by_rank:
        assert g.dtype == torch.float32
        acc = acc + scaled(g, coef)
    return acc


def rule_step(kind, w, m, v, g, step, mu=0.0, scale=1.0, b1=B1, b2=B2, eps=EPS):
    """(w', m', v') in fp64 after one step from fp32 (or fp64) w, m, v, g; m / v pass through
    where the rule has none.  b1, b2, eps: Adam's, by default the decimal values."""
    d = lambda t: None if t is None else t.detach().double().cpu()  # noqa: E731
    w, m, v, g = d(w), d(m), d(v), d(g)
    if kind == COPY:
        return g.clone(), m, v
    if kind == MOMENTUM:
        w2, m2 = momentum_closed_form(w, m, [g], step, mu, scale)
        return w2, m2, v
    gs = g * scale
    m2 = m + (gs - m) * (1 - b1)
    v2 = v + (gs * gs - v) * (1 - b2)
    return w - step * m2 / (v2.sqrt() + eps), m2, v2


# ---- geometry: the host arithmetic of xgmi_plan.h (PeerExchange, AsyncPeer) ---------------------
def equal_slices(c, max_slices=128, per_wg=1024):
    """Float4 counts of the workgroup slices of a chunk of c floats."""
    ns = max(1, min((c + per_wg - 1) // per_wg, max_slices))
    sl = ((c + ns - 1) // ns + 3) & ~3
    return [(min(c, s + sl) - s) // 4 for s in range(0, c, sl)]


def async_slices(n, max_slices=512):
    return equal_slices(n, max_slices, 2048)


def owner_slices(runs, max_slices=128):
    """(float4 counts of all slices, first slice of each run and the total)."""
    n = sum(runs)
    ns = max(len(runs), min((n + 1023) // 1024, max_slices))
    per = ((n + ns - 1) // ns + 3) & ~3
    out, first = [], []
    for rn in runs:
        first.append(len(out))
        out += [(min(rn, s + per) - s) // 4 for s in range(0, rn, per)]
    return out, first + [len(out)]


def bucket_regions(bucket, world, repl):
    """Per rank, the (plan lo, n, state offset) spans whose update that rank computes.
    bucket: ("equal", lo, hi, state_off) or ("owner", [(lo, hi)], state_offs, owner)."""
    if bucket[0] == "owner":
        _, runs, soffs, owner = bucket
        return [[(lo, hi - lo, so) for (lo, hi), so in zip(runs, soffs)] if r == owner else []
                for r in range(world)]
    _, lo, hi, so = bucket
    if repl:
        return [[(lo, hi - lo, so)] for _ in range(world)]
    c = (hi - lo) // world
    return [[(lo + r * c, c, so)] for r in range(world)]


def sync_round(params, m, v, grads, regions, repl, kind, step, mu=0.0, scale=1.0, coef=1.0):
    """One round of one bucket.  params, m, v, grads: per rank (m[r] / v[r]: rank r's state buffer
    of the bucket, or None).  Every rank updates its `regions` from the rank-order sum with its
    own parameters and state, and every rank receives the result (the replicated bucket: each
    rank keeps its own).  Returns fp64 (params', m', v') per rank."""
    world = len(params)
    g = rank_order_sum(grads, coef)
    d = lambda t: None if t is None else t.detach().double().cpu().clone()  # noqa: E731
    P, M, V = [d(p) for p in params], [d(x) for x in m], [d(x) for x in v]
    for r in range(world):
        for lo, n, so in regions[r]:
            w2, m2, v2 = rule_step(kind, params[r][lo:lo + n],
                                   None if m[r] is None else m[r][so:so + n],
                                   None if v[r] is None else v[r][so:so + n],
                                   g[lo:lo + n], step, mu, scale)
            if kind != COPY:
                M[r][so:so + n] = m2
            if kind == ADAM:
                V[r][so:so + n] = v2
            for q in ([r] if repl else range(world)):
                P[q][lo:lo + n] = w2
    return P, M, V


def async_round(ps, grads, shards, kind, t0, mu=0.0, scale=1.0, coef=1.0):
    """One asynchronous round.  ps[p] = (w, m, v): PS p's private copy and state of its shard;
    shards[p] = (lo, n, host); t0[p]: applies PS p has done.  A PS applies worker 0..W-1 in that
    order, each one step of its own counter from that worker's (scaled) gradient, and worker w
    receives the copy as it stands after its own apply.
    Returns (after, workers): after[p][w] = fp64 (w, m, v) of PS p after worker w's apply, and
    workers[w][p] = the shard worker w holds at the end of the round (= after[p][w][0])."""
    world = len(grads)
    after = []
    for p, (lo, n, _) in enumerate(shards):
        w, m, v = ps[p]
        hist = []
        for q in range(world):
            w, m, v = rule_step(kind, w, m, v, scaled(grads[q][lo:lo + n], coef),
                                step_size(kind, t0[p] + q + 1), mu, scale)
            hist.append((w, m, v))
        after.append(hist)
    workers = [[after[p][q][0] for p in range(len(shards))] for q in range(world)]
    return after, workers
