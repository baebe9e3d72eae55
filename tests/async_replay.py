"""Replay of an asynchronous parameter-server run from its recorded apply orders.

An asynchronous run at W > 1 is not deterministic: which worker's push a PS serves next depends
on timing.  But the run has only three rules, and together they make the per-PS apply orders the
ONLY free choice:

1. each PS applies its pushes serially, one update of its own state (parameters, m, v, and the
   step counter t that sets the Adam step size) per push;
2. an apply stores the shard it has just produced into the pushing worker's buffer, and nowhere
   else;
3. a worker computes the gradient of its step s + 1 only once every PS has applied its step s
   (staleness of one round: the blocking pull).

Given, for every PS, the list of (worker, step) in the order it applied them, every bit of every
buffer follows.  The services log exactly that with ``check_provenance=True``, as
``(worker, ps, step, t)``; ``apply_orders`` turns the logs into the orders (refusing logs that
cannot be a run) and ``replay`` runs the three rules as an event-driven simulation, with the
gradient and the update rule supplied by the caller.

Plain Python: this module imports nothing (no engine, no extension, no torch).  The buffers it
moves are the caller's (torch tensors on any device: ``clone``, ``new_zeros``, slices and
``copy_`` are all it uses).
"""


class ReplayError(ValueError):
    """The recorded log or order cannot be the record of an asynchronous PS run."""


def _host_of(hosts, p):
    if hosts is None:
        return None
    return hosts[p]


def apply_orders(recs, world, steps, hosts=None, t0=0):
    """{ps: [(worker, step), ...]} in apply order, i.e. by t = t0 + 1 .. t0 + world * steps.

    ``recs`` is the union of the ranks' provenance logs, entries ``(worker, ps, step, t)`` with t
    the PS's step counter AFTER that apply.  ``t0`` is the counter every PS started from (an int,
    or {ps: int}).

    The xGMI service (csrc/kernels/xgmi_async.hip AsyncService::serve) logs every apply, the
    host's own included.  The Python ``AsyncExchange`` (parallel/comm.py) logs only REMOTE pushes:
    the host's worker thread applies its own push under the PS lock without a log entry.  For
    such a log pass ``hosts`` ({ps: rank} or a list): the t values missing from PS p's log are
    then the pushes of worker hosts[p], and because a worker pushes its steps in order they are
    its steps 0, 1, ... in increasing t.  That reconstruction is only made when the log of that
    PS holds no entry of the host at all and exactly ``steps`` values are missing; with
    ``hosts`` given the PS set is ``range(len(hosts))`` (a PS whose every push is local has no
    log entry), otherwise it is the set of PS named in the log.

    Refused (ReplayError naming the PS): a duplicate t, a t outside the run, a missing t that
    cannot be the host's, and a (worker, ps) whose steps are not 0 .. steps - 1 in order.
    """
    recs = [tuple(int(x) for x in r) for r in recs]
    if hosts is not None:
        ps_ids = sorted(hosts) if isinstance(hosts, dict) else list(range(len(hosts)))
    else:
        ps_ids = sorted({p for (_, p, _, _) in recs})
    known = set(ps_ids)
    for (_, p, _, _) in recs:
        if p not in known:
            raise ReplayError(f"PS {p}: logged, but not a PS of this run")
    out = {}
    for p in ps_ids:
        base = t0[p] if isinstance(t0, dict) else t0
        first, last = base + 1, base + world * steps
        by_t = {}
        for (w, pp, s, t) in recs:
            if pp != p:
                continue
            if t in by_t:
                raise ReplayError(f"PS {p}: t = {t} logged twice, for (worker, step) {by_t[t]} "
                                  f"and {(w, s)}")
            if not first <= t <= last:
                raise ReplayError(f"PS {p}: t = {t} outside this run's {first} .. {last}")
            if not 0 <= w < world:
                raise ReplayError(f"PS {p}: worker {w} of a world of {world}")
            by_t[t] = (w, s)
        missing = [t for t in range(first, last + 1) if t not in by_t]
        if missing:
            h = _host_of(hosts, p)
            logged_host = h is not None and any(w == h for (w, _) in by_t.values())
            if h is None or logged_host or len(missing) != steps:
                why = ("no host given" if h is None else
                       f"host {h} is logged too" if logged_host else
                       f"{len(missing)} missing, the host pushes {steps}")
                raise ReplayError(f"PS {p}: no apply logged for t = {missing[:6]}"
                                  f"{' ...' if len(missing) > 6 else ''} and they cannot be "
                                  f"the host's own pushes ({why})")
            for s, t in enumerate(missing):  # the host's pushes, in step order
                by_t[t] = (h, s)
        order = [by_t[t] for t in range(first, last + 1)]
        for w in range(world):
            got = [s for (ww, s) in order if ww == w]
            if got != list(range(steps)):
                raise ReplayError(f"PS {p}: worker {w}'s steps are applied as {got}, not "
                                  f"0 .. {steps - 1} in order")
        out[p] = order
    return out


class PSState:
    """One PS's state: its private copy of its shard, the optimizer slots and the counter."""

    def __init__(self, w, t=0):
        self.w = w
        self.m = w.new_zeros(w.shape)
        self.v = w.new_zeros(w.shape)
        self.t = t

    def astuple(self):
        return self.w, self.m, self.v, self.t


def replay(order, ranges, init, world, steps, grad_fn, update_fn, t0=0):
    """Run the recorded per-PS apply ``order`` ({ps: [(worker, step), ...]}) from ``init``.

    ``ranges[p]`` is PS p's [lo, hi) of the flat buffer; every worker's buffer and every PS's
    private copy start as ``init`` (m and v as zeros, t as ``t0``).

    * worker r computes ``grad_fn(r, s, params_r)`` (a NEW flat buffer: the replay keeps it
      until every PS has applied it) once every PS has applied its step s - 1;
    * PS p applies its next logged (w, s) once worker w's step-s gradient exists:
      ``update_fn(p, state_p, g[lo:hi], t)`` with t the PS's own counter after this apply
      updates ``state_p.w / .m / .v`` in place, then the new shard is copied into
      ``params_w[lo:hi]``.

    Returns ``(params, states)``: every worker's final buffer, and {ps: (w, m, v, t)}.

    If a pass over all workers and PS makes no progress before the orders are exhausted, the
    order is not realisable under the one-round staleness rule: ReplayError names the PS and the
    entry at which it stopped.
    """
    ps_ids = sorted(order)
    rng = {p: (int(ranges[p][0]), int(ranges[p][1])) for p in ps_ids}
    for p in ps_ids:
        if len(order[p]) != world * steps:
            raise ReplayError(f"PS {p}: {len(order[p])} applies recorded, the run has "
                              f"{world * steps}")
    params = [init.clone() for _ in range(world)]
    state = {p: PSState(init[rng[p][0]:rng[p][1]].clone(),
                        t0[p] if isinstance(t0, dict) else t0) for p in ps_ids}
    pos = {p: 0 for p in ps_ids}                       # next entry of PS p's order
    applied = {p: [0] * world for p in ps_ids}         # applies of worker w's pushes at PS p
    grad = [None] * world                              # worker r's gradient in flight
    grad_step = [-1] * world                           # ... and the step it belongs to
    while True:
        progress = False
        for r in range(world):
            s = grad_step[r] + 1
            if s < steps and all(applied[p][r] >= s for p in ps_ids):
                grad[r] = grad_fn(r, s, params[r])
                grad_step[r] = s
                progress = True
        for p in ps_ids:
            lo, hi = rng[p]
            while pos[p] < len(order[p]):
                w, s = order[p][pos[p]]
                if not (0 <= w < world and 0 <= s < steps):
                    raise ReplayError(f"PS {p}: entry {pos[p]} = (worker {w}, step {s}) is not "
                                      f"of this run")
                if applied[p][w] != s:
                    raise ReplayError(f"PS {p}: entry {pos[p]} = (worker {w}, step {s}) out of "
                                      f"that worker's step order (its step {applied[p][w]} is "
                                      f"next here)")
                if grad_step[w] != s:
                    break  # that gradient does not exist yet
                st = state[p]
                st.t += 1
                update_fn(p, st, grad[w][lo:hi], st.t)
                params[w][lo:hi].copy_(st.w)
                applied[p][w] += 1
                pos[p] += 1
                progress = True
        if all(pos[p] == len(order[p]) for p in ps_ids):
            break
        if not progress:
            stuck = [p for p in ps_ids if pos[p] < len(order[p])]
            p = stuck[0]
            w, s = order[p][pos[p]]
            raise ReplayError(
                f"PS {p}: stopped at entry {pos[p]} = (worker {w}, step {s}): that gradient "
                f"needs every PS to have applied the worker's step {s - 1} first, and the "
                f"recorded orders of PS {stuck} wait for each other (not realisable with one "
                f"round of staleness)")
    return params, {p: state[p].astuple() for p in ps_ids}


def adjacent_swaps(order):
    """Every order that differs from ``order`` by two adjacent applies of DIFFERENT workers
    swapped in one PS, as (ps, index, order).  Not all of them are realisable."""
    for p in sorted(order):
        od = order[p]
        for i in range(len(od) - 1):
            if od[i][0] != od[i + 1][0]:
                sw = dict(order)
                sw[p] = od[:i] + [od[i + 1], od[i]] + od[i + 2:]
                yield p, i, sw


def order_string(order_p):
    """One PS's order as its workers' digits, e.g. '021020202012111'."""
    return "".join(str(w) if w < 10 else f"[{w}]" for (w, _) in order_p)


def staleness_exercised(order, steps):
    """True if some PS served one worker twice in a row while another worker still had pushes
    outstanding at that PS: worker a's pushes of two successive steps applied with none of
    worker b's in between, although b had not finished.  "In a row" is relative to b: with three
    workers a third one's applies may fall in between (the order 021020202012111 serves worker
    0 four times between two pushes of worker 1, never twice back to back); with two workers it
    is the literal reading."""
    for p, od in order.items():
        workers = sorted({w for (w, _) in od})
        left = {w: steps for w in workers}
        # since[a][b]: applies of a since b's last apply (or the start)
        since = {a: {b: 0 for b in workers if b != a} for a in workers}
        for (w, _) in od:
            left[w] -= 1
            for b in since[w]:
                since[w][b] += 1
                if since[w][b] >= 2 and left[b] > 0:
                    return True
            for a in workers:
                if a != w:
                    since[a][w] = 0
    return False


def mismatch_report(what, got, want, spans):
    """Lines describing where flat buffer ``got`` differs from ``want``: per span
    ``(lo, hi, label)`` the first differing index, and the largest |difference|.  Empty if the
    bits agree."""
    lines = []
    for lo, hi, label in spans:
        a, b = got[lo:hi], want[lo:hi]
        ne = a != b
        if not bool(ne.any()):
            continue
        i = int(ne.nonzero()[0]) + lo
        d = float((a.double() - b.double()).abs().max())
        lines.append(f"{what}: {label} [{lo}, {hi}): {int(ne.sum())} elements differ, first at "
                     f"{i}, max |diff| {d:.3e}")
    return lines
