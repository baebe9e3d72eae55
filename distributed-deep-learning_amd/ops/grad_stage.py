"""What a step does to its worker's whole gradient before anything consumes it: the Python twin of
``GradStage`` in ``csrc/kernels/api.h``.

One object per trainer holds the clip triple ``(max_norm, ranges, out)``, the accumulation triple
``(K, ranges, acc)`` and the count of micro-batches accumulated in the open step (as
``AccumSite::done`` does).  An exchange whose step runs in a native runner hands the triples over
(``attach``); one whose step the host drives calls ``after_micro`` after every backward and
``finish`` after the step's last, which run the CPU twin (``ops/accum.py``, ``ops/clip.py``) or the
native op (``accum.hip``, ``clip.hip``) by where the gradient buffer lives.
"""
from __future__ import annotations

from . import accum as accum_ops
from . import clip as clip_ops
from . import native


class GradStage:
    def __init__(self, clip=None, accum=None):
        self.clip = clip      # (max_norm, [(lo, n)] payload ranges, the {norm, coef} buffer)
        self.accum = accum    # (K, [(lo, n)] payload ranges, the accumulator)
        self.done = 0         # micro-batches accumulated so far in the open step

    @property
    def whole(self) -> bool:
        """The backward runs whole: nothing is handed over per segment."""
        return self.clip is not None or self.accum is not None

    def attach(self, runner) -> None:
        """A native runner clips and accumulates itself."""
        if self.clip is not None:
            runner.set_clip(*self.clip)
        if self.accum is not None:
            runner.set_accum(*self.accum)

    def after_micro(self, grads) -> None:
        """The accumulation pass after a micro-batch: the sum into the accumulator, after the
        step's last one the mean into ``grads``."""
        if self.accum is None:
            return
        k, ranges, acc = self.accum
        mode = accum_ops.mode_of(self.done, k)
        self.done = (self.done + 1) % k
        if grads.is_cuda:
            native.ops().accum_grads(grads, acc, ranges, mode, k)
        else:
            accum_ops.accum_grads_(grads, acc, ranges, mode, k)

    def finish(self, grads) -> None:
        """After the step's last micro-batch: clip ``grads`` in place; the norm and the
        coefficient stay in the clip triple's buffer."""
        if self.clip is None:
            return
        max_norm, ranges, out = self.clip
        if grads.is_cuda:
            native.ops().clip_grads(grads, ranges, max_norm, out)
        else:
            out[0], out[1] = clip_ops.clip_grads_(grads, ranges, max_norm)
