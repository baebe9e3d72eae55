"""The yardstick of the update-modifier tests: the fp64 closed form of every variant of the update
rule (csrc/kernels/update.h) over k steps,

    w  <- w - lr * wd * w                                  (decoupled weight decay, if wd > 0:
                                                            the plain lr under Adam too)
    Adam:      m' = m + (1 - b1) (s g - m),   v' = v + (1 - b2) ((s g)^2 - v)
               w' = w - lr_t m' / (sqrt(v') + eps),   lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
    momentum:  m' = mu m + s g,   w' = w - lr u,   u = mu m' + s g (Nesterov) or m'

with s the gradient scale and t = t0 + 1, t0 + 2, ... the step.  mu = 0 is plain SGD.

tests/test_update_modifiers_cpu.py pins it against torch.optim.AdamW / SGD(nesterov=True) and
against ParameterServer's pure-torch branches; tests/test_update_modifiers_gpu.py measures the HIP
kernels against it."""
import math

import torch


def _d(x):
    return x.detach().double().cpu().clone()


def adam_step_size(lr, b1, b2, t):
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def update_closed_form(kind, w, m, v, grads, lr, *, b1=0.9, b2=0.999, eps=1e-8, mu=0.9,
                       weight_decay=0.0, nesterov=False, scale=1.0, t0=0):
    """(w_k, m_k, v_k) in fp64 after one step per gradient in `grads`, from fp32 (or fp64) w, m,
    v at step t0.  kind: "adam" or "momentum"; v is passed through under momentum (may be None)."""
    assert kind in ("adam", "momentum")
    assert not nesterov or kind == "momentum"
    w, m = _d(w), _d(m)
    v = _d(v) if v is not None else None
    for k, g in enumerate(grads):
        gs = scale * _d(g)
        if weight_decay:
            w = w - (lr * weight_decay) * w
        if kind == "adam":
            m = m + (1.0 - b1) * (gs - m)
            v = v + (1.0 - b2) * (gs * gs - v)
            w = w - adam_step_size(lr, b1, b2, t0 + k + 1) * m / (v.sqrt() + eps)
        else:
            m = mu * m + gs
            w = w - lr * ((mu * m + gs) if nesterov else m)
    return w, m, v
