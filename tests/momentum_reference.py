"""The yardstick of the momentum / plain-SGD tests: the fp64 closed form of common.h momentum1,

    m' = mu * m + scale * g,    w' = w - lr * m'        (mu = 0: plain SGD, m' = scale * g)

over k steps.  tests/test_momentum_reference_cpu.py pins it against ParameterServer's pure-torch
branches; tests/test_momentum_tail_gpu.py measures the HIP kernels against it."""
import torch


def momentum_closed_form(w, m, grads, lr, mu, scale=1.0):
    """(w_k, m_k) in fp64 after one step per gradient in `grads`, from fp32 (or fp64) w, m."""
    w, m = w.detach().double().cpu().clone(), m.detach().double().cpu().clone()
    for g in grads:
        m = mu * m + scale * g.detach().double().cpu()
        w = w - lr * m
    return w, m
