"""float64 numpy restatement of one optimizer step as torch.optim defines it (SGD, Adam, AdamW) and of ModelEMA's update (reference:
train.py:228-233, metayolo/common.py:128-155).  Pure functions, no torch: tests/test_optim_ref_host.py holds them against torch.optim on
float64 CPU tensors, tests/test_gpu_optim.py holds hd_yolo_amd.optim (csrc/optim.hip, hdy_opt_step) against them."""
import math

import numpy as np


def _f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """-> (p, momentum buffer or None).  buf None with momentum != 0: the first step, torch starts the buffer as a copy of g'."""
    p, g, buf = _f64(p), _f64(g), _f64(buf)
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.copy() if buf is None else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    else:
        buf = None
    return p - lr * g, buf


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
    """-> (p, exp_avg, exp_avg_sq).  step = this step's count (1 on the first); m, v None = zeros.  decoupled: AdamW."""
    p, g = _f64(p), _f64(g)
    m = np.zeros_like(p) if m is None else _f64(m)
    v = np.zeros_like(p) if v is None else _f64(v)
    beta1, beta2 = betas
    if weight_decay != 0:
        if decoupled:
            p = p * (1 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m = m + (g - m) * (1 - beta1)
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return p - (lr / bc1) * m / (np.sqrt(v) / bc2 ** 0.5 + eps), m, v


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    return adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled=True)


def ema_decay(updates, decay=0.9999):
    """ModelEMA.decay"""
    return decay * (1 - math.exp(-updates / 2000))


def ema_step(ema, p, d):
    return d * _f64(ema) + (1 - d) * _f64(p)
