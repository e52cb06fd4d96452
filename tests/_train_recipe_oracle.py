"""float64 restatement of `train`'s recipe — the yardstick of po_train.hip's grad_axpy_kernel,
grad_sqsum_kernel + grad_norm_final_kernel and adamw_apply_kernel: the weighted sum of micro-batch gradients, the global
L2 norm (an exactly rounded sum of exact squares), tf.clip_by_global_norm's rule, and AdamW = _train_oracle.adam's update
(Keras Adam) on the clipped gradient plus the decoupled decay lr · weight_decay · p.  A gradient whose norm is not finite
skips the step: parameters, m, v and t stay."""
import math

import numpy as np


def accumulate(grads, weights):
    """sum_j weights[j] · grads[j] in float64"""
    out = np.zeros(np.asarray(grads[0]).shape, dtype=np.float64)
    for g, w in zip(grads, weights):
        out += float(w) * np.asarray(g, dtype=np.float64)
    return out


def global_norm(g):
    """sqrt of the exactly rounded sum of the squares (each square of a float32 is exact in float64)"""
    sq = np.asarray(g, dtype=np.float64).ravel() ** 2
    return math.sqrt(math.fsum(sq)) if np.all(np.isfinite(sq)) else float(np.sqrt(np.sum(sq)))


def clip_scale(norm, clip_norm):
    return clip_norm / norm if clip_norm > 0 and norm > clip_norm else 1.0


class AdamW:
    """p, m, v (float64) and t; step(g, lr) is one optimizer step and returns (norm, applied)"""

    def __init__(self, p, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.0, clip_norm=0.0, m=None, v=None, t=0):
        self.p = np.asarray(p, dtype=np.float64).copy()
        self.m = np.zeros_like(self.p) if m is None else np.asarray(m, dtype=np.float64).copy()
        self.v = np.zeros_like(self.p) if v is None else np.asarray(v, dtype=np.float64).copy()
        self.t = int(t)
        self.beta1, self.beta2, self.eps, self.weight_decay, self.clip_norm = beta1, beta2, eps, weight_decay, clip_norm

    def step(self, g, lr):
        g = np.asarray(g, dtype=np.float64)
        norm = global_norm(g)
        if not math.isfinite(norm):
            return norm, False
        g = g * clip_scale(norm, self.clip_norm)
        self.t += 1
        t, p0 = self.t, self.p.copy()
        # _train_oracle.adam's three lines
        self.m += (g - self.m) * (1 - self.beta1)
        self.v += (g * g - self.v) * (1 - self.beta2)
        self.p -= lr * np.sqrt(1 - self.beta2 ** t) / (1 - self.beta1 ** t) * self.m / (np.sqrt(self.v) + self.eps)
        self.p -= lr * self.weight_decay * p0
        return norm, True


def adamw(p, grads, lrs, **kw):
    """p after one step per gradient (lrs: one rate, or one per step)"""
    o = AdamW(p, **kw)
    lrs = [lrs] * len(grads) if np.isscalar(lrs) else lrs
    for g, lr in zip(grads, lrs):
        o.step(g, lr)
    return o.p
