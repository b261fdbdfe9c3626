"""Restatement of decoupled weight decay (tnt_adamw_ring_f32 / tnt_sgdw_f32 / tnt_dense_dw_adamw_f32, definition in
include/tnt_hip.h) in float64, written from the header text on top of the existing oracle updates (oracle.ops.adam_update,
sgd_momentum_update) and not on a second copy of Adam:

    theta' = (theta - (lr * wd) * theta) - step  =  plain_update(theta) - (lr * wd) * theta      (equal up to one float64 ulp)

``AdamWState`` is the model-level oracle optimizer with a per-variable decay, ``WeightDecayMockBackend`` a MockBackend with
the decaying ops: each runs the plain mock op and then takes the decay of the theta the step started from."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import MockBackend, flat


def adamw_update(theta, m, v, g, t, lr, wd, b1=0.9, b2=0.98, eps=1e-8):
    """oracle.ops.adam_update followed by the decay of the theta the gradient was taken at; wd scalar or array"""
    th, m1, v1 = O.adam_update(theta, m, v, g, t, lr, b1, b2, eps)
    return th - (lr * wd) * theta, m1, v1


def sgdw_update(theta, mom, g, lr, wd, momentum=0.9):
    th, mo = O.sgd_momentum_update(theta, mom, g, lr, momentum)
    return th - (lr * wd) * theta, mo


def decay_of(names, wd, exact=(), substrings=()):
    """keras's rule as a dict name -> decay: every variable decays unless it is named exactly or contains a substring"""
    return {n: (0.0 if (n in exact or any(s in n for s in substrings)) else float(wd)) for n in names}


class AdamWState(M.AdamState):
    """oracle.models.AdamState plus a decay per variable name (``wd``: dict; a missing name does not decay).  ``lr`` may
    be reassigned between steps (a schedule's value): the decay of a step uses the same ``lr`` as its Adam update."""

    def __init__(self, params, wd, **kw):
        super().__init__(params, **kw)
        self.wd = dict(wd)

    def apply(self, params, grads, sparse_norms=None):
        old = {k: params[k].copy() for k, g in grads.items() if g is not None}
        super().apply(params, grads, sparse_norms)
        for k, w in old.items():
            params[k] = params[k] - (self.lr * self.wd.get(k, 0.0)) * w


class SGDWState:
    """keras SGD(lr, momentum, clipnorm, weight_decay) with the interface of oracle.models.AdamState: per-variable clip
    (oracle.ops.clip_by_norm's rule, the IndexedSlices norm where given), oracle.ops.sgd_momentum_update, then the decay"""

    def __init__(self, params, wd, lr=1e-2, momentum=0.9, clipnorm=None):
        self.lr, self.momentum, self.clipnorm, self.wd = lr, momentum, clipnorm, dict(wd)
        self.t = 0
        self.mom = {k: np.zeros_like(v) for k, v in params.items()}

    def apply(self, params, grads, sparse_norms=None):
        self.t += 1
        for k, g in grads.items():
            if g is None:
                continue
            if self.clipnorm is not None:
                n = np.sqrt((g * g).sum())
                if sparse_norms is not None and k in sparse_norms:
                    n = sparse_norms[k]
                g = g * self.clipnorm / np.maximum(n, self.clipnorm)
            params[k], self.mom[k] = sgdw_update(params[k], self.mom[k], g, self.lr, self.wd.get(k, 0.0), self.momentum)


class WeightDecayMockBackend(MockBackend):
    """MockBackend plus tnt_adamw_ring_f32, tnt_sgdw_f32 and tnt_dense_dw_adamw_f32 from the header text; ``wd_calls`` logs
    the name, the learning rate each call read and the decays it was given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.wd_calls = []

    @staticmethod
    def _tripped(guard):
        return guard is not None and int(guard[0]) != 0

    def _decay_spans(self, theta, before, span_seg, span_off, span_len, nspan, lr, seg_wd):
        th, wd = flat(theta), flat(seg_wd)
        for s, o, n in self._segs(span_seg, span_off, span_len, nspan):
            th[o:o + n] = th[o:o + n].astype(np.float64) - (lr * float(wd[s])) * before[o:o + n]

    def adamw(self, theta, m, v, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr_t, lr_t_dev, beta1, beta2,
              eps, clipnorm, lr, seg_wd, guard=None, met=None, ring=None, ring_t=None):
        assert lr is not None and seg_wd is not None and lr.element_size() == 4 and seg_wd.dtype == lr.dtype
        before = flat(theta).astype(np.float64)
        MockBackend.adam(self, theta, m, v, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr_t, lr_t_dev,
                         beta1, beta2, eps, clipnorm, guard=guard, met=met, ring=ring, ring_t=ring_t)
        if self._tripped(guard):
            return
        rate = float(flat(lr)[0])
        self.wd_calls.append(dict(name="adamw", lr=rate, wd=flat(seg_wd).tolist()))
        self._decay_spans(theta, before, span_seg, span_off, span_len, nspan, rate, seg_wd)

    def sgdw(self, theta, mom, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr_dev, momentum, clipnorm,
             seg_wd, guard=None):
        assert lr_dev is not None and seg_wd is not None
        before = flat(theta).astype(np.float64)
        MockBackend.sgd(self, theta, mom, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, 0.0, lr_dev,
                        momentum, clipnorm, guard=guard)
        if self._tripped(guard):
            return
        rate = float(flat(lr_dev)[0])
        self.wd_calls.append(dict(name="sgdw", lr=rate, wd=flat(seg_wd).tolist()))
        self._decay_spans(theta, before, span_seg, span_off, span_len, nspan, rate, seg_wd)

    def dense_dw_adamw(self, x, dpre, theta, m, v, l2, sq, sq_override, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk, ldx, lr,
                       wd, guard=None):
        assert lr is not None and isinstance(wd, float) and 0.0 <= wd < float("inf")
        n = N * E
        before = flat(theta)[:n].astype(np.float64)
        MockBackend.dense_dw_adam(self, x, dpre, theta, m, v, l2, sq, sq_override, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk,
                                  ldx, guard=guard)
        if self._tripped(guard):
            return
        rate = float(flat(lr)[0])
        self.wd_calls.append(dict(name="dense_dw_adamw", lr=rate, wd=[wd]))
        th = flat(theta)
        th[:n] = th[:n].astype(np.float64) - (rate * wd) * before
