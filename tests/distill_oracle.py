"""Restatement of the distillation head (tnt_softmax_cce_distill_f32, definition in include/tnt_hip.h) in float64: a
per-row ``reference`` straight from the definition -- plain softmaxes and np.log, not the kernel's rearranged kl -- with
the quantities the GPU test's error model reads, a float32 twin, a MockBackend with the op, ``distill_metrics`` (the loss
/ kl / accuracy a step reports, from the oracle models' own probabilities) and ``distilled(...)``, which substitutes
oracle.ops.cce_softmax_bwd -- the one loss step of the float64 oracle models that receives the whole (B, T) ids -- by the
distilled gradient for the duration of a ``with`` block."""
import contextlib
import math

import numpy as np

from oracle import ops as O
from mock_backend import MockBackend, flat, mat

LO, HI = O.CCE_EPS, 1 - O.CCE_EPS


def _softmax_log(z):
    """(softmax(z), log softmax(z)) of the rows of z, the log taken from the logits"""
    d = z - z.max(-1, keepdims=True)
    e = np.exp(d)
    Z = e.sum(-1, keepdims=True)
    return e / Z, d - np.log(Z)


def reference(x, u, y, alpha, t, gscale, dtype=np.float64):
    """the definition, per row, for student logits x and teacher logits u (rows, V), target ids y, alpha in [0, 1],
    temperature t > 0.  Returns loss, kl, corr, grad and the intermediates a bound needs: p, pt, qt, dx = x - max x,
    du = u - max u, ce, my, py, logZ1 / logZt / logZu, amax"""
    f = dtype
    x, u = np.asarray(x).astype(f), np.asarray(u).astype(f)
    alpha, t, gscale = f(alpha), f(t), f(gscale)
    rows, V = x.shape
    y = np.asarray(y, np.int64).reshape(-1)
    ok = (y >= 0) & (y < V)
    dx, du = x - x.max(1, keepdims=True), u - u.max(1, keepdims=True)
    p, _ = _softmax_log(x)
    pt, lpt = _softmax_log(x / t)
    qt, lqt = _softmax_log(u / t)
    with np.errstate(invalid="ignore"):
        kl = np.where(qt > 0, qt * (lqt - lpt), f(0)).sum(1)
    py = np.where(ok, p[np.arange(rows), np.where(ok, y, 0)], f(0))
    my = (ok & (py >= f(LO)) & (py <= f(HI))).astype(f)
    ce = -np.log(np.clip(py, f(LO), f(HI)))
    oh = np.zeros_like(p)
    oh[np.arange(rows)[ok], y[ok]] = 1
    hard = ((1 - alpha) * my)[:, None] * (p - oh)
    soft = alpha * t * (pt - qt)
    ref = dict(y=y, ok=ok, p=p, pt=pt, qt=qt, dx=dx, du=du, py=py, my=my, ce=ce, kl=kl,
               loss=(1 - alpha) * ce + alpha * t * t * kl, grad=gscale * (hard + soft), hard=gscale * hard,
               soft_p=gscale * alpha * t * pt, soft_q=gscale * alpha * t * qt,
               logZ1=np.log(np.exp(dx).sum(1)), logZt=np.log(np.exp(dx / t).sum(1)), logZu=np.log(np.exp(du / t).sum(1)),
               amax=np.argmax(np.asarray(x), 1), nser=math.ceil(V / 256))
    ref["corr"] = (ref["amax"] == y).astype(f)
    return ref


def reference32(x, u, y, alpha, t, gscale):
    """the float32 twin: the same text evaluated in float32"""
    return reference(x, u, y, alpha, t, gscale, dtype=np.float32)


def _tmajor(a):
    Bq, Tq, V = a.shape
    return a.transpose(1, 0, 2).reshape(Tq * Bq, V)


def _from_probs(probs):
    """logits that the (B, T, V) probabilities of an oracle model are the softmax of, as (T * B, V) rows"""
    with np.errstate(divide="ignore"):
        return np.log(_tmajor(np.asarray(probs, np.float64)))


def distill_metrics(probs, teacher_logits, y_ids, alpha, t):
    """(loss, distill_kl, accuracy) a step reports, from the oracle student's (B, T, V) probabilities, the oracle teacher's
    (B, T, V) logits and the (B, T) ids: the means of loss_row, kl_row and correct_row over the B * T positions"""
    ref = reference(_from_probs(probs), _tmajor(np.asarray(teacher_logits, np.float64)), np.asarray(y_ids).T.reshape(-1),
                    alpha, t, 1.0)
    return ref["loss"].mean(), ref["kl"].mean(), ref["corr"].mean()


@contextlib.contextmanager
def distilled(teacher_logits, alpha, t):
    """inside the block the oracle models' backward starts from the gradient of the distilled loss against the (B, T, V)
    teacher logits"""
    old = O.cce_softmax_bwd
    ut = _tmajor(np.asarray(teacher_logits, np.float64))

    def bwd(p, y_ids, dl, e=None):
        if np.ndim(y_ids) != 2:
            return old(p, y_ids, dl)
        Bq, Tq, V = p.shape
        gs = np.broadcast_to(dl, (Bq, Tq)).T.reshape(-1)
        g = reference(_from_probs(p), ut, np.asarray(y_ids).T.reshape(-1), alpha, t, 1.0)["grad"] * gs[:, None]
        return g.reshape(Tq, Bq, V).transpose(1, 0, 2)
    O.cce_softmax_bwd = bwd
    try:
        yield
    finally:
        O.cce_softmax_bwd = old


class DistillMockBackend(MockBackend):
    """MockBackend plus tnt_softmax_cce_distill_f32 from the header text; ``ds_calls`` logs each call's arguments and keeps
    float64 copies of both logits rows"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ds_calls = []

    def softmax_cce_distill(self, logits, teacher, target, loss_row, kl_row, correct_row, dlogits, rows, V, ld, ld_teacher,
                            gscale, alpha, temperature):
        assert rows >= 0 and V > 0 and ld >= V and ld_teacher >= V
        assert logits is not None and teacher is not None and target is not None
        assert 0.0 <= alpha <= 1.0 and 0.0 < temperature < float("inf")
        for o in (loss_row, kl_row, correct_row, dlogits):
            assert o is None or o.data_ptr() != teacher.data_ptr(), "teacher aliases an output"
        if rows == 0:
            return
        x = mat(logits, rows, V, ld).astype(np.float64)
        u = mat(teacher, rows, V, ld_teacher).astype(np.float64)
        assert np.isfinite(u).all(), "teacher logits must be finite"
        y = flat(target)[:rows].astype(np.int64)
        self.ds_calls.append(dict(rows=rows, V=V, ld=ld, ld_teacher=ld_teacher, gscale=gscale, alpha=alpha,
                                  temperature=temperature, logits=x.copy(), teacher=u.copy(), target=y.copy(),
                                  teacher_tensor=teacher, want_grad=dlogits is not None))
        ref = reference(x, u, y, alpha, temperature, gscale)
        if loss_row is not None:
            flat(loss_row)[:rows] = ref["loss"]
        if kl_row is not None:
            flat(kl_row)[:rows] = ref["kl"]
        if correct_row is not None:
            flat(correct_row)[:rows] = ref["corr"]
        if dlogits is not None:
            mat(dlogits, rows, V, ld)[...] = ref["grad"]
