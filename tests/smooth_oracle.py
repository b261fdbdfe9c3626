"""Restatement of the label-smoothed head (tnt_softmax_cce_smooth_f32, definition in include/tnt_hip.h): the loss and its
gradient through keras's element-wise clip in float64, a per-row ``reference`` with the quantities the GPU test's error
model reads, a MockBackend with the op, and ``smoothed(eps)``, which substitutes the two loss steps of the float64 oracle
models (oracle.ops.cce_from_probs / cce_softmax_bwd) by their smoothed forms for the duration of a ``with`` block."""
import contextlib
import math

import numpy as np

from oracle import ops as O
from mock_backend import MockBackend, flat, mat

LO, HI = O.CCE_EPS, 1 - O.CCE_EPS


def smooth_targets(shape, y, eps):
    """ys = (1 - eps) onehot(y) + eps / V; an id outside [0, V) matches no class"""
    V = shape[-1]
    ys = np.full(shape, eps / V)
    y = np.asarray(y, np.int64)
    ok = (y >= 0) & (y < V)
    oh = np.zeros(shape)
    np.put_along_axis(oh, np.where(ok, y, 0)[..., None], 1.0, -1)
    return ys + (1 - eps) * oh * ok[..., None]


def smooth_cce_from_probs(p, y, eps):
    """-sum_v ys_v log(clip(p_v / sum p, 1e-7, 1 - 1e-7)) over the last axis"""
    q = np.clip(p / p.sum(-1, keepdims=True), LO, HI)
    return -(smooth_targets(p.shape, y, eps) * np.log(q)).sum(-1)


def smooth_cce_softmax_bwd(p, y, dl, eps):
    """gradient with respect to the logits, p = softmax(logits), upstream dl per row: dl (c p_v - m_v ys_v)"""
    m = ((p >= LO) & (p <= HI)).astype(p.dtype)
    ys = smooth_targets(p.shape, y, eps)
    c = (m * ys).sum(-1, keepdims=True)
    return np.asarray(dl)[..., None] * (c * p - m * ys)


@contextlib.contextmanager
def smoothed(eps):
    """inside the block the oracle models' loss is the smoothed one (metrics and backward both go through these two)"""
    old = O.cce_from_probs, O.cce_softmax_bwd
    O.cce_from_probs = lambda p, y_ids, e=None: smooth_cce_from_probs(p, y_ids, eps)
    O.cce_softmax_bwd = lambda p, y_ids, dl, e=None: smooth_cce_softmax_bwd(p, y_ids, dl, eps)
    try:
        yield
    finally:
        O.cce_from_probs, O.cce_softmax_bwd = old


def reference(x32, y, gscale, eps):
    """float64 softmax / loss / gradient of float32 logits x32 (rows, V), plus what the error model needs: d = x - max,
    logZ, w = sum p |d|, the clip masks, n_u, c, and Sabs = sum over the unclipped classes of |d|"""
    x = x32.astype(np.float64)
    rows, V = x.shape
    m = x.max(1)
    d = x - m[:, None]
    p = O.softmax(x)
    ref = {"p": p, "d": d, "m": m, "logZ": np.log(np.exp(d).sum(1)), "w": (p * -d).sum(1), "nser": math.ceil(V / 256),
           "amax": np.argmax(x32, 1)}
    if y is None:
        return ref
    y = np.asarray(y, np.int64)
    mask = (p >= LO) & (p <= HI)
    ys = smooth_targets(p.shape, y, eps)
    ref.update(y=y, mask=mask, ys=ys, n_u=mask.sum(1), c=(mask * ys).sum(1), Sabs=(mask * -d).sum(1),
               loss=smooth_cce_from_probs(p, y, eps), grad=smooth_cce_softmax_bwd(p, y, np.full(rows, gscale), eps))
    return ref


class SmoothMockBackend(MockBackend):
    """MockBackend plus tnt_softmax_cce_smooth_f32 from the header text; ``smooth_calls`` logs each call's arguments and
    keeps a float64 copy of the logits it was given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.smooth_calls = []

    def softmax_cce_smooth(self, logits, target, probs, loss_row, correct_row, dlogits, rows, V, ld, gscale, label_smoothing):
        assert rows >= 0 and V > 0 and ld >= V and logits is not None
        assert 0.0 <= label_smoothing < 1.0
        x = mat(logits, rows, V, ld).astype(np.float64)
        self.smooth_calls.append(dict(rows=rows, V=V, ld=ld, gscale=gscale, eps=label_smoothing, logits=x.copy(),
                                      target=None if target is None else flat(target)[:rows].astype(np.int64).copy(),
                                      want_grad=dlogits is not None, want_probs=probs is not None))
        p = O.softmax(x)
        if target is not None:
            y = flat(target)[:rows].astype(np.int64)
            if loss_row is not None:
                flat(loss_row)[:rows] = smooth_cce_from_probs(p, y, label_smoothing)
            if correct_row is not None:
                flat(correct_row)[:rows] = (p.argmax(-1) == y)
            if dlogits is not None:
                mat(dlogits, rows, V, ld)[...] = smooth_cce_softmax_bwd(p, y, np.full(rows, gscale), label_smoothing)
        elif dlogits is not None:
            mat(dlogits, rows, V, ld)[...] = 0
        if probs is not None and (dlogits is None or probs.data_ptr() != dlogits.data_ptr()):
            mat(probs, rows, V, ld)[...] = p
