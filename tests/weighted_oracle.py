"""Restatement of the weighted head (tnt_softmax_cce_weighted_f32, definition in include/tnt_hip.h) in float64: the token
weights, the focal factor, the normalisation by the weight sum, the loss and its gradient, a per-row ``reference`` with
the quantities the GPU test's error model reads, a MockBackend with the op, ``weighted_metrics`` (the loss / accuracy a
step reports, from the oracle models' own probabilities) and ``weighted(...)``, which substitutes
oracle.ops.cce_softmax_bwd -- the one loss step of the float64 oracle models that receives the whole (B, T) ids -- by the
weighted gradient for the duration of a ``with`` block.

W is summed in float64 here, in no particular order: the header's float32 order is the kernel's, and its distance from
this sum is part of the GPU test's bound."""
import contextlib
import math

import numpy as np

from oracle import ops as O
from mock_backend import MockBackend, flat, mat

LO, HI = O.CCE_EPS, 1 - O.CCE_EPS


def row_weights(y, cw, V):
    """w_r = cw[y] for 0 <= y < V if cw is given, else 1"""
    y = np.asarray(y, np.int64).reshape(-1)
    if cw is None:
        return np.ones(y.size)
    ok = (y >= 0) & (y < V)
    return np.where(ok, np.asarray(cw, np.float64)[np.where(ok, y, 0)], 1.0)


def target_prob(p, y):
    """(p_y, m_y): the target's probability -- 0 for an id outside [0, V), which matches no class -- and whether the clip
    of ce is inactive there"""
    V = p.shape[-1]
    ok = (y >= 0) & (y < V)
    py = np.where(ok, p[np.arange(p.shape[0]), np.where(ok, y, 0)], 0.0)
    return py, ok & (py >= LO) & (py <= HI)


def terms(p, target, cw, gamma, normalise):
    """every scalar of the definition, per row (W and k once): w, py, my, pc, ce, f, g, W, k, kw = k w (0 where w == 0)"""
    y = np.asarray(target, np.int64).reshape(-1)
    rows, V = p.shape
    w = row_weights(y, cw, V)
    py, my = target_prob(p, y)
    pc = np.clip(py, LO, HI)
    ce = -np.log(pc)
    if gamma == 0:
        f = g = np.ones(rows)
    else:
        f = (1 - pc) ** gamma
        g = f + gamma * pc * (1 - pc) ** (gamma - 1) * ce
    W = w.sum()
    k = 1.0 if not normalise else (rows / W if W != 0 else 0.0)
    kw = np.where(w == 0, 0.0, k * w)
    return dict(y=y, w=w, py=py, my=my.astype(np.float64), pc=pc, ce=ce, f=f, g=g, W=W, k=k, kw=kw)


def wt_loss(p, target, cw, gamma, normalise):
    """loss_row = k w f ce"""
    t = terms(p, target, cw, gamma, normalise)
    return t["kw"] * t["f"] * t["ce"]


def wt_correct(p, target, cw, gamma, normalise):
    """correct_row = [argmax == y], times k w under normalise"""
    t = terms(p, target, cw, gamma, normalise)
    hit = (p.argmax(-1) == t["y"]).astype(np.float64)
    return hit * t["kw"] if normalise else hit


def wt_grad(p, target, cw, gscale, gamma, normalise):
    """dlogits_v = gscale k w m_y g (p_v - [v == y]); gscale a scalar or one value per row"""
    t = terms(p, target, cw, gamma, normalise)
    rows, V = p.shape
    gs = np.broadcast_to(np.asarray(gscale, np.float64), (rows,))
    oh = np.zeros_like(p)
    ok = (t["y"] >= 0) & (t["y"] < V)
    oh[np.arange(rows)[ok], t["y"][ok]] = 1.0
    return (gs * t["kw"] * t["my"] * t["g"])[:, None] * (p - oh)


def _tmajor(probs, y_ids):
    Bq, Tq, V = probs.shape
    p = probs.transpose(1, 0, 2).reshape(Tq * Bq, V)
    return p / p.sum(-1, keepdims=True), np.asarray(y_ids).T.reshape(-1)


def weighted_metrics(probs, y_ids, cw, gamma, normalise):
    """(loss, accuracy) a step reports, from the oracle models' own (B, T, V) probabilities and (B, T) ids: the means of
    loss_row and correct_row over the B * T positions"""
    p, y = _tmajor(probs, y_ids)
    return wt_loss(p, y, cw, gamma, normalise).mean(), wt_correct(p, y, cw, gamma, normalise).mean()


@contextlib.contextmanager
def weighted(cw, gamma, normalise):
    """inside the block the oracle models' backward starts from the gradient of the weighted loss"""
    old = O.cce_softmax_bwd

    def bwd(p, y_ids, dl, e=None):
        if np.ndim(y_ids) != 2:
            return old(p, y_ids, dl)
        Bq, Tq, V = p.shape
        pt, y = _tmajor(p, y_ids)
        g = wt_grad(pt, y, cw, np.broadcast_to(dl, (Bq, Tq)).T.reshape(-1), gamma, normalise)
        return g.reshape(Tq, Bq, V).transpose(1, 0, 2)
    O.cce_softmax_bwd = bwd
    try:
        yield
    finally:
        O.cce_softmax_bwd = old


def reference(x32, target, cw32, gscale, gamma, normalise):
    """float64 softmax / loss / correct / gradient of float32 logits x32 (rows, V) and float32 weights cw32 (or None),
    plus what the error model needs: d = x - max, logZ, w = sum p |d| (as in test_gpu_head.reference; the row weights of
    ``terms`` are under "wr" here)"""
    x = x32.astype(np.float64)
    rows, V = x.shape
    m = x.max(1)
    d = x - m[:, None]
    p = O.softmax(x)
    ref = {"p": p, "d": d, "m": m, "logZ": np.log(np.exp(d).sum(1)), "w": (p * -d).sum(1), "nser": math.ceil(V / 256),
           "amax": np.argmax(x32, 1)}
    if target is None:
        return ref
    cw = None if cw32 is None else np.asarray(cw32, np.float32).astype(np.float64)
    t = terms(p, target, cw, gamma, normalise)
    t["wr"] = t.pop("w")
    ref.update(t)
    ref.update(loss=wt_loss(p, target, cw, gamma, normalise), corr=wt_correct(p, target, cw, gamma, normalise),
               grad=wt_grad(p, target, cw, gscale, gamma, normalise))
    return ref


class WeightedMockBackend(MockBackend):
    """MockBackend plus tnt_softmax_cce_weighted_f32 from the header text; ``wt_calls`` logs each call's arguments, keeps
    a float64 copy of the logits and of the weights it was given, and the weight tensor itself (``cw_tensor``)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.wt_calls = []

    def softmax_cce_weighted(self, logits, target, class_weight, probs, loss_row, correct_row, dlogits, rows, V, ld, gscale,
                             gamma=0.0, normalise=False):
        assert rows >= 0 and V > 0 and ld >= V and logits is not None
        assert 0.0 <= gamma < float("inf") and normalise in (0, 1, False, True)
        normalise = bool(normalise)
        x = mat(logits, rows, V, ld).astype(np.float64)
        cw = None if class_weight is None else flat(class_weight)[:V].astype(np.float64).copy()
        self.wt_calls.append(dict(rows=rows, V=V, ld=ld, gscale=gscale, gamma=gamma, normalise=normalise, logits=x.copy(),
                                  cw=cw, cw_tensor=class_weight,
                                  target=None if target is None else flat(target)[:rows].astype(np.int64).copy(),
                                  want_grad=dlogits is not None, want_probs=probs is not None))
        p = O.softmax(x)
        if target is not None:
            y = flat(target)[:rows].astype(np.int64)
            if loss_row is not None:
                flat(loss_row)[:rows] = wt_loss(p, y, cw, gamma, normalise)
            if correct_row is not None:
                flat(correct_row)[:rows] = wt_correct(p, y, cw, gamma, normalise)
            if dlogits is not None:
                mat(dlogits, rows, V, ld)[...] = wt_grad(p, y, cw, gscale, gamma, normalise)
        elif dlogits is not None:
            mat(dlogits, rows, V, ld)[...] = 0
        if probs is not None and (dlogits is None or probs.data_ptr() != dlogits.data_ptr()):
            mat(probs, rows, V, ld)[...] = p
