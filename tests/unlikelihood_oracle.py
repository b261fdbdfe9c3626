"""Restatement of the unlikelihood head (tnt_softmax_cce_unlikely_f32, definition in include/tnt_hip.h) in float64: the
candidate sets, the loss and its gradient, a per-row ``reference`` with the quantities the GPU test's error model reads,
a MockBackend with the op, and ``unlikely(alpha)``, which substitutes oracle.ops.cce_softmax_bwd -- the one loss step of
the float64 oracle models that receives the whole (B, T) ids -- by one that adds the unlikelihood gradient for the
duration of a ``with`` block.  (The oracle models' forward calls oracle.ops.cce_from_probs per time step and so cannot see
a prefix: a test adds ``alpha * ul_mean(probs, y_ids)`` to the oracle's loss itself.)

Rows are t-major everywhere here, as in the header: row r = t * B + b."""
import contextlib
import math

import numpy as np

from oracle import ops as O
from mock_backend import MockBackend, flat, mat

LO, HI = O.CCE_EPS, 1 - O.CCE_EPS


def candidates(target, B, T, V):
    """list of T * B sorted id lists: C of row (t, b) = the distinct target[j * B + b], j < t, without the row's own
    target, without 0 and without ids outside [0, V)"""
    tg = np.asarray(target, np.int64).reshape(T, B)
    out = []
    for t in range(T):
        for b in range(B):
            out.append(sorted({int(c) for c in tg[:t, b] if 0 < c < V and c != tg[t, b]}))
    return out


def candidate_mask(target, B, T, V):
    """(T * B, V) bool: [v in C] per row"""
    mask = np.zeros((T * B, V), bool)
    for r, C in enumerate(candidates(target, B, T, V)):
        mask[r, C] = True
    return mask


def ul_terms(p, cmask):
    """per row: ul = -sum_{c in C} log(max(1 - p_c, 1e-7)), q (rows, V) = [v in C] m_v p_v / (1 - p_v), Q = sum_v q_v"""
    omp = 1.0 - p
    ul = -(cmask * np.log(np.maximum(omp, LO))).sum(-1)
    live = cmask & (omp >= LO)
    q = np.where(live, p / np.where(live, omp, 1.0), 0.0)
    return ul, q, q.sum(-1)


def target_prob(p, y):
    """(p_y, m_y): the target's probability -- 0 for an id outside [0, V), which matches no class -- and whether the clip
    of ce is inactive there"""
    V = p.shape[-1]
    ok = (y >= 0) & (y < V)
    py = np.where(ok, p[np.arange(p.shape[0]), np.where(ok, y, 0)], 0.0)
    return py, ok & (py >= LO) & (py <= HI)


def ul_loss(p, target, B, T, alpha):
    """loss_row = ce + alpha ul of probabilities p (T * B, V); returns (loss, ce, ul)"""
    y = np.asarray(target, np.int64).reshape(-1)
    ce = -np.log(np.clip(target_prob(p, y)[0], LO, HI))
    ul = ul_terms(p, candidate_mask(y, B, T, p.shape[-1]))[0]
    return ce + alpha * ul, ce, ul


def ul_grad(p, target, B, T, gscale, alpha):
    """dlogits_v = gscale (m_y (p_v - [v == y]) + alpha ([v in C] q_v - p_v Q)); gscale a scalar or one value per row"""
    y = np.asarray(target, np.int64).reshape(-1)
    rows, V = p.shape
    gs = np.broadcast_to(np.asarray(gscale, np.float64), (rows,))
    _, q, Q = ul_terms(p, candidate_mask(y, B, T, V))
    my = target_prob(p, y)[1]
    oh = np.zeros_like(p)
    oh[np.arange(rows)[my], y[my]] = 1.0
    return gs[:, None] * (my[:, None] * (p - oh) + alpha * (q - p * Q[:, None]))


def ul_mean(probs, y_ids):
    """mean over (B, T) of ul, from the oracle models' own (B, T, V) probabilities and (B, T) ids"""
    Bq, Tq, V = probs.shape
    p = probs.transpose(1, 0, 2).reshape(Tq * Bq, V)
    p = p / p.sum(-1, keepdims=True)
    return ul_terms(p, candidate_mask(np.asarray(y_ids).T.reshape(-1), Bq, Tq, V))[0].mean()


@contextlib.contextmanager
def unlikely(alpha):
    """inside the block the oracle models' backward starts from the gradient of ce + alpha ul"""
    old = O.cce_softmax_bwd

    def bwd(p, y_ids, dl, e=None):
        if np.ndim(y_ids) != 2:
            return old(p, y_ids, dl)
        Bq, Tq, V = p.shape
        pt = p.transpose(1, 0, 2).reshape(Tq * Bq, V)
        g = ul_grad(pt / pt.sum(-1, keepdims=True), np.asarray(y_ids).T.reshape(-1), Bq, Tq,
                    np.broadcast_to(dl, (Bq, Tq)).T.reshape(-1), alpha)
        return g.reshape(Tq, Bq, V).transpose(1, 0, 2)
    O.cce_softmax_bwd = bwd
    try:
        yield
    finally:
        O.cce_softmax_bwd = old


def reference(x32, target, B, T, gscale, alpha):
    """float64 softmax / loss / gradient of float32 logits x32 (T * B, V), plus what the error model needs: d = x - max,
    logZ, w = sum p |d|, the candidate mask, q, Q, ul, ce and m_y"""
    x = x32.astype(np.float64)
    rows, V = x.shape
    assert rows == T * B
    m = x.max(1)
    d = x - m[:, None]
    p = O.softmax(x)
    ref = {"p": p, "d": d, "m": m, "logZ": np.log(np.exp(d).sum(1)), "w": (p * -d).sum(1), "nser": math.ceil(V / 256),
           "amax": np.argmax(x32, 1)}
    if target is None:
        return ref
    y = np.asarray(target, np.int64).reshape(-1)
    cmask = candidate_mask(y, B, T, V)
    ul, q, Q = ul_terms(p, cmask)
    py, my = target_prob(p, y)
    ce = -np.log(np.clip(py, LO, HI))
    ref.update(y=y, cmask=cmask, q=q, Q=Q, ul=ul, ce=ce, py=py, my=my.astype(np.float64), loss=ce + alpha * ul,
               grad=ul_grad(p, y, B, T, gscale, alpha))
    return ref


class UnlikelihoodMockBackend(MockBackend):
    """MockBackend plus tnt_softmax_cce_unlikely_f32 from the header text; ``ul_calls`` logs each call's arguments and
    keeps a float64 copy of the logits it was given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ul_calls = []

    def softmax_cce_unlikely(self, logits, target, probs, loss_row, correct_row, dlogits, B, T, V, ld, gscale, alpha):
        assert B >= 0 and 1 <= T <= 64 and V > 0 and ld >= V and logits is not None
        assert 0.0 <= alpha < float("inf")
        rows = T * B
        x = mat(logits, rows, V, ld).astype(np.float64)
        self.ul_calls.append(dict(B=B, T=T, V=V, ld=ld, gscale=gscale, alpha=alpha, logits=x.copy(),
                                  target=None if target is None else flat(target)[:rows].astype(np.int64).copy(),
                                  want_grad=dlogits is not None, want_probs=probs is not None))
        p = O.softmax(x)
        if target is not None:
            y = flat(target)[:rows].astype(np.int64)
            if loss_row is not None:
                flat(loss_row)[:rows] = ul_loss(p, y, B, T, alpha)[0]
            if correct_row is not None:
                flat(correct_row)[:rows] = (p.argmax(-1) == y)
            if dlogits is not None:
                mat(dlogits, rows, V, ld)[...] = ul_grad(p, y, B, T, gscale, alpha)
        elif dlogits is not None:
            mat(dlogits, rows, V, ld)[...] = 0
        if probs is not None and (dlogits is None or probs.data_ptr() != dlogits.data_ptr()):
            mat(probs, rows, V, ld)[...] = p
