"""Restatement of global-norm gradient clipping (tnt_global_sqnorm_f32 and the *_gclip_f32 update entries, definition in
include/tnt_hip.h) in float64, written from the header text on top of the existing oracle updates:

    G  = sum_s q_s                q_s the squared clip-norm input of variable s (the IndexedSlices norm where one is given)
    cs = c / max(sqrt(G), c)      every gradient element of every variable is scaled by cs; G <= c^2 gives 1

``GlobalClip`` wraps a model-level oracle optimizer (oracle.models.AdamState, weight_decay_oracle.AdamWState / SGDWState,
built with clipnorm=None), ``GlobalClipMockBackend`` is a MockBackend with the reduction launch and the gclip ops: each
runs the plain (or decaying) mock op with the global norm in the place of every variable's own.

``gsq_rel_bound`` is the float32 summation bound of the order the header states for G."""
import numpy as np
import torch

from mock_backend import MockBackend, flat
from weight_decay_oracle import WeightDecayMockBackend

EPS32 = 2.0 ** -24        # unit round-off of float32


def global_sqnorm(qs):
    """G: the float64 sum of the per-variable squared norms"""
    return float(np.sum(np.asarray(qs, dtype=np.float64)))


def clip_scale(G, c):
    return float(c) / max(np.sqrt(G), float(c))


def clip_by_global_norm(grads, c, sparse_norms=None):
    """tf.clip_by_global_norm over a dict of gradients (None entries skipped): (scaled dict, global norm).  sparse_norms:
    name -> the l2 norm tf.linalg.global_norm takes for an IndexedSlices gradient (its un-deduplicated values)"""
    qs = []
    for k, g in grads.items():
        if g is None:
            continue
        qs.append(float(sparse_norms[k]) ** 2 if sparse_norms is not None and k in sparse_norms else float((g * g).sum()))
    G = global_sqnorm(qs)
    cs = clip_scale(G, c)
    return {k: (None if g is None else g * cs) for k, g in grads.items()}, np.sqrt(G)


def gsq_rel_bound(nterms, per_variable=1e-5):
    """|G_kernel - G| <= bound * G for nterms non-negative q_s, each given to ``per_variable`` relative (the norm tolerance
    of test_gpu_optim_tail).  The header's order: thread t adds its ceil(nterms / 256) terms serially, the wave tree adds
    6 levels, the four wave sums 2 more -- a term passes through at most d = ceil(nterms / 256) + 8 float32 additions, each
    within EPS32 relative of a partial sum that is <= G (all terms >= 0): d * EPS32 (1 + d * EPS32) to second order."""
    d = -(-int(nterms) // 256) + 8
    return per_variable + d * EPS32 * (1 + d * EPS32)


class GlobalClip:
    """an oracle optimizer state (built with clipnorm=None) behind tf.clip_by_global_norm at threshold ``c``; ``norm`` is
    the global norm of the last apply()"""

    def __init__(self, state, c):
        assert getattr(state, "clipnorm", None) is None
        self.state, self.c, self.norm = state, float(c), None

    def __getattr__(self, name):
        return getattr(self.__dict__["state"], name)

    def __setattr__(self, name, value):
        if name in ("state", "c", "norm"):
            self.__dict__[name] = value
        else:
            setattr(self.state, name, value)

    def apply(self, params, grads, sparse_norms=None):
        scaled, self.norm = clip_by_global_norm(grads, self.c, sparse_norms)
        self.state.apply(params, scaled, None)


class GlobalClipMockBackend(WeightDecayMockBackend):
    """WeightDecayMockBackend plus tnt_global_sqnorm_f32 and the gclip update entries from the header text; ``gclip_calls``
    logs the name, the threshold and the word each update call read"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.gclip_calls = []

    def global_sqnorm(self, gsq, nseg, sq_override=None, partial=None, seg_first=None, extra_part=None, n_extra=0, extra_seg=-1,
                      sq=None):
        assert (partial is None) != (sq is None) and nseg > 0
        ov = flat(sq_override)[:nseg] if sq_override is not None else np.full(nseg, -1.0)
        qs = []
        for s in range(nseg):
            if partial is not None and s == extra_seg and n_extra > 0 and extra_part is not None:
                qs.append(flat(extra_part)[:n_extra].astype(np.float64).sum())
            elif ov[s] >= 0:
                qs.append(float(ov[s]))
            elif partial is not None:
                k0, k1 = int(flat(seg_first)[s]), int(flat(seg_first)[s + 1])
                qs.append(flat(partial)[2 * k0:2 * k1:2].astype(np.float64).sum())
            else:
                qs.append(float(flat(sq)[s]))
        flat(gsq)[0] = global_sqnorm(qs)

    def _log(self, name, clipnorm, gsq):
        assert gsq is not None and clipnorm > 0 and np.isfinite(clipnorm)
        self.gclip_calls.append(dict(name=name, c=float(clipnorm), gsq=float(flat(gsq)[0])))

    def adam_gclip(self, theta, m, v, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr_t, lr_t_dev, beta1,
                   beta2, eps, clipnorm, gsq, lr=None, seg_wd=None, guard=None, met=None, ring=None, ring_t=None):
        self._log("adam_gclip", clipnorm, gsq)
        every = torch.full_like(sq, float(flat(gsq)[0]))          # the one norm in every variable's place
        args = (theta, m, v, grad, span_seg, span_off, span_len, seg_l2, every, None, nspan, lr_t, lr_t_dev, beta1, beta2, eps,
                clipnorm)
        if seg_wd is None:
            MockBackend.adam(self, *args, guard=guard, met=met, ring=ring, ring_t=ring_t)
        else:
            WeightDecayMockBackend.adamw(self, *args, lr, seg_wd, guard=guard, met=met, ring=ring, ring_t=ring_t)

    def sgd_gclip(self, theta, mom, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr, lr_dev, momentum,
                  clipnorm, gsq, seg_wd=None, guard=None):
        self._log("sgd_gclip", clipnorm, gsq)
        every = torch.full_like(sq, float(flat(gsq)[0]))
        args = (theta, mom, grad, span_seg, span_off, span_len, seg_l2, every, None, nspan)
        if seg_wd is None:
            MockBackend.sgd(self, *args, lr, lr_dev, momentum, clipnorm, guard=guard)
        else:
            WeightDecayMockBackend.sgdw(self, *args, lr_dev, momentum, clipnorm, seg_wd, guard=guard)

    def dense_dw_adam_gclip(self, x, dpre, theta, m, v, l2, sq, sq_override, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk, ldx,
                            gsq, lr=None, wd=0.0, guard=None):
        self._log("dense_dw_adam_gclip", clipnorm, gsq)
        args = (x, dpre, theta, m, v, l2, gsq, None, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk, ldx)
        if lr is None:
            MockBackend.dense_dw_adam(self, *args, guard=guard)
        else:
            WeightDecayMockBackend.dense_dw_adamw(self, *args, lr, float(wd), guard=guard)
