"""Restatement of per-variable learning-rate multipliers and frozen variables (the *_lrmul_f32 entries, definition in
include/tnt_hip.h) in float64, written from the header text on top of the existing oracle updates (oracle.ops.adam_update,
sgd_momentum_update):

    frozen (mul == 0): the variable is not touched and not read -- no update, no decay, no share in the global norm
    else             : the plain update at learning rate mul * lr, decay (mul * lr * wd) * theta; mul enters no norm

``FinetuneState`` is the model-level oracle optimizer (Adam / AdamW / SGD with momentum, per-variable or global clip),
``FinetuneMockBackend`` a GlobalClipMockBackend with the table forms of the norm, reduction and update launches."""
import numpy as np

from oracle import ops as O
from global_clip_oracle import GlobalClipMockBackend, clip_scale, global_sqnorm
from mock_backend import MockBackend, flat


def selected(grads, mul):
    """the gradients an update may read: not None and not of a frozen variable"""
    return {k: g for k, g in grads.items() if g is not None and float(mul.get(k, 1.0)) != 0.0}


class FinetuneState:
    """kind "adam" (wd: AdamW) or "sgd" (momentum).  ``mul``: dict name -> multiplier (missing: 1), ``wd``: dict name ->
    decay (missing: 0); both, and ``lr``, may be reassigned between steps.  ``t`` counts every apply: the bias correction
    is global, a variable unfrozen later resumes with its old moments.  ``norm``: the global norm of the last apply."""

    def __init__(self, params, kind="adam", lr=1e-3, mul=None, wd=None, clipnorm=None, global_clipnorm=None, b1=0.9, b2=0.98,
                 eps=1e-8, momentum=0.9):
        assert kind in ("adam", "sgd") and not (clipnorm is not None and global_clipnorm is not None)
        self.kind, self.lr, self.mul, self.wd = kind, lr, dict(mul or {}), dict(wd or {})
        self.clipnorm, self.global_clipnorm = clipnorm, global_clipnorm
        self.b1, self.b2, self.eps, self.momentum = b1, b2, eps, momentum
        self.t, self.norm = 0, None
        self.m = {k: np.zeros_like(v) for k, v in params.items()}
        self.v = {k: np.zeros_like(v) for k, v in params.items()}

    def apply(self, params, grads, sparse_norms=None):
        self.t += 1
        live = selected(grads, self.mul)
        sq = {k: (float(sparse_norms[k]) ** 2 if sparse_norms is not None and k in sparse_norms else float((g * g).sum()))
              for k, g in live.items()}
        cs = None
        if self.global_clipnorm is not None:
            G = global_sqnorm(list(sq.values()))
            self.norm, cs = np.sqrt(G), clip_scale(G, self.global_clipnorm)
        for k, g in live.items():
            if cs is not None:
                g = g * cs
            elif self.clipnorm is not None:
                g = g * self.clipnorm / max(np.sqrt(sq[k]), self.clipnorm)
            old, rate = params[k], float(self.mul.get(k, 1.0)) * self.lr
            if self.kind == "adam":
                th, self.m[k], self.v[k] = O.adam_update(old, self.m[k], self.v[k], g, self.t, rate, self.b1, self.b2, self.eps)
            else:
                th, self.m[k] = O.sgd_momentum_update(old, self.m[k], g, rate, self.momentum)
            params[k] = th - (rate * float(self.wd.get(k, 0.0))) * old


class FinetuneMockBackend(GlobalClipMockBackend):
    """GlobalClipMockBackend plus the *_lrmul entries from the header text.  A frozen variable's theta, slots and gradient
    are never indexed: the mock would carry a NaN left in its gradient buffer into whatever read it.  ``lrm_calls`` logs
    the name and the table each call was given."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.lrm_calls = []

    def _lrm(self, name, seg_lrm):
        assert seg_lrm is not None and seg_lrm.element_size() == 4
        tab = flat(seg_lrm).astype(np.float64)
        assert np.isfinite(tab).all() and (tab >= 0).all()
        self.lrm_calls.append(dict(name=name, tab=tab.tolist()))
        return tab

    def span_sqnorm_lrmul(self, theta, grad, span_seg, span_off, span_len, seg_l2, partial, nspan, seg_lrm, lr_job=None,
                          skip=None):
        lrm = self._lrm("span_sqnorm_lrmul", seg_lrm)
        th, gr, l2, pa = flat(theta), flat(grad), flat(seg_l2), flat(partial)
        ov = flat(skip) if skip is not None else None
        for k, (s, o, n) in enumerate(self._segs(span_seg, span_off, span_len, nspan)):
            t = th[o:o + n].astype(np.float64)
            need_g = lrm[s] != 0 and not (ov is not None and ov[s] >= 0)
            g = gr[o:o + n].astype(np.float64) + 2 * float(l2[s]) * t if need_g else np.zeros(1)
            pa[2 * k], pa[2 * k + 1] = (g * g).sum(), (t * t).sum()
        if lr_job is not None:
            adam_t, lr, lr_t, b1, b2 = lr_job
            t = int(flat(adam_t)[0]) + 1
            flat(lr_t)[0] = float(flat(lr)[0]) * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)

    def seg_sqnorm_lrmul(self, theta, grad, span_seg, span_off, span_len, seg_first, seg_l2, partial, sq, wsq, l2_out, nspan,
                         nseg, seg_lrm):
        lrm = self._lrm("seg_sqnorm_lrmul", seg_lrm)
        th, gr, l2 = flat(theta), flat(grad), flat(seg_l2)
        q, w = np.zeros(nseg), np.zeros(nseg)
        first = flat(seg_first)[:nseg + 1]
        for k, (s, o, n) in enumerate(self._segs(span_seg, span_off, span_len, nspan)):
            t = th[o:o + n].astype(np.float64)
            loc = int(np.searchsorted(first, k, side="right")) - 1
            if lrm[s] != 0:
                g = gr[o:o + n].astype(np.float64) + 2 * float(l2[s]) * t
                q[loc] += (g * g).sum()
            w[loc] += (t * t).sum()
        flat(sq)[:nseg] = q
        flat(wsq)[:nseg] = w
        if l2_out is not None:
            flat(l2_out)[0] = (l2[:nseg].astype(np.float64) * w).sum()

    def global_sqnorm_lrmul(self, gsq, nseg, seg_lrm, sq_override=None, partial=None, seg_first=None, extra_part=None,
                            n_extra=0, extra_seg=-1, sq=None):
        lrm = self._lrm("global_sqnorm_lrmul", seg_lrm)
        assert (partial is None) != (sq is None) and nseg > 0
        ov = flat(sq_override)[:nseg] if sq_override is not None else np.full(nseg, -1.0)
        qs = []
        for s in range(nseg):
            if lrm[s] == 0:
                continue
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

    def _scale(self, sq, sq_override, s, clipnorm, gsq):
        if gsq is not None:
            assert clipnorm > 0 and np.isfinite(clipnorm)
            return clip_scale(float(flat(gsq)[0]), clipnorm)
        return self._clip(sq, sq_override, s, clipnorm)

    def adam_lrmul(self, theta, m, v, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr_t, lr_t_dev, beta1,
                   beta2, eps, clipnorm, seg_lrm, gsq=None, lr=None, seg_wd=None, guard=None, met=None, ring=None, ring_t=None):
        lrm = self._lrm("adam_lrmul", seg_lrm)
        assert seg_wd is None or lr is not None
        # the metrics ring job, before the guard check: the plain mock launch over no spans
        MockBackend.adam(self, theta, m, v, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, 0, lr_t, lr_t_dev, beta1,
                         beta2, eps, clipnorm, guard=guard, met=met, ring=ring, ring_t=ring_t)
        if guard is not None and int(guard[0]) != 0:
            return
        if lr_t_dev is not None:
            lr_t = float(flat(lr_t_dev)[0])
        th, mm, vv, gr, l2 = flat(theta), flat(m), flat(v), flat(grad), flat(seg_l2)
        for s, o, n in self._segs(span_seg, span_off, span_len, nspan):
            mul = lrm[s]
            if mul == 0:
                continue
            t = th[o:o + n].astype(np.float64)
            g = (gr[o:o + n].astype(np.float64) + 2 * float(l2[s]) * t) * self._scale(sq, sq_override, s, clipnorm, gsq)
            m1 = mm[o:o + n] + (g - mm[o:o + n]) * (1 - beta1)
            v1 = vv[o:o + n] + (g * g - vv[o:o + n]) * (1 - beta2)
            dk = mul * float(flat(lr)[0]) * float(flat(seg_wd)[s]) if seg_wd is not None else 0.0
            th[o:o + n] = (t - dk * t) - (mul * lr_t) * m1 / (np.sqrt(v1) + eps)
            mm[o:o + n] = m1
            vv[o:o + n] = v1

    def dense_dw_adam_lrmul(self, x, dpre, theta, m, v, l2, sq, sq_override, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk, ldx,
                            lrm, gsq=None, lr=None, wd=0.0, guard=None):
        """the encoder's fused update at a scalar multiplier: the plain mock update (its own clip norm, or the global word
        in its place), theta's step scaled by lrm -- Adam's step is linear in the rate --, then the decay at lrm * lr"""
        assert isinstance(lrm, float) and 0.0 <= lrm < float("inf") and (lr is not None or wd == 0.0)
        self.lrm_calls.append(dict(name="dense_dw_adam_lrmul", tab=[lrm]))
        if lrm == 0.0 or (guard is not None and int(guard[0]) != 0):
            return
        n = N * E
        before = flat(theta)[:n].astype(np.float64)
        norm, ovr = (gsq, None) if gsq is not None else (sq, sq_override)
        MockBackend.dense_dw_adam(self, x, dpre, theta, m, v, l2, norm, ovr, lr_t_dev, beta1, beta2, eps, clipnorm, N, E, Bk, ldx,
                                  guard=guard)
        th = flat(theta)
        rate = lrm * float(flat(lr)[0]) if lr is not None else 0.0
        th[:n] = before + lrm * (th[:n].astype(np.float64) - before) - (rate * float(wd)) * before

    def sgd_lrmul(self, theta, mom, grad, span_seg, span_off, span_len, seg_l2, sq, sq_override, nspan, lr, lr_dev, momentum,
                  clipnorm, seg_lrm, gsq=None, seg_wd=None, guard=None):
        lrm = self._lrm("sgd_lrmul", seg_lrm)
        assert seg_wd is None or lr_dev is not None
        if guard is not None and int(guard[0]) != 0:
            return
        if lr_dev is not None:
            lr = float(flat(lr_dev)[0])
        th, mo, gr, l2 = flat(theta), flat(mom), flat(grad), flat(seg_l2)
        for s, o, n in self._segs(span_seg, span_off, span_len, nspan):
            mul = lrm[s]
            if mul == 0:
                continue
            t = th[o:o + n].astype(np.float64)
            g = (gr[o:o + n].astype(np.float64) + 2 * float(l2[s]) * t) * self._scale(sq, sq_override, s, clipnorm, gsq)
            mv = momentum * mo[o:o + n] - (mul * lr) * g
            dk = mul * lr * float(flat(seg_wd)[s]) if seg_wd is not None else 0.0
            mo[o:o + n] = mv
            th[o:o + n] = (t - dk * t) + mv
