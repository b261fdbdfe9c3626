"""Restatement of the attention coverage penalty (tnt_attention_coverage_f32, definition in include/tnt_hip.h) in float64:
value and gradient for both axes; the backward chain of tests/lc_chain_oracle.py with an arbitrary per-step gradient of the
attention weights riding along (``chain_bwd_ext``, the reference of tnt_lc_seq_bwd_ext_f32 / tnt_attention_step_bwd_ext_f32);
``CoverageLcNIC``, the float64 oracle model whose training step differentiates CE + L2 + weight * coverage; and
``CoverageMockBackend``, the CPU stand-in with the three new backend calls.  Nothing here imports the package under test.

    alpha [T][B][R]
    axis "time":   s[b][r] = sum_t alpha[t][b][r],  N = B R
    axis "batch":  s[t][r] = sum_b alpha[t][b][r],  N = T R      (the `attention` metric's own sum)
    coverage = (1 / N) sum (1 - s)^2
    d (weight * coverage) / d alpha[t][b][r] = (2 weight / N) (s - 1),  s the sum that holds the element

The restatement is checked against central differences of the scalar loss in tests/test_host_coverage.py."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import MockBackend, flat, _keep
from test_gpu_ops import il, unil

AXES = ("time", "batch")
SLOPE = 0.2


def sums(alpha, axis):
    """s: [B][R] for "time", [T][R] for "batch" """
    alpha = np.asarray(alpha, np.float64)
    assert alpha.ndim == 3 and axis in AXES
    return alpha.sum(axis=0 if axis == "time" else 1)


def coverage(alpha, axis):
    """the unweighted value"""
    s = sums(alpha, axis)
    return ((1.0 - s) ** 2).mean()


def ext_rows(alpha, weight, axis):
    """what the kernel writes to ``ext``: coef * (s - 1) with coef = 2 weight / N, one row per sum ([B][R] or [T][R])"""
    s = sums(alpha, axis)
    return (2.0 * weight / s.size) * (s - 1.0)


def coverage_grad(alpha, weight, axis):
    """d (weight * coverage) / d alpha, [T][B][R]"""
    alpha = np.asarray(alpha, np.float64)
    e = ext_rows(alpha, weight, axis)
    return np.broadcast_to(e[None] if axis == "time" else e[:, None], alpha.shape).copy()


def strides(axis, R):
    """(ext_ts, ext_bs) of the rider for the kernel's ``ext`` layout"""
    return (0, R) if axis == "time" else (R, 0)


def ext_view(ext, ts, bs, T, B, R):
    """the [T][B][R] gradient a flat ``ext`` with element strides (ts, bs) stands for"""
    ext = np.asarray(ext, np.float64).reshape(-1)
    idx = np.arange(T)[:, None, None] * ts + np.arange(B)[None, :, None] * bs + np.arange(R)[None, None, :]
    return ext[idx]


def chain_bwd_ext(F, P, W2, v, Wc, Ur, qpre, alpha, gates, cs, dout, ext, r_attn=0.0, r_in=0.0, masks=None,
                  alpha_mse_coef=0.0, out_drop=None):
    """lc_chain_oracle.chain_bwd with ``ext`` [T][B][R] added to every step's dalpha (next to the alpha_mse term): the same
    loop over oracle.ops.attention_step_bwd(dalpha_ext=)."""
    c = lambda x: np.asarray(x, np.float64)
    F, P, W2, v, qpre, alpha, cs, dout, ext = map(c, (F, P, W2, v, qpre, alpha, cs, dout, ext))
    T, B, U = dout.shape
    assert ext.shape == alpha.shape
    Wc_k, Ur_k, g_k = unil(c(Wc)), unil(c(Ur)), unil(c(gates))
    ka, ki = masks if masks is not None else ([None] * T, [None] * T)
    dz, dqpre = [None] * T, [None] * T
    dP, dF, dvb = np.zeros_like(P), np.zeros_like(F), np.zeros((B, P.shape[2]))
    dh_next, dc = np.zeros((B, U)), np.zeros((B, U))
    for i in range(T - 1, -1, -1):
        do = dout[i] if out_drop is None else O.dropout_bwd(dout[i], out_drop[1][i], out_drop[0])
        gi, gf, gg, go = (g_k[i][:, k * U:(k + 1) * U] for k in range(4))
        dz_k, dh_rec, dc = O.lstm_step_bwd(do + dh_next, dc, (gi, gf, gg, go, cs[i], np.tanh(cs[i + 1]), None), Ur_k)
        dz[i] = il(dz_k, U)
        dctx = O.dropout_bwd(dz_k @ Wc_k.T, ki[i], r_in)
        s = np.tanh(P + O.act_fwd(qpre[i], O.ACT_LEAKY, SLOPE)[:, None, :])
        sd = O.dropout_fwd(s, ka[i], r_attn)
        e = alpha_mse_coef * (alpha[i] - 1) + ext[i]
        cache = (np.zeros((B, W2.shape[0])), qpre[i], s, sd, alpha[i], ka[i], r_attn)
        dh_att, dF_i, dsum, _, _, _, _ = O.attention_step_bwd(dctx, F, W2, v[:, None], cache, SLOPE, dalpha_ext=e)
        dqpre[i] = O.act_bwd(qpre[i], dsum.sum(axis=1), O.ACT_LEAKY, SLOPE)
        dalpha = (dctx[:, None, :] * F).sum(axis=2) + e
        de = alpha[i] * (dalpha - (alpha[i] * dalpha).sum(axis=1, keepdims=True))
        dvb += (sd * de[:, :, None]).sum(axis=1)
        dP += dsum; dF += dF_i
        dh_next = dh_rec + dh_att
    return dict(dz=np.stack(dz), dqpre=np.stack(dqpre), dP=dP, dF=dF, dvb=dvb, dh0=dh_next, dc0=dc)


class CoverageLcNIC(M.LcNIC):
    """oracle.models.LcNIC whose backward differentiates CE + L2 + weight * coverage(alpha, axis): every step's
    oracle.ops.attention_step_bwd receives its slab of coverage_grad as dalpha_ext.  ``coverage = None`` (or weight 0) is
    the plain model.  train_step / test_step report the unweighted ``coverage`` next to the plain metrics."""
    coverage = None         # (weight, axis)

    def _on(self):
        return self.coverage is not None and self.coverage[0] > 0

    def backward(self, probs, cache, y_ids):
        if not self._on():
            return super().backward(probs, cache, y_ids)
        weight, axis = self.coverage
        alpha = np.stack([st["acache"][4] for st in cache["steps"]])
        grad = coverage_grad(alpha, weight, axis)
        by_cache = {id(st["acache"]): grad[i] for i, st in enumerate(cache["steps"])}
        old = O.attention_step_bwd

        def bwd(dctx, F, W2, v, acache, slope=0.2, dalpha_ext=None):
            e = by_cache[id(acache)]
            return old(dctx, F, W2, v, acache, slope, dalpha_ext=e if dalpha_ext is None else dalpha_ext + e)
        O.attention_step_bwd = bwd
        try:
            return super().backward(probs, cache, y_ids)
        finally:
            O.attention_step_bwd = old

    def scalar_loss(self, data, y_ids, drop):
        """CE + L2 + weight * coverage in float64 (what backward differentiates)"""
        (probs, attn), _ = self.forward(data, training=True, drop=drop)
        ce, _, _ = self.metrics(probs, attn, y_ids)
        w, axis = self.coverage if self._on() else (0.0, "time")
        return ce + self.l2_loss() + w * coverage(attn[..., 0], axis)

    def train_step(self, data, y_ids, opt, drop=None):
        res, grads, (probs, attn) = super().train_step(data, y_ids, opt, drop)
        if self._on():
            res["coverage"] = coverage(attn[..., 0], self.coverage[1])
        return res, grads, (probs, attn)

    def test_step(self, data, y_ids):
        res, (probs, attn) = super().test_step(data, y_ids)
        if self._on():
            res["coverage"] = coverage(attn[..., 0], self.coverage[1])
        return res, (probs, attn)


class CoverageMockBackend(MockBackend):
    """MockBackend plus tnt_attention_coverage_f32 and the ``ext`` rider of attention_step_bwd, from the header text;
    ``cov_calls`` logs each coverage call's arguments and keeps a float64 copy of the attention weights it was given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.cov_calls = []

    def attention_coverage(self, alpha, T, B, R, axis, coef, ext, out, work, tstride=0):
        assert T > 0 and B > 0 and R > 0 and axis in (0, 1) and alpha is not None and work is not None
        ts = tstride if tstride > 0 else B * R
        al = np.lib.stride_tricks.as_strided(flat(alpha), (T, B, R), (ts * 4, R * 4, 4)).astype(np.float64)
        name = AXES[axis]
        rows = B if axis == 0 else T
        assert flat(work).size >= rows * ((R + 255) // 256)
        self.cov_calls.append(dict(T=T, B=B, R=R, axis=name, coef=coef, alpha=al.copy(), want_ext=ext is not None,
                                   want_out=out is not None, ext_tensor=ext))
        s = sums(al, name)
        if ext is not None:
            assert flat(ext).size >= rows * R
            flat(ext)[:rows * R] = (coef * (s - 1.0)).reshape(-1)
        if out is not None:
            flat(out)[0] = ((1.0 - s) ** 2).mean()

    def attention_step_bwd(self, dctx_d, F, P, W2, v, qpre, alpha, dP, dF, dvb, dqpre, dh, B, R, D, A, U, slope,
                           rate_attn, rate_in, in_lwidth, seed, site_attn, site_in, step, step_dev=None, dz=None,
                           Wc=None, dctx_part=None, nparts=0, keep4=None, alpha_mse=0.0, fresh=False, ext=None, ext_bs=0):
        if ext is None:
            return super().attention_step_bwd(dctx_d, F, P, W2, v, qpre, alpha, dP, dF, dvb, dqpre, dh, B, R, D, A, U, slope,
                                              rate_attn, rate_in, in_lwidth, seed, site_attn, site_in, step, step_dev, dz, Wc,
                                              dctx_part, nparts, keep4, alpha_mse, fresh)
        # the step of MockBackend.attention_step_bwd with dalpha += ext[b * ext_bs + r]
        if step_dev is not None:
            step = (step + int(step_dev[0])) & 0xFFFFFFFF
        f64 = lambda t, *s: flat(t)[:int(np.prod(s))].reshape(*s).astype(np.float64)
        keep = _keep(np.arange(B * R * A).reshape(B, R, A), rate_attn, seed, site_attn, step) if rate_attn > 0 else None
        self._check_keep4(keep4, keep, B * R * A)
        kin = _keep(np.arange(B)[:, None] * in_lwidth + np.arange(D)[None, :], rate_in, seed, site_in, step) if rate_in > 0 else None
        if dctx_part is not None:
            raw = f64(dctx_part, nparts, B, D).sum(0)
        else:
            raw = f64(dz, B, 4 * U) @ f64(Wc, D, 4 * U).T if dz is not None else f64(dctx_d, B, D)
        dctx = O.dropout_bwd(raw, kin, rate_in)
        Fm, Pm, W2m, vm, qp, al = f64(F, B, R, D), f64(P, B, R, A), f64(W2, U, A), f64(v, A)[:, None], f64(qpre, B, A), f64(alpha, B, R)
        e = flat(ext).astype(np.float64)[np.arange(B)[:, None] * ext_bs + np.arange(R)[None, :]]
        q = O.act_fwd(qp, O.ACT_LEAKY, slope)
        s = np.tanh(Pm + q[:, None, :])
        sd = O.dropout_fwd(s, keep, rate_attn)
        dalpha = (dctx[:, None, :] * Fm).sum(2) + alpha_mse * (al - 1.0) + e
        dFv = al[:, :, None] * dctx[:, None, :]
        de = al * (dalpha - (al * dalpha).sum(1, keepdims=True))
        dv = (sd * de[:, :, None]).sum(1)
        dsum = O.dropout_bwd(de[:, :, None] * vm[:, 0], keep, rate_attn) * (1 - s * s)
        dq = O.act_bwd(qp, dsum.sum(1), O.ACT_LEAKY, slope)
        if fresh:
            flat(dP)[:B * R * A] = 0
            flat(dF)[:B * R * D] = 0
            flat(dvb)[:B * (A + 1)] = 0
        flat(dP)[:B * R * A] += dsum.reshape(-1).astype(np.float32)
        flat(dF)[:B * R * D] += dFv.reshape(-1).astype(np.float32)
        dvbm = flat(dvb)[:B * (A + 1)].reshape(B, A + 1)
        dvbm[:, :A] += dv
        dvbm[:, A] += de.sum(1)
        flat(dqpre)[:B * A] = dq.reshape(-1)
        flat(dh)[:B * U] = (dq @ W2m.T).reshape(-1)
