"""Restatement of the contrastive sentence-embedding loss (tnt_contrastive_loss_f32; definition in include/tnt_hip.h) in
float64: ``contrastive_loss``; ``ContrastiveNIC``, tests/semantic_oracle.SemanticNIC with that term in the cosine term's place;
and ``ContrastiveMockBackend``, the CPU stand-in with the new backend call.  Nothing here imports the package under test.

    iz_i = 1/sqrt(max(sum z_i^2, eps)),  ig_j likewise,  zn = z iz,  gn = g ig,  eps = 1e-12
    valid_j = (sum g_j^2 > eps),  Bv = number of valid rows
    L_ij = (zn_i . gn_j) inv_t                              over valid i, j only
    Q_ij = [i == j] (hard)   or   Q_i. = softmax_j((gn_i . gn_j) soft_inv_t) over valid j (soft)
    lr_i = -sum_j Q_ij log softmax_j(L_i.)_j,   lc_i = -sum_j Q_ij log softmax_j(L_.i)_j
    row_i = symmetric ? 0.5 (lr_i + lc_i) : lr_i,   loss = sum_i row_i / max(Bv, 1)
    hit_i = valid_i and (first argmax over valid j of L_ij) == i,   top1 = sum hit / max(Bv, 1)
    dL_ij = weight / max(Bv, 1) ((1 - b)(Pr_ij - Q_ij) + b (Pc_ij - Q_ji)),   b = symmetric ? 0.5 : 0
    dzn_i = inv_t sum_j dL_ij gn_j,   dz_i = iz_i (dzn_i - zn_i (zn_i . dzn_i))   (dz_i = iz_i dzn_i where sum z_i^2 <= eps)

The restatement is checked against central differences and torch autograd in tests/test_host_contrastive.py."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import flat, mat
import semantic_oracle as SO

EPS = 1e-12


def _lse(X, axis):
    m = X.max(axis, keepdims=True)
    return (m + np.log(np.exp(X - m).sum(axis, keepdims=True))).squeeze(axis)


def logits(z, g, inv_t):
    """(L over all rows, valid, zn, gn, iz, szz) in float64"""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    szz, sgg = (z * z).sum(1), (g * g).sum(1)
    iz, ig = 1.0 / np.sqrt(np.maximum(szz, EPS)), 1.0 / np.sqrt(np.maximum(sgg, EPS))
    zn, gn = z * iz[:, None], g * ig[:, None]
    return (zn @ gn.T) * inv_t, sgg > EPS, zn, gn, iz, szz


def evaluate(z, g, inv_t, soft_inv_t=0.0, symmetric=True, weight=1.0, column_term=True):
    """every quantity of the definition in float64, as a dict; the B x B matrices over the valid rows ``v`` only"""
    L, valid, zn, gn, iz, szz = logits(z, g, inv_t)
    B = L.shape[0]
    v = np.flatnonzero(valid)
    Bv = len(v)
    d = dict(L=L, valid=valid, v=v, Bv=Bv, zn=zn, gn=gn, iz=iz, szz=szz, loss_row=np.zeros(B), hit=np.zeros(B, np.int64),
             dz=np.zeros_like(zn), loss=0.0, top1=0.0)
    if Bv == 0:
        return d
    Lv = L[np.ix_(v, v)]
    if soft_inv_t > 0:
        Sv = (gn[v] @ gn[v].T) * soft_inv_t
        Sv = 0.5 * (Sv + Sv.T)                               # symmetric in i, j before the softmax
        Q = np.exp(Sv - _lse(Sv, 1)[:, None])
    else:
        Q = np.eye(Bv)
    logPr = Lv - _lse(Lv, 1)[:, None]                         # row softmax
    logPc = Lv - _lse(Lv, 0)[None, :]                         # Pc_ij: the softmax over rows of column j
    lr = -(Q * logPr).sum(1)
    lc = -(Q * logPc.T).sum(1)                                # log softmax_j(L_.i)_j = logPc[j][i]
    b = 0.5 if symmetric else 0.0
    Pr, Pc = np.exp(logPr), np.exp(logPc)
    if not column_term:
        lc, Pc, QT = np.zeros(Bv), np.zeros_like(Pc), np.zeros_like(Q)
    else:
        QT = Q.T
    d["loss_row"][v] = (1 - b) * lr + b * lc
    d["hit"][v] = v[np.argmax(Lv, 1)] == v                    # np.argmax: the first maximum
    dL = (weight / Bv) * ((1 - b) * (Pr - Q) + b * (Pc - QT))
    dzn = inv_t * (dL @ gn[v])
    k = np.where(szz[v] > EPS, (zn[v] * dzn).sum(1), 0.0)
    d["dz"][v] = iz[v, None] * (dzn - zn[v] * k[:, None])
    d.update(Lv=Lv, Q=Q, QT=QT, Pr=Pr, Pc=Pc, b=b, dzn=dzn, loss=d["loss_row"].sum() / Bv, top1=d["hit"].sum() / Bv)
    return d


def contrastive_loss(z, g, inv_t, soft_inv_t=0.0, symmetric=True, weight=1.0, column_term=True):
    """(loss_row [B], hit [B] int, loss, top1, dz [B][G]) in float64.  ``column_term=False`` drops the caption -> scan
    direction from a symmetric loss (the wrong answer tests/test_gpu_contrastive.py shows its bound to reject)."""
    d = evaluate(z, g, inv_t, soft_inv_t, symmetric, weight, column_term)
    return d["loss_row"], d["hit"], d["loss"], d["top1"], d["dz"]


class ContrastiveNIC(SO.SemanticNIC):
    """SemanticNIC with the contrastive term in the cosine term's place: the scalar that backward differentiates is
    CE + L2 + weight * semantic with semantic the contrastive mean; metrics add ``semantic_top1``."""
    inv_t, soft_inv_t, symmetric = 1.0 / 0.07, 0.0, True

    def configure_loss(self, temperature=0.07, symmetric=True, soft_temperature=None):
        self.inv_t = 1.0 / float(temperature)
        self.soft_inv_t = 0.0 if soft_temperature is None else 1.0 / float(soft_temperature)
        self.symmetric = bool(symmetric)
        return self

    def _term(self, cache):
        return contrastive_loss(cache["z"], cache["guse"], self.inv_t, self.soft_inv_t, self.symmetric, self.weight)

    def semantic(self, cache):
        return self._term(cache)[2]

    def top1(self, cache):
        return self._term(cache)[3]

    def backward(self, probs, cache, y_ids):
        # SemanticNIC.backward with this term's dz: the tail of NICDense.backward is linear in the feature gradient
        g, sparse = M.NICDense.backward(self, probs, cache, y_ids)
        p, dz = self.p, self._term(cache)[4]
        W = p["guse_out/kernel"]
        g["guse_out/kernel"] = cache["f_d"].T @ dz + 2 * self.reg * W
        g["guse_out/bias"] = dz.sum(0)
        df = O.dropout_bwd((dz @ W.T)[:, None, :], cache["k_l0"], self.r_lstm)[:, 0, :]
        if self.norm == "batch":
            dyd, dgam, dbet = O.batchnorm_bwd(df, p["batch_norm/gamma"], cache["bn"])
        else:
            dyd, dgam, dbet = O.layernorm_bwd(df, p["batch_norm/gamma"], cache["bn"])
        dy = O.dropout_bwd(dyd, cache["k_feat"], self.r_feat)
        _, dK, db = O.dense_bwd(cache["xd"], p["dense_img/kernel"], cache["pre"], dy, O.ACT_LEAKY, need_dx=False)
        for k, v in (("batch_norm/gamma", dgam), ("batch_norm/beta", dbet), ("dense_img/kernel", dK), ("dense_img/bias", db)):
            g[k] = g[k] + v
        return g, sparse

    def train_step(self, data, y_ids, opt, drop=None):
        drop = drop or M.DropCtx(training=True)
        probs, cache = self.forward(data, training=True, drop=drop)
        ce, acc = self.metrics(probs, y_ids)
        l2, sem, top1 = self.l2_loss(), self.semantic(cache), self.top1(cache)
        grads, sparse = self.backward(probs, cache, y_ids)
        self.last_sparse = sparse
        opt.apply(self.p, grads, sparse)
        self.p["batch_norm/moving_mean"] = cache["new_mm"]
        self.p["batch_norm/moving_variance"] = cache["new_mv"]
        return {"loss": ce, "L2": l2, "accuracy": acc, "semantic": sem, "semantic_top1": top1}, grads, probs

    def test_step(self, data, y_ids):
        probs, cache = self.forward(data, training=False)
        ce, acc = self.metrics(probs, y_ids)
        return {"loss": ce, "L2": self.l2_loss(), "accuracy": acc, "semantic": self.semantic(cache),
                "semantic_top1": self.top1(cache)}, probs


def work_floats(B, soft):
    """TNT_CONTRASTIVE_WORK_FLOATS of include/tnt_hip.h"""
    return 5 * B + (2 if soft else 1) * B * B


class ContrastiveMockBackend:
    """mixin: tnt_contrastive_loss_f32 from the header text, in the shape of SemanticMockBackend's calls"""

    def contrastive_loss(self, z, ldz, g, ldg, dz, work, loss_row, hit_row, out, B, G, inv_temperature, soft_inv_temperature,
                         symmetric, weight):
        assert 1 <= B <= 1024 and 1 <= G <= 2048 and ldz >= G and ldg >= G
        assert all(t is not None for t in (z, g, work, loss_row, hit_row))
        assert np.isfinite(inv_temperature) and inv_temperature > 0 and np.isfinite(soft_inv_temperature)
        assert soft_inv_temperature >= 0 and symmetric in (0, 1, False, True) and np.isfinite(weight) and weight >= 0
        assert flat(work).size >= work_floats(B, soft_inv_temperature > 0)
        lrow, hit, loss, top1, d = contrastive_loss(mat(z, B, G, ldz), mat(g, B, G, ldg), inv_temperature,
                                                    soft_inv_temperature, bool(symmetric), weight)
        flat(loss_row)[:B] = lrow
        flat(hit_row)[:B] = hit
        if out is not None:
            flat(out)[0], flat(out)[1] = loss, top1
        if dz is not None:
            mat(dz, B, G, ldz)[...] = d
