"""Restatement of the sentence-embedding target (tnt_cosine_loss_f32, tnt_row_inv_norm_f32, tnt_cosine_topk_f32; definitions
in include/tnt_hip.h): ``cosine_loss`` / ``row_inv_norm`` in float64, ``similarity_f32`` (the float32 multiplication order of the
selection) and ``topk`` (its order); ``SemanticNIC``, the float64 dense-model step of oracle/models.py with the term added; and
``SemanticMockBackend``, the CPU stand-in with the three new backend calls.  Nothing here imports the package under test.

    z = x W + bias                                  x [B][E] the feature rows the first LSTM step is fed
    nz = sqrt(max(sum z^2, 1e-12)), ng likewise     keras l2_normalize, epsilon 1e-12
    cos = sum (z / nz) (g / ng),  loss = 1 - cos,   semantic = mean_b loss_b
    d (gscale sum_b loss_b) / dz = -gscale (gn - cos zn) / nz        where sum z^2 > 1e-12
                                 = -gscale gn / nz                   below (the normaliser is constant there)

The restatement is checked against central differences in tests/test_host_semantic.py."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import MockBackend, flat, mat

EPS = 1e-12
NAMES = ("guse_out/kernel", "guse_out/bias")


def cosine_loss(z, g, gscale=None):
    """(loss [B], cos [B], dz [B][G] or None) in float64"""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    szz, sgg = (z * z).sum(1), (g * g).sum(1)
    nz, ng = np.sqrt(np.maximum(szz, EPS)), np.sqrt(np.maximum(sgg, EPS))
    zn, gn = z / nz[:, None], g / ng[:, None]
    cos = (zn * gn).sum(1)
    dz = None
    if gscale is not None:
        k = np.where(szz > EPS, cos, 0.0)
        dz = -gscale * (gn - k[:, None] * zn) / nz[:, None]
    return 1.0 - cos, cos, dz


def row_inv_norm(X):
    X = np.asarray(X, np.float64)
    return 1.0 / np.sqrt(np.maximum((X * X).sum(1), EPS))


def similarity_f32(S, qinv, binv):
    """(S[b][m] * qinv[b]) * binv[m]: two float32 multiplications in this order"""
    S, qinv, binv = np.asarray(S, np.float32), np.asarray(qinv, np.float32), np.asarray(binv, np.float32)
    return ((S * qinv[:, None]).astype(np.float32) * binv[None, :]).astype(np.float32)


def topk(c, k):
    """(idx [B][k] int32, val [B][k]) of the k first entries of every row in the selection's total order: larger first, equal
    values (-0 equals +0) by ascending index, NaN behind -inf and among NaNs by ascending index"""
    c = np.asarray(c)
    B, Mm = c.shape
    assert 1 <= k <= Mm
    idx = np.zeros((B, k), np.int32)
    for b in range(B):
        nan = np.isnan(c[b])
        key = np.where(nan, -np.inf, c[b].astype(np.float64))
        # lexsort: last key first -- NaN flag ascending (numbers first), then value descending, then index ascending
        order = np.lexsort((np.arange(Mm), -key, nan))
        idx[b] = order[:k]
    return idx, np.take_along_axis(c, idx.astype(np.int64), 1)


class SemanticNIC(M.NICDense):
    """oracle.models.NICDense with the sentence-embedding target: data = (betas, cap, a0, c0, guse); the scalar that
    backward differentiates is CE + L2 + weight * semantic, with x the post-Dropout feature row ``f_d`` of the forward."""
    G, weight, reg = 0, 1.0, 0.0

    def configure(self, dim, weight=1.0, reg=0.0):
        self.G, self.weight, self.reg = int(dim), float(weight), float(reg)
        return self

    def init_params(self, rng, dtype=np.float64):
        super().init_params(rng, dtype)
        lim = np.sqrt(6.0 / (self.E + self.G))
        self.p["guse_out/kernel"] = rng.uniform(-lim, lim, (self.E, self.G)).astype(dtype)
        self.p["guse_out/bias"] = (0.01 * rng.standard_normal(self.G)).astype(dtype)
        return self

    def forward(self, data, training=False, drop=None):
        probs, cache = super().forward(tuple(data[:4]), training, drop)
        z = cache["f_d"] @ self.p["guse_out/kernel"] + self.p["guse_out/bias"]
        cache["z"], cache["guse"] = z, np.asarray(data[4], np.float64)
        return probs, cache

    def embed(self, x):
        """predict_embedding: the inference encoder's feature row times the layer"""
        B = x.shape[0]
        data = (x, np.zeros((B, 1), np.int32), np.zeros((B, self.U)), np.zeros((B, self.U)), np.zeros((B, self.G)))
        return self.forward(data, training=False)[1]["z"]

    def semantic(self, cache):
        return cosine_loss(cache["z"], cache["guse"])[0].mean()

    def l2_loss(self):
        return super().l2_loss() + M._l2(self.reg, self.p["guse_out/kernel"])

    def backward(self, probs, cache, y_ids):
        g, sparse = super().backward(probs, cache, y_ids)
        p, B = self.p, y_ids.shape[0]
        _, _, dz = cosine_loss(cache["z"], cache["guse"], self.weight / B)
        W = p["guse_out/kernel"]
        g["guse_out/kernel"] = cache["f_d"].T @ dz + 2 * self.reg * W
        g["guse_out/bias"] = dz.sum(0)
        # the term's share of the encoder gradients: the tail of NICDense.backward is linear in the feature gradient
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

    def scalar_loss(self, data, y_ids, drop):
        """CE + L2 + weight * semantic in float64 (what backward differentiates)"""
        probs, cache = self.forward(data, training=True, drop=drop)
        return self.metrics(probs, y_ids)[0] + self.l2_loss() + self.weight * self.semantic(cache)

    def train_step(self, data, y_ids, opt, drop=None):
        drop = drop or M.DropCtx(training=True)
        probs, cache = self.forward(data, training=True, drop=drop)
        ce, acc = self.metrics(probs, y_ids)
        l2, sem = self.l2_loss(), self.semantic(cache)
        grads, sparse = self.backward(probs, cache, y_ids)
        self.last_sparse = sparse
        opt.apply(self.p, grads, sparse)
        self.p["batch_norm/moving_mean"] = cache["new_mm"]
        self.p["batch_norm/moving_variance"] = cache["new_mv"]
        return {"loss": ce, "L2": l2, "accuracy": acc, "semantic": sem}, grads, probs

    def test_step(self, data, y_ids):
        probs, cache = self.forward(data, training=False)
        ce, acc = self.metrics(probs, y_ids)
        return {"loss": ce, "L2": self.l2_loss(), "accuracy": acc, "semantic": self.semantic(cache)}, probs


class SemanticMockBackend(MockBackend):
    """MockBackend plus tnt_cosine_loss_f32 / tnt_row_inv_norm_f32 / tnt_cosine_topk_f32, from the header text"""

    def cosine_loss(self, z, ldz, g, ldg, dz, loss_row, cos_row, out, B, G, gscale):
        assert B >= 1 and 1 <= G <= 2048 and ldz >= G and ldg >= G
        assert all(t is not None for t in (z, g, loss_row, cos_row))
        loss, cos, d = cosine_loss(mat(z, B, G, ldz), mat(g, B, G, ldg), gscale if dz is not None else None)
        flat(loss_row)[:B] = loss
        flat(cos_row)[:B] = cos
        if out is not None:
            flat(out)[0] = loss.mean()
        if dz is not None:
            mat(dz, B, G, ldz)[...] = d

    def row_inv_norm(self, X, ldx, inv, rows, G):
        assert rows >= 1 and G >= 1 and ldx >= G and X is not None and inv is not None
        flat(inv)[:rows] = row_inv_norm(mat(X, rows, G, ldx))

    def cosine_topk(self, S, lds, qinv, binv, idx, sim, B, M_, k):
        assert B >= 1 and M_ >= 1 and 1 <= k <= min(64, M_) and lds >= M_
        assert all(t is not None for t in (S, qinv, binv, idx, sim))
        c = similarity_f32(mat(S, B, M_, lds), flat(qinv)[:B], flat(binv)[:M_])
        i, v = topk(c, k)
        flat(idx)[:B * k] = i.reshape(-1)
        flat(sim)[:B * k] = v.reshape(-1)
