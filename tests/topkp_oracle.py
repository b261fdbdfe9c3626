"""Float64 restatement of top-k / nucleus sampling (tnt_sample_topkp_f32, definition in include/tnt_hip.h), the dense
model's sampled decode driven by it, and a MockBackend with the op."""
import warnings

import numpy as np

from oracle import models as M
from oracle import ops as O
from oracle.philox import uniform24
from mock_backend import MockBackend, flat


def _gap(a, b):
    """relative gap of two weights a >= b whose order is a decision; an exact tie is resolved by index, no decision"""
    return np.inf if a == b else (a - b) / a


def filter_weights(w, top_k, top_p):
    """kept mask of one row of weights (float64, >= 0) and the margin of the filter's decisions: the weight gap at the
    K boundary and at the nucleus cutoff (relative to the larger weight) and the distance of the mass before each
    candidate to top_p * S_K (relative to S_K)."""
    V = w.shape[0]
    order = np.lexsort((np.arange(V), -w))          # w descending, ties: the lower index first
    K = min(top_k, V) if top_k >= 1 else V
    cand = order[:K]
    margin = np.inf
    if K < V:
        margin = min(margin, _gap(w[order[K - 1]], w[order[K]]))
    keep = np.zeros(V, bool)
    if top_p < 1:
        S = w[cand].sum()
        before = np.cumsum(w[cand]) - w[cand]
        kr = before < top_p * S
        if S > 0:
            margin = min(margin, np.abs(before - top_p * S).min() / S)
        n = int(kr.sum())
        if n < K:                                        # the weights either side of the cutoff: their order decides
            margin = min(margin, _gap(w[cand[n - 1]], w[cand[n]]))
        keep[cand[kr]] = True
    else:
        keep[cand] = True
    return keep, margin


def sample_topkp(x, temperature, top_k, top_p, from_logits, seed, site, step):
    """ids and per-row margins of tnt_sample_topkp_f32 over the rows of x (rows, V).  The margin is the smallest
    relative distance of any decision to its edge: the K-boundary gap, the nucleus cutoff, u*sum against the kept CDF."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # all-NaN rows
        l = x if from_logits else np.log(x)
        w = np.exp((l - np.nanmax(l, axis=-1, keepdims=True)) / temperature)
    w = np.where(np.isnan(w), 0.0, w)
    u = uniform24(x.shape[0], int(seed), int(site), int(step) & 0xFFFFFFFF).astype(np.float64)
    ids = np.zeros(x.shape[0], np.int64)
    margins = np.zeros(x.shape[0])
    for r in range(x.shape[0]):
        keep, m = filter_weights(w[r], top_k, top_p)
        cdf = np.cumsum(np.where(keep, w[r], 0.0))
        if cdf[-1] > 0:
            target = u[r] * cdf[-1]
            ids[r] = int(np.searchsorted(cdf, target, side='right'))
            m = min(m, np.abs(cdf - target).min() / cdf[-1])
        margins[r] = m
    return ids, margins


class TopkpMockBackend(MockBackend):
    """MockBackend plus tnt_sample_topkp_f32 from its definition (this restatement); counts its calls"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.topkp_calls = 0

    def sample_topkp(self, x, out, rows, V, ld, temperature, top_k, top_p, from_logits, seed, site, step, step_dev=None):
        self.topkp_calls += 1
        st = (step + (int(flat(step_dev)[0]) if step_dev is not None else 0)) & 0xFFFFFFFF
        ids, _ = sample_topkp(flat(x)[:rows * ld].reshape(rows, ld)[:, :V], temperature, top_k, top_p, from_logits, seed,
                              site, st)
        flat(out)[:rows] = ids


class SampledNICDense(M.NICDense):
    """the dense model's decode (NICDense.greedy_predict) with the argmax replaced by sampler(probs, i) -> ids"""

    def sample_predict(self, x, a0, c0, start_seq, max_len, sampler):
        """returns (ids (B, max_len, 1) int64, probs (max_len, B, 1, V))"""
        p = self.p
        dt = p['dense_img/kernel'].dtype
        y, _ = O.dense_fwd(x.astype(dt), p['dense_img/kernel'], p['dense_img/bias'], O.ACT_LEAKY)
        if self.norm == 'batch':
            f, _, _, _ = O.batchnorm_fwd(y, p['batch_norm/gamma'], p['batch_norm/beta'],
                                         p['batch_norm/moving_mean'], p['batch_norm/moving_variance'], False)
        else:
            f, _ = O.layernorm_fwd(y, p['batch_norm/gamma'], p['batch_norm/beta'])
        Wl, Ul, bl = p['lstm/kernel'], p['lstm/recurrent_kernel'], p['lstm/bias']
        a, c, _ = O.lstm_step_fwd(f @ Wl + bl, a0.astype(dt), c0.astype(dt), Ul)
        word = np.asarray(start_seq).reshape(-1)
        m = np.ones((word.shape[0], 1), bool)
        outs, ids = [], []
        for i in range(max_len):
            e = p['emb_text/embeddings'][word]
            h2, c2, _ = O.lstm_step_fwd(e @ Wl + bl, a, c, Ul)
            whole = np.where(m, h2, 0)
            a = np.where(m, h2, a)
            c = np.where(m, c2, c)
            probs = O.softmax(whole @ p['time_distributed_softmax/kernel'] + p['time_distributed_softmax/bias'])
            outs.append(probs[:, None, :])
            word = np.asarray(sampler(probs, i))
            ids.append(word[:, None])
            m = (word != 0)[:, None]
        return np.stack(ids, axis=1).astype(np.int64), np.stack(outs, axis=0)
