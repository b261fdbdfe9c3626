"""Float64 restatement of beam search over the dense model (nic.NIC.beam_search), of the length normalisation of its
results (model_base.length_normalise), and a MockBackend with tnt_beam_step_f32 from its header definition."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import MockBackend, flat, mat


class BeamMockBackend(MockBackend):
    """MockBackend plus tnt_beam_step_f32 (include/tnt_hip.h): the expansion of tnt_beam_topk_f32 in float32, then the
    state rows gathered by parent; counts its calls"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.beam_step_calls = 0

    def beam_step(self, probs, ld, score_in, fin_in, B, V, k, end_id, score_out, parent, token, fin_out, h_in, c_in, ldh,
                  U, h_out, c_out):
        self.beam_step_calls += 1
        assert B > 0 and V > 0 and 1 <= k <= 16 and ld >= V and 0 <= U <= ldh
        self.beam_topk(probs, score_in, fin_in, B, V, ld, k, end_id, score_out, parent, token, fin_out)
        if U == 0:
            return
        assert h_out.data_ptr() not in (h_in.data_ptr(), c_in.data_ptr())
        assert c_out.data_ptr() not in (h_in.data_ptr(), c_in.data_ptr())
        par = flat(parent)[:B * k].astype(np.int64)
        for src, dst in ((h_in, h_out), (c_in, c_out)):
            mat(dst, B * k, U, ldh)[...] = mat(src, B * k, U, ldh)[par].copy()


class BeamNICDense(M.NICDense):
    """the dense model's decode (NICDense.greedy_predict, its mask rule included) driven by beam search"""

    def _features(self, x, a0, c0):
        p = self.p
        dt = p['dense_img/kernel'].dtype
        y, _ = O.dense_fwd(x.astype(dt), p['dense_img/kernel'], p['dense_img/bias'], O.ACT_LEAKY)
        if self.norm == 'batch':
            f, _, _, _ = O.batchnorm_fwd(y, p['batch_norm/gamma'], p['batch_norm/beta'],
                                         p['batch_norm/moving_mean'], p['batch_norm/moving_variance'], False)
        else:
            f, _ = O.layernorm_fwd(y, p['batch_norm/gamma'], p['batch_norm/beta'])
        a, c, _ = O.lstm_step_fwd(f @ p['lstm/kernel'] + p['lstm/bias'], a0.astype(dt), c0.astype(dt),
                                  p['lstm/recurrent_kernel'])
        return a, c

    def _step(self, word, m, a, c):
        """one decode step of greedy_predict: (probs, a, c); m masks the LSTM step (state carried, output zeros)"""
        p = self.p
        e = p['emb_text/embeddings'][word]
        h2, c2, _ = O.lstm_step_fwd(e @ p['lstm/kernel'] + p['lstm/bias'], a, c, p['lstm/recurrent_kernel'])
        whole = np.where(m, h2, 0)
        a = np.where(m, h2, a)
        c = np.where(m, c2, c)
        return O.softmax(whole @ p['time_distributed_softmax/kernel'] + p['time_distributed_softmax/bias']), a, c

    def beam_search(self, x, a0, c0, start_seq, max_len, k=5, end_id=-1):
        """Returns (sequences (B, k, max_len) int64, scores (B, k), margin (B,) = the smallest gap between the k-th kept
        and the best dropped candidate, and between consecutive kept ones, over all steps), as LcNIC.beam_search."""
        B = x.shape[0]
        V = self.V
        a, c = self._features(x, a0, c0)
        a, c = np.repeat(a, k, axis=0), np.repeat(c, k, axis=0)
        word = np.repeat(np.asarray(start_seq).reshape(-1), k)
        m = np.ones((B * k, 1), bool)                  # step 0: the start token's mask is lost, as in greedy_predict
        score = np.zeros((B, k)); score[:, 1:] = -1e30
        fin = np.zeros((B, k), bool)
        seqs = np.zeros((B, k, 0), np.int64)
        margin = np.full(B, np.inf)
        for _ in range(max_len):
            probs, a, c = self._step(word, m, a, c)
            cand = score[:, :, None] + np.log(np.maximum(probs, 1e-30)).reshape(B, k, V)
            frozen = np.full((B, k, V), -np.inf); frozen[:, :, 0] = score
            cand = np.where(fin[:, :, None], frozen, cand).reshape(B, k * V)
            order = np.argsort(-cand, axis=1, kind='stable')          # ties: lower flat index first
            top = order[:, :k]
            best = np.take_along_axis(cand, top, axis=1)
            if k > 1:
                margin = np.minimum(margin, np.min(best[:, :-1] - best[:, 1:], axis=1))
            if k * V > k:
                margin = np.minimum(margin, best[:, -1] - np.take_along_axis(cand, order[:, k:k + 1], axis=1)[:, 0])
            pj, tv = top // V, top % V
            rows = (np.arange(B)[:, None] * k + pj).reshape(-1)
            a, c = a[rows], c[rows]
            seqs = np.concatenate([np.take_along_axis(seqs, pj[:, :, None], axis=1), tv[:, :, None]], axis=2)
            fin = np.take_along_axis(fin, pj, axis=1) | (tv == end_id)
            score = best
            word = tv.reshape(-1)
            m = (word != 0)[:, None]
        return seqs, score, margin

    def path_score(self, x, a0, c0, start_seq, seqs, end_id=-1):
        """the score the definition gives each path of seqs (B, k, T): the sum of the log-probabilities of its tokens up
        to and including its first end_id (the decoder fed the path itself, with greedy_predict's mask rule)"""
        B, k, T = seqs.shape
        a, c = self._features(x, a0, c0)
        a, c = np.repeat(a, k, axis=0), np.repeat(c, k, axis=0)
        word = np.repeat(np.asarray(start_seq).reshape(-1), k)
        m = np.ones((B * k, 1), bool)
        flat_seqs = seqs.reshape(B * k, T)
        total = np.zeros(B * k)
        live = np.ones(B * k, bool)
        for i in range(T):
            probs, a, c = self._step(word, m, a, c)
            tok = flat_seqs[:, i]
            total += np.where(live, np.log(np.maximum(probs[np.arange(B * k), tok], 1e-30)), 0.0)
            live &= tok != end_id
            word = tok
            m = (word != 0)[:, None]
        return total.reshape(B, k)


def length_normalise(seqs, scores, end_id, length_penalty):
    """restatement of model_base.length_normalise, one sample and one result at a time"""
    B, k, T = seqs.shape
    out_s, out_k = np.zeros_like(seqs), np.zeros((B, k), np.float32)
    for b in range(B):
        keys = []
        for r in range(k):
            hits = [i for i in range(T) if seqs[b, r, i] == end_id]
            L = hits[0] + 1 if hits else T
            keys.append(float(np.float32(scores[b, r])) / ((5.0 + L) / 6.0) ** length_penalty)
        for slot, r in enumerate(sorted(range(k), key=lambda r: (-keys[r], r))):
            out_s[b, slot] = seqs[b, r]
            out_k[b, slot] = keys[r]
    return out_s, out_k
