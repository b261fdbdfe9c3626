"""Restatement of diverse (group) beam search (tnt_beam_step_diverse_f32, definition in include/tnt_hip.h): the step in
float64, the diverse searches of both caption models on the decode-step restatements of tests/constrain_oracle.py
(tests/dense_beam_oracle.py's BeamNICDense and oracle.models.LcNIC underneath; with members > 1 the mixture of
tests/consensus_oracle.py in the softmax's place), and a mock-backend mixin with the op in float32 from the header text."""
import numpy as np

from mock_backend import flat, mat
from constrain_oracle import ConstrainMockBackend, constrain_rows
import consensus_oracle as CO


# ---------------------------------------------------------------------------------------------------- the step
def diverse_step(probs, score, fin, groups, lam, end_id, dtype=np.float64):
    """One sample's step: probs (k, V), score (k,), fin (k,) of its k beams, ``groups`` = Gd groups of k' = k / Gd choosing
    in ascending order.  Returns (score_out (k,), parent (k,) local row, token (k,), fin_out (k,) bool, gap, nv_max):
    gap is the smallest difference between two adjacent selection keys the step had to order, over all groups -- between
    consecutive kept keys and between the k'-th kept and the best dropped one; nv_max the largest count n_v that a group
    found in front of it.  ``dtype`` float32 computes the score and the key in the kernel's operations."""
    probs = np.asarray(probs)
    k, V = probs.shape
    kp = k // groups
    assert kp * groups == k
    lam = dtype(lam)
    fin = np.asarray(fin).astype(bool)
    cand = np.full((k, V), -np.inf, dtype)
    with np.errstate(divide="ignore"):
        for j in range(k):
            if fin[j]:
                cand[j, 0] = score[j]                   # a finished beam: token 0 at its own score
            else:
                cand[j] = dtype(score[j]) + np.log(np.maximum(probs[j].astype(dtype), dtype(1e-30))).astype(dtype)
    count = np.zeros(V, np.int64)                       # n_v: live choices of the groups so far
    s_out, par, tok = np.zeros(k, dtype), np.zeros(k, np.int64), np.zeros(k, np.int64)
    f_out = np.zeros(k, bool)
    gap, nv_max = np.inf, 0
    for g in range(groups):
        r0 = g * kp
        nv_max = max(nv_max, int(count.max()))
        pen = (lam * count.astype(dtype)).astype(dtype)
        key = np.where(fin[r0:r0 + kp, None], cand[r0:r0 + kp], (cand[r0:r0 + kp] - pen[None, :]).astype(dtype)).reshape(-1)
        order = np.argsort(-key, kind="stable")         # ties: the lower j*V + v first
        ranked = key[order[:kp + 1]].astype(np.float64)
        if ranked.shape[0] > 1:
            gap = min(gap, float(np.min(ranked[:-1] - ranked[1:])))
        for r, cnd in enumerate(order[:kp]):
            j, v = divmod(int(cnd), V)
            s_out[r0 + r], par[r0 + r], tok[r0 + r] = cand[r0 + j, v], r0 + j, v
            f_out[r0 + r] = fin[r0 + j] or v == end_id
            if not fin[r0 + j]:
                count[v] += 1
    return s_out, par, tok, f_out, gap, nv_max


# ---------------------------------------------------------------------------------------------------- the mock
class DiverseBeamMock:
    """mixin for a MockBackend: tnt_beam_step_diverse_f32 from the header text in float32, then the state rows gathered by
    parent; counts its calls"""

    beam_step_diverse_calls = 0

    def beam_step_diverse(self, probs, ld, score_in, fin_in, B, V, k, end_id, score_out, parent, token, fin_out, h_in, c_in,
                          ldh, U, h_out, c_out, groups, lam):
        self.beam_step_diverse_calls += 1
        assert B > 0 and V > 0 and 1 <= k <= 16 and ld >= V and 0 <= U <= ldh
        assert groups >= 1 and k % groups == 0 and np.isfinite(lam) and lam >= 0
        assert score_out.data_ptr() != score_in.data_ptr() and fin_out.data_ptr() != fin_in.data_ptr()
        P = mat(probs, B * k, V, ld)
        sc, fn = flat(score_in)[:B * k].reshape(B, k), flat(fin_in)[:B * k].reshape(B, k)
        so, pa, to, fo = flat(score_out), flat(parent), flat(token), flat(fin_out)
        for b in range(B):
            s, p, t, f, _, _ = diverse_step(P[b * k:(b + 1) * k], sc[b], fn[b], groups, lam, end_id, np.float32)
            so[b * k:(b + 1) * k], pa[b * k:(b + 1) * k], to[b * k:(b + 1) * k], fo[b * k:(b + 1) * k] = s, b * k + p, t, f
        if U == 0:
            return
        assert h_out.data_ptr() not in (h_in.data_ptr(), c_in.data_ptr())
        assert c_out.data_ptr() not in (h_in.data_ptr(), c_in.data_ptr())
        par = pa[:B * k].astype(np.int64)
        for src, dst in ((h_in, h_out), (c_in, c_out)):
            mat(dst, B * k, U, ldh)[...] = mat(src, B * k, U, ldh)[par].copy()


class DiverseMockBackend(DiverseBeamMock, ConstrainMockBackend):
    """the mock backend of the constrained decodes (tnt_beam_step_f32, tnt_decode_constrain_f32, ...) plus
    tnt_beam_step_diverse_f32"""


# ---------------------------------------------------------------------------------------------------- the searches
def diverse_beam(orc, x, a0, c0, start_seq, max_len, k, groups, lam, end_id=-1, con=None, members=1, mode="mean", w=None):
    """Diverse beam search of ``orc`` (ConstrainedNICDense: the dense model; ConstrainedLcNIC / ConsensusMsLcNIC: the
    attention models): the loop of constrain_oracle.constrained_beam / consensus_oracle.consensus_beam with diverse_step as
    the expansion and every group started from its own copy of the start state.  ``con``: constraints, applied to every
    live row from its own path; ``members`` = G > 1: x, a0, c0 hold G*M rows member-major and the M*k mixed rows are
    expanded.  Returns (sequences (M, k, max_len) int64 group-major, scores (M, k), margin (M,): the smallest key gap of
    diverse_step over the steps)."""
    start = np.asarray(start_seq).reshape(-1)
    Mn, V, G = start.shape[0], orc.V, members
    Mk, kp = Mn * k, k // groups
    assert x.shape[0] == G * Mn and kp * groups == k
    st = orc.dec_init(x, a0, c0, k)
    word = np.repeat(np.tile(start, G), k)
    score = np.zeros((Mn, groups, kp)); score[:, :, 1:] = -1e30
    score = score.reshape(Mn, k)
    fin = np.zeros((Mn, k), bool)
    seqs = np.zeros((Mn, k, 0), np.int64)
    margin = np.full(Mn, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, np.tile(seqs.reshape(Mk, i), (G, 1)), con, i, live=np.tile(~fin.reshape(-1), G))
        probs, _ = CO.mix(logits, G, w, mode)                      # G = 1: the softmax
        pj, tv = np.zeros((Mn, k), np.int64), np.zeros((Mn, k), np.int64)
        new_score, new_fin = np.zeros((Mn, k)), np.zeros((Mn, k), bool)
        for b in range(Mn):
            new_score[b], pj[b], tv[b], new_fin[b], gap, _ = diverse_step(probs[b * k:(b + 1) * k], score[b], fin[b], groups,
                                                                          lam, end_id)
            margin[b] = min(margin[b], gap)
        parent = (np.arange(Mn)[:, None] * k + pj).reshape(-1)
        orc.dec_reorder(st, CO.spread(None, parent, None, Mk, G)[1])
        seqs = np.concatenate([np.take_along_axis(seqs, pj[:, :, None], axis=1), tv[:, :, None]], axis=2)
        score, fin = new_score, new_fin
        word = np.tile(tv.reshape(-1), G)
    return seqs, score, margin
