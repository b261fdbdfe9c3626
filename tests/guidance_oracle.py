"""Restatement of classifier-free guidance for caption decoding (tnt_guidance_mix_f32, definition in include/tnt_hip.h) in
float64: the kernel, and the guided greedy, sampled and beam decodes of the caption models, built on the decode-step
restatements of tests/constrain_oracle.py and the helpers of tests/consensus_oracle.py with the scan's and the null scan's
distributions contrasted at every step and the common word fed back to both.  Rows are member-major with two members:
conditional row r, null row Rm + r."""
import numpy as np

from oracle import models as M
from constrain_oracle import constrain_rows
from consensus_oracle import first_max, rel_gap, spread, golden_case  # noqa: F401  (golden_case: for the tests)
from topkp_oracle import sample_topkp


# ---------------------------------------------------------------------------------------------------- the kernel
def mix(logits, scale, plaus=0.0, dtype=np.float64):
    """logits (2*Rm, V) -> (p (Rm, V), token (Rm,)): the guided distribution and its first maximum.  ``dtype`` float32
    restates the same formula in float32 arithmetic (numpy's summation order, no fused multiply-add)."""
    x = np.asarray(logits, dtype)
    V = x.shape[1]
    x = x.reshape(2, -1, V)
    scale = dtype(scale)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=-1, keepdims=True)
        empty = ~(m > -np.inf)                       # a row with nothing above -inf: m = 0, s = 1
        m = np.where(empty, dtype(0), m)
        s = np.where(empty, dtype(1), np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype))
        l = (x - m) - np.log(s)
        lc, ln = l[0], l[1]
        both = np.isfinite(lc) & np.isfinite(ln)
        g = np.where(both, lc + scale * (np.where(both, lc, 0) - np.where(both, ln, 0)), lc)   # lc = -inf stays -inf
        if plaus > 0:
            g = np.where(lc < np.log(dtype(plaus)) + lc.max(axis=-1, keepdims=True), -np.inf, g)
        g = g.astype(dtype)
        Gm = g.max(axis=-1, keepdims=True)
        none = ~(Gm > -np.inf)                       # every g_v is -inf: the row is all zero
        e = np.exp(g - np.where(none, dtype(0), Gm))
        p = np.where(none, dtype(0), e / np.where(none, dtype(1), e.sum(axis=-1, keepdims=True, dtype=dtype)))
    return p.astype(dtype), first_max(p)


# ---------------------------------------------------------------------------------------------------- the decodes
def member_rows(x, a0, c0, null=None):
    """the 2*M decoder inputs of a guided decode: the scans and behind them the null scans (None: zeros; (N,): one for every
    image; (M, N): one per image), a0 / c0 repeated"""
    x = np.asarray(x)
    nul = np.zeros_like(x) if null is None else np.broadcast_to(np.asarray(null, x.dtype), x.shape)
    return np.concatenate([x, nul], axis=0), np.concatenate([a0, a0], axis=0), np.concatenate([c0, c0], axis=0)


def guided_decode(orc, x, a0, c0, start_seq, max_len, scale, plaus=0.0, null=None, con=None, sampler=None):
    """Greedy (sampler None) or sampled (sampler = (temperature, top_k, top_p, seed, step), tnt_sample_topkp_f32 on the
    guided rows) guided decode of the M scans ``x``.  ``con``: the constraints of tests/constrain_oracle.py, applied to both
    member rows from the common history.  Returns (ids (M, max_len), probs (max_len, M, V): the guided distributions, gap
    (M,): the smallest relative top-2 gap of the guided distribution over the steps (greedy) or the sampler's smallest
    margin)."""
    start = np.asarray(start_seq).reshape(-1)
    Mn = start.shape[0]
    xs, a2, c2 = member_rows(x, a0, c0, null)
    assert xs.shape[0] == 2 * Mn
    word = np.tile(start, 2)
    st = orc.dec_init(xs, a2, c2)
    ids = np.zeros((Mn, 0), np.int64)
    probs, gap = [], np.full(Mn, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, np.tile(ids, (2, 1)), con, i)
        p, tok = mix(logits, scale, plaus)
        if sampler is None:
            gap = np.minimum(gap, rel_gap(p))
        else:
            t, k, tp, seed, step = sampler
            tok, mg = sample_topkp(p, t, k, tp, False, seed, M.S_SAMPLE + i, step)
            gap = np.minimum(gap, mg)
        probs.append(p)
        ids = np.concatenate([ids, tok[:, None]], axis=1)
        word = np.tile(tok, 2)
    return ids, np.stack(probs, axis=0), gap


def guided_beam(orc, x, a0, c0, start_seq, max_len, scale, plaus=0.0, null=None, k=5, end_id=-1, con=None):
    """Beam search on the guided distribution (the loop of consensus_oracle.consensus_beam with two members and the guided
    mix): decoder rows [2][M][k].  Returns (sequences (M, k, max_len), scores (M, k), margin (M,): the smallest score gap
    that decided a rank)."""
    start = np.asarray(start_seq).reshape(-1)
    Mn, V = start.shape[0], orc.V
    Mk = Mn * k
    xs, a2, c2 = member_rows(x, a0, c0, null)
    st = orc.dec_init(xs, a2, c2, k)
    word = np.repeat(np.tile(start, 2), k)
    score = np.zeros((Mn, k)); score[:, 1:] = -1e30
    fin = np.zeros((Mn, k), bool)
    seqs = np.zeros((Mn, k, 0), np.int64)
    margin = np.full(Mn, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, np.tile(seqs.reshape(Mk, i), (2, 1)), con, i, live=np.tile(~fin.reshape(-1), 2))
        probs, _ = mix(logits, scale, plaus)
        cand = score[:, :, None] + np.log(np.maximum(probs, 1e-30)).reshape(Mn, k, V)
        frozen = np.full((Mn, k, V), -np.inf); frozen[:, :, 0] = score
        cand = np.where(fin[:, :, None], frozen, cand).reshape(Mn, k * V)
        order = np.argsort(-cand, axis=1, kind='stable')          # ties: lower flat index first
        top = order[:, :k]
        best = np.take_along_axis(cand, top, axis=1)
        if k > 1:
            margin = np.minimum(margin, np.min(best[:, :-1] - best[:, 1:], axis=1))
        margin = np.minimum(margin, best[:, -1] - np.take_along_axis(cand, order[:, k:k + 1], axis=1)[:, 0])
        pj, tv = top // V, top % V
        parent = (np.arange(Mn)[:, None] * k + pj).reshape(-1)
        orc.dec_reorder(st, spread(None, parent, None, Mk, 2)[1])
        seqs = np.concatenate([np.take_along_axis(seqs, pj[:, :, None], axis=1), tv[:, :, None]], axis=2)
        fin = np.take_along_axis(fin, pj, axis=1) | (tv == end_id)
        score = best
        word = np.tile(tv.reshape(-1), 2)
    return seqs, score, margin
