"""Float64 restatement of tnt_caption_rouge_f32 (include/tnt_hip.h) on padded id arrays: captions cut at the first
terminator, the longest common subsequence by the plain O(len^2) table, the F-score of the two separately maximised
ratios in the header's operation order, both baselines and the counted positions.  Written from the header's definition,
not from evaluate.rouge_l or the kernel's bit-vector recurrence, which tests/test_host_rouge.py and
tests/test_gpu_rouge.py compare it with.  ``lcs_fn`` / ``joint`` / ``beta`` swap in the near misses the tests' inputs have
to tell apart: the longest common substring, the maximum of the per-reference F-scores, beta = 1.  RougeMockMixin gives a
mock backend ``caption_rouge``."""
import numpy as np

from reward_oracle import caption, counted

BETA = 1.2


def lcs(a, b):
    """the length of the longest common subsequence, the full (len(a)+1) x (len(b)+1) table"""
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def substring(a, b):
    """NEAR MISS: the length of the longest common substring (contiguous)"""
    best = 0
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            if a[i - 1] == b[j - 1]:
                t[i][j] = t[i - 1][j - 1] + 1
                best = max(best, t[i][j])
    return best


def f_score(P, R, beta):
    """((1 + b2) * P) * R / (R + b2 * P), every operation a float64 rounding of its own, 0 when P == 0"""
    if P == 0.0:
        return 0.0
    b2 = beta * beta
    num = ((1.0 + b2) * P) * R
    den = R + b2 * P
    return num / den


def rouge_l(cand, refs, beta=BETA, lcs_fn=lcs, joint=False):
    """the score of one candidate caption against its reference captions (lists of ids, already cut)"""
    if not cand:
        return 0.0
    P = R = best = 0.0
    for ref in refs:
        if not ref:
            continue
        n = float(lcs_fn(cand, ref))
        p, r = n / float(len(cand)), n / float(len(ref))
        P, R = max(P, p), max(R, r)
        best = max(best, f_score(p, r, beta))
    return best if joint else f_score(P, R, beta)


def rouge(fed, last, greedy, refs, n_refs, end_id, beta, baseline, K, lcs_fn=lcs, joint=False):
    """the kernel on its own arrays: fed (R, T) and last (R,) (row b*K + k; tokens fed[r, 1:], last[r]), greedy (T, ld) or
    None, refs (B, M, Lr), n_refs (B,).  Returns (adv float64 (R,), score (B, K+1), counted int (R,), lcs int (B, K+1, M))."""
    fed, last, refs = np.asarray(fed), np.asarray(last), np.asarray(refs)
    R, T = fed.shape
    B, M = R // K, refs.shape[1]
    samples = np.concatenate([fed[:, 1:], last[:, None]], 1)
    score = np.zeros((B, K + 1), np.float64)
    adv = np.zeros(R, np.float64)
    table = np.zeros((B, K + 1, M), np.int64)
    for b in range(B):
        nr = min(max(int(n_refs[b]), 0), M)
        rs = [caption(refs[b, j], end_id) for j in range(nr)]
        cands = [caption(samples[b * K + k], end_id) for k in range(K)]
        if baseline == 0:
            cands.append(caption(np.asarray(greedy)[:T, b], end_id))
        for c, cand in enumerate(cands):
            score[b, c] = rouge_l(cand, rs, beta, lcs_fn, joint)
            for j, r in enumerate(rs):
                table[b, c, j] = lcs_fn(cand, r)
        if baseline == 0:
            adv[b * K:(b + 1) * K] = score[b, :K] - score[b, K]
        else:
            tot = 0.0
            for k in range(K):
                tot += score[b, k]
            adv[b * K:(b + 1) * K] = score[b, :K] - (tot - score[b, :K]) / (K - 1)
    cnt = np.array([counted(row, end_id) for row in samples], np.int64)
    return adv, score, cnt, table


class RougeMockMixin:
    """``caption_rouge`` of a mock backend (tests/mock_backend.py's buffers), the header's refusals as assertions"""

    def caption_rouge(self, fed, T, last, greedy, ldg, refs, n_refs, M_, Lr, B_, K, end_id, beta, baseline, adv, score=None,
                      counted=None, lcs=None):
        from mock_backend import flat
        assert B_ > 0 and 1 <= T <= 64 and 1 <= Lr <= 64 and 1 <= K <= 16 and 1 <= M_ <= 8 and beta > 0 and np.isfinite(beta)
        assert baseline in (0, 1) and (baseline == 0 or K >= 2) and (baseline == 1 or (greedy is not None and ldg >= B_))
        assert adv is not None and counted is not None
        R = B_ * K
        a, s, c, t = rouge(flat(fed)[:R * T].reshape(R, T), flat(last)[:R],
                           None if baseline else flat(greedy)[:T * ldg].reshape(T, ldg),
                           flat(refs)[:B_ * M_ * Lr].reshape(B_, M_, Lr), flat(n_refs)[:B_], end_id, beta, baseline, K)
        flat(adv)[:R] = a.astype(np.float32)
        if score is not None:
            flat(score)[:B_ * (K + 1)] = s.reshape(-1)
        flat(counted)[:R] = c
        if lcs is not None:
            flat(lcs)[:B_ * (K + 1) * M_] = t.reshape(-1)
