"""Float64 restatement of tnt_caption_reward_f32 (include/tnt_hip.h) on padded id arrays: captions cut at the first
terminator, 64-bit gram keys, the table lookup, CIDEr-D and BLEU-4 from their definitions, and both baselines.  Written
from the header's definition and the published formulas, not from evaluate.CiderD / evaluate.sentence_bleu, which
tests/test_host_reward.py compares it with."""
import math

import numpy as np


def caption(ids, end_id):
    """the tokens before the first end_id or 0 (end_id < 0: only 0 terminates)"""
    out = []
    for w in ids:
        w = int(w)
        if w == 0 or (end_id >= 0 and w == end_id):
            break
        out.append(w)
    return out


def counted(ids, end_id):
    """positions up to and including the first terminator, at most len(ids)"""
    return min(len(caption(ids, end_id)) + 1, len(ids))


def gram_key(gram):
    """w0 | w1<<16 | w2<<32 | w3<<48, or None when a word is outside [1, 65535] (such a gram is in no table)"""
    key = 0
    for i, w in enumerate(gram):
        if not 1 <= w <= 65535:
            return None
        key |= w << (16 * i)
    return key


def table_of(corpus):
    """(keys uint64 ascending, idf float64, params float64 {log(ndoc), sigma = 6}) of a corpus: a list of documents, each
    a list of references; df(g) = the number of documents with g in some reference"""
    ndoc = len(corpus)
    df = {}
    for doc in corpus:
        seen = set()
        for ref in doc:
            ref = [int(w) for w in ref]
            for k in range(1, 5):
                for i in range(len(ref) - k + 1):
                    seen.add(gram_key(ref[i:i + k]))
        for key in seen:
            df[key] = df.get(key, 0) + 1
    logn = math.log(float(max(ndoc, 1)))
    keys = sorted(df)
    idf = [logn - math.log(max(1.0, float(df[k]))) for k in keys]
    return np.array(keys, np.uint64), np.array(idf, np.float64), np.array([logn, 6.0], np.float64)


def tf(seq, k):
    """{k-gram: count}, in the order of the first positions"""
    out = {}
    for i in range(len(seq) - k + 1):
        g = tuple(seq[i:i + k])
        out[g] = out.get(g, 0) + 1
    return out


def idf_of(gram, keys, idf, logn):
    key = gram_key(gram)
    if key is None or len(keys) == 0:
        return logn
    i = int(np.searchsorted(keys, np.uint64(key)))
    return float(idf[i]) if i < len(keys) and int(keys[i]) == key else logn


def cider_d(cand, refs, keys, idf, params):
    """10 * mean over the references and k = 1..4 of the clipped tf-idf cosine times the Gaussian length penalty"""
    if not refs:
        return 0.0
    logn, sigma = float(params[0]), float(params[1])
    total = 0.0
    for ref in refs:
        pen = math.exp(-float(len(cand) - len(ref)) ** 2 / (2.0 * sigma * sigma))
        s = 0.0
        for k in range(1, 5):
            tc, tr = tf(cand, k), tf(ref, k)
            w = {g: idf_of(g, keys, idf, logn) for g in list(tc) + list(tr)}
            num = sum(min(c, tr.get(g, 0)) * tr.get(g, 0) * w[g] ** 2 for g, c in tc.items())
            nc = sum((c * w[g]) ** 2 for g, c in tc.items())
            nr = sum((c * w[g]) ** 2 for g, c in tr.items())
            if nc * nr != 0.0:
                s += num / math.sqrt(nc * nr) * pen
        total += s / 4.0
    return 10.0 * total / len(refs)


def bleu4(cand, refs, eps=0.1):
    """BLEU-4, uniform weights, method-1 smoothing, match counts clipped by the maximum over the references, brevity
    penalty against the closest reference length (the shorter on a tie)"""
    if not refs or not cand:
        return 0.0
    n = []
    for k in range(1, 5):
        tc = tf(cand, k)
        trs = [tf(r, k) for r in refs]
        n.append(sum(min(c, max(t.get(g, 0) for t in trs)) for g, c in tc.items()))
    if n[0] == 0:
        return 0.0
    rl = sorted((abs(len(r) - len(cand)), len(r)) for r in refs)[0][1]
    bp = 1.0 if len(cand) > rl else math.exp(1.0 - rl / len(cand))
    s = sum(0.25 * math.log((n[k] if n[k] > 0 else eps) / max(1, len(cand) - k)) for k in range(4))
    return bp * math.exp(s)


def reward(fed, last, greedy, refs, n_refs, keys, idf, params, end_id, kind, baseline, K):
    """the kernel on its own arrays: fed (R, T) and last (R,) (row b*K + k; tokens fed[r, 1:], last[r]), greedy (T, ld) or
    None, refs (B, M, Lr), n_refs (B,).  Returns (adv float64 (R,), score (B, K+1), counted int (R,))."""
    fed, last, refs = np.asarray(fed), np.asarray(last), np.asarray(refs)
    R, T = fed.shape
    B = R // K
    samples = np.concatenate([fed[:, 1:], last[:, None]], 1)
    score = np.zeros((B, K + 1), np.float64)
    adv = np.zeros(R, np.float64)
    fn = (lambda c, rs: cider_d(c, rs, keys, idf, params)) if kind == 0 else bleu4
    for b in range(B):
        nr = min(max(int(n_refs[b]), 0), refs.shape[1])
        rs = [caption(refs[b, j], end_id) for j in range(nr)]
        for k in range(K):
            score[b, k] = fn(caption(samples[b * K + k], end_id), rs)
        if baseline == 0:
            score[b, K] = fn(caption(np.asarray(greedy)[:T, b], end_id), rs)
            adv[b * K:(b + 1) * K] = score[b, :K] - score[b, K]
        else:
            tot = 0.0
            for k in range(K):
                tot += score[b, k]
            adv[b * K:(b + 1) * K] = score[b, :K] - (tot - score[b, :K]) / (K - 1)
    cnt = np.array([counted(row, end_id) for row in samples], np.int64)
    return adv, score, cnt
