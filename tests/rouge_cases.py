"""The inputs tests/test_gpu_rouge.py gives tnt_caption_rouge_f32, built on the host so that tests/test_host_rouge.py can
check, without a GPU, that they tell the definition from its near misses.  Every case is a dict in the layout of
tests/test_gpu_reward.py's make_case; ``want(name, baseline)`` is the restatement's answer, computed once per process."""
import functools

import numpy as np

import rouge_oracle as RG

END = 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# (B, K, T, M, Lr, vocabulary): B in {1, 3, 5}, T and Lr in {1, 2, 15, 63, 64}, K in {1, 2, 16}, M in {1, 8}, vocabularies of
# 2, 3 and 50 words (the small ones give long subsequences with many ties); more than one workgroup, more pairs than waves
SHAPES = [(1, 1, 1, 1, 1, 2), (3, 2, 2, 8, 2, 3), (5, 16, 15, 8, 15, 3), (3, 2, 63, 1, 64, 2), (5, 2, 64, 8, 63, 50),
          (1, 16, 64, 1, 64, 3), (3, 1, 15, 8, 64, 50), (5, 2, 64, 8, 64, 2), (3, 16, 2, 1, 15, 2)]


def rows(rng, n, L, vocab):
    """n rows of L ids over the ``vocab`` words 3 .. 3 + vocab - 1: row i % 4 == 0 has no terminator, i % 4 == 1 a zero and
    behind it an end token (where L >= 3), i % 4 == 2 an early end token followed by garbage, i % 4 == 3 words, zeros and
    end tokens at random"""
    out = np.empty((n, L), np.int32)
    for i in range(n):
        row = rng.integers(3, 3 + vocab, L)
        if i % 4 == 1 and L >= 3:
            z = int(rng.integers(1, L - 1))
            row[z], row[int(rng.integers(z + 1, L))] = 0, END
        elif i % 4 == 2:
            row[int(rng.integers(0, max(1, L // 2)))] = END
        elif i % 4 == 3:
            stop = rng.random(L) < 0.04
            row = np.where(stop, rng.integers(0, 2, L) * END, row)
        out[i] = row
    return out


def pack(w, greedy, refs, n_refs, rng, extra=2):
    """samples w (R, T), greedy (B, T), refs (B, M, Lr) -> the kernel's arrays; greedy gets ``extra`` columns of garbage
    behind its B (ldg > B), fed a column 0 that is never read"""
    R, T = w.shape
    B, M, Lr = refs.shape
    fed = np.concatenate([rng.integers(-5, 99, (R, 1)).astype(np.int32), w[:, :T - 1]], 1)
    g = np.concatenate([greedy.T, rng.integers(I32_MIN, I32_MAX, (T, extra)).astype(np.int32)], 1)
    return dict(fed=np.ascontiguousarray(fed, np.int32), last=np.ascontiguousarray(w[:, T - 1], np.int32),
                greedy=np.ascontiguousarray(g, np.int32), refs=np.ascontiguousarray(refs, np.int32),
                n_refs=np.asarray(n_refs, np.int32), w=w, B=B, K=R // B, T=T, M=M, Lr=Lr)


def make_case(seed, B, K, T, M, Lr, vocab):
    rng = np.random.default_rng(seed)
    w = rows(rng, B * K, T, vocab)
    greedy = rows(rng, B, T, vocab)
    refs = rows(rng, B * M, Lr, vocab).reshape(B, M, Lr)
    n_refs = rng.integers(1, M + 1, B).astype(np.int32)
    n_refs[0] = M
    return pack(w, greedy, refs, n_refs, rng)


def forced_case():
    """B = 5, K = 2, T = Lr = 64, M = 2, lengths and values set by hand:
      scan 0  sample 0 is 64 words without a terminator and reference 0 is the same row (lcs = 64: the all-ones mask),
              reference 1 and sample 1 are its reverse; the greedy caption opens with the end token (length 0)
      scan 1  sample 0 has length 1, sample 1 opens with the end token; reference 0 opens with a 0 (length 0), reference 1
              has length 1; the greedy caption is 64 equal words
      scan 2  ids at INT32_MIN, INT32_MAX and above 65535, against references that hold the same ids and ones that differ
              in the high 16 bits only
      scan 3  n_refs = 0;  scan 4  n_refs = 11, above M (clamped to 2)"""
    rng = np.random.default_rng(77)
    B, K, T, M, Lr = 5, 2, 64, 2, 64
    w = rows(rng, B * K, T, 3)
    greedy = rows(rng, B, T, 3)
    refs = rows(rng, B * M, Lr, 3).reshape(B, M, Lr)
    full = rng.integers(3, 53, 64).astype(np.int32)
    w[0], w[1], refs[0, 0], refs[0, 1] = full, full[::-1], full, full[::-1]
    greedy[0, 0] = END
    w[2, :] = 0
    w[2, 0] = 7
    w[3, 0] = END
    refs[1, 0, 0] = 0
    refs[1, 1, :] = 0
    refs[1, 1, 0] = 7
    greedy[1, :] = 7
    wide = np.array([I32_MIN, 70000, I32_MAX, 65536 + 3, 3, -1, 70000, I32_MIN + 1], np.int64)
    w[4, :] = 0
    w[4, :8] = wide
    w[5, :] = 0
    w[5, :8] = wide[::-1]
    greedy[2, :] = 0
    greedy[2, :4] = [3, 4464, 65535, 2 ** 16]                                  # 70000 & 0xffff == 4464
    refs[2, 0, :] = 0
    refs[2, 0, :8] = wide
    refs[2, 1, :] = 0
    refs[2, 1, :6] = [0x7fff0000, 4464, 65535, 3, 65536 + 3, I32_MAX]
    case = pack(w, greedy, refs, [2, 2, 2, 0, 11], rng)
    return case


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "forced":
        return forced_case()
    i = int(name)
    return make_case(1000 + i, *SHAPES[i])


NAMES = tuple(str(i) for i in range(len(SHAPES))) + ("forced",)


@functools.lru_cache(maxsize=None)
def want(name, baseline, end_id=END, beta=RG.BETA, variant="true"):
    """(adv, score, counted, lcs) of the restatement, or of a near miss: ``variant`` "substring", "joint"; treat the tuple
    as read only"""
    c = case(name)
    kw = dict(substring=dict(lcs_fn=RG.substring), joint=dict(joint=True)).get(variant, {})
    return RG.rouge(c["fed"], c["last"], c["greedy"], c["refs"], c["n_refs"], end_id, beta, baseline, c["K"], **kw)


def baselines(name):
    return (0, 1) if case(name)["K"] >= 2 else (0,)
