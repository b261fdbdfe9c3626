"""Restatement of consensus decoding (tnt_consensus_mix_f32 / tnt_consensus_spread_i32, definitions in include/tnt_hip.h)
in float64: the two kernels, and the consensus greedy, sampled and beam decodes of the caption models, built on the
decode-step restatements of tests/constrain_oracle.py (oracle.models underneath) with the members' distributions mixed at
every step and the common word fed back to all of them.  Rows are member-major: member g of mixed row r is row g*Rm + r."""
import numpy as np

from oracle import models as M
from oracle.models_ms import MsLcNIC
from constrain_oracle import ConstrainedLcNIC, ConstrainedNICDense, constrain_rows
from topkp_oracle import sample_topkp

MODES = ("mean", "logmean")


# ---------------------------------------------------------------------------------------------------- the kernels
def first_max(p):
    """tnt_argmax_rows_f32's rule on rows of p: the first maximum, NaN entries ignored, nothing above -inf gives 0"""
    q = np.where(np.isnan(p), -np.inf, p)
    return np.where(np.max(q, axis=-1) > -np.inf, np.argmax(q, axis=-1), 0).astype(np.int64)


def mix(logits, G, w=None, mode="mean"):
    """logits (G*Rm, V) -> (p (Rm, V) float64, token (Rm,)): the mixture of the members' softmaxes and its first maximum"""
    x = np.asarray(logits, np.float64)
    V = x.shape[1]
    x = x.reshape(G, -1, V)
    w = np.full(G, 1.0 / G) if w is None else np.asarray(w, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=-1, keepdims=True)
        empty = ~(m > -np.inf)                       # a member row with nothing above -inf: m = 0, s = 1
        m = np.where(empty, 0.0, m)
        s = np.where(empty, 1.0, np.exp(x - m).sum(axis=-1, keepdims=True))
        if mode == "mean":
            p = np.zeros(x.shape[1:])
            for g in range(G):                       # ascending member order
                p = p + w[g] * np.exp(x[g] - m[g]) / s[g]
        else:
            l = np.zeros(x.shape[1:])
            for g in range(G):
                l = l + w[g] * ((x[g] - m[g]) - np.log(s[g]))
            L = l.max(axis=-1, keepdims=True)
            none = ~(L > -np.inf)                    # every l_v is -inf: the row is all zero
            e = np.exp(l - np.where(none, 0.0, L))
            p = np.where(none, 0.0, e / np.where(none, 1.0, e.sum(axis=-1, keepdims=True)))
    return p, first_max(p)


def spread(token, parent, fin, Rm, G):
    """what a step chose on the Rm mixed rows -> the G*Rm member rows; each of token / parent / fin may be None"""
    off = np.repeat(np.arange(G, dtype=np.int64) * Rm, Rm)
    t = None if token is None else np.tile(np.asarray(token)[:Rm], G)
    p = None if parent is None else (np.tile(np.asarray(parent)[:Rm], G) + off).astype(np.asarray(parent).dtype)
    f = None if fin is None else np.tile(np.asarray(fin)[:Rm], G)
    return t, p, f


# ---------------------------------------------------------------------------------------------------- the models
class ConsensusMsLcNIC(ConstrainedLcNIC, MsLcNIC):
    """the multi-subject model's decode step: subject q's inference encoder on batch slice q, the shared decoder"""

    def _encode(self, x, training, drop):
        Bs = x.shape[0] // self.S
        Fs = [self._encode_s(x[q * Bs:(q + 1) * Bs], q, training, drop)[0] for q in range(self.S)]
        return np.concatenate(Fs, axis=0), None


def rel_gap(p):
    """(p1 - p2) / p1 of the two largest entries of every row"""
    s = np.sort(p, axis=-1)
    return (s[:, -1] - s[:, -2]) / s[:, -1]


def consensus_decode(orc, x, a0, c0, start_seq, max_len, G, mode="mean", w=None, con=None, sampler=None):
    """Greedy (sampler None) or sampled (sampler = (temperature, top_k, top_p, seed, step), tnt_sample_topkp_f32 on the
    mixed rows) consensus decode: x, a0, c0 hold G*M rows member-major, start_seq M entries.  ``con``: the constraints of
    tests/constrain_oracle.py, applied to every member row from the common history.  Returns (ids (M, max_len), probs
    (max_len, M, V): the mixtures, gap (M,): the smallest relative top-2 gap of the mixture over the steps (greedy) or the
    sampler's smallest margin)."""
    start = np.asarray(start_seq).reshape(-1)
    Mn = start.shape[0]
    assert x.shape[0] == G * Mn
    word = np.tile(start, G)
    st = orc.dec_init(x, a0, c0)
    ids = np.zeros((Mn, 0), np.int64)
    probs, gap = [], np.full(Mn, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, np.tile(ids, (G, 1)), con, i)
        p, tok = mix(logits, G, w, mode)
        if sampler is None:
            gap = np.minimum(gap, rel_gap(p))
        else:
            t, k, tp, seed, step = sampler
            tok, mg = sample_topkp(p, t, k, tp, False, seed, M.S_SAMPLE + i, step)
            gap = np.minimum(gap, mg)
        probs.append(p)
        ids = np.concatenate([ids, tok[:, None]], axis=1)
        word = np.tile(tok, G)
    return ids, np.stack(probs, axis=0), gap


def consensus_beam(orc, x, a0, c0, start_seq, max_len, G, k=5, end_id=-1, mode="mean", w=None, con=None):
    """Beam search on the mixture (the loop of constrain_oracle.constrained_beam with the M*k mixed rows in the softmax's
    place): decoder rows [G][M][k].  Returns (sequences (M, k, max_len), scores (M, k), margin (M,): the smallest score gap
    that decided a rank)."""
    start = np.asarray(start_seq).reshape(-1)
    Mn, V = start.shape[0], orc.V
    Mk = Mn * k
    assert x.shape[0] == G * Mn
    st = orc.dec_init(x, a0, c0, k)
    word = np.repeat(np.tile(start, G), k)
    score = np.zeros((Mn, k)); score[:, 1:] = -1e30
    fin = np.zeros((Mn, k), bool)
    seqs = np.zeros((Mn, k, 0), np.int64)
    margin = np.full(Mn, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, np.tile(seqs.reshape(Mk, i), (G, 1)), con, i, live=np.tile(~fin.reshape(-1), G))
        probs, _ = mix(logits, G, w, mode)
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
        orc.dec_reorder(st, spread(None, parent, None, Mk, G)[1])
        seqs = np.concatenate([np.take_along_axis(seqs, pj[:, :, None], axis=1), tv[:, :, None]], axis=2)
        fin = np.take_along_axis(fin, pj, axis=1) | (tv == end_id)
        score = best
        word = np.tile(tv.reshape(-1), G)
    return seqs, score, margin


# ---------------------------------------------------------------------------------------------------- shared test cases
def golden_case(kind):
    """(orc, ctor, kw): the float64 decode restatement loaded with the weights of the tiny golden fixture of ``kind``
    ("dense": nic_dense_tiny, "lc": lc_nic_tiny, "ms": ms2_tiny), the positional constructor arguments the restatement and
    the device model share, and the keyword ones"""
    import os
    import sys
    gold_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if gold_dir not in sys.path:
        sys.path.insert(0, gold_dir)
    import make_golden as G
    name = {"dense": "nic_dense_tiny", "lc": "lc_nic_tiny", "ms": "ms2_tiny"}[kind]
    with np.load(os.path.join(gold_dir, name + ".npz"), allow_pickle=False) as z:
        gold = {k: z[k] for k in z.files}
    weights = {k[2:]: v for k, v in gold.items() if k.startswith("w/")}
    kw = {}
    if kind == "dense":
        ctor = (G.N, G.U, G.ET, G.V, G.T, 0, 0, 0, 0.01, 3e-5, 1e-5)
        orc = ConstrainedNICDense(*ctor)
    else:
        groups = [gold["gidx"][a:b] for a, b in zip(gold["goff"][:-1], gold["goff"][1:])]
        ctor = ((groups, [G.D] * G.R), G.U, 512, G.ET, G.A, G.V, G.T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
        if kind == "ms":
            kw = dict(n_subjects=2)
            orc = ConsensusMsLcNIC(*ctor, **kw)
        else:
            orc = ConstrainedLcNIC(*ctor)
    # the device model holds float32 weights: the restatement computes in float64 from the same values
    orc.p = {k: np.asarray(v).astype(np.float32).astype(np.float64) for k, v in weights.items()}
    return orc, ctor, kw


def scans(G, Mn, seed, identical=False):
    """(x (G*Mn, N) float32 member-major, z (G*Mn, U) zeros, start (Mn,)) at the tiny fixtures' shape: G different scans per
    image, or G copies of the same Mn scans"""
    from make_golden import N, U                    # golden_case has put tests/golden on the path
    rng = np.random.default_rng(seed)
    x = np.tile(rng.standard_normal((Mn, N)), (G, 1)) if identical else rng.standard_normal((G * Mn, N))
    return x.astype(np.float32), np.zeros((G * Mn, U), np.float32), np.ones(Mn, np.int64)
