"""Restatement of constrained caption decoding (tnt_decode_constrain_f32, definition in include/tnt_hip.h): the rules on
one row of logits in float64 and as the bitwise float32 expectation, a MockBackend with the op (ping-pong history with
parents included), and the constrained greedy, sampled and beam decodes of both caption models, built on the existing
float64 restatements (oracle.models, tests/dense_beam_oracle.py, tests/topkp_oracle.py) with the rule applied to each
step's logits."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import flat, mat
from dense_beam_oracle import BeamMockBackend, BeamNICDense
from topkp_oracle import TopkpMockBackend, sample_topkp


# ---------------------------------------------------------------------------------------------------- the rules
def touched(history, V, n, m, end_id, bad_ids, i):
    """(penalised, banned): the in-range distinct history tokens, and the banned tokens, of step i"""
    h = [int(t) for t in history]
    assert len(h) == i, (len(h), i)
    distinct = {v for v in h if 0 <= v < V}
    banned = {int(v) for v in bad_ids if 0 <= int(v) < V}
    if i < m and 0 <= end_id < V:
        banned.add(int(end_id))
    if n >= 1 and i >= n:
        ctx = h[i - n + 1:]                                   # the last n-1 tokens
        for s in range(0, i - n + 1):                         # s + n - 1 <= i - 1
            if h[s:s + n - 1] == ctx and 0 <= h[s + n - 1] < V:
                banned.add(h[s + n - 1])
    return distinct, banned


def _apply(x, history, theta, n, m, end_id, bad_ids, i, dtype):
    x = np.array(x, dtype=dtype)
    V = x.shape[0]
    th = dtype(theta)
    distinct, banned = touched(history, V, n, m, end_id, bad_ids, i)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in distinct:                                   # once per distinct token
            x[v] = x[v] / th if x[v] > 0 else x[v] * th
    for v in banned:                                         # a ban overrides the penalty
        x[v] = -np.inf
    return x


def constrain_logits(x, history, theta, n, m, end_id, bad_ids, i):
    """the constrained logits of one row at step i, float64"""
    return _apply(x, history, theta, n, m, end_id, bad_ids, i, np.float64)


def constrain_logits_f32(x, history, theta, n, m, end_id, bad_ids, i):
    """the same in float32, one correctly rounded operation per written value: the kernel's bits"""
    return _apply(x, history, theta, n, m, end_id, bad_ids, i, np.float32)


def constrain_rows(x, hist, con, i, live=None, f32=False):
    """rows of logits (rows, V) with their histories (rows, i); ``con`` = dict(theta, n, m, end_id, bad_ids); rows with
    live False keep their logits"""
    fn = constrain_logits_f32 if f32 else constrain_logits
    out = np.array(x, dtype=np.float32 if f32 else np.float64)
    for r in range(out.shape[0]):
        if live is None or live[r]:
            out[r] = fn(out[r], hist[r], con["theta"], con["n"], con["m"], con["end_id"], con["bad_ids"], i)
    return out


def as_dict(c, end_id=-1):
    """model_base.DecodeConstraints (and beam search's end_id) -> the restatement's parameters"""
    eid = c.end_id if c.end_id >= 0 else end_id
    return dict(theta=c.repetition_penalty, n=c.no_repeat_ngram_size, m=c.min_length, end_id=eid if c.min_length > 0 else -1,
                bad_ids=tuple(c.bad_ids))


# ---------------------------------------------------------------------------------------------------- the mock
class ConstrainMockBackend(BeamMockBackend, TopkpMockBackend):
    """MockBackend (with tnt_beam_step_f32 and tnt_sample_topkp_f32) plus tnt_decode_constrain_f32 from the header text;
    logs its calls, and the history it left, in ``constrain_calls``"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.constrain_calls = []

    def decode_constrain(self, logits, ld, V, rows, i, hist_in, hist_out, ldh, last_token, parent, fin, theta, n, m, end_id,
                         bad_ids, n_bad):
        assert rows > 0 and V > 0 and ld >= V and 0 <= i <= 64 and ldh >= max(i, 1)
        assert np.isfinite(np.float32(theta)) and theta >= 1 and n >= 0 and m >= 0 and (m == 0 or end_id >= 0)
        assert 0 <= n_bad <= 64 and (n_bad == 0 or bad_ids is not None)
        assert logits is not None and hist_out is not None
        assert i == 0 or (hist_in is not None and last_token is not None)
        assert hist_in is None or hist_in.data_ptr() != hist_out.data_ptr()
        X = mat(logits, rows, V, ld)
        ho = mat(hist_out, rows, max(i, 1), ldh)
        if i > 0:
            par = np.arange(rows)
            if parent is not None:
                p = flat(parent)[:rows].astype(np.int64)
                par = np.where((p >= 0) & (p < rows), p, par)
            ho[:, :i] = np.concatenate([mat(hist_in, rows, i - 1, ldh)[par], flat(last_token)[:rows, None]], axis=1)
        hist = ho[:, :i].copy()
        live = np.ones(rows, bool) if fin is None else flat(fin)[:rows] == 0
        con = dict(theta=theta, n=n, m=m, end_id=end_id, bad_ids=tuple(flat(bad_ids)[:n_bad].tolist()) if n_bad else ())
        X[...] = constrain_rows(X, hist, con, i, live, f32=True)
        self.constrain_calls.append(dict(i=i, rows=rows, hist=hist, parent=None if parent is None else flat(parent)[:rows].copy()))


# ---------------------------------------------------------------------------------------------------- the decodes
class ConstrainedNICDense(BeamNICDense):
    """the dense model's decode step as logits: BeamNICDense._step in front of its softmax"""

    def dec_init(self, x, a0, c0, k=1):
        a, c = self._features(x, a0, c0)
        return dict(a=np.repeat(a, k, axis=0), c=np.repeat(c, k, axis=0), first=True)

    def dec_logits(self, st, word):
        p = self.p
        m = np.ones((word.shape[0], 1), bool) if st["first"] else (word != 0)[:, None]    # greedy_predict's mask rule
        e = p['emb_text/embeddings'][word]
        h2, c2, _ = O.lstm_step_fwd(e @ p['lstm/kernel'] + p['lstm/bias'], st["a"], st["c"], p['lstm/recurrent_kernel'])
        whole = np.where(m, h2, 0)
        st.update(a=np.where(m, h2, st["a"]), c=np.where(m, c2, st["c"]), first=False)
        return whole @ p['time_distributed_softmax/kernel'] + p['time_distributed_softmax/bias']

    def dec_reorder(self, st, rows):
        st.update(a=st["a"][rows], c=st["c"][rows])


class ConstrainedLcNIC(M.LcNIC):
    """the attention model's decode step as logits: the loop body of LcNIC.greedy_predict in front of its softmax"""

    def dec_init(self, x, a0, c0, k=1):
        p = self.p
        dt = p['lstm/kernel'].dtype
        F, _ = self._encode(x.astype(dt), False, M.DropCtx(training=False))
        P, _ = O.attention_proj_fwd(F, p['attention/W1/kernel'], p['attention/W1/bias'])
        rep = lambda t: np.repeat(t, k, axis=0)
        return dict(F=rep(F), P=rep(P), a=rep(a0.astype(dt)), c=rep(c0.astype(dt)))

    def dec_logits(self, st, word):
        p = self.p
        text = p['emb_text/embeddings'][word]
        (ctx, _, _), _ = O.attention_step_fwd(st["a"], st["F"], st["P"], p['attention/W2/kernel'], p['attention/W2/bias'],
                                              p['attention/V/kernel'], p['attention/V/bias'])
        a, c = self._cell(np.concatenate([ctx, text], axis=1), st["a"], st["c"])
        st.update(a=a, c=c)
        inter, _ = O.dense_fwd(a, p['time_distributed_nonlinear/kernel'], p['time_distributed_nonlinear/bias'], O.ACT_LEAKY)
        return inter @ p['time_distributed_softmax/kernel'] + p['time_distributed_softmax/bias']

    def dec_reorder(self, st, rows):
        st.update(a=st["a"][rows], c=st["c"][rows])


def _top2_gap(probs):
    """log p of the best token minus log p of the runner-up, per row"""
    s = np.sort(probs, axis=-1)
    with np.errstate(divide="ignore"):
        return np.log(s[:, -1]) - np.log(np.maximum(s[:, -2], 1e-300))


def constrained_decode(orc, x, a0, c0, start_seq, max_len, con=None, sampler=None):
    """Greedy (sampler None) or sampled (sampler = (temperature, top_k, top_p, seed, step): tnt_sample_topkp_f32 on the
    stream (seed, S_SAMPLE + position, step)) decode of ``orc`` with the constraints ``con`` (None: none) applied to every
    step's logits from the row's own tokens.  Returns (ids (B, max_len) int64, probs (max_len, B, V): the constrained
    distributions, margin (B,): the smallest decision margin over the steps -- the log-probability gap of the two best
    tokens for greedy, the sampler's own margin for a draw)."""
    word = np.asarray(start_seq).reshape(-1)
    B = word.shape[0]
    st = orc.dec_init(x, a0, c0)
    ids = np.zeros((B, 0), np.int64)
    probs, margin = [], np.full(B, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if con is not None:
            logits = constrain_rows(logits, ids, con, i)
        p = O.softmax(logits)
        if sampler is None:
            word = p.argmax(-1)
            margin = np.minimum(margin, _top2_gap(p))
        else:
            t, k, tp, seed, step = sampler
            word, mg = sample_topkp(p, t, k, tp, False, seed, M.S_SAMPLE + i, step)
            margin = np.minimum(margin, mg)
        probs.append(p)
        ids = np.concatenate([ids, word[:, None]], axis=1)
    return ids, np.stack(probs, axis=0), margin


def constrained_beam(orc, x, a0, c0, start_seq, max_len, k=5, end_id=-1, con=None, trace=None):
    """Beam search of ``orc`` (the loop of BeamNICDense.beam_search / LcNIC.beam_search) with the constraints applied to
    every live row's logits from the row's own path.  Returns (sequences (B, k, max_len) int64, scores (B, k), margin
    (B,)) as those do.  ``trace`` (a list) receives every step's (B*k, i) histories."""
    B, V = x.shape[0], orc.V
    st = orc.dec_init(x, a0, c0, k)
    word = np.repeat(np.asarray(start_seq).reshape(-1), k)
    score = np.zeros((B, k)); score[:, 1:] = -1e30
    fin = np.zeros((B, k), bool)
    seqs = np.zeros((B, k, 0), np.int64)
    margin = np.full(B, np.inf)
    for i in range(max_len):
        logits = orc.dec_logits(st, word)
        if trace is not None:
            trace.append(seqs.reshape(B * k, i).copy())
        if con is not None:
            logits = constrain_rows(logits, seqs.reshape(B * k, i), con, i, live=~fin.reshape(-1))
        probs = O.softmax(logits)
        cand = score[:, :, None] + np.log(np.maximum(probs, 1e-30)).reshape(B, k, V)
        frozen = np.full((B, k, V), -np.inf); frozen[:, :, 0] = score
        cand = np.where(fin[:, :, None], frozen, cand).reshape(B, k * V)
        order = np.argsort(-cand, axis=1, kind='stable')          # ties: lower flat index first
        top = order[:, :k]
        best = np.take_along_axis(cand, top, axis=1)
        if k > 1:
            margin = np.minimum(margin, np.min(best[:, :-1] - best[:, 1:], axis=1))
        margin = np.minimum(margin, best[:, -1] - np.take_along_axis(cand, order[:, k:k + 1], axis=1)[:, 0])
        pj, tv = top // V, top % V
        orc.dec_reorder(st, (np.arange(B)[:, None] * k + pj).reshape(-1))
        seqs = np.concatenate([np.take_along_axis(seqs, pj[:, :, None], axis=1), tv[:, :, None]], axis=2)
        fin = np.take_along_axis(fin, pj, axis=1) | (tv == end_id)
        score = best
        word = tv.reshape(-1)
    return seqs, score, margin


# ---------------------------------------------------------------------------------------------------- properties
def violations(seq, n, m, end_id, bad_ids):
    """what one emitted sequence violates, looking at its tokens up to and including the first end_id: a set out of
    {"ngram", "min_length", "bad"}"""
    seq = [int(t) for t in seq]
    if end_id >= 0 and end_id in seq:
        seq = seq[:seq.index(end_id) + 1]
    out = set()
    if n >= 1:
        grams = [tuple(seq[s:s + n]) for s in range(len(seq) - n + 1)]
        if len(set(grams)) < len(grams):
            out.add("ngram")
    if end_id >= 0 and end_id in seq[:m]:
        out.add("min_length")
    if set(seq) & set(int(v) for v in bad_ids):
        out.add("bad")
    return out


# ---------------------------------------------------------------------------------------------------- shared test cases
# the shapes of the tiny and the mid-size golden fixtures (tests/golden/make_golden.py)
SHAPES = {"tiny": dict(B=3, N=37, R=4, D=16, A=3, U=16, ET=6, V=11, T=4),
          "mid": dict(B=8, N=2000, R=36, D=32, A=32, U=64, ET=64, V=501, T=15)}
HEAD_SCALE = {"tiny": 8.0, "mid": 40.0}


def restatement_case(kind, shape, seed):
    """(orc, x, z, start, T, ctor): a restatement model of ``kind`` ("dense" / "lc") at a fixture shape, its weights
    rounded to float32 (a device model holds the same values) and its head kernel scaled so that the decisions are not
    near ties; ``ctor`` = the positional constructor arguments both the restatement and the device model take"""
    from helpers import tiny_groups
    d = SHAPES[shape]
    rng = np.random.default_rng(seed)
    if kind == "dense":
        ctor = (d["N"], d["U"], d["ET"], d["V"], d["T"], 0, 0, 0, 0.01, 3e-5, 1e-5)
        orc = ConstrainedNICDense(*ctor).init_params(rng)
    else:
        g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
        ctor = (g, d["U"], 512, d["ET"], d["A"], d["V"], d["T"], 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
        orc = ConstrainedLcNIC(*ctor).init_params(rng)
    orc.p['time_distributed_softmax/kernel'] = orc.p['time_distributed_softmax/kernel'] * HEAD_SCALE[shape]
    orc.p = {k: v.astype(np.float32).astype(np.float64) for k, v in orc.p.items()}
    x = rng.standard_normal((d["B"], d["N"])).astype(np.float32)
    z = np.zeros((d["B"], d["U"]), np.float32)
    return orc, x, z, np.ones(d["B"], np.int64), d["T"], ctor


def case_constraints(shape):
    """(DecodeConstraints arguments, beam width, end id) of the model-level comparisons at a fixture shape"""
    if shape == "tiny":                          # V = 11: 1 + 4 + 1 + 3 <= 11
        return dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=2, bad_ids=(3,)), 3, 2
    return dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3, bad_ids=(0, 1, 4)), 5, 2


def run_path(orc, path, x, z, start, T, con, k, end_id, seed):
    """one of the three decode paths of the restatement -> (ids, probs or scores, margin); ids (B, T) or (B, k, T)"""
    if path == "greedy":
        return constrained_decode(orc, x, z, z, start, T, con)
    if path == "sample":
        return constrained_decode(orc, x, z, z, start, T, con, (0.9, 8, 0.95, seed, 3))
    return constrained_beam(orc, x, z, z, start, T, k=k, end_id=end_id, con=con)
