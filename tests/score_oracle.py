"""Float64 restatement of caption log-likelihood scoring (score_captions of nic.NIC and lc_nic.NIC): the kernel
tnt_caption_score_f32 from its header definition, model-level scoring on the inference forwards of oracle.models, and a
MockBackend that adds the kernel and records the row count of every encoder-side call."""
import numpy as np

from mock_backend import MockBackend, flat, mat


def counted(cap, end_id, steps=None):
    """(R, steps) bool: position j = 1..steps is counted iff none of w_1..w_{j-1} is end_id or 0, and w_j != 0"""
    cap = np.asarray(cap)
    steps = cap.shape[1] - 1 if steps is None else steps
    w = cap[:, 1:steps + 1]
    term = (w == 0) | (w == end_id)
    before = np.cumsum(term, 1) - term
    return (before == 0) & (w != 0)


def caption_score(logits, cap, end_id, steps=None):
    """tnt_caption_score_f32 in float64.  logits (steps*R, V) t-major (row (j-1)*R + r) or (steps, R, V); cap (R, T).
    Returns (tok_lp (steps, R), cap_lp (R,), cap_len (R,)); a counted id outside [0, V) gives NaN"""
    cap = np.asarray(cap)
    R, T = cap.shape
    steps = T - 1 if steps is None else steps
    x = np.asarray(logits, np.float64).reshape(steps, R, -1)
    V = x.shape[2]
    m = counted(cap, end_id, steps).T                               # (steps, R)
    w = cap[:, 1:steps + 1].T
    bad = m & ((w < 0) | (w >= V))
    ws = np.clip(w, 0, V - 1)
    tok = np.zeros((steps, R))
    for j in range(steps):
        for r in range(R):
            if m[j, r]:                                             # rows that do not count are not read
                row = x[j, r]
                mx = row.max()
                tok[j, r] = row[ws[j, r]] - (mx + np.log(np.exp(row - mx).sum()))
    tok[bad] = np.nan
    return tok, tok.sum(0), m.sum(0).astype(np.int32)


def model_logits(orc, data):
    """the logits (T-1, B, V) float64 of the oracle's inference forward that score positions 1..T-1"""
    _, cache = orc.forward(tuple(np.asarray(v) for v in data), training=False)
    return np.asarray(cache["logits"], np.float64)[:, :-1].transpose(1, 0, 2)


def score_model(orc, x, a0, c0, captions, end_id):
    """score_captions in float64: captions (B, T) or (B, C, T) -> (logprob, length, tok_lp (B, [C,] T-1)).  Every
    (scan, candidate) pair is one row of the oracle's inference forward (moving statistics: rows are independent)."""
    caps = np.asarray(captions)
    flat2 = caps.ndim == 2
    caps = caps[:, None, :] if flat2 else caps
    B, C, T = caps.shape
    rep = lambda v: np.repeat(np.asarray(v), C, axis=0)
    rows = caps.reshape(B * C, T)
    lg = model_logits(orc, (rep(x), rows, rep(a0), rep(c0)))
    tok, lp, ln = caption_score(lg, rows, end_id)
    lp, ln, tok = lp.reshape(B, C), ln.reshape(B, C), tok.T.reshape(B, C, T - 1)
    return (lp[:, 0], ln[:, 0], tok[:, 0]) if flat2 else (lp, ln, tok)


def ranks(scores, captions):
    """rank of caption b for scan b: distinct candidates scoring strictly higher, by a stable argsort of the row"""
    caps = np.asarray(captions)
    B = len(caps)
    out = np.zeros(B, np.int64)
    for b in range(B):
        order = np.argsort(-scores[b], kind="stable")
        seen, r = set(), 0
        for c in order:
            if scores[b, c] <= scores[b, b]:
                break
            key = tuple(caps[c])
            if key not in seen:
                seen.add(key)
                r += 1
        out[b] = r
    return out


class ScoreMockBackend(MockBackend):
    """MockBackend plus tnt_caption_score_f32 (include/tnt_hip.h).  ``enc_rows``: (call, rows) of every launch that works
    on the voxel-wide input or the encoder's normalisation; ``score_rows``: the R of every scoring launch"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.enc_rows, self.score_rows, self.input_width = [], [], None

    def caption_score(self, logits, ld, V, cap, T, steps, R, end_id, tok_lp, cap_lp, cap_len=None):
        assert ld >= V and end_id < V and 1 <= steps <= T - 1 and cap_lp is not None
        self.score_rows.append(R)
        c = flat(cap)[:R * T].reshape(R, T)
        x = mat(logits, steps * R, V, ld).astype(np.float64)
        tok, lp, ln = caption_score(x, c, end_id, steps)
        if tok_lp is not None:
            flat(tok_lp)[:steps * R] = tok.reshape(-1)
        flat(cap_lp)[:R] = lp
        if cap_len is not None:
            flat(cap_len)[:R] = ln

    def gemm(self, A, B, C, M, N, K, *a, **k):
        if K == self.input_width:
            self.enc_rows.append(("gemm", M))
        return super().gemm(A, B, C, M, N, K, *a, **k)

    def batchnorm_fwd(self, x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, *a, **k):
        self.enc_rows.append(("batchnorm_fwd", rows))
        return super().batchnorm_fwd(x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, *a, **k)

    def locally_dense_fwd(self, x, ldx, idx, goff, W, bias, pre, y, B, *a, **k):
        self.enc_rows.append(("locally_dense_fwd", B))
        return super().locally_dense_fwd(x, ldx, idx, goff, W, bias, pre, y, B, *a, **k)


# ---------------------------------------------------------------------------------------------------- shared test inputs
END = 2
TINY = {"dense": dict(B=5, N=23, T=6, V=13, U=16, E=10), "attention": dict(B=4, N=41, R=5, D=16, A=6, U=16, Et=12, V=13, T=5)}
SMALL = {"dense": dict(B=8, N=500, T=6, V=101, U=32, E=32), "attention": dict(B=8, N=2000, R=36, D=32, A=32, U=64, Et=64, V=501, T=15)}


def make_captions(rng, R, T, V, end_id=END):
    """(R, T) int32 captions, start token 1; by row: terminator at position 1, mid-caption, never, a 0 before the
    terminator, all padding, terminator at the last position"""
    cap = rng.integers(3, V, (R, T)).astype(np.int32)
    cap[:, 0] = 1
    for r in range(R):
        kind = r % 6
        if kind == 0:
            cap[r, 1] = end_id if end_id > 0 else 0
            cap[r, 2:] = 0
        elif kind == 1:
            cap[r, T // 2] = end_id if end_id > 0 else 0
            cap[r, T // 2 + 1:] = 0
        elif kind == 3:
            cap[r, 2] = 0
            cap[r, T - 1] = end_id if end_id > 0 else 0
        elif kind == 4:
            cap[r, 1:] = 0
        elif kind == 5 and end_id > 0:
            cap[r, T - 1] = end_id
    return cap


def build_pair(kind, d, rng, device="cpu", seed=11, **kw):
    """(model, float64 oracle with the same weights) of nic.NIC ("dense") or lc_nic.NIC ("attention") at dims ``d``, with
    Dropout rates that an inference forward must ignore and moving statistics away from (0, 1)"""
    from oracle import models as M
    from helpers import tiny_groups
    if kind == "dense":
        from masters_thesis_amd.nic import NIC
        args = (d["N"], d["U"], d["E"], d["V"], d["T"], 0.1, 0.2, 0.2, 0.01, 3e-5, 1e-5)
        model, orc = NIC(*args, device=device, seed=seed, **kw), M.NICDense(*args)
    else:
        from masters_thesis_amd.lc_nic import NIC
        g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
        args = (g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], 0.1, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 3e-5, 1e-5)
        model, orc = NIC(*args, device=device, seed=seed, **kw), M.LcNIC(*args)
    orc.init_params(rng)
    for k in orc.p:
        if k.endswith("moving_mean"):
            orc.p[k] = orc.p[k] + 0.1 * rng.standard_normal(orc.p[k].shape)
        elif k.endswith("moving_variance"):
            orc.p[k] = orc.p[k] * (0.5 + rng.random(orc.p[k].shape))
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def scans(rng, d):
    """(betas (B, N), a0, c0) float32 with non-zero initial state"""
    x = rng.standard_normal((d["B"], d["N"])).astype(np.float32)
    a0 = (0.1 * rng.standard_normal((d["B"], d["U"]))).astype(np.float32)
    c0 = (0.1 * rng.standard_normal((d["B"], d["U"]))).astype(np.float32)
    return x, a0, c0


def ident_case(kind, device="cpu", seed=7, **kw):
    """the small-shape identification case both the host and the GPU ranking tests use: (model, oracle, (x, a0, c0),
    captions (B, T))"""
    rng = np.random.default_rng(seed)
    d = SMALL[kind]
    model, orc = build_pair(kind, d, rng, device, **kw)
    x, a0, c0 = scans(rng, d)
    caps = make_captions(rng, d["B"], d["T"], d["V"])
    caps[4, 1:3] = (5, END)                    # row 4 (all padding in make_captions) gets a short caption instead
    return model, orc, (x, a0, c0), caps


def rank_margin_check(got_scores, want_scores, caps):
    """the ranking check of both suites: for scan b and candidate c != b, the device order of (c, b) equals the float64
    order wherever the float64 scores differ by more than twice the model-level bound 1e-4 * max(1, |logprob|); returns
    (pairs checked, pairs left out, mismatches)"""
    B = len(caps)
    left = bad = checked = 0
    for b in range(B):
        for c in range(B):
            if c == b or tuple(caps[c]) == tuple(caps[b]):
                continue
            bound = 1e-4 * max(1.0, abs(want_scores[b, c]), abs(want_scores[b, b]))
            if abs(want_scores[b, c] - want_scores[b, b]) <= 2 * bound:
                left += 1
                continue
            checked += 1
            bad += (got_scores[b, c] > got_scores[b, b]) != (want_scores[b, c] > want_scores[b, b])
    return checked, left, bad
