"""Float64 restatement of scheduled sampling for the dense model (nic.NIC(scheduled_sampling=...)): the schedule, the
coin and the draw from oracle/philox.py, the per-row decisions on a float64 NICDense with the fed ids forced, and a
MockBackend with tnt_scheduled_feedback_f32 from its header definition."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from oracle.philox import uniform24
from mock_backend import MockBackend, flat, mat, _keep

S_LSTM_IN = 48
S_SS_COIN, S_SS_DRAW = 176, 208


def schedule_p(kind, params, i):
    """p after i updates: kind 0 linear (p0, slope, p_max), kind 1 inverse sigmoid (k, -, p_max); float64, then float32"""
    a, b, c = (float(v) for v in params)
    i = float(i)
    if kind == 0:
        return np.float32(np.clip(a + b * i, 0.0, c))
    with np.errstate(over="ignore"):
        return np.float32(c * (1.0 - a / (a + np.exp(np.float64(i) / a))))


def spec_p(spec, i):
    return schedule_p(spec.kind_id, spec.params(), i)


def coin(B, p, seed, site, step):
    """True where row b feeds the model's token: element b of (seed, site, step) dropped at rate p (u < p)"""
    return uniform24(B, int(seed), int(site), int(step)) < np.float32(p)


def greedy_ids(logits):
    """argmax per row, ties to the lowest index, NaN never wins, a row without a winner gives 0; and the top-2 margin"""
    x = np.where(np.isnan(logits), -np.inf, np.asarray(logits, np.float64))
    ids = x.argmax(-1)
    srt = np.sort(x, -1)
    margin = srt[:, -1] - srt[:, -2] if x.shape[1] > 1 else np.full(x.shape[0], np.inf)
    return ids, np.where(np.isfinite(margin), margin, np.inf)


def model_tokens(logits, mode, seed, site, step):
    """(ids, margin) of the model's tokens for every row: mode 0 greedy, mode 1 tnt_sample_rows_f32's draw at T = 1"""
    if mode == 0:
        return greedy_ids(logits)
    return O.sample_rows(logits, 1.0, True, seed, site, step)


class SSMockBackend(MockBackend):
    """MockBackend plus tnt_scheduled_feedback_f32 (include/tnt_hip.h); counts its calls and records each call's coins"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ss_calls = 0
        self.ss_log = []

    def scheduled_feedback(self, logits, ld, V, table, E, w, ldw, N, fed, T, col, text, ldt, xz, ldz, B, rate, seed, site,
                           step, step_dev, lwidth, lcol0, kind, mode, sched, counter, coin_site, draw_site):
        self.ss_calls += 1
        assert 1 <= col < T and E % 4 == 0 and ld >= V and ldw >= N and ldz >= N and ldt >= E
        st = (step + (int(flat(step_dev)[0]) if step_dev is not None else 0)) & 0xFFFFFFFF
        p = schedule_p(kind, flat(sched)[:3], int(flat(counter)[0]))
        c = coin(B, p, seed, coin_site, st)
        f = flat(fed)[:B * T].reshape(B, T)
        ids = np.clip(f[:, col].astype(np.int64), 0, V - 1)
        if c.any():
            mids, _ = model_tokens(mat(logits, B, V, ld), mode, seed, draw_site, st)
            ids = np.where(c, mids, ids)
            f[c, col] = ids[c]
        self.ss_log.append((col, float(p), c.copy(), ids.copy()))
        rows = mat(table, V, E, E)[ids].astype(np.float32)
        if rate > 0:
            e = np.arange(B)[:, None].astype(np.int64) * lwidth + lcol0 + np.arange(E)[None, :]
            k = _keep(e, rate, seed, site, st)
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
            rows = np.where(k, rows * scale, np.float32(0))
        mat(text, B, E, ldt)[...] = rows
        mat(xz, B, N, ldz)[...] = rows.astype(np.float64) @ mat(w, E, N, ldw).astype(np.float64)


class SSNICDense(M.NICDense):
    """NICDense with the fed ids forced, and the float64 decisions of the scheduled-sampling forward"""

    def decide(self, data, drop, spec, i):
        """the fed ids (B, T) of one training step after i updates, stream step drop.step; also the margin of every
        model decision (inf for ground-truth positions) and the coins (B, T-1)"""
        x, cap, a0, c0 = data
        fed = np.array(cap, np.int64)
        B, T = fed.shape
        p = spec_p(spec, i)
        margin = np.full((B, T), np.inf)
        coins = np.zeros((B, T - 1), bool)
        for j in range(T - 1):
            _, cache = self.forward((x, fed, a0, c0), training=True, drop=drop)
            c = coin(B, p, drop.seed, S_SS_COIN + j, drop.step)
            coins[:, j] = c
            if c.any():
                ids, mg = model_tokens(cache["logits"][:, j], spec.mode_id, drop.seed, S_SS_DRAW + j, drop.step)
                fed[c, j + 1] = ids[c]
                margin[c, j + 1] = mg[c]
        return fed, margin, coins

    def loss_and_grads(self, data, fed, y_ids, drop):
        """loss, accuracy and every gradient (with the L2 terms) of the step run on the fed ids, against y_ids"""
        x, _, a0, c0 = data
        probs, cache = self.forward((x, fed, a0, c0), training=True, drop=drop)
        ce, acc = self.metrics(probs, y_ids)
        grads, _ = self.backward(probs, cache, y_ids)
        return ce, acc, grads
