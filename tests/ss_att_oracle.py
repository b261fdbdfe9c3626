"""Float64 restatement of scheduled sampling for the attention model (lc_nic.NIC(scheduled_sampling=...)) -- TEST
INFRASTRUCTURE ONLY.  The definition is tnt_scheduled_feedback2_f32's (include/tnt_hip.h).

``SSAttLcNIC`` is ``oracle.models.LcNIC`` plus the step-by-step decisions: for token position j + 1 (j = 0 .. T-2) the
teacher-forced decoder runs on the ids fed so far, step j's logits give the model's token (argmax, or tnt_sample_rows_f32's
draw), and the coin of ss_oracle picks between it and the caption.  The decoder is causal, so step j's logits only depend
on positions 0 .. j.  ``fed_ids`` (B, T) forces the ids the later steps are run on (float32 and float64 argmaxes may
differ where two logits nearly tie, as in tests/naive_oracle.py), so every decision is checked on the device's history.
Loss and gradients are the teacher-forced oracle's over the fed ids: every Dropout mask is the teacher-forced one.

``SSAttMockBackend`` adds tnt_scheduled_feedback2_f32, restated from its header text, to ss_oracle's mock backend.
"""
import numpy as np

from oracle import models as M
from mock_backend import flat, mat, _keep
from ss_oracle import SSMockBackend, coin, model_tokens, schedule_p, spec_p, S_SS_COIN, S_SS_DRAW  # noqa: F401


def masked_rows(rows, B, E, masks, seed, step):
    """table rows (B, E) float32 through the masks [(rate, site, lwidth, lcol0), ...] in order: element
    b*lwidth + lcol0 + e kept -> x / (1 - rate) in float32, dropped -> 0"""
    rows = np.asarray(rows, np.float32)
    for rate, site, lwidth, lcol0 in masks:
        if rate > 0:
            e = np.arange(B)[:, None].astype(np.int64) * lwidth + lcol0 + np.arange(E)[None, :]
            k = _keep(e, rate, seed, site, step)
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
            rows = np.where(k, rows * scale, np.float32(0))
    return rows


class SSAttMockBackend(SSMockBackend):
    """SSMockBackend plus tnt_scheduled_feedback2_f32; counts its calls and records each call's (col, p, coins, ids)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ss2_calls = 0
        self.ss2_log = []

    def scheduled_feedback2(self, logits, ld, V, table, E, w, ldw, N, fed, T, col, text, ldt, xz, ldz, B, rate, seed, site,
                            step, step_dev, lwidth, lcol0, kind, mode, sched, counter, coin_site, draw_site, rate_t, site_t,
                            lwidth_t, lcol0_t):
        self.ss2_calls += 1
        assert 1 <= col < T and E % 4 == 0 and ld >= V and ldw >= N and ldz >= N and ldt >= E
        assert rate_t == 0 or (lwidth_t % 4 == 0 and lcol0_t % 4 == 0 and 0 <= lcol0_t and lcol0_t + E <= lwidth_t)
        st = (step + (int(flat(step_dev)[0]) if step_dev is not None else 0)) & 0xFFFFFFFF
        p = schedule_p(kind, flat(sched)[:3], int(flat(counter)[0]))
        c = coin(B, p, seed, coin_site, st)
        f = flat(fed)[:B * T].reshape(B, T)
        ids = np.clip(f[:, col].astype(np.int64), 0, V - 1)
        if c.any():
            mids, _ = model_tokens(mat(logits, B, V, ld), mode, seed, draw_site, st)
            ids = np.where(c, mids, ids)
            f[c, col] = ids[c]
        self.ss2_log.append((col, float(p), c.copy(), ids.copy()))
        rows = masked_rows(mat(table, V, E, E)[ids], B, E, [(rate_t, site_t, lwidth_t, lcol0_t), (rate, site, lwidth, lcol0)],
                           seed, st)
        mat(text, B, E, ldt)[...] = rows
        mat(xz, B, N, ldz)[...] = rows.astype(np.float64) @ mat(w, E, N, ldw).astype(np.float64)


class SSAttLcNIC(M.LcNIC):
    """LcNIC with the scheduled-sampling decisions of one training step"""

    def decide(self, data, drop, spec, i, fed_ids=None):
        """the fed ids (B, T) of one training step after i updates on the stream step drop.step; the top-2 margin of every
        model decision (inf at ground-truth positions and column 0) and the coins (B, T-1).
        fed_ids (B, T): the history is forced -- step j runs on fed_ids[:, :j+1] (column 0: the caption's) -- and the
        result is the restatement's own decision at every position given that history."""
        x, cap, a0, c0 = data
        fed = np.array(cap, np.int64)
        B, T = fed.shape
        p = spec_p(spec, i)
        margin = np.full((B, T), np.inf)
        coins = np.zeros((B, T - 1), bool)
        F, _ = self._encode(np.asarray(x).astype(self.p['lstm/kernel'].dtype), True, drop)
        if fed_ids is not None:               # causal decoder: one pass over the forced history gives every step's logits
            hist = np.array(fed_ids, np.int64)
            hist[:, 0] = fed[:, 0]
            logits = self._decode_fwd(F, hist, a0, c0, True, drop)[1]['logits']
        for j in range(T - 1):
            if fed_ids is None:
                logits = self._decode_fwd(F, fed, a0, c0, True, drop)[1]['logits']
            c = coin(B, p, drop.seed, S_SS_COIN + j, drop.step)
            coins[:, j] = c
            if c.any():
                ids, mg = model_tokens(logits[:, j], spec.mode_id, drop.seed, S_SS_DRAW + j, drop.step)
                margin[c, j + 1] = mg[c]
                fed[c, j + 1] = ids[c]
        return fed, margin, coins

    def loss_and_grads(self, data, fed, y_ids, drop):
        """loss, accuracy, attention metric and every gradient (with the L2 terms) of the teacher-forced step on the fed
        ids, against y_ids"""
        x, _, a0, c0 = data
        (probs, attn), cache = self.forward((x, np.asarray(fed, np.int64), a0, c0), training=True, drop=drop)
        ce, acc, al = self.metrics(probs, attn, y_ids)
        grads, _ = self.backward(probs, cache, y_ids)
        return ce, acc, al, grads
