"""Restatement of the learned initial LSTM state (tnt_init_state_fwd_f32 / tnt_init_state_bwd_f32, definitions in
include/tnt_hip.h) in float64: ``init_fwd`` / ``init_bwd``; ``InitLcNIC``, the float64 oracle model whose decoder starts from
the state its own region features predict and whose backward adds that branch; and ``InitMockBackend``, the CPU stand-in
with the two new backend calls.  Nothing here imports the package under test.

    F [B][R][D]                      the region features the attention reads
    m = mean_r F                     [B][D]
    h0 = tanh(m Wh + bh),  c0 = tanh(m Wc + bc)
    gh = dh0 (1 - h0^2),   gc = dc0 (1 - c0^2)
    dWh = m^T gh, dbh = sum_b gh, dWc, dbc likewise;  dF[b][r] += (gh Wh^T + gc Wc^T)[b] / R

The restatement is checked against central differences in tests/test_host_init_state.py."""
import numpy as np

from oracle import models as M
from oracle import ops as O
from mock_backend import MockBackend, flat

LAYERS = ("hidden_init", "carry_init")
NAMES = tuple(f"{nm}/{w}" for nm in LAYERS for w in ("kernel", "bias"))


def init_fwd(F, Wh, bh, Wc, bc):
    """(h0, c0, m)"""
    F, Wh, bh, Wc, bc = (np.asarray(x, np.float64) for x in (F, Wh, bh, Wc, bc))
    m = F.mean(axis=1)
    return np.tanh(m @ Wh + bh), np.tanh(m @ Wc + bc), m


def init_bwd(dh0, dc0, h0, c0, m, Wh, Wc, R):
    """dict(dWh, dbh, dWc, dbc, dm, dF_row): dF_row [B][D] is what every region row of dF receives"""
    dh0, dc0, h0, c0, m, Wh, Wc = (np.asarray(x, np.float64) for x in (dh0, dc0, h0, c0, m, Wh, Wc))
    gh, gc = dh0 * (1.0 - h0 * h0), dc0 * (1.0 - c0 * c0)
    dm = gh @ Wh.T + gc @ Wc.T
    return dict(dWh=m.T @ gh, dbh=gh.sum(axis=0), dWc=m.T @ gc, dbc=gc.sum(axis=0), dm=dm, dF_row=dm / R)


class InitLcNIC(M.LcNIC):
    """oracle.models.LcNIC with the learned initial state: forward / greedy_predict / beam_search take (h0, c0) from the
    region features F of the scans they were given (the a0 / c0 arguments are ignored), backward adds the gradients of the
    two layers and the branch's share of dF.  ``reg`` is the L2 coefficient of the two kernels.  ``branch_dF = False`` leaves
    the share of dF out and ``zero_h0 = True`` starts the hidden state from zeros: the two ablations the GPU test uses to show
    that the branch is visible in the gradients it is checked in."""
    reg = 0.0
    branch_dF = True
    zero_h0 = False

    def init_params(self, rng, dtype=np.float64, scale=1.0):
        super().init_params(rng, dtype)
        lim = scale * np.sqrt(6.0 / (self.D + self.U))
        for nm in LAYERS:
            self.p[f"{nm}/kernel"] = rng.uniform(-lim, lim, (self.D, self.U)).astype(dtype)
            self.p[f"{nm}/bias"] = (0.01 * rng.standard_normal(self.U)).astype(dtype)
        return self

    def state(self, F):
        p = self.p
        h0, c0, m = init_fwd(F, p["hidden_init/kernel"], p["hidden_init/bias"], p["carry_init/kernel"], p["carry_init/bias"])
        if self.zero_h0:
            h0 = np.zeros_like(h0)
        return h0, c0, m

    def _decode_fwd(self, F, ids, a0, c0, training, drop):
        h0, c0, m = self.state(F)
        out, cache = super()._decode_fwd(F, ids, h0, c0, training, drop)
        cache["init"] = (h0, c0, m)
        return out, cache

    def l2_loss(self):
        return super().l2_loss() + sum(M._l2(self.reg, self.p[f"{nm}/kernel"]) for nm in LAYERS)

    def _decode_bwd(self, probs, cache, y_ids):
        """the plain decoder backward with the last (step 0) results of the two step backwards captured: dh0 = dh_prev +
        dh_att and dc0 = dc of step 0, as CoverageLcNIC wraps oracle.ops.attention_step_bwd"""
        last = {}
        old_l, old_a = O.lstm_step_bwd, O.attention_step_bwd

        def lstm_bwd(*a, **k):
            out = old_l(*a, **k)
            last["dh_prev"], last["dc"] = out[1], out[2]
            return out

        def att_bwd(*a, **k):
            out = old_a(*a, **k)
            last["dh_att"] = out[0]
            return out
        O.lstm_step_bwd, O.attention_step_bwd = lstm_bwd, att_bwd
        try:
            g, sparse, dF = super()._decode_bwd(probs, cache, y_ids)
        finally:
            O.lstm_step_bwd, O.attention_step_bwd = old_l, old_a
        p = self.p
        h0, c0, m = cache["init"]
        dh0 = np.zeros_like(h0) if self.zero_h0 else last["dh_prev"] + last["dh_att"]
        self.last_state_grads = (dh0, last["dc"])
        b = init_bwd(dh0, last["dc"], h0, c0, m, p["hidden_init/kernel"], p["carry_init/kernel"], self.R)
        g["hidden_init/kernel"] = b["dWh"] + 2 * self.reg * p["hidden_init/kernel"]
        g["hidden_init/bias"] = b["dbh"]
        g["carry_init/kernel"] = b["dWc"] + 2 * self.reg * p["carry_init/kernel"]
        g["carry_init/bias"] = b["dbc"]
        if self.branch_dF:
            dF = dF + b["dF_row"][:, None, :]
        return g, sparse, dF

    def scalar_loss(self, data, y_ids, drop):
        """CE + L2 in float64 (what backward differentiates)"""
        (probs, attn), _ = self.forward(data, training=True, drop=drop)
        return self.metrics(probs, attn, y_ids)[0] + self.l2_loss()

    def learn_init_state(self, x):
        F, _ = self._encode(np.asarray(x).astype(self.p["lstm/kernel"].dtype), False, M.DropCtx(training=False))
        return self.state(F)[:2]

    def greedy_predict(self, x, a0, c0, start_seq, max_len, sampler=None):
        h0, c0 = self.learn_init_state(x)
        return super().greedy_predict(x, h0, c0, start_seq, max_len, sampler)

    def beam_search(self, x, a0, c0, start_seq, max_len, k=5, end_id=-1):
        h0, c0 = self.learn_init_state(x)
        return super().beam_search(x, h0, c0, start_seq, max_len, k, end_id)


class InitMockBackend(MockBackend):
    """MockBackend plus tnt_init_state_fwd_f32 / tnt_init_state_bwd_f32, from the header text"""

    def init_state_fwd(self, F, Wh, bh, Wc, bc, fmean, h0, c0, B, R, D, U):
        assert B >= 1 and R >= 1 and U >= 1 and 1 <= D <= 64
        assert all(t is not None for t in (F, Wh, bh, Wc, bc, h0, c0))
        f64 = lambda t, *s: flat(t)[:int(np.prod(s))].reshape(*s).astype(np.float64)
        h, c, m = init_fwd(f64(F, B, R, D), f64(Wh, D, U), f64(bh, U), f64(Wc, D, U), f64(bc, U))
        if fmean is not None:
            flat(fmean)[:B * D] = m.reshape(-1)
        flat(h0)[:B * U] = h.reshape(-1)
        flat(c0)[:B * U] = c.reshape(-1)

    def init_state_bwd(self, dh0, dc0, h0, c0, fmean, Wh, Wc, dWh, dbh, dWc, dbc, dF, B, R, D, U):
        assert B >= 1 and R >= 1 and U >= 1 and 1 <= D <= 64
        assert all(t is not None for t in (dh0, dc0, h0, c0, fmean, Wh, Wc))
        outs = (dWh, dbh, dWc, dbc)
        assert all(t is None for t in outs) or all(t is not None for t in outs)
        f64 = lambda t, *s: flat(t)[:int(np.prod(s))].reshape(*s).astype(np.float64)
        b = init_bwd(f64(dh0, B, U), f64(dc0, B, U), f64(h0, B, U), f64(c0, B, U), f64(fmean, B, D), f64(Wh, D, U),
                     f64(Wc, D, U), R)
        if dWh is not None:                      # written, not accumulated
            flat(dWh)[:D * U] = b["dWh"].reshape(-1)
            flat(dbh)[:U] = b["dbh"]
            flat(dWc)[:D * U] = b["dWc"].reshape(-1)
            flat(dbc)[:U] = b["dbc"]
        if dF is not None:                       # added to
            v = flat(dF)[:B * R * D].reshape(B, R, D)
            v += b["dF_row"][:, None, :].astype(np.float32)
