"""numpy reference of the recurrent part of the attention caption model: the chain of T attention -> LSTM steps that
tnt_lc_seq_fwd[_drop]_f32 / tnt_lc_seq_bwd[_drop]_f32 run as one launch each (include/tnt_hip.h), restated from the
per-step oracles of oracle/ops.py and the Philox streams of oracle/philox.py.  float64 by default; ``dtype=np.float32``
evaluates the same formulas in float32 (the measure of what float32 arithmetic costs at a given shape).

Layouts are the library's: gate-interleaved xz / gates / dz [T][B][U][4], Wc [D][U][4], Ur [U][U][4], bias [U][4]
(il / unil of tests/test_gpu_ops.py convert to and from keras' [.., 4U] gate blocks), v [A], hs / cs [T+1][B][U] with
slab 0 the initial state.  Nothing here imports the package under test."""
import numpy as np

from oracle import ops as O
from oracle.philox import keep_mask
from test_gpu_ops import il, unil

SLOPE = 0.2


def chain_masks(T, B, R, D, A, r_attn, r_in, in_lwidth, seed, site_attn0, site_in0, step):
    """the keep masks of the T steps: attention dropout over the flat [B][R][A] scores (site_attn0 + i), context input
    dropout over the logical [B][in_lwidth] LSTM input row, of which the context is columns [0, D) (site_in0 + i)"""
    ka = [keep_mask((B, R, A), r_attn, seed, site_attn0 + i, step) if r_attn > 0 else None for i in range(T)]
    ki = [keep_mask((B, in_lwidth), r_in, seed, site_in0 + i, step)[:, :D] if r_in > 0 else None for i in range(T)]
    return ka, ki


def out_masks(T, B, U, rate, seed, site_out0, step):
    """the Dropout behind the LSTM: one site per step, rows_per_site = B (tnt_dropout_f32)"""
    return [keep_mask((B, U), rate, seed, site_out0 + i, step) if rate > 0 else None for i in range(T)]


def chain_fwd(F, P, W2, b2, v, bv, xz, Wc, Ur, zb, h0, c0, r_attn=0.0, r_in=0.0, masks=None, out_drop=None,
              dtype=np.float64):
    """T steps of: attention on hs[i] -> context input dropout -> LSTM step with z = xz[i] + bias + ctx_d Wc + h Ur.
    masks = chain_masks(...); out_drop = (rate, out_masks(...)) adds ``hd`` = Dropout(hs[1:]).
    Returns a dict of hs, cs [T+1][B][U], gates [T][B][U][4], qpre [T][B][A], alpha [T][B][R], ctx, ctx_d [T][B][D]."""
    c = lambda x: np.asarray(x, dtype)
    F, P, W2, b2, v, bv, xz, h0, c0 = map(c, (F, P, W2, b2, v, bv, xz, h0, c0))
    T, B, U = xz.shape[0], xz.shape[1], xz.shape[2]
    Wc_k, Ur_k, zb_k, xz_k = unil(c(Wc)), unil(c(Ur)), unil(c(zb)), unil(xz)
    ka, ki = masks if masks is not None else ([None] * T, [None] * T)
    hs, cs = [h0], [c0]
    out = {k: [] for k in ("gates", "qpre", "alpha", "ctx", "ctx_d")}
    for i in range(T):
        (ctx, alpha, _), cache = O.attention_step_fwd(hs[i], F, P, W2, b2, v[:, None], bv, ka[i], r_attn, SLOPE)
        ctx_d = O.dropout_fwd(ctx, ki[i], r_in)
        h2, c2, (gi, gf, gg, go, _, _, _) = O.lstm_step_fwd(xz_k[i] + zb_k + ctx_d @ Wc_k, hs[i], cs[i], Ur_k)
        hs.append(h2); cs.append(c2)
        out["gates"].append(il(np.concatenate([gi, gf, gg, go], axis=1), U))
        out["qpre"].append(cache[1]); out["alpha"].append(alpha); out["ctx"].append(ctx); out["ctx_d"].append(ctx_d)
    res = {k: np.stack(x) for k, x in out.items()}
    res["hs"], res["cs"] = np.stack(hs), np.stack(cs)
    if out_drop is not None:
        rate, ko = out_drop
        res["hd"] = np.stack([O.dropout_fwd(res["hs"][i + 1], ko[i], rate) for i in range(T)])
    return res


def chain_bwd(F, P, W2, v, Wc, Ur, qpre, alpha, gates, cs, dout, r_attn=0.0, r_in=0.0, masks=None, alpha_mse_coef=0.0,
              out_drop=None, dtype=np.float64):
    """The reverse of chain_fwd from the values the forward stored (gates, cs, alpha, qpre; tanh(P + q) and the masks are
    recomputed, as in the kernels), for i = T-1 .. 0: the LSTM step backward on dout[i] + the recurrent and the
    attention query gradients of step i+1, the context gradient dz[i] Wc^T through the input dropout, the attention step
    backward.  dout [T][B][U] is the gradient w.r.t. hs[1:], or w.r.t. Dropout(hs[1:]) with out_drop = (rate, masks).
    alpha_mse_coef: dalpha += coef (alpha - 1), the gradient of c sum (1 - alpha)^2 with coef = 2c.
    Returns dz [T][B][U][4] (= the gradient w.r.t. xz), dqpre [T][B][A], the accumulated dP [B][R][A], dF [B][R][D]
    (F and P taken as independent inputs) and dvb [B][A] (per-sample parts of dv), dh0 and dc0."""
    c = lambda x: np.asarray(x, dtype)
    F, P, W2, v, qpre, alpha, cs, dout = map(c, (F, P, W2, v, qpre, alpha, cs, dout))
    T, B, U = dout.shape
    Wc_k, Ur_k, g_k = unil(c(Wc)), unil(c(Ur)), unil(c(gates))
    ka, ki = masks if masks is not None else ([None] * T, [None] * T)
    dz, dqpre = [None] * T, [None] * T
    dP, dF, dvb = np.zeros_like(P), np.zeros_like(F), np.zeros((B, P.shape[2]), dtype)
    dh_next, dc = np.zeros((B, U), dtype), np.zeros((B, U), dtype)       # gradients reaching hs[i+1] / cs[i+1] from step i+1
    for i in range(T - 1, -1, -1):
        do = dout[i] if out_drop is None else O.dropout_bwd(dout[i], out_drop[1][i], out_drop[0])
        gi, gf, gg, go = (g_k[i][:, k * U:(k + 1) * U] for k in range(4))
        dz_k, dh_rec, dc = O.lstm_step_bwd(do + dh_next, dc, (gi, gf, gg, go, cs[i], np.tanh(cs[i + 1]), None), Ur_k)
        dz[i] = il(dz_k, U)
        dctx = O.dropout_bwd(dz_k @ Wc_k.T, ki[i], r_in)
        s = np.tanh(P + O.act_fwd(qpre[i], O.ACT_LEAKY, SLOPE)[:, None, :])
        sd = O.dropout_fwd(s, ka[i], r_attn)
        ext = alpha_mse_coef * (alpha[i] - 1) if alpha_mse_coef else None
        cache = (np.zeros((B, W2.shape[0]), dtype), qpre[i], s, sd, alpha[i], ka[i], r_attn)
        dh_att, dF_i, dsum, _, _, _, _ = O.attention_step_bwd(dctx, F, W2, v[:, None], cache, SLOPE, dalpha_ext=ext)
        dqpre[i] = O.act_bwd(qpre[i], dsum.sum(axis=1), O.ACT_LEAKY, SLOPE)
        # the per-sample parts of dv (the oracle's dv is their sum over the batch): de as in attention_step_bwd
        dalpha = (dctx[:, None, :] * F).sum(axis=2) + (ext if ext is not None else 0)
        de = alpha[i] * (dalpha - (alpha[i] * dalpha).sum(axis=1, keepdims=True))
        dvb += (sd * de[:, :, None]).sum(axis=1)
        dP += dsum; dF += dF_i
        dh_next = dh_rec + dh_att
    return dict(dz=np.stack(dz), dqpre=np.stack(dqpre), dP=dP, dF=dF, dvb=dvb, dh0=dh_next, dc0=dc)
