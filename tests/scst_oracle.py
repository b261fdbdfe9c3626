"""Float64 restatement of self-critical sequence training for the dense model (nic.NIC(self_critical=...)): the loss
kernel tnt_scst_cce_f32 from its header definition, a MockBackend that adds it, and the whole step -- the rollout (the
scheduled-sampling decisions of tests/ss_oracle.py at p = 1 in sample mode, plus the last draw), the greedy baseline
(NICDense.greedy_predict), the advantages, and the loss and every gradient by torch autograd of
(1/R) sum_r -adv_r sum_t m_rt log p(w_rt) with the sampled ids held fixed."""
import numpy as np
import torch

from oracle import models as M
from oracle import ops as O
from mock_backend import flat, mat
from ss_oracle import SSMockBackend, SSNICDense

S_SCST_LAST = 240


def counted_mask(fed, last, end_id):
    """m (R, T): 1 for the tokens w_1..w_T up to and including the first terminator (end_id or 0)"""
    w = np.concatenate([np.asarray(fed)[:, 1:], np.asarray(last).reshape(-1, 1)], 1)
    term = (w == 0) | (w == end_id)
    before = np.cumsum(term, 1) - term            # terminators among w_1..w_{t-1}
    return (before == 0).astype(np.float64), w


def scst_cce(logits, fed, last, adv, end_id, gscale):
    """tnt_scst_cce_f32 in float64: logits (T*R, V), row (t-1)*R + r.  Returns (loss_row, lp_row, dlogits, m (R, T))"""
    fed = np.asarray(fed)
    R, T = fed.shape
    m, w = counted_mask(fed, last, end_id)
    x = np.asarray(logits, np.float64).reshape(T, R, -1)
    V = x.shape[2]
    mx = x.max(-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(x - mx).sum(-1))
    wt = w.T                                                           # (T, R)
    lp = np.take_along_axis(x, wt[..., None], 2)[..., 0] - lse
    mt = m.T
    a = np.asarray(adv, np.float64)[None, :]
    counted = (mt > 0) & (a != 0)
    loss = np.where(counted, -a * lp, 0.0)
    p = np.exp(x - lse[..., None])
    oh = np.zeros_like(p)
    np.put_along_axis(oh, wt[..., None], 1.0, 2)
    d = np.where(counted[..., None], gscale * a[..., None] * (p - oh), 0.0)
    return loss.reshape(-1), np.where(mt > 0, lp, 0.0).reshape(-1), d.reshape(T * R, V), m


class SCSTMockBackend(SSMockBackend):
    """SSMockBackend plus tnt_scst_cce_f32 (include/tnt_hip.h); counts its calls"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.scst_calls = 0

    def scst_cce(self, logits, ld, V, fed, T, last, adv, end_id, loss_row, lp_row, dlogits, R, gscale):
        self.scst_calls += 1
        assert ld >= V and end_id < V
        x = mat(logits, T * R, V, ld).astype(np.float64)
        f = flat(fed)[:R * T].reshape(R, T)
        la = flat(last)[:R]
        assert np.all((la >= 0) & (la < V)) and np.all((f >= 0) & (f < V))
        loss, lp, d, _ = scst_cce(x, f, la, flat(adv)[:R], end_id, gscale)
        if loss_row is not None:
            flat(loss_row)[:T * R] = loss
        if lp_row is not None:
            flat(lp_row)[:T * R] = lp
        mat(dlogits, T * R, V, ld)[...] = d


def expand(data, K):
    """the R = B*K rows of a step: row b*K + k is copy k of scan b"""
    return tuple(np.repeat(np.asarray(v), K, axis=0) for v in data[:4])


def rollout(orc, data_r, drop):
    """the sampled ids of the rollout over the expanded rows: fed (R, T) (cap[:, 0] kept, w_1..w_{T-1} drawn on
    S_SS_DRAW + j), last (R,) drawn from step T's logits on S_SCST_LAST; and the draw margins"""
    from masters_thesis_amd.model_base import ScheduledSampling
    spec = ScheduledSampling.linear(1.0, 0.0, 1.0, mode="sample")
    fed, margin, _ = orc.decide(data_r, drop, spec, 0)
    x, _, a0, c0 = data_r
    _, cache = orc.forward((x, fed, a0, c0), training=True, drop=drop)
    last, mg = O.sample_rows(cache["logits"][:, -1], 1.0, True, drop.seed, S_SCST_LAST, drop.step)
    return fed, last, np.minimum(margin[:, 1:].min(1), mg)


def greedy(orc, data, T):
    """the greedy baseline captions (B, T): NICDense.greedy_predict from cap[:, 0]"""
    x, cap, a0, c0 = data
    probs = orc.greedy_predict(np.asarray(x), np.asarray(a0), np.asarray(c0), np.asarray(cap)[:, 0], T)
    return probs[:, :, 0, :].argmax(-1).T


def policy_grads(orc, data_r, fed, last, adv, end_id, drop):
    """(loss, grads with the L2 terms) of (1/R) sum_r -adv_r sum_t m log p(w_rt) + L2 by torch autograd in float64, the
    sampled ids and the Dropout masks of the step held fixed"""
    p = orc.p
    x, _, a0, c0 = data_r
    _, cache = orc.forward((x, fed, a0, c0), training=True, drop=drop)      # masks and dropped-out input
    R, T = fed.shape
    U = orc.U
    tp = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k in M.NICDense.TRAINABLE) for k, v in p.items()}
    keep = lambda k, rate: 1.0 if k is None else torch.tensor(np.asarray(k, np.float64) / (1.0 - np.float64(np.float32(rate))))
    pre = torch.tensor(cache["xd"]) @ tp["dense_img/kernel"] + tp["dense_img/bias"]
    y = torch.where(pre > 0, pre, 0.2 * pre) * keep(cache["k_feat"], orc.r_feat)
    if orc.norm == "batch":
        mean, var = y.mean(0), ((y - y.mean(0)) ** 2).mean(0)
    else:
        mean, var = y.mean(1, keepdim=True), ((y - y.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    f = (y - mean) / torch.sqrt(var + O.BN_EPS) * tp["batch_norm/gamma"] + tp["batch_norm/beta"]
    Wl, Ul, bl = tp["lstm/kernel"], tp["lstm/recurrent_kernel"], tp["lstm/bias"]

    def cell(xz, h, c):
        z = xz + h @ Ul
        i, fg, g, o = (torch.sigmoid(z[:, :U]), torch.sigmoid(z[:, U:2 * U]), torch.tanh(z[:, 2 * U:3 * U]),
                       torch.sigmoid(z[:, 3 * U:]))
        c2 = fg * c + i * g
        return o * torch.tanh(c2), c2
    k_l0 = cache["k_l0"][:, 0] if cache["k_l0"] is not None else None
    h, c = cell((f * keep(k_l0, orc.r_lstm)) @ Wl + bl, torch.tensor(a0, dtype=torch.float64),
                torch.tensor(c0, dtype=torch.float64))
    emb = tp["emb_text/embeddings"][torch.tensor(fed, dtype=torch.long)] * keep(cache["k_l1"], orc.r_lstm)
    out = torch.zeros(R, U, dtype=torch.float64)
    m, w = counted_mask(fed, last, end_id)
    lps = []
    for t in range(T):
        h2, c2 = cell(emb[:, t] @ Wl + bl, h, c)
        live = torch.tensor(fed[:, t] != 0)[:, None]
        h, c, out = torch.where(live, h2, h), torch.where(live, c2, c), torch.where(live, h2, out)
        logits = out @ tp["time_distributed_softmax/kernel"] + tp["time_distributed_softmax/bias"]
        lps.append(torch.log_softmax(logits, -1)[torch.arange(R), torch.tensor(w[:, t], dtype=torch.long)])
    lp = torch.stack(lps, 1)
    loss = -(torch.tensor(adv, dtype=torch.float64)[:, None] * torch.tensor(m) * lp).sum() / R
    l2 = (orc.l2_in * (tp["dense_img/kernel"] ** 2).sum() + orc.l2_lstm * (tp["lstm/kernel"] ** 2).sum()
          + orc.l2_out * (tp["time_distributed_softmax/kernel"] ** 2).sum())
    (loss + l2).backward()
    return float(loss.detach()), {k: tp[k].grad.numpy().copy() for k in M.NICDense.TRAINABLE}


class SCSTNICDense(SSNICDense):
    """SSNICDense with the self-critical step"""

    def scst_step(self, sc, data, drop, references=None):
        """one float64 step's sampled ids, advantages, loss and gradients (before the update).  Returns a dict."""
        K = sc.n_samples
        data_r = expand(data, K)
        fed, last, margin = rollout(self, data_r, drop)
        T = fed.shape[1]
        g = greedy(self, data, T) if sc.baseline == "greedy" else None
        if references is None:
            references = [[sc.truncate(row[1:])] for row in np.asarray(data[1])]
        samples = np.concatenate([fed[:, 1:], last[:, None]], 1)
        adv, reward, base, counted = sc.advantages(samples, references, g)
        loss, grads = policy_grads(self, data_r, fed, last, adv, sc.end_id, drop)
        return dict(fed=fed, last=last, margin=margin, greedy=g, adv=adv, reward=reward, base=base, counted=counted,
                    loss=loss, grads=grads, data_r=data_r)
