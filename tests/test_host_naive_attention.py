"""Free-running training of the attention model (lc_nic.NIC(teacher_forcing=False), lc_NIC.call_naive_attention) on CPU:
host orchestration through the mock backend against the float64 restatement (tests/naive_oracle.py), the restatement's
gradients against torch autograd, and the refusals."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd.lc_nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from oracle import ops as O
from helpers import synth_batch, tiny_groups
from mock_backend import MockBackend, flat, mat, _keep
from naive_oracle import NaiveLcNIC, S_NOUT


class NaiveMockBackend(MockBackend):
    """MockBackend plus tnt_greedy_feedback_f32 from its definition in include/tnt_hip.h"""

    def greedy_feedback(self, logits, ld, V, table, E, w, ldw, N, fed, T, col, text, ldt, xz, ldz, B, rate, seed, site,
                        step, step_dev=None, lwidth=0, lcol0=0):
        if step_dev is not None:
            step = (step + int(step_dev[0])) & 0xFFFFFFFF
        x = mat(logits, B, V, ld)
        ids = np.zeros(B, np.int64)
        for b in range(B):
            ok = ~np.isnan(x[b])
            if ok.any():
                ids[b] = np.flatnonzero(x[b] == x[b][ok].max())[0]      # ties: lowest index; NaN never wins
        flat(fed)[np.arange(B) * T + col] = ids
        rows = mat(table, V, E, E)[ids]
        if rate > 0:
            keep = _keep(np.arange(B)[:, None] * lwidth + lcol0 + np.arange(E)[None, :], rate, seed, site, step)
            rows = np.where(keep, rows * (np.float32(1.0) / (np.float32(1.0) - np.float32(rate))), np.float32(0))
        mat(text, B, E, ldt)[...] = rows
        mat(xz, B, N, ldz)[...] = rows.astype(np.float64) @ mat(w, E, N, ldw).astype(np.float64)


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    ops.set_backend(NaiveMockBackend())
    yield
    ops.set_backend(old)


ARGS = dict(B=4, N=41, R=5, D=16, A=6, U=16, Et=12, V=13, T=5)
RATES = [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)]


def make_pair(rng, rates, seed=11, depth=0, teacher_forcing=False, **d):
    d = {**ARGS, **d}
    groups = tiny_groups(d["N"], d["R"], rng)
    g = (groups, [d["D"]] * d["R"])
    model = NIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=seed,
                depth=depth, teacher_forcing=teacher_forcing)
    orc = NaiveLcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5,
                     depth=depth).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc, d


# ---------------------------------------------------------------------------------------------------- restatement
def _torch_decoder_loss(orc, F, data, tgt, drop, fed):
    """call_naive_attention after the encoder in torch float64 (fed tokens forced), CE + L2 of the decoder weights;
    returns (loss, leaf tensors)"""
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in orc.p.items() if "moving" not in k}
    Ft = torch.tensor(F, dtype=torch.float64, requires_grad=True)
    x, cap, a0, c0 = data
    B, T = cap.shape
    D, U, Et, R, A = orc.D, orc.U, orc.Et, orc.R, orc.A
    t = lambda m: None if m is None else torch.tensor(m, dtype=torch.float64)
    dropf = lambda v, m, r: v if m is None else v * t(m) / (1.0 - float(np.float32(r)))     # the rate as a float32 (oracle/ops.py)
    lrelu = lambda v: torch.where(v > 0, v, 0.2 * v)
    E = p["emb_text/embeddings"]
    km = drop.mask((B, T, Et), orc.r_text, M.S_TEXT)
    text = dropf(E[torch.tensor(cap[:, 0])], None if km is None else km[:, 0], orc.r_text)
    P = lrelu(Ft @ p["attention/W1/kernel"] + p["attention/W1/bias"])
    a = torch.tensor(a0, dtype=torch.float64)
    c = torch.tensor(c0, dtype=torch.float64)
    loss = 0.0
    for i in range(T):
        q = lrelu(a @ p["attention/W2/kernel"] + p["attention/W2/bias"])
        s = torch.tanh(P + q[:, None, :])
        sd = dropf(s, drop.mask((B, R, A), orc.r_attn, M.S_ATTN + i), orc.r_attn)
        e = (sd @ p["attention/V/kernel"])[..., 0] + p["attention/V/bias"]
        alpha = torch.softmax(e, dim=1)
        ctx = (alpha[..., None] * Ft).sum(1)
        sample = torch.cat([ctx, text], 1)
        k_li = drop.mask((B, 1, D + Et), orc.r_lstm, M.S_LSTM_IN + i)
        sample = dropf(sample, None if k_li is None else k_li[:, 0], orc.r_lstm)
        z = sample @ p["lstm/kernel"] + p["lstm/bias"] + a @ p["lstm/recurrent_kernel"]
        ig, fg, gg, og = torch.sigmoid(z[:, :U]), torch.sigmoid(z[:, U:2 * U]), torch.tanh(z[:, 2 * U:3 * U]), torch.sigmoid(z[:, 3 * U:])
        c = fg * c + ig * gg
        a = og * torch.tanh(c)
        out = dropf(dropf(a, drop.mask((B, U), orc.r_lstm, M.S_LSTM_OUT + i), orc.r_lstm),
                    drop.mask((B, U), orc.r_out, S_NOUT + i), orc.r_out)
        inter = lrelu(out @ p["time_distributed_nonlinear/kernel"] + p["time_distributed_nonlinear/bias"])
        probs = torch.softmax(inter @ p["time_distributed_softmax/kernel"] + p["time_distributed_softmax/bias"], dim=1)
        py = probs[torch.arange(B), torch.tensor(tgt[:, i])]
        loss = loss - torch.log(torch.clamp(py, 1e-7, 1 - 1e-7)).mean() / T
        if i + 1 < T:
            text = E[torch.tensor(fed[:, i + 1])]
    l2 = (orc.l2_attn * ((p["attention/W1/kernel"] ** 2).sum() + (p["attention/W2/kernel"] ** 2).sum())
          + orc.l2_lstm * (p["lstm/kernel"] ** 2).sum()
          + orc.l2_out * ((p["time_distributed_nonlinear/kernel"] ** 2).sum() + (p["time_distributed_softmax/kernel"] ** 2).sum()))
    return loss + l2, p, Ft


@pytest.mark.parametrize("rates", RATES)
def test_restatement_gradients_equal_autograd(rates):
    """The restatement's explicit backward (fed tokens forced) equals torch autograd in float64 for every decoder
    parameter and for dF; the encoder's backward is the teacher-forced oracle's (tests/test_oracle.py), entered through
    the second feature Dropout'."""
    rng = np.random.default_rng(5)
    _, orc, d = make_pair(rng, rates)
    data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
    fed = rng.integers(0, d["V"], size=(d["B"], d["T"]))
    drop = M.DropCtx(seed=11, step=2, training=True)
    (probs, attn), cache = orc.forward(data, True, drop, fed_ids=fed)
    assert np.array_equal(cache["fed"][:, 1:], fed[:, 1:]) and np.array_equal(cache["fed"][:, 0], data[1][:, 0])
    g, _, dF = orc._decode_bwd(probs, cache, tgt)
    # cache["F"]: the features behind both feature Dropouts, the decoder's input
    loss, p, Ft = _torch_decoder_loss(orc, cache["F"], data, tgt, drop, cache["fed"])
    ce = orc.metrics(probs, attn, tgt)[0]
    assert abs(float(loss.detach()) - (ce + orc.l2_loss() - sum(M._l2(orc.l2_in, orc.p[f"dense_in/{r}/kernel"]) for r in range(orc.R)))) < 1e-9
    loss.backward()
    for k, v in p.items():
        if k in g:
            want = v.grad.numpy()
            assert np.allclose(g[k], want, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(want).max())), (k, np.abs(g[k] - want).max())
    want_dF = O.dropout_bwd(Ft.grad.numpy(), cache["k_f2"], orc.r_feat)
    assert np.allclose(dF, want_dF, rtol=1e-9, atol=1e-14), np.abs(dF - want_dF).max()


# ---------------------------------------------------------------------------------------------------- model vs restatement
@pytest.mark.parametrize("rates,depth", [(RATES[0], 0), (RATES[1], 0), (RATES[1], 1)])
def test_train_steps_match_restatement(rates, depth, **dims):
    rng = np.random.default_rng(41)
    model, orc, d = make_pair(rng, rates, depth=depth, **dims)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        got = model.train_step((data, tgt)).as_floats()
        fed = model.fed_ids()
        assert np.array_equal(fed[:, 0], data[1][:, 0])
        res, grads, (_, _, cache) = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True), fed_ids=fed)
        # the device's fed ids are the restatement's own argmaxes (no near ties at these sizes)
        assert np.array_equal(cache["preds"][:, :-1], fed[:, 1:]), step
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) < 3e-5 * max(1, abs(res[k])), (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        for k, v in orc.p.items():
            w = model.get_weight(k)
            atol = 3e-3 * (step + 1) if k == "attention/V/bias" else 3e-6
            assert np.allclose(w, v, rtol=2e-4, atol=atol), (step, k, np.abs(w - v).max())


@pytest.mark.parametrize("rates", RATES)
def test_train_steps_match_restatement_unfused_head_tail(rates, monkeypatch):
    """dense_inter width % 4 != 0: the head backward takes its unfused tail (column sums, LeakyReLU', the two products of
    the nonlinear layer as separate launches); B=3, T=4"""
    monkeypatch.setattr(NIC, "H", 30)
    monkeypatch.setattr(M.LcNIC, "H", 30)
    test_train_steps_match_restatement(rates, 0, B=3, T=4)


def test_inference_matches_greedy_predict_and_test_step():
    rng = np.random.default_rng(43)
    model, orc, d = make_pair(rng, RATES[1])
    B, T, U = d["B"], d["T"], d["U"]
    data, tgt = synth_batch(B, d["N"], T, d["V"], U, rng)
    probs, attn, ids = model.call_naive_attention(data, training=False, return_ids=True)
    assert tuple(probs.shape) == (B, T, d["V"]) and tuple(attn.shape) == (T, B, d["R"], 1) and tuple(ids.shape) == (B, T)
    z = np.zeros((B, U), np.float32)
    ww, wp, wa, _ = M.LcNIC.greedy_predict(orc, data[0], z, z, data[1][:, 0], T)
    assert np.array_equal(ids.numpy(), ww[:, :, 0])
    assert np.allclose(probs.numpy(), wp, rtol=1e-4, atol=1e-6) and np.allclose(attn.numpy(), wa, rtol=1e-4, atol=1e-7)
    # __call__ of a free-running model is call_naive_attention
    p2, _ = model(data, training=False)
    assert np.array_equal(p2.numpy(), probs.numpy())
    want, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    for k in want:
        assert abs(got[k] - want[k]) < 3e-5 * max(1, abs(want[k])), (k, got[k], want[k])


def test_unsupported_combinations_refuse():
    rng = np.random.default_rng(44)
    d = ARGS
    g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
    args = (d["U"], 512, d["Et"], d["A"], d["V"], d["T"], 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        NIC(g, *args, device="cpu", n_subjects=2, teacher_forcing=False)
    with pytest.raises(NotImplementedError, match="use_layer_norm"):
        NIC(g, *args, device="cpu", use_layer_norm=True, teacher_forcing=False)
    lm = NIC(g, *args, device="cpu", use_layer_norm=True)           # the method refuses on a teacher-forced model too
    data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
    with pytest.raises(NotImplementedError, match="use_layer_norm"):
        lm.call_naive_attention(data)
    model = NIC(g, *args, device="cpu", teacher_forcing=False)
    model.compile(Adam(1e-3))
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam((data, tgt))
    from masters_thesis_amd import dp
    with pytest.raises(NotImplementedError, match="data parallel"):
        dp.attach(model, world=1, rank=0)
    model.grad_sync = lambda m: None
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.train_step((data, tgt))


def test_teacher_forcing_default_is_unchanged():
    """teacher_forcing=True is the existing model: two training steps leave bit-identical weights to a model built
    without the keyword; the free-running model trains differently on the same data."""
    rng = np.random.default_rng(45)
    d = ARGS
    g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
    args = (d["U"], 512, d["Et"], d["A"], d["V"], d["T"], 0.1, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 3e-5, 1e-5)
    models = [NIC(g, *args, device="cpu", seed=3), NIC(g, *args, device="cpu", seed=3, teacher_forcing=True),
              NIC(g, *args, device="cpu", seed=3, teacher_forcing=False)]
    batches = [synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng) for _ in range(2)]
    for m in models:
        m.compile(Adam(1e-3, clipnorm=0.1))
        for data, tgt in batches:
            m.train_step((data, tgt))
    for k in models[0].keras_shapes:
        assert np.array_equal(models[0].get_weight(k), models[1].get_weight(k)), k
    assert any(not np.array_equal(models[0].get_weight(k), models[2].get_weight(k)) for k in models[0].keras_shapes)
