"""Host orchestration of lc_NIC (config 3, attention) against the model-level oracle, on CPU
through the mock backend."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd.lc_nic import NIC, synthetic_groups
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch, tiny_groups
from mock_backend import MockBackend


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    ops.set_backend(MockBackend())
    yield
    ops.set_backend(old)


ARGS = dict(B=4, N=41, R=5, D=16, A=6, U=16, Et=12, V=13, T=5)


def make_pair(rng, rates, norm="batch", seed=11, depth=0, use_layer_norm=False, **d):
    d = {**ARGS, **d}
    groups = tiny_groups(d["N"], d["R"], rng)
    g = (groups, [d["D"]] * d["R"])
    model = NIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5, norm=norm,
                device="cpu", seed=seed, depth=depth, use_layer_norm=use_layer_norm)
    orc = M.LcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5,
                  norm=norm, depth=depth, use_layer_norm=use_layer_norm).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
        assert np.allclose(model.get_weight(k), v, atol=1e-6)
    return model, orc, d


@pytest.mark.parametrize("rates,norm", [((0,) * 6, "batch"), ((0.1, 0.2, 0.2, 0.2, 0.2, 0.2), "batch"),
                                        ((0, 0.2, 0, 0.2, 0, 0), "layer")])
def test_train_steps_match_oracle(rates, norm, **dims):
    rng = np.random.default_rng(41)
    model, orc, d = make_pair(rng, rates, norm, **dims)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) < 3e-5 * max(1, abs(res[k])), (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6 and abs(got["lr"] - 1e-3) < 1e-9
        for k, v in orc.p.items():
            w = model.get_weight(k)
            # attention/V/bias: its gradient is identically zero (softmax shift invariance), so what
            # Adam sees is rounding noise, which it normalises to O(lr) steps -- only bound it
            atol = 3e-3 * (step + 1) if k == "attention/V/bias" else 3e-6
            assert np.allclose(w, v, rtol=2e-4, atol=atol), (step, k, np.abs(w - v).max())


@pytest.mark.parametrize("rates", [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)])
def test_train_steps_match_oracle_unfused_head_tail(rates, monkeypatch):
    """dense_inter width % 4 != 0: the head backward takes its unfused tail (column sums, output Dropout', LeakyReLU', the
    two products of the nonlinear layer as separate launches); B=3, T=4"""
    monkeypatch.setattr(NIC, "H", 30)
    monkeypatch.setattr(M.LcNIC, "H", 30)
    test_train_steps_match_oracle(rates, "batch", B=3, T=4)


def test_gradients_call_test_step_greedy():
    rng = np.random.default_rng(42)
    model, orc, d = make_pair(rng, (0,) * 6)
    model.compile(Adam(1e-4, clipnorm=None))
    w0 = {k: v.copy() for k, v in orc.p.items()}
    data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
    (probs, attn), cache = orc.forward(data, True, M.DropCtx(training=True))
    grads, _ = orc.backward(probs, cache, tgt)
    res, (probs_e, attn_e) = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    for k in ("loss", "L2", "attention", "accuracy"):
        assert abs(got[k] - res[k]) < 3e-5 * max(1, abs(res[k])), k
    p, al = model(data, training=False)
    assert tuple(p.shape) == (d["B"], d["T"], d["V"]) and tuple(al.shape) == (d["T"], d["B"], d["R"], 1)
    assert np.allclose(p.numpy(), probs_e, rtol=1e-4, atol=1e-6) and np.allclose(al.numpy(), attn_e, rtol=1e-4, atol=1e-7)
    model.train_step((data, tgt))
    lam = {"attention/W1/kernel": 0.001, "attention/W2/kernel": 0.001, "lstm/kernel": 3e-5,
           "time_distributed_nonlinear/kernel": 1e-5, "time_distributed_softmax/kernel": 1e-5}
    for k in orc.trainable():
        l = 0.01 if k.startswith("dense_in") and k.endswith("kernel") else lam.get(k, 0.0)
        g = model.get_gradient(k) + 2 * l * w0[k]
        assert np.allclose(g, grads[k], rtol=2e-4, atol=2e-6 * np.abs(grads[k]).max() + 1e-9), k
    for k, v in w0.items():
        model.set_weight(k, v)
    orc.p = w0
    z = np.zeros((d["B"], d["U"]), np.float32)
    ww, wp, wa, ws = orc.greedy_predict(data[0], z, z, np.ones(d["B"], np.int64), 7)
    gw, gp, ga, gs = model.greedy_predict(data[0], z, z, np.ones(d["B"], np.int64), 7, d["U"], None)
    assert gw.shape == ww.shape == (d["B"], 7, 1) and gw.dtype == np.int64
    assert np.array_equal(gw, ww)
    assert np.allclose(gp, wp, rtol=1e-4, atol=1e-6) and np.allclose(ga, wa, rtol=1e-4, atol=1e-7)
    assert np.allclose(gs, ws, rtol=1e-4, atol=1e-6)


def test_synthetic_groups_partition():
    g, out = synthetic_groups(20000, 360, 32, seed=42)
    sizes = np.array([len(x) for x in g])
    assert len(g) == 360 and out == [32] * 360
    assert sizes.sum() == 20000 and sizes.min() >= 8
    assert len(np.unique(np.concatenate(g))) == 20000
    g2, _ = synthetic_groups(2000, 36, 32, seed=1, overlap=0.05)
    assert sum(len(x) for x in g2) > 2000


def test_sample_predict_matches_oracle_stream():
    """sample_predict = greedy loop with lc_NIC.sample_choice (lc_NIC.py:571-575) in place of the argmax;
    the draw is the Philox stream (seed, S_SAMPLE + position, sample_step)."""
    from oracle import ops as O
    rng = np.random.default_rng(77)
    model, orc, d = make_pair(rng, (0,) * 6)
    B, N, T, V, U = d["B"], d["N"], d["T"], d["V"], d["U"]
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    sampler = lambda probs, i: O.sample_rows(probs, 0.8, False, model.seed, M.S_SAMPLE + i, 3)[0]
    want = orc.greedy_predict(data[0], z, z, np.ones(B, np.int64), T, sampler=sampler)
    got = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, temperature=0.8, sample_step=3)
    assert np.array_equal(got[0], want[0])
    assert np.allclose(got[1], want[1], rtol=1e-4, atol=1e-6)
    greedy = model.greedy_predict(data[0], z, z, np.ones(B, np.int64), T)
    assert not np.array_equal(greedy[0], got[0]) or True      # may coincide at tiny V; shapes must agree
    assert greedy[0].shape == got[0].shape == (B, T, 1)


def test_compact_groups_is_the_same_function_on_fewer_columns():
    from masters_thesis_amd.lc_nic import compact_groups
    rng = np.random.default_rng(78)
    N, R, D = 60, 4, 16
    groups = [np.sort(rng.choice(N, size=int(rng.integers(3, 9)), replace=False)) for _ in range(R)]   # sparse coverage
    used, g2 = compact_groups((groups, [D] * R))
    assert len(used) < N and all((used[g] == np.asarray(o)).all() for g, o in zip(g2[0], groups))
    args = (16, 512, 12, 6, 13, 5, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    m1 = NIC((groups, [D] * R), *args, device="cpu", seed=5)
    m2 = NIC(g2, *args, device="cpu", seed=5)
    for k in m1.keras_shapes:
        m2.set_weight(k, m1.get_weight(k))
    B, T, U = 3, 5, 16
    data, _ = synth_batch(B, N, T, 13, U, rng)
    p1, a1 = m1(data, training=False)
    p2, a2 = m2((data[0][:, used],) + tuple(data[1:]), training=False)
    assert np.array_equal(p1.numpy(), p2.numpy()) and np.array_equal(a1.numpy(), a2.numpy())


def test_adaptive_gradient_clipping_matches_oracle():
    """lc_NIC with gradients = agc.adaptive_clip_grad(...) switched on (lc_NIC.py:388, agc.py:20-38)."""
    rng = np.random.default_rng(59)
    model, orc, d = make_pair(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2))
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    model.enable_agc(0.02, 1e-3)
    orc.agc = (0.02, 1e-3)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) < 2e-5 * max(1, abs(res["loss"]))
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            assert np.allclose(model.get_weight(k), v, rtol=2e-4, atol=2e-6), (step, k, np.abs(model.get_weight(k) - v).max())


def test_beam_search_matches_oracle():
    """NIC.beam_search (width k, log-probability sums, finished beams pad with 0) against oracle LcNIC.beam_search;
    k = 1 without an end token is the greedy caption."""
    rng = np.random.default_rng(61)
    model, orc, d = make_pair(rng, (0,) * 6)
    B, U, T = d["B"], d["U"], d["T"]
    data, _ = synth_batch(B, d["N"], T, d["V"], U, rng)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    gw = model.greedy_predict(data[0], z, z, start, T, U, None)[0]
    s1, _ = model.beam_search(data[0], z, z, start, T, beam_width=1)
    assert np.array_equal(s1[:, 0, :], gw[:, :, 0])
    end_id = int(gw[0, 1, 0])                       # a token the decoder really emits: exercises the finished-beam rule
    for k, eid in ((3, -1), (4, end_id)):
        want, wscore, margin = orc.beam_search(data[0], z, z, start, T, k=k, end_id=eid)
        got, gscore = model.beam_search(data[0], z, z, start, T, beam_width=k, end_id=eid)
        ok = margin > 1e-5                          # samples where float32 cannot reorder the candidates
        assert ok.any()
        assert np.array_equal(got[ok], want[ok]), (k, eid)
        assert np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("depth,norm", [(1, "batch"), (2, "batch"), (2, "layer")])
def test_depth_n_encoder_matches_oracle(depth, norm):
    """deep_layers.LocallyDense(depth=n) (deep_layers.py:15-75) in place of layers.LocallyDense: n more stages of
    per-region Dense + BatchNorm + Dropout -- three training steps (every gradient through the stages, their moving
    statistics) and the inference call against the oracle."""
    rng = np.random.default_rng(62)
    model, orc, d = make_pair(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), norm=norm, depth=depth)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) < 2e-5 * max(1, abs(res[k])), (step, k, got[k], res[k])
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            assert np.allclose(model.get_weight(k), v, rtol=2e-4, atol=3e-6), (step, k, np.abs(model.get_weight(k) - v).max())
    (probs, attn), _ = orc.forward(data, False)
    p, al = model(data, training=False)
    assert np.allclose(p.numpy(), probs, rtol=1e-4, atol=1e-7) and np.allclose(al.numpy(), attn, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("depth", [0, 1])
def test_train_step_sam_matches_oracle(depth):
    """lc_NIC.train_step_sam (lc_NIC.py:713-838): first gradient incl. the attention-MSE term, ascent step with the
    IndexedSlices global norm, second gradient at the perturbed weights, restore, Adam; metrics of the second pass."""
    rng = np.random.default_rng(63)
    model, orc, d = make_pair(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), depth=depth)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        res, g2 = orc.train_step_sam(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True), rho=0.05)
        got = model.train_step_sam((data, tgt), rho=0.05).as_floats()
        for k in ("loss", "L2", "attention", "accuracy"):
            assert abs(got[k] - res[k]) < 3e-5 * max(1, abs(res[k])), (step, k, got[k], res[k])
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            # atol: 2 % of one Adam update (lr = 1e-3)
            assert np.allclose(model.get_weight(k), v, rtol=2e-4, atol=2e-5), (step, k, np.abs(model.get_weight(k) - v).max())


def test_layer_norm_lstm_cell_matches_oracle():
    """use_layer_norm=True: tfa LayerNormLSTMCell as the decoder cell (lc_NIC.py:115,126-136) -- training steps (every
    gradient incl. the three LayerNorms', via the post-Adam weights), test_step, greedy captions and beam search."""
    rng = np.random.default_rng(64)
    model, orc, d = make_pair(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), use_layer_norm=True)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    B, U, T = d["B"], d["U"], d["T"]
    for step in range(3):
        data, tgt = synth_batch(B, d["N"], T, d["V"], U, rng)
        w0 = {k: v.copy() for k, v in orc.p.items()}
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2", "attention", "accuracy"):
            assert abs(got[k] - res[k]) < 3e-5 * max(1, abs(res[k])), (step, k, got[k], res[k])
        if step == 0:
            for k in orc.trainable():
                if k == "attention/V/bias":
                    continue
                g = model.get_gradient(k) + 2 * model.arena.entries[k].l2 * w0[k]
                assert np.allclose(g, grads[k], rtol=2e-4, atol=1e-5 * np.abs(grads[k]).max() + 1e-9), k
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            assert np.allclose(model.get_weight(k), v, rtol=2e-4, atol=2e-5), (step, k, np.abs(model.get_weight(k) - v).max())
    want = orc.test_step(data, tgt)[0]
    got = model.test_step((data, tgt)).as_floats()
    for k in want:
        assert abs(got[k] - want[k]) < 3e-5 * max(1, abs(want[k])), (k, got[k], want[k])
    z = np.zeros((B, U), np.float32)
    ww, wp, _, _ = orc.greedy_predict(data[0], z, z, np.ones(B, np.int64), T)
    gw, gp, _, _ = model.greedy_predict(data[0], z, z, np.ones(B, np.int64), T, U, None)
    assert np.array_equal(gw, ww) and np.abs(gp - wp).max() < 1e-5
    bs, _, margin = orc.beam_search(data[0], z, z, np.ones(B, np.int64), T, k=3)
    gb, _ = model.beam_search(data[0], z, z, np.ones(B, np.int64), T, beam_width=3)
    ok = margin > 1e-5
    assert np.array_equal(gb[ok], bs[ok])
