"""Unlikelihood training through the models on the GPU: one train_step and one test_step of nic.NIC and lc_nic.NIC at small
sizes (B = 6, T = 6, V = 101, U = 32), dropout off, unlikelihood = 1.0, captions over three words so that most rows have
candidates, against the float64 oracle with the gradient substituted (unlikelihood_oracle.unlikely) and alpha * mean(ul)
of the oracle's own probabilities added to its loss; a scheduled-sampling step at p = 0 against the teacher-forced step;
a captured step against the eager one; unlikelihood = 0 against a model compiled without the argument.  The tolerances
are the ones tests/test_gpu_nic.py, tests/test_gpu_lcnic.py and tests/test_gpu_scheduled_sampling.py apply to the step
without the feature."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch
import test_gpu_nic as TN
import test_gpu_lcnic as TL
from unlikelihood_oracle import candidates, ul_mean, unlikely

pytestmark = pytest.mark.gpu

ALPHA = 1.0
DIMS_NIC = (6, 200, 6, 101, 32, 32)                      # B, N, T, V, U, E
DIMS_LC = (6, 200, 8, 16, 16, 32, 32, 101, 6)            # B, N, R, D, A, U, Et, V, T
LAM_NIC = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}       # test_gpu_nic.py
LAM_LC = {"attention/W1/kernel": 0.001, "attention/W2/kernel": 0.001, "lstm/kernel": 3e-5,             # test_gpu_lcnic.py
          "time_distributed_nonlinear/kernel": 1e-5, "time_distributed_softmax/kernel": 1e-5}


def loss_obj(alpha=ALPHA):
    from masters_thesis_amd.optimizers import CategoricalCrossentropy
    return CategoricalCrossentropy(from_logits=False, reduction="none", unlikelihood=alpha)


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def sharpen(model, orc, scale=8.0, lift=3.0):
    """at initialisation p is near uniform and every q_c near 1 / V: scale the vocabulary kernel, and lift the bias of the
    three words the captions are made of, as in a model that has learnt to repeat them"""
    k, kb = "time_distributed_softmax/kernel", "time_distributed_softmax/bias"
    orc.p[k] = orc.p[k] * scale
    orc.p[kb] = orc.p[kb].copy()
    orc.p[kb][3:6] += lift
    for n in (k, kb):
        model.set_weight(n, orc.p[n])


def repeating_batch(B, N, T, V, U, rng):
    """synth_batch with every caption drawn from three words: repeats, so candidates, from the third position on"""
    (x, cap, a0, c0), _ = synth_batch(B, N, T, V, U, rng)
    for b in range(B):
        cap[b, 1:T - 1] = rng.integers(3, 6, T - 2)
        cap[b, T - 1] = 2
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    n = sum(len(c) > 0 for c in candidates(tgt.T.reshape(-1), B, T, V))
    assert n > B * T // 2, "most rows should have candidates"
    return (x, cap, a0, c0), tgt


def oracle_step(orc, opt, data, tgt):
    """(metrics with the unlikelihood term in the loss, gradients) of the patched float64 training step"""
    out, cache = orc.forward(data, True, M.DropCtx(seed=11, step=0, training=True))
    probs = out[0] if isinstance(out, tuple) else out          # the attention model returns (probs, attention)
    extra = ALPHA * ul_mean(probs, tgt)
    plain = orc.backward(probs, cache, tgt)[0]
    with unlikely(ALPHA):
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    # the comparison can tell the step from the plain one: the term moves the loss and the head-bias gradient far past
    # the tolerances below
    k = "time_distributed_softmax/bias"
    assert extra > 100 * 1e-4 * res["loss"] and np.abs(plain[k] - grads[k]).max() > 100 * 2e-4 * np.abs(grads[k]).max()
    res = dict(res)
    res["loss"] = res["loss"] + extra
    return res, grads


def oracle_test_loss(orc, data, tgt):
    want, out = orc.test_step(data, tgt)
    return want["loss"] + ALPHA * ul_mean(out[0] if isinstance(out, tuple) else out, tgt)


def test_dense_train_and_test_step_match_the_patched_oracle():
    rng = np.random.default_rng(31)
    B, N, T, V, U, E = DIMS_NIC
    model, orc = TN.build(rng, (0, 0, 0), DIMS_NIC, use_graph=False)
    sharpen(model, orc)
    model.compile(adam(), loss_obj())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = repeating_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    res, grads = oracle_step(orc, opt, data, tgt)
    got = model.train_step((data, tgt)).as_floats()
    # test_gpu_nic.test_train_parity: loss 1e-4 relative, accuracy 1e-6; test_forward_gradients_greedy: gradients 1e-4 of
    # the largest + 1e-9; test_train_parity: weights 2e-2 * lr + 1e-4 of the largest (+ 1e-3 where the gradient is noise)
    assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]), (got, res)
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    for k in orc.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM_NIC.get(k, 0.0) * w0[k]
        assert np.abs(g - grads[k]).max() <= 1e-4 * np.abs(grads[k]).max() + 1e-9, k
    for k, v in orc.p.items():
        tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()
        if k in grads and grads[k] is not None:
            tol = tol + 1e-3 * (np.abs(grads[k]) < 1e-8)
        assert (np.abs(model.get_weight(k) - v) <= tol).all(), (k, np.abs(model.get_weight(k) - v).max())
    data, tgt = repeating_batch(B, N, T, V, U, rng)
    want = oracle_test_loss(orc, data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want) <= 1e-4 * abs(want), (got, want)


def test_attention_train_and_test_step_match_the_patched_oracle():
    rng = np.random.default_rng(51)
    B, N, R, D, A, U, Et, V, T = DIMS_LC
    model, orc = TL.build(rng, (0,) * 6, DIMS_LC, use_graph=False)
    sharpen(model, orc)
    model.compile(adam(), loss_obj())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = repeating_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    res, grads = oracle_step(orc, opt, data, tgt)
    got = model.train_step((data, tgt)).as_floats()
    # test_gpu_lcnic.test_train_parity: metrics 1e-4 relative + 1e-7, weights 2e-2 * lr + 1e-4 of the largest (not
    # attention/V/bias); test_forward_gradients_greedy: gradients 2e-4 of the largest + 1e-9
    for k in ("loss", "L2", "attention"):
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    for k in orc.trainable():
        if k == "attention/V/bias":
            assert np.abs(model.get_gradient(k)).max() < 1e-5
            continue
        l = 0.01 if k.startswith("dense_in") and k.endswith("kernel") else LAM_LC.get(k, 0.0)
        g = model.get_gradient(k) + 2 * l * w0[k]
        assert np.abs(g - grads[k]).max() <= 2e-4 * np.abs(grads[k]).max() + 1e-9, (k, np.abs(g - grads[k]).max())
    for k, v in orc.p.items():
        if k == "attention/V/bias":
            continue
        assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), k
    data, tgt = repeating_batch(B, N, T, V, U, rng)
    want = oracle_test_loss(orc, data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want) <= 1e-4 * abs(want) + 1e-7, (got, want)


def test_scheduled_sampling_at_p_zero_is_the_teacher_forced_step():
    """p = 0 feeds the ground truth: the same forward through the per-step kernels, the same unlikelihood launch.
    tests/test_gpu_scheduled_sampling.py's bounds for its p = 0 test: loss 1e-5, gradients 1e-5 of the largest."""
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    from masters_thesis_amd.nic import NIC
    B, N, T, V, U, E = DIMS_NIC
    orc = M.NICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(np.random.default_rng(7))
    orc.p["time_distributed_softmax/kernel"] *= 8.0
    orc.p["time_distributed_softmax/bias"][3:6] += 3.0
    mt = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, seed=11, use_graph=False)
    ms = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, seed=11, use_graph=False, scheduled_sampling=SS.linear(0.0, 0.0))
    for m in (mt, ms):
        for k, v in orc.p.items():
            m.set_weight(k, v)
    for m in (mt, ms):
        m.compile(adam(), loss_obj())
    data, tgt = repeating_batch(B, N, T, V, U, np.random.default_rng(8))
    rs, rt = ms.train_step((data, tgt)).as_floats(), mt.train_step((data, tgt)).as_floats()
    assert np.array_equal(ms.cap.cpu().numpy(), data[1])
    assert abs(rs["loss"] - rt["loss"]) < 1e-5 * max(1, abs(rt["loss"]))
    for k in mt.trainable_names():
        a, b = ms.get_gradient(k), mt.get_gradient(k)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-12, k


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_captured_step_replays_bit_identically(kind):
    """eager, capture / record, replay, replay against four eager steps: the same launches, the same bits"""
    models = []
    for use_graph in (False, True):
        rng = np.random.default_rng(9)
        if kind == "dense":
            m, orc = TN.build(rng, (0, 0, 0), DIMS_NIC, use_graph=use_graph)
            B, N, T, V, U, E = DIMS_NIC
        else:
            m, orc = TL.build(rng, (0,) * 6, DIMS_LC, use_graph=use_graph)
            B, N, R, D, A, U, Et, V, T = DIMS_LC
        sharpen(m, orc)
        m.compile(adam(), loss_obj())
        models.append(m)
    rng = np.random.default_rng(10)
    for step in range(4):
        data, tgt = repeating_batch(B, N, T, V, U, rng)
        ra, rb = (m.train_step((data, tgt)).as_floats() for m in models)
        assert ra == rb, (step, ra, rb)
    torch.cuda.synchronize()
    a, b = models
    assert b._graphs, "the second model never captured its step"
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_unlikelihood_zero_gives_the_bits_of_a_model_compiled_without_it(kind):
    from masters_thesis_amd.optimizers import CategoricalCrossentropy
    models = []
    for loss in (CategoricalCrossentropy(from_logits=False, reduction="none"), loss_obj(0.0)):
        rng = np.random.default_rng(12)
        if kind == "dense":
            m, orc = TN.build(rng, (0.1, 0.2, 0.2), DIMS_NIC)
            B, N, T, V, U, E = DIMS_NIC
        else:
            m, orc = TL.build(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), DIMS_LC)
            B, N, R, D, A, U, Et, V, T = DIMS_LC
        m.compile(adam(), loss)
        models.append(m)
    a, b = models
    assert a.unlikelihood == 0.0 and b.unlikelihood == 0.0
    rng = np.random.default_rng(13)
    for step in range(3):
        data, tgt = repeating_batch(B, N, T, V, U, rng)
        ra, rb = a.train_step((data, tgt)).as_floats(), b.train_step((data, tgt)).as_floats()
        assert ra == rb, (step, ra, rb)
    assert a.test_step((data, tgt)).as_floats() == b.test_step((data, tgt)).as_floats()
    torch.cuda.synchronize()
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    assert set(a._graphs) == set(b._graphs)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_more_than_64_loss_positions_is_refused_before_any_launch(kind):
    """the ValueError of the first step comes while the batch is staged: nothing is enqueued or captured, and the model
    goes on to run a step of a length the kernel takes"""
    if kind == "dense":
        B, N, T, V, U, E = DIMS_NIC
        build = lambda Tq: TN.build(np.random.default_rng(14), (0, 0, 0), (B, N, Tq, V, U, E))[0]
    else:
        B, N, R, D, A, U, Et, V, T = DIMS_LC
        build = lambda Tq: TL.build(np.random.default_rng(14), (0,) * 6, (B, N, R, D, A, U, Et, V, Tq))[0]
    model = build(65)
    model.compile(adam(), loss_obj())
    data, tgt = synth_batch(B, N, 65, V, U, np.random.default_rng(15))
    for step in (model.train_step, model.test_step):
        with pytest.raises(ValueError, match="64"):
            step((data, tgt))
    assert not model._graphs
    model = build(64)
    model.compile(adam(), loss_obj())
    data, tgt = synth_batch(B, N, 64, V, U, np.random.default_rng(15))
    got = model.train_step((data, tgt)).as_floats()
    assert np.isfinite(list(got.values())).all()
