"""Scheduled sampling for the dense model (nic.NIC(scheduled_sampling=...)) on the CPU: the schedule and argument
validation, and the model's host orchestration through a mock backend that follows tnt_scheduled_feedback_f32's header
definition, against the float64 restatement of tests/ss_oracle.py."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import dp
from masters_thesis_amd.model_base import ScheduledSampling as SS, S_SS_COIN, S_SS_DRAW
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch
from ss_oracle import SSMockBackend, SSNICDense, schedule_p, spec_p

LAM = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}
B, N, T, V, U, E = 6, 23, 6, 13, 16, 12


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = SSMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def make(rng, ss, rates=(0, 0, 0), seed=11, bias0=None):
    model = NIC(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, device="cpu", seed=seed, scheduled_sampling=ss)
    orc = SSNICDense(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5).init_params(rng)
    if bias0 is not None:
        orc.p["time_distributed_softmax/bias"][0] = bias0
    for k, v in orc.p.items():
        orc.p[k] = v.astype(np.float32).astype(np.float64)        # the oracle decides on the model's float32 weights
        model.set_weight(k, orc.p[k])
    model.compile(Adam(1e-3, clipnorm=None))
    return model, orc


def check_grads(model, grads, w0, rtol=1e-4):
    for k in M.NICDense.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM.get(k, 0.0) * w0[k]
        assert np.allclose(g, grads[k], rtol=rtol, atol=1e-6 * np.abs(grads[k]).max() + 1e-9), k


# ---------------------------------------------------------------------------------------------------- schedule
def test_linear_schedule_values_and_clamps():
    s = SS.linear(0.1, 0.01, 0.5)
    assert s.p(0) == np.float32(0.1) and s.p(20) == np.float32(0.1 + 0.01 * 20) and s.p(100) == np.float32(0.5)
    assert SS.linear(0.3, 0.0).p(10 ** 9) == np.float32(0.3)                 # constant p
    assert SS.linear(0.8, -0.1).p(20) == np.float32(0.0)                     # clamped at 0
    for i in (0, 1, 7, 39, 40, 41, 10 ** 6):
        assert s.p(i) == schedule_p(0, s.params(), i)
    ps = [s.p(i) for i in range(200)]
    assert all(b >= a for a, b in zip(ps, ps[1:]))


def test_inverse_sigmoid_schedule_values_and_monotone():
    s = SS.inverse_sigmoid(10.0, p_max=0.75)
    assert s.p(0) == np.float32(0.75 * (1 - 10 / 11))
    ps = np.array([s.p(i) for i in range(0, 2000, 7)])
    assert np.all(np.diff(ps) >= 0) and ps[-1] == np.float32(0.75) and ps.max() <= np.float32(0.75)
    assert s.p(10 ** 9) == np.float32(0.75)                                   # exp overflows to inf: p = p_max
    for i in (0, 3, 17, 50, 400):
        assert s.p(i) == schedule_p(1, s.params(), i)
    assert SS.inverse_sigmoid(1.0).p(0) == np.float32(0.5)


@pytest.mark.parametrize("make_bad", [
    lambda: SS("constant"), lambda: SS.linear(0.1, 0.0, mode="beam"), lambda: SS.linear(float("nan"), 0.0),
    lambda: SS.linear(0.1, float("inf")), lambda: SS.linear(-0.1, 0.0), lambda: SS.linear(1.5, 0.0),
    lambda: SS.linear(0.1, 0.0, p_max=1.01), lambda: SS.inverse_sigmoid(0.5), lambda: SS.inverse_sigmoid(float("inf")),
    lambda: SS.inverse_sigmoid(5.0, p_max=-0.2), lambda: SS.linear(True, 0.0), lambda: SS.linear("0.1", 0.0)])
def test_bad_schedules_raise(make_bad):
    with pytest.raises(ValueError):
        make_bad()


def test_model_refusals(mock_backend):
    with pytest.raises(ValueError):
        NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", scheduled_sampling="linear")
    with pytest.raises(ValueError):
        NIC(N, U, 10, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", scheduled_sampling=SS.linear(0.5, 0.0))
    rng = np.random.default_rng(1)
    model, _ = make(rng, SS.linear(0.5, 0.0))
    with pytest.raises(NotImplementedError):
        dp.attach(model, world=1, rank=0)
    data, tgt = synth_batch(B, N, 34, V, U, rng)
    with pytest.raises(ValueError):
        model.train_step((data, tgt))                                     # 33 token positions: more than the sites
    model.grad_sync = lambda m: None
    data, tgt = synth_batch(B, N, T, V, U, rng)
    with pytest.raises(NotImplementedError):
        model.train_step((data, tgt))
    assert mock_backend.ss_calls == 0
    assert S_SS_COIN >= 176 and S_SS_DRAW >= S_SS_COIN + 32


# ---------------------------------------------------------------------------------------------------- model
def test_none_trains_to_bit_identical_weights(mock_backend):
    rng = np.random.default_rng(2)
    ma, orc = make(rng, None, rates=(0.1, 0.2, 0.2))
    mb = NIC(N, U, E, V, T, 0.1, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    for k, v in orc.p.items():
        mb.set_weight(k, v)
    mb.compile(Adam(1e-3, clipnorm=None))
    for _ in range(3):
        data, tgt = synth_batch(B, N, T, V, U, rng)
        ra, rb = ma.train_step((data, tgt)).as_floats(), mb.train_step((data, tgt)).as_floats()
        assert ra == rb
    for k in orc.p:
        assert np.array_equal(ma.get_weight(k), mb.get_weight(k)), k
    assert mock_backend.ss_calls == 0


@pytest.mark.parametrize("rates", [(0, 0, 0), (0.1, 0.2, 0.25)])
def test_p_zero_is_the_teacher_forced_step(mock_backend, rates):
    rng = np.random.default_rng(3)
    ms, orc = make(rng, SS.linear(0.0, 0.0), rates=rates)
    mt = NIC(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    for k, v in orc.p.items():
        mt.set_weight(k, v)
    mt.compile(Adam(1e-3, clipnorm=None))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    rs, rt = ms.train_step((data, tgt)).as_floats(), mt.train_step((data, tgt)).as_floats()
    assert mock_backend.ss_calls == T - 1
    assert np.array_equal(ms.cap.numpy(), data[1])
    assert abs(rs["loss"] - rt["loss"]) < 1e-6 and abs(rs["accuracy"] - rt["accuracy"]) < 1e-9
    for k in M.NICDense.TRAINABLE:
        gs, gt = ms.get_gradient(k), mt.get_gradient(k)
        assert np.allclose(gs, gt, rtol=1e-6, atol=1e-6 * np.abs(gt).max() + 1e-12), k


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("p,rates", [(1.0, (0, 0, 0)), (0.5, (0, 0, 0)), (0.5, (0.1, 0.2, 0.25))])
def test_fed_ids_loss_and_gradients_match_float64(mode, p, rates):
    rng = np.random.default_rng(4)
    spec = SS.linear(p, 0.0, mode=mode)
    model, orc = make(rng, spec, rates=rates)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    data, tgt = synth_batch(B, N, T, V, U, rng)
    drop = M.DropCtx(seed=11, step=0, training=True)
    fed, margin, coins = orc.decide(data, drop, spec, 0)
    got = model.train_step((data, tgt)).as_floats()
    ok = margin > 1e-5
    assert ok.sum() >= ok.size - 2
    assert np.array_equal(model.cap.numpy()[ok], fed[ok])
    if p == 1.0:
        assert coins.all() and not np.array_equal(fed[:, 1:], data[1][:, 1:])
    else:
        assert coins.any() and not coins.all()
    assert np.array_equal(fed[~np.pad(coins, ((0, 0), (1, 0)))], data[1][~np.pad(coins, ((0, 0), (1, 0)))])
    ce, acc, grads = orc.loss_and_grads(data, model.cap.numpy().astype(np.int64), tgt, drop)
    assert abs(got["loss"] - ce) < 2e-5 * max(1, abs(ce)) and abs(got["accuracy"] - acc) < 1e-6
    check_grads(model, grads, w0)


def test_fed_zero_masks_the_next_step():
    rng = np.random.default_rng(5)
    spec = SS.linear(1.0, 0.0)
    model, orc = make(rng, spec, bias0=6.0)            # token 0 dominates: the model feeds 0
    w0 = {k: v.copy() for k, v in orc.p.items()}
    data, tgt = synth_batch(B, N, T, V, U, rng)
    model.train_step((data, tgt))
    fed = model.cap.numpy()
    assert np.all(fed[:, 1:] == 0)
    out = model.Out.numpy()                            # (T, B, U): a masked step repeats the previous output
    assert np.array_equal(out[2], out[1]) and np.array_equal(out[T - 1], out[1])
    drop = M.DropCtx(seed=11, step=0, training=True)
    ce, _, grads = orc.loss_and_grads(data, fed.astype(np.int64), tgt, drop)
    check_grads(model, grads, w0)


def test_schedule_is_read_live_from_the_update_counter(mock_backend):
    rng = np.random.default_rng(6)
    spec = SS.linear(0.0, 1.0)                         # p(0) = 0, p(1) = 1
    model, orc = make(rng, spec)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    model.train_step((data, tgt))
    assert np.array_equal(model.cap.numpy(), data[1])
    model.train_step((data, tgt))
    ps = [e[1] for e in mock_backend.ss_log]
    assert ps == [0.0] * (T - 1) + [1.0] * (T - 1)
    assert all(e[2].all() for e in mock_backend.ss_log[T - 1:])
    assert spec_p(spec, 0) == 0.0 and spec_p(spec, 1) == 1.0


def test_inference_and_test_step_are_unchanged(mock_backend):
    rng = np.random.default_rng(7)
    ms, orc = make(rng, SS.inverse_sigmoid(2.0, mode="sample"), rates=(0.1, 0.2, 0.2))
    mt = NIC(N, U, E, V, T, 0.1, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    for k, v in orc.p.items():
        mt.set_weight(k, v)
    mt.compile(Adam(1e-3, clipnorm=None))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    assert ms.test_step((data, tgt)).as_floats() == mt.test_step((data, tgt)).as_floats()
    assert np.array_equal(ms(data).numpy(), mt(data).numpy())
    assert np.array_equal(ms.call(data, training=True).numpy(), mt.call(data, training=True).numpy())
    z = np.zeros((B, U), np.float32)
    st = np.ones(B, np.int64)
    assert np.array_equal(ms.greedy_predict(data[0], z, z, st, T), mt.greedy_predict(data[0], z, z, st, T))
    assert mock_backend.ss_calls == 0
