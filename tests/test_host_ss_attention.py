"""Scheduled sampling for the attention model (lc_nic.NIC(scheduled_sampling=...)) on the CPU: the model's host
orchestration through a mock backend that follows tnt_scheduled_feedback2_f32's header definition, against the float64
restatement of tests/ss_att_oracle.py; the teacher-forced and inference paths unchanged; the refusals."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import dp
from masters_thesis_amd.lc_nic import NIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, S_SS_COIN, SS_MAX_POSITIONS
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch, tiny_groups
from ss_att_oracle import SSAttLcNIC, SSAttMockBackend, masked_rows, spec_p

ARGS = dict(B=6, N=41, R=5, D=16, A=8, U=16, Et=12, V=13, T=6)
R0, R1 = (0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.25)
S_TEXT, S_LSTM_IN = 3, 48


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = SSAttMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def _groups(rng):
    d = ARGS
    return (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])


def _args(rates):
    d = ARGS
    return (d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5)


def make(rng, ss, rates=R0, seed=11, depth=0, **kw):
    """the model with scheduled_sampling=ss and its float64 restatement on the model's float32 weights"""
    g = _groups(rng)
    model = NIC(g, *_args(rates), device="cpu", seed=seed, depth=depth, scheduled_sampling=ss, **kw)
    orc = SSAttLcNIC(g, *_args(rates), depth=depth).init_params(rng)
    for k, v in orc.p.items():
        orc.p[k] = v.astype(np.float32).astype(np.float64)
        model.set_weight(k, orc.p[k])
    model.compile(Adam(1e-3, clipnorm=None))
    return model, orc, g


def twin(g, orc, rates, seed=11, depth=0, **kw):
    """a model on the same weights built without the keyword"""
    m = NIC(g, *_args(rates), device="cpu", seed=seed, depth=depth, **kw)
    for k, v in orc.p.items():
        m.set_weight(k, v)
    m.compile(Adam(1e-3, clipnorm=None))
    return m


def batch(rng):
    d = ARGS
    return synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)


def check_grads(model, grads, w0, rtol=1e-4):
    for k in grads:
        if k == "attention/V/bias":          # identically zero (softmax shift invariance): rounding noise only
            continue
        g = model.get_gradient(k) + 2 * model.arena.entries[k].l2 * w0[k]
        assert np.allclose(g, grads[k], rtol=rtol, atol=1e-5 * np.abs(grads[k]).max() + 1e-9), (k, np.abs(g - grads[k]).max())


# ---------------------------------------------------------------------------------------------------- the mock kernel
def test_mock_kernel_text_rows_are_the_teacher_forced_embedding_rows(mock_backend):
    """with every coin on the ground truth, the rows of scheduled_feedback2 are the rows embedding_fwd_drop(mask2=...)
    makes for that column, bit for bit, and rate_t = 0 gives scheduled_feedback's rows"""
    import torch
    rng = np.random.default_rng(1)
    B, T, E, V, D, N, col = 5, 4, 8, 11, 16, 12, 2
    table = torch.from_numpy(rng.standard_normal((V, E)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((E, N)).astype(np.float32))
    cap = torch.from_numpy(rng.integers(0, V, (B, T)).astype(np.int32))
    logits = torch.from_numpy(rng.standard_normal((B, V)).astype(np.float32))
    sd = torch.tensor([2], dtype=torch.int32)
    sched = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    cnt = torch.zeros(1, dtype=torch.int64)
    full = torch.zeros(T * B, E)
    mock_backend.embedding_fwd_drop(table, cap, None, full, B, T, E, E, V, 0.2, 7, S_TEXT, 0, sd,
                                    mask2=(0.3, S_LSTM_IN, D + E, D))
    text, xz = torch.zeros(B, E), torch.zeros(B, N)
    mock_backend.scheduled_feedback2(logits, V, V, table, E, w, N, N, cap, T, col, text, E, xz, N, B, 0.3, 7,
                                     S_LSTM_IN + col, 0, sd, D + E, D, 0, 0, sched, cnt, S_SS_COIN + col - 1, 0, 0.2, S_TEXT,
                                     T * E, col * E)
    assert torch.equal(text, full[col * B:(col + 1) * B])
    t1, x1, t2, x2 = torch.zeros(B, E), torch.zeros(B, N), torch.zeros(B, E), torch.zeros(B, N)
    sched[0] = 1.0
    mock_backend.scheduled_feedback2(logits, V, V, table, E, w, N, N, cap.clone(), T, col, t1, E, x1, N, B, 0.3, 7, 50, 0, sd,
                                     D + E, D, 0, 1, sched, cnt, 9, 10, 0.0, S_TEXT, T * E, col * E)
    mock_backend.scheduled_feedback(logits, V, V, table, E, w, N, N, cap.clone(), T, col, t2, E, x2, N, B, 0.3, 7, 50, 0, sd,
                                    D + E, D, 0, 1, sched, cnt, 9, 10)
    assert torch.equal(t1, t2) and torch.equal(x1, x2)
    rows = masked_rows(table.numpy()[[0, 1]], 2, E, [(0.0, 1, 8, 0)], 7, 2)
    assert np.array_equal(rows, table.numpy()[[0, 1]])


# ---------------------------------------------------------------------------------------------------- the model
def test_none_trains_to_bit_identical_weights(mock_backend):
    rng = np.random.default_rng(2)
    ma, orc, g = make(rng, None, rates=R1)
    mb = twin(g, orc, R1)
    for _ in range(3):
        data, tgt = batch(rng)
        assert ma.train_step((data, tgt)).as_floats() == mb.train_step((data, tgt)).as_floats()
    for k in orc.p:
        assert np.array_equal(ma.get_weight(k), mb.get_weight(k)), k
    assert mock_backend.ss2_calls == 0 and mock_backend.ss_calls == 0


@pytest.mark.parametrize("rates", [R0, R1])
def test_p_zero_is_the_teacher_forced_step(mock_backend, rates):
    rng = np.random.default_rng(3)
    ms, orc, g = make(rng, SS.linear(0.0, 0.0), rates=rates)
    mt = twin(g, orc, rates)
    data, tgt = batch(rng)
    rs, rt = ms.train_step((data, tgt)).as_floats(), mt.train_step((data, tgt)).as_floats()
    T = ARGS["T"]
    assert mock_backend.ss2_calls == T - 1
    assert np.array_equal(ms.cap.numpy(), data[1])
    assert not any(e[2].any() for e in mock_backend.ss2_log)
    for k in ("loss", "attention", "L2"):
        assert abs(rs[k] - rt[k]) < 1e-6 * max(1, abs(rt[k])), k
    assert abs(rs["accuracy"] - rt["accuracy"]) < 1e-9
    for k in orc.p:
        if "moving" in k:
            continue
        gs, gt = ms.get_gradient(k), mt.get_gradient(k)
        assert np.allclose(gs, gt, rtol=1e-5, atol=1e-6 * np.abs(gt).max() + 1e-12), k


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("p,rates,depth", [(1.0, R0, 0), (0.5, R0, 0), (1.0, R1, 0), (0.5, R1, 0), (1.0, R1, 1),
                                           (0.5, R1, 1)])
def test_fed_ids_loss_and_gradients_match_float64(mode, p, rates, depth):
    rng = np.random.default_rng(4)
    spec = SS.linear(p, 0.0, mode=mode)
    model, orc, _ = make(rng, spec, rates=rates, depth=depth)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    data, tgt = batch(rng)
    drop = M.DropCtx(seed=11, step=0, training=True)
    got = model.train_step((data, tgt)).as_floats()
    dev = model.cap.numpy().astype(np.int64)
    fed, margin, coins = orc.decide(data, drop, spec, 0)
    own, margin_f, coins_f = orc.decide(data, drop, spec, 0, fed_ids=dev)       # on the device's history
    assert np.array_equal(coins, coins_f)
    ok = margin_f > 1e-5
    assert ok.sum() >= ok.size - 2
    assert np.array_equal(dev[ok], own[ok])
    if ok.all():
        assert np.array_equal(dev, fed)
    gt_pos = ~np.pad(coins, ((0, 0), (1, 0)))
    assert np.array_equal(dev[gt_pos], data[1][gt_pos])                           # ground-truth positions exactly
    if p == 1.0:
        assert coins.all() and not np.array_equal(dev[:, 1:], data[1][:, 1:])
    else:
        assert coins.any() and not coins.all()
    ce, acc, al, grads = orc.loss_and_grads(data, dev, tgt, drop)
    assert abs(got["loss"] - ce) < 2e-5 * max(1, abs(ce)) and abs(got["accuracy"] - acc) < 1e-6
    assert abs(got["attention"] - al) < 2e-5 * max(1, abs(al))
    check_grads(model, grads, w0)


def test_schedule_is_read_live_from_the_update_counter(mock_backend):
    rng = np.random.default_rng(6)
    spec = SS.linear(0.0, 1.0)                         # p(0) = 0, p(1) = 1
    model, _, _ = make(rng, spec, rates=R1)
    T = ARGS["T"]
    data, tgt = batch(rng)
    model.train_step((data, tgt))
    assert np.array_equal(model.cap.numpy(), data[1])
    model.train_step((data, tgt))
    ps = [e[1] for e in mock_backend.ss2_log]
    assert ps == [0.0] * (T - 1) + [1.0] * (T - 1)
    assert all(e[2].all() for e in mock_backend.ss2_log[T - 1:])
    assert [e[0] for e in mock_backend.ss2_log] == list(range(1, T)) * 2
    assert spec_p(spec, 0) == 0.0 and spec_p(spec, 1) == 1.0


def test_inference_and_test_step_are_unchanged(mock_backend):
    rng = np.random.default_rng(7)
    ms, orc, g = make(rng, SS.inverse_sigmoid(2.0, mode="sample"), rates=R1)
    mt = twin(g, orc, R1)
    d = ARGS
    data, tgt = batch(rng)
    assert ms.test_step((data, tgt)).as_floats() == mt.test_step((data, tgt)).as_floats()
    for training in (False, True):
        (pa, aa), (pb, ab) = ms(data, training=training), mt(data, training=training)
        assert np.array_equal(pa.numpy(), pb.numpy()) and np.array_equal(aa.numpy(), ab.numpy())
    z = np.zeros((d["B"], d["U"]), np.float32)
    st = np.ones(d["B"], np.int64)
    for a, b in zip(ms.greedy_predict(data[0], z, z, st, d["T"]), mt.greedy_predict(data[0], z, z, st, d["T"])):
        assert np.array_equal(a, b)
    for a, b in zip(ms.sample_predict(data[0], z, z, st, d["T"], sample_step=3),
                    mt.sample_predict(data[0], z, z, st, d["T"], sample_step=3)):
        assert np.array_equal(a, b)
    assert mock_backend.ss2_calls == 0


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(mock_backend):
    rng = np.random.default_rng(8)
    g = _groups(rng)
    spec = SS.linear(0.5, 0.0)
    with pytest.raises(ValueError, match="ScheduledSampling"):
        NIC(g, *_args(R0), device="cpu", scheduled_sampling="linear")
    with pytest.raises(ValueError, match="teacher_forcing=False"):
        NIC(g, *_args(R0), device="cpu", scheduled_sampling=spec, teacher_forcing=False)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        NIC(g, *_args(R0), device="cpu", scheduled_sampling=spec, n_subjects=2)
    with pytest.raises(NotImplementedError, match="use_layer_norm"):
        NIC(g, *_args(R0), device="cpu", scheduled_sampling=spec, use_layer_norm=True)
    d = ARGS
    for et in (10, 1020):
        args = (d["U"], 512, et, d["A"], d["V"], d["T"], *R0, 0.01, 0.001, 3e-5, 1e-5)
        with pytest.raises(ValueError, match="embedding_text"):
            NIC(g, *args, device="cpu", scheduled_sampling=spec)
    model, _, _ = make(rng, spec)
    with pytest.raises(NotImplementedError, match="data parallel"):
        dp.attach(model, world=1, rank=0)
    data, tgt = synth_batch(d["B"], d["N"], SS_MAX_POSITIONS + 2, d["V"], d["U"], rng)
    with pytest.raises(ValueError, match="token positions"):
        model.train_step((data, tgt))                         # 33 decided positions: more than the Philox sites
    data, tgt = batch(rng)
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam((data, tgt))
    model.grad_sync = lambda m: None
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.train_step((data, tgt))
    assert mock_backend.ss2_calls == 0
    # SS_MAX_POSITIONS decided positions are accepted
    model.grad_sync = None
    data, tgt = synth_batch(d["B"], d["N"], SS_MAX_POSITIONS + 1, d["V"], d["U"], rng)
    model.train_step((data, tgt))
    assert mock_backend.ss2_calls == SS_MAX_POSITIONS
