"""Knowledge distillation through the models on the GPU: one train_step of nic.NIC and of lc_nic.NIC at the tiny golden
sizes of tests/test_gpu_nic.py / tests/test_gpu_lcnic.py (their DIMS[0], their build()), dropout off, under a second tiny
model built with another seed and a sharpened vocabulary kernel as the teacher, against the float64 oracle step with the
distilled gradient substituted (distill_oracle.distilled) and the oracle teacher's own logits; the dense student under
the attention teacher; a recorded launch plan and a captured hipGraph against the eager step, with the teacher's weights
changed by set_weight between two replays.  The tolerances are the ones tests/test_gpu_nic.py and
tests/test_gpu_lcnic.py apply to the plain step."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch
import test_gpu_nic as TN
import test_gpu_lcnic as TL
from test_gpu_weighted_models import LAM_NIC, LAM_LC, DIMS_REPLAY_NIC, DIMS_REPLAY_LC, adam, sharpen
from distill_oracle import distill_metrics, distilled

pytestmark = pytest.mark.gpu

ALPHA, TEMP = 0.5, 2.0
HEAD_BIAS = "time_distributed_softmax/bias"


def loss_obj(alpha=ALPHA, t=TEMP):
    from masters_thesis_amd.optimizers import CategoricalCrossentropy, Distillation
    return CategoricalCrossentropy(from_logits=False, reduction="none", distillation=Distillation(alpha, t))


def build(kind, seed, dims, use_graph=False, scale=8.0):
    """(model, oracle) of either family with the vocabulary kernel sharpened: at initialisation p is near uniform, and so
    is a teacher's, which then teaches nothing"""
    rng = np.random.default_rng(seed)
    if kind == "dense":
        model, orc = TN.build(rng, (0, 0, 0), dims, use_graph=use_graph)
    else:
        model, orc = TL.build(rng, (0,) * 6, dims, use_graph=use_graph)
    sharpen(model, orc, scale)
    return model, orc


def probs_of(orc, data, training):
    out, cache = orc.forward(data, training, M.DropCtx(seed=11, step=0, training=training))
    return (out[0] if isinstance(out, tuple) else out), cache


def oracle_step(orc, torc, opt, data, tgt, alpha=ALPHA, t=TEMP):
    """(metrics of the distilled loss, gradients) of the patched float64 training step; the teacher's logits are the
    oracle teacher's own (log of its inference probabilities: softmax(u / t) does not see the row constant)"""
    u = np.log(probs_of(torc, data, False)[0])
    assert np.isfinite(u).all()
    probs, cache = probs_of(orc, data, True)
    loss, kl, acc = distill_metrics(probs, u, tgt, alpha, t)
    plain = orc.backward(probs, cache, tgt)[0]
    with distilled(u, alpha, t):
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    # the comparison can tell the step from the plain one: the loss and the head-bias gradient move far past the
    # tolerances below
    assert abs(loss - res["loss"]) > 100 * 1e-4 * res["loss"]
    assert np.abs(plain[HEAD_BIAS] - grads[HEAD_BIAS]).max() > 100 * 2e-4 * np.abs(grads[HEAD_BIAS]).max()
    res = dict(res)
    res["loss"], res["distill_kl"], res["accuracy"] = loss, kl, acc
    return res, grads


def check_dense(model, orc, w0, res, grads, got):
    # test_gpu_nic.test_train_parity: loss 1e-4 relative, accuracy 1e-6; test_forward_gradients_greedy: gradients 1e-4 of
    # the largest + 1e-9; test_train_parity: weights 2e-2 * lr + 1e-4 of the largest (+ 1e-3 where the gradient is noise)
    for k in ("loss", "distill_kl"):
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]), (k, got, res)
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    for k in orc.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM_NIC.get(k, 0.0) * w0[k]
        assert np.abs(g - grads[k]).max() <= 1e-4 * np.abs(grads[k]).max() + 1e-9, k
    for k, v in orc.p.items():
        tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()
        if k in grads and grads[k] is not None:
            tol = tol + 1e-3 * (np.abs(grads[k]) < 1e-8)
        assert (np.abs(model.get_weight(k) - v) <= tol).all(), (k, np.abs(model.get_weight(k) - v).max())


def dense_student_step(teacher_kind):
    dims = TN.DIMS[0]
    B, N, T, V, U, E = dims
    model, orc = build("dense", 31, dims)
    teacher, torc = build(teacher_kind, 77, dims if teacher_kind == "dense" else TL.DIMS[0], scale=16.0)
    model.compile(adam(), loss_obj())
    model.set_teacher(teacher)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = synth_batch(B, N, T, V, U, np.random.default_rng(32))
    w0 = {k: v.copy() for k, v in orc.p.items()}
    t0 = teacher.arena.theta.clone()
    res, grads = oracle_step(orc, torc, opt, data, tgt)
    got = model.train_step((data, tgt)).as_floats()
    check_dense(model, orc, w0, res, grads, got)
    assert torch.equal(teacher.arena.theta, t0)
    plain = model.test_step((data, tgt)).as_floats()             # the plain cross-entropy, no teacher
    want = orc.test_step(data, tgt)[0]
    assert "distill_kl" not in plain and abs(plain["loss"] - want["loss"]) <= 1e-4 * abs(want["loss"])


def test_dense_train_step_matches_the_distilled_oracle():
    dense_student_step("dense")


def test_dense_student_under_the_attention_teacher():
    (B, N, T, V, U, _), lc = TN.DIMS[0], TL.DIMS[0]
    assert (B, N, T, V, U) == (lc[0], lc[1], lc[8], lc[7], lc[5])        # the two tiny models take the same batch: no adapt=
    dense_student_step("attention")


def test_attention_train_step_matches_the_distilled_oracle():
    dims = TL.DIMS[0]
    B, N, R, D, A, U, Et, V, T = dims
    model, orc = build("attention", 51, dims)
    teacher, torc = build("attention", 78, dims, scale=16.0)
    model.compile(adam(), loss_obj())
    model.set_teacher(teacher)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = synth_batch(B, N, T, V, U, np.random.default_rng(52))
    w0 = {k: v.copy() for k, v in orc.p.items()}
    res, grads = oracle_step(orc, torc, opt, data, tgt)
    got = model.train_step((data, tgt)).as_floats()
    # test_gpu_lcnic.test_train_parity: metrics 1e-4 relative + 1e-7, weights 2e-2 * lr + 1e-4 of the largest (not
    # attention/V/bias); test_forward_gradients_greedy: gradients 2e-4 of the largest + 1e-9
    for k in ("loss", "distill_kl", "L2", "attention"):
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


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_a_teacher_rebuilt_between_two_replays_is_read_where_it_now_lives(kind):
    """The teacher allocates new buffers when it is staged at another shape (here its own test_step at B + 2) and drops
    only its own recordings.  The student's plan / graph holds the address of teacher.logits: it has to be recorded again.
    The old logits tensor is kept alive and poisoned, so a replay that still read it would give NaN, not the eager bits."""
    dims = DIMS_REPLAY_NIC if kind == "dense" else DIMS_REPLAY_LC
    if kind == "dense":
        B, N, T, V, U, E = dims
    else:
        B, N, R, D, A, U, Et, V, T = dims
    models = []
    for use_graph, plan in ((False, True), (True, True), (True, False)):
        m, _ = build(kind, 9, dims, use_graph=use_graph)
        t, _ = build(kind, 19, dims, use_graph=use_graph, scale=16.0)
        m.plan_step = plan
        m.compile(adam(), loss_obj())
        m.set_teacher(t)
        models.append(m)
    rng = np.random.default_rng(12)
    other = synth_batch(B + 2, N, T, V, U, np.random.default_rng(13))
    stale = []
    for step in range(7):
        if step == 4:
            for m in models:
                old = m.teacher.logits
                m.teacher.test_step(other)
                assert m.teacher.logits is not old and m.teacher.logits.data_ptr() != old.data_ptr()
                old.fill_(float("nan"))
                stale.append(old)
        data, tgt = synth_batch(B, N, T, V, U, rng)
        ra, rb, rc = (m.train_step((data, tgt)).as_floats() for m in models)
        assert ra == rb == rc and np.isfinite(list(ra.values())).all(), (step, ra, rb, rc)
    torch.cuda.synchronize()
    eager, planned, graphed = models
    assert any(isinstance(v, tuple) for v in planned._graphs.values()), "the second model did not replay a launch plan"
    assert any(isinstance(v, torch.cuda.CUDAGraph) for v in graphed._graphs.values()), "the third model did not replay a graph"
    for m in (planned, graphed):
        assert torch.equal(eager.arena.theta, m.arena.theta) and torch.equal(eager.opt_m, m.opt_m)
        assert m._teacher_held[0] == m.teacher.logits.data_ptr()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_replay_graph_replay_and_eager_step_are_bit_identical(kind):
    """eager / a recorded launch plan / a captured hipGraph over eager -> record or capture -> replay -> replay with a
    fresh batch each, then set_weight on all three teachers and two more replays: the same bits, nothing recorded again
    (the replay reads the new teacher); a fourth, eager model whose teacher keeps its weights shows that the new ones
    change the step"""
    dims = DIMS_REPLAY_NIC if kind == "dense" else DIMS_REPLAY_LC
    if kind == "dense":
        B, N, T, V, U, E = dims
    else:
        B, N, R, D, A, U, Et, V, T = dims
    models = []
    for use_graph, plan in ((False, True), (True, True), (True, False), (False, True)):
        m, _ = build(kind, 9, dims, use_graph=use_graph)
        t, torc = build(kind, 19, dims, use_graph=use_graph, scale=16.0)
        m.plan_step = plan
        m.compile(adam(), loss_obj())
        m.set_teacher(t)
        models.append(m)
    eager, planned, graphed, kept = models
    rng = np.random.default_rng(11)
    k = "time_distributed_softmax/kernel"
    keys = None
    for step in range(6):
        if step == 4:
            keys = [set(m._graphs) for m in (planned, graphed)] + [set(m.teacher._graphs) for m in (planned, graphed)]
            for m in (eager, planned, graphed):
                m.teacher.set_weight(k, 0.5 * torc.p[k])
        data, tgt = synth_batch(B, N, T, V, U, rng)
        ra, rb, rc, rd = (m.train_step((data, tgt)).as_floats() for m in models)
        assert ra == rb == rc, (step, ra, rb, rc)
        assert "distill_kl" in ra and (ra == rd) == (step < 4), (step, ra, rd)
    torch.cuda.synchronize()
    assert [set(m._graphs) for m in (planned, graphed)] + [set(m.teacher._graphs) for m in (planned, graphed)] == keys, \
        "set_weight on the teacher recorded / captured a step again"
    assert any(key[-1] == "distill" for key in planned._graphs) and ("teach", B, T) in graphed.teacher._graphs
    assert any(isinstance(v, tuple) for v in planned._graphs.values()), "the second model did not replay a launch plan"
    assert any(isinstance(v, torch.cuda.CUDAGraph) for v in graphed._graphs.values()), "the third model did not replay a graph"
    assert isinstance(graphed.teacher._graphs[("teach", B, T)], torch.cuda.CUDAGraph)
    for m in (planned, graphed):
        assert torch.equal(eager.arena.theta, m.arena.theta) and torch.equal(eager.opt_m, m.opt_m)
        assert torch.equal(eager.opt_v, m.opt_v)
    assert not torch.equal(eager.arena.theta, kept.arena.theta)
