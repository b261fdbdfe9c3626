"""Knowledge distillation on the CPU through a mock backend that follows tnt_softmax_cce_distill_f32's header definition
(tests/distill_oracle.py): the float64 restatement against torch.autograd and against its float32 twin, the descriptor,
the config key and compile's exclusions, the launches of a distilled step, the neutral settings, the teacher's state
around a student step, a training step of both models against the oracle models with the distilled gradient, every
refusal, test_step, a dense student under an attention teacher through adapt=, and fit."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd import think_and_tell as TT
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical as SC
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import (Adam, CategoricalCrossentropy, Distillation, check_distillation, loss_distillation)
from oracle import models as M
from helpers import synth_batch, tiny_groups
from smooth_oracle import SmoothMockBackend
from constrain_oracle import ConstrainMockBackend
from score_oracle import ScoreMockBackend
from ss_att_oracle import SSAttMockBackend
from distill_oracle import DistillMockBackend, distill_metrics, distilled, reference, reference32

B, N, T, V, U, E = 5, 23, 6, 13, 16, 16
LC = dict(R=4, D=16, A=5, Et=12)
HEAD_SCALE = 8.0       # on the vocabulary kernel: at initialisation p is near uniform and a teacher teaches nothing


class RecordingBackend(DistillMockBackend, SmoothMockBackend, ConstrainMockBackend, ScoreMockBackend, SSAttMockBackend):
    """the mock with every public call's name logged in ``names``"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if not name.startswith("_") and callable(v) and name not in ("names",):
            object.__getattribute__(self, "names").append(name)
        return v


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def loss_obj(alpha=0.5, t=2.0, **kw):
    return CategoricalCrossentropy(from_logits=False, reduction="none", distillation=Distillation(alpha, t), **kw)


def dense(rng, units=U, scale=HEAD_SCALE, **kw):
    model = NIC(N, units, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw)
    orc = M.NICDense(N, units, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    orc.p["time_distributed_softmax/kernel"] *= scale
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def attention(rng, cls=LcNIC, orc_cls=M.LcNIC, units=U, scale=HEAD_SCALE, **kw):
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    args = (g, units, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    model = cls(*args, device="cpu", seed=11, **kw)
    orc = orc_cls(*args).init_params(rng) if orc_cls is not None else None
    if orc is not None:
        orc.p["time_distributed_softmax/kernel"] *= scale
        for k, v in orc.p.items():
            model.set_weight(k, v)
    return model, orc


MAKE = {"dense": dense, "attention": attention}


def batch(rng, b=B):
    return synth_batch(b, N, T, V, U, rng)


def oracle_probs(orc, data, training, step=0):
    out = orc.forward(data, training, M.DropCtx(seed=11, step=step, training=training))[0]
    return out[0] if isinstance(out, tuple) else out


def teacher_logits(torc, data):
    """what the oracle teacher's inference forward gives, as logits: softmax(u / t) does not see the row constant log Z"""
    return np.log(oracle_probs(torc, data, False))


# ---------------------------------------------------------------------------------------------------- the restatement
def _rows(rng, rows=7, Vv=11):
    x, u = rng.standard_normal((rows, Vv)) * 2, rng.standard_normal((rows, Vv)) * 3
    y = rng.integers(0, Vv, rows)
    y[3] = Vv + 2                                            # outside [0, V): ce constant, no hard gradient
    x[5, y[5]] = x[5].max() - 40.0                           # the target clipped low: likewise
    return x, u, y


@pytest.mark.parametrize("alpha,t", [(0.0, 1.0), (0.5, 1.0), (0.5, 2.0), (1.0, 4.0), (0.3, 0.5)])
def test_reference_gradient_against_autograd(alpha, t):
    x, u, y = _rows(np.random.default_rng(12))
    rows, Vv = x.shape
    gscale = 0.37
    ref = reference(x, u, y, alpha, t, gscale)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ut = torch.tensor(u, dtype=torch.float64)
    p = torch.softmax(xt, 1)
    ok = torch.tensor((y >= 0) & (y < Vv))
    py = torch.where(ok, p[torch.arange(rows), torch.tensor(np.where((y >= 0) & (y < Vv), y, 0))], torch.zeros(rows, dtype=torch.float64))
    ce = -torch.log(torch.clamp(py, 1e-7, 1 - 1e-7))
    kl = (torch.softmax(ut / t, 1) * (torch.log_softmax(ut / t, 1) - torch.log_softmax(xt / t, 1))).sum(1)
    loss = (1 - alpha) * ce + alpha * t * t * kl
    (gscale * loss.sum()).backward()
    assert np.abs(ref["loss"] - loss.detach().numpy()).max() < 1e-12 and np.abs(ref["kl"] - kl.detach().numpy()).max() < 1e-12
    assert np.abs(ref["grad"] - xt.grad.numpy()).max() < 1e-13
    assert ref["my"][3] == 0 and ref["my"][5] == 0 and (ref["kl"] > 0).all()
    if alpha == 0:
        keep = ref["ok"]
        assert np.abs(ref["loss"][keep] - M.O.cce_from_probs(ref["p"][keep], y[keep])).max() < 1e-15
        assert np.abs(ref["grad"][keep] - M.O.cce_softmax_bwd(ref["p"][keep], y[keep], np.full(keep.sum(), gscale))).max() < 1e-15
        assert (ref["grad"][[3, 5]] == 0).all()
    else:
        assert np.abs(ref["grad"][[3, 5]]).max() > 1e-3                          # the teacher's term has no clip


def test_float32_twin_and_planted_rows():
    x, u, y = _rows(np.random.default_rng(13))
    x32, u32 = x.astype(np.float32), u.astype(np.float32)
    r64, r32 = reference(x32, u32, y, 0.5, 2.0, 0.25), reference32(x32, u32, y, 0.5, 2.0, 0.25)
    assert r32["grad"].dtype == np.float32 and r32["loss"].dtype == np.float32
    for k in ("loss", "kl", "grad"):
        assert np.abs(r32[k] - r64[k]).max() < 2e-5
    same = reference(x32, x32, y, 1.0, 2.0, 1.0)                              # teacher == student
    assert (same["kl"] == 0).all() and (same["grad"] == 0).all()
    hot = x32.copy(); hot[:, 2] = hot.max(1) + 60                              # qt underflows to exactly 0 elsewhere at t = 0.05
    r = reference(x32, hot, y, 1.0, 0.05, 1.0)
    assert (np.delete(r["qt"], 2, 1) == 0).all() and np.isfinite(r["kl"]).all() and np.isfinite(r["grad"]).all()
    assert np.allclose(r["kl"], -np.log(r["pt"][:, 2]))


def test_mock_op_follows_the_restatement(mock_backend):
    rng = np.random.default_rng(10)
    x, u, y = _rows(rng, 8, 11)
    rows, Vv = x.shape
    ld, ldt = Vv + 3, Vv + 1
    buf, tbuf = torch.full((rows, ld), 7.0), torch.full((rows, ldt), 9.0)
    buf[:, :Vv], tbuf[:, :Vv] = torch.tensor(x, dtype=torch.float32), torch.tensor(u, dtype=torch.float32)
    x32, u32 = buf[:, :Vv].numpy().copy(), tbuf[:, :Vv].numpy().copy()
    loss, kl, corr = torch.zeros(rows), torch.zeros(rows), torch.zeros(rows)
    mock_backend.softmax_cce_distill(buf, tbuf, torch.tensor(y, dtype=torch.int32), loss, kl, corr, buf, rows, Vv, ld, ldt, 0.25,
                                     0.5, 2.0)
    ref = reference(x32, u32, y, 0.5, 2.0, 0.25)
    assert np.allclose(loss.numpy(), ref["loss"], rtol=1e-6) and np.allclose(kl.numpy(), ref["kl"], rtol=1e-6, atol=1e-9)
    assert np.array_equal(corr.numpy(), ref["corr"].astype(np.float32))
    assert np.allclose(buf[:, :Vv].numpy(), ref["grad"], rtol=1e-6, atol=1e-9) and (buf[:, Vv:] == 7.0).all()
    assert np.array_equal(tbuf[:, :Vv].numpy(), u32) and (tbuf[:, Vv:] == 9.0).all()
    with pytest.raises(AssertionError):
        mock_backend.softmax_cce_distill(buf, tbuf, torch.tensor(y, dtype=torch.int32), loss, kl, corr, tbuf, rows, Vv, ldt, ldt,
                                         0.25, 0.5, 2.0)


# ---------------------------------------------------------------------------------------------------- the descriptor
def test_descriptor_and_checks():
    d = Distillation()
    assert (d.alpha, d.temperature, d.neutral) == (0.5, 2.0, False)
    assert Distillation(0, 3).neutral and Distillation(1, 0.5).alpha == 1.0
    assert Distillation(0.25, 4) == Distillation(0.25, 4.0) and Distillation(0.25, 4) != Distillation(0.25, 2)
    assert hash(Distillation(0.25, 4)) == hash(Distillation(0.25, 4.0)) and "0.25" in repr(Distillation(0.25, 4))
    for bad in (-0.1, 1.1, float("nan"), float("inf"), True, "0.5", None, [0.5]):
        with pytest.raises(ValueError):
            Distillation(alpha=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), True, "2", None):
        with pytest.raises(ValueError):
            Distillation(temperature=bad)
    assert CategoricalCrossentropy().distillation is None
    assert loss_distillation(None) is None and loss_distillation(object()) is None
    assert loss_distillation(loss_obj(0.0, 2.0)) is None                     # neutral
    assert loss_distillation(loss_obj(0.3, 1.5)) == Distillation(0.3, 1.5)
    assert check_distillation({"alpha": 0.3, "temperature": 1.5}) == Distillation(0.3, 1.5)
    assert check_distillation({"alpha": 0.3}) == Distillation(0.3, 2.0)
    for bad in ({"alpha": 2}, {"beta": 1}, 0.5, "x", (0.5, 2.0)):
        with pytest.raises(ValueError):
            CategoricalCrossentropy(distillation=bad)


def _config(**extra):
    c = dict(top_k=V - 1, units=U, embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], max_length=T,
             dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
             input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", clipnorm=0.1, alpha=1e-4)
    c.update(extra)
    return c


def test_build_model_config_key(mock_backend):
    rng = np.random.default_rng(8)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    m = cfg.build_model(_config(), g, device="cpu")
    assert m.distillation is None and not m._distill_on()
    m = cfg.build_model(_config(distillation={"alpha": 0.25, "temperature": 3.0}), g, device="cpu")
    assert m.distillation == Distillation(0.25, 3.0) and m._distill_on() and m.teacher is None
    assert cfg.build_model(_config(distillation={"alpha": 0.0}), g, device="cpu").distillation is None
    for bad in ({"alpha": -1}, {"temperature": 0}, {"alpha": 0.5, "t": 2}, 0.5):
        with pytest.raises(ValueError):
            cfg.build_model(_config(distillation=bad), g, device="cpu")
    with pytest.raises(NotImplementedError):
        cfg.build_model(_config(distillation={"alpha": 0.5}), None, mode="fc", input_size=N, device="cpu")
    assert mock_backend.names == []


@pytest.mark.parametrize("other", [dict(label_smoothing=0.1), dict(unlikelihood=0.5), dict(class_weight={0: 0.0}),
                                   dict(focal_gamma=2.0), dict(normalise="weights")])
def test_compile_refuses_another_head(other, mock_backend):
    model, _ = dense(np.random.default_rng(1))
    with pytest.raises(ValueError, match="one head kernel"):
        model.compile(Adam(1e-3), loss_obj(**other))
    assert model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(0.0, 2.0, **other))                   # the neutral descriptor goes with anything
    assert model.distillation is None and mock_backend.names == []


def test_weights_behind_compile_are_refused(mock_backend):
    """set_class_weight and fit(class_weight=) on a distilling model: compile's exclusion, before any launch"""
    rng = np.random.default_rng(1)
    model, _ = dense(rng)
    model.compile(Adam(1e-3), loss_obj())
    model.set_teacher(dense(rng)[0])
    with pytest.raises(ValueError, match="one head kernel"):
        model.set_class_weight({0: 0.0})
    with pytest.raises(ValueError, match="one head kernel"):
        model.fit([batch(rng)], epochs=1, verbose=0, class_weight={0: 0.0})
    assert model.class_weight is None and not model._token_weights_on() and mock_backend.names == []
    model.set_class_weight(None)                                               # clearing is always fine
    model.compile(Adam(1e-3), loss_obj(0.0))                                   # the neutral descriptor goes with weights
    model.set_class_weight({0: 0.0})
    assert model._token_weights_on()


def test_compile_refuses_self_critical(mock_backend):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, self_critical=SC(2))
    with pytest.raises(ValueError, match="self_critical"):
        model.compile(Adam(1e-3), loss_obj())
    with pytest.raises(NotImplementedError, match="self_critical"):
        model.set_teacher(dense(np.random.default_rng(1))[0])
    assert mock_backend.names == []


# ---------------------------------------------------------------------------------------------------- the step's launches
@pytest.mark.parametrize("teacher_kind", ["dense", "attention"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_launches_of_a_distilled_step(kind, teacher_kind, mock_backend):
    rng = np.random.default_rng(3)
    model, _ = MAKE[kind](rng)
    teacher, _ = MAKE[teacher_kind](rng)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(0.5, 2.0))
    model.set_teacher(teacher)
    data, tgt = batch(rng)
    # the teacher's part alone: its staging and its inference forward (the second time: the first one builds its buffers)
    for _ in range(2):
        mock_backend.names.clear()
        teacher._stage_batch(data, None, teacher._input_width())
        teacher._forward(B, T, False)
    teach = list(mock_backend.names)
    assert teach and not any(n.startswith("softmax_cce") or n.startswith("dropout") for n in teach)
    mock_backend.names.clear()
    got = model.train_step((data, tgt))
    names = list(mock_backend.names)
    assert names.count("softmax_cce_distill") == 1 and "softmax_cce" not in names and "softmax_cce_live" not in names
    assert "stage_batch_map" not in names and "dense_fwd_stream_gram_stage" not in names       # head_map=False
    at = names.index("softmax_cce_distill")
    starts = [i for i in range(at) if names[i:i + len(teach)] == teach]
    assert starts, "the teacher's forward launches are not in front of the head launch"
    assert "distill_kl" in got and set(got) >= {"loss", "L2", "accuracy"}
    (c,) = mock_backend.ds_calls
    assert (c["rows"], c["V"], c["alpha"], c["temperature"], c["gscale"]) == (T * B, V, 0.5, 2.0, 1.0 / (T * B))
    assert c["want_grad"] and c["teacher_tensor"] is teacher.logits and c["ld"] == model.ldV and c["ld_teacher"] == teacher.ldV
    assert np.array_equal(c["target"].reshape(T, B).T, tgt)
    # test_step, __call__, the decodes and score_captions never run the teacher: none of its methods is entered
    ran = []
    for name in ("_stage_batch", "_stage_inputs", "_forward", "_run_captured"):
        def spy(*a, _f=getattr(teacher, name), _n=name, **k):
            ran.append(_n)
            return _f(*a, **k)
        setattr(teacher, name, spy)
    x, cap, a0, c0 = data
    start = np.ones(B, np.int64)
    mock_backend.names.clear()
    model.test_step((data, tgt))
    model(data)
    model.greedy_predict(x, a0, c0, start, T)
    model.beam_search(x, a0, c0, start, T, beam_width=2, end_id=2)
    model.score_captions(x, a0, c0, cap)
    assert ran == [] and "softmax_cce_distill" not in mock_backend.names and len(mock_backend.ds_calls) == 1
    model.train_step((data, tgt))
    assert "_forward" in ran and len(mock_backend.ds_calls) == 2            # (the spies do see a teacher that runs)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_neutral_settings_issue_the_plain_step(kind, mock_backend):
    logs = []
    for how in ("plain", "alpha 0", "alpha 0 and a teacher", "teacher detached"):
        rng = np.random.default_rng(2)
        model, _ = MAKE[kind](rng)
        teacher, _ = MAKE[kind](np.random.default_rng(99))
        model.compile(Adam(1e-3, clipnorm=0.1), None if how == "plain" else loss_obj(0.0, 2.0))
        if how in ("alpha 0 and a teacher", "teacher detached"):
            model.set_teacher(teacher)
        if how == "teacher detached":
            model._graphs = {"x": 1}
            model.set_teacher(None)
            assert model.teacher is None and model._graphs == {}               # ... and drops the recordings
        data, tgt = batch(rng)
        mock_backend.names.clear()
        m1 = model.train_step((data, tgt)).as_floats()
        m2 = model.test_step((data, tgt)).as_floats()
        logs.append((list(mock_backend.names), m1, m2, model.arena.theta.clone()))
    for l in logs[1:]:
        assert l[:3] == logs[0][:3] and torch.equal(l[3], logs[0][3])
    assert "distill_kl" not in logs[0][1] and mock_backend.ds_calls == [] and model.kl_row is None


def test_set_teacher_drops_the_recordings_and_checks_the_pair(mock_backend):
    rng = np.random.default_rng(4)
    model, _ = dense(rng)
    teacher, _ = attention(rng)
    model._graphs = {"x": 1}
    model.set_teacher(teacher, adapt=lambda d: d)
    assert model.teacher is teacher and model._graphs == {}
    with pytest.raises(ValueError, match="adapt"):
        model.set_teacher(None, adapt=lambda d: d)
    with pytest.raises(ValueError, match="adapt"):
        model.set_teacher(teacher, adapt=3)
    other = NIC(N, U, E, V + 1, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    with pytest.raises(ValueError, match="vocabulary"):
        model.set_teacher(other)
    other = NIC(N, U, E, V, T + 1, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    with pytest.raises(ValueError, match="caption length"):
        model.set_teacher(other)
    assert model.teacher is teacher and mock_backend.names == []


@pytest.mark.parametrize("teacher_kind", ["dense", "attention"])
def test_a_rebuilt_teacher_drops_the_students_recordings(teacher_kind, mock_backend):
    """the teacher allocates new buffers whenever it is staged at another shape and drops only its own recordings: the
    student's, which hold the address of teacher.logits, go with them"""
    rng = np.random.default_rng(4)
    model, _ = dense(rng)
    teacher, _ = MAKE[teacher_kind](rng)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj())
    model.set_teacher(teacher)
    data, tgt = batch(rng)
    model.train_step((data, tgt))
    model._graphs = {"kept": 1}
    model.train_step((data, tgt))
    assert model._graphs == {"kept": 1}                                       # nothing moved: nothing dropped
    old = teacher.logits
    teacher.test_step(batch(rng, B + 2))                                       # the teacher's own use at another batch size
    assert teacher.logits is not old
    model.train_step((data, tgt))
    assert "kept" not in model._graphs and teacher.logits is not old
    assert mock_backend.ds_calls[-1]["teacher_tensor"] is teacher.logits
    assert model._teacher_held[0] == teacher.logits.data_ptr()
    model._graphs = {"kept": 1}
    model.train_step((data, tgt))
    assert model._graphs == {"kept": 1}


def test_a_teacher_trained_with_scheduled_sampling_runs_teacher_forced(mock_backend):
    rng = np.random.default_rng(4)
    model, _ = dense(rng)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj())
    data, tgt = batch(rng)
    logs = []
    for kw in ({}, dict(scheduled_sampling=SS.linear(0.5, 0.0))):
        teacher, _ = dense(np.random.default_rng(5), **kw)
        model.set_teacher(teacher)
        model.train_step((data, tgt))                                          # (the first step builds the teacher)
        mock_backend.names.clear()
        model.train_step((data, tgt))
        logs.append((list(mock_backend.names), mock_backend.ds_calls[-1]["teacher"]))
    assert logs[0][0] == logs[1][0] and "scheduled_feedback" not in logs[1][0]
    assert np.array_equal(logs[0][1], logs[1][1])


# ---------------------------------------------------------------------------------------------------- the teacher's state
def _state(m):
    out = [m.arena.theta.clone(), m.drop_step.clone()] + [t.clone() for t in m.state_tensors()]
    for k in ("opt_m", "opt_v", "adam_t"):
        if getattr(m, k, None) is not None:
            out.append(getattr(m, k).clone())
    return out


@pytest.mark.parametrize("teacher_kind", ["dense", "attention"])
def test_a_student_step_leaves_the_teacher_alone(teacher_kind, mock_backend):
    rng = np.random.default_rng(5)
    data, tgt = batch(rng)
    data2, tgt2 = batch(rng)
    runs = {}
    for behind in (False, True):
        r = np.random.default_rng(6)
        student, _ = dense(r)
        teacher, _ = MAKE[teacher_kind](r)
        teacher.compile(Adam(1e-3, clipnorm=0.1))
        teacher.train_step((data, tgt))                                        # a teacher with moments and moved statistics
        if behind:
            student.compile(Adam(1e-3, clipnorm=0.1), loss_obj())
            student.set_teacher(teacher)
            before = _state(teacher)
            its = teacher.optimizer.iterations
            student.train_step((data2, tgt2)).as_floats()
            after = _state(teacher)
            assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
            assert teacher.optimizer.iterations == its
        m = teacher.train_step((data2, tgt2)).as_floats()                      # ... and trains on as if nothing had happened
        runs[behind] = (m, _state(teacher))
    assert runs[True][0] == runs[False][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[True][1], runs[False][1]))


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("alpha,t", [(0.5, 2.0), (1.0, 4.0)])
@pytest.mark.parametrize("teacher_kind", ["dense", "attention"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_train_step_matches_the_distilled_oracle(kind, teacher_kind, alpha, t, mock_backend):
    rng = np.random.default_rng(7)
    model, orc = MAKE[kind](rng)
    teacher, torc = MAKE[teacher_kind](rng, scale=2 * HEAD_SCALE)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), loss_obj(alpha, t))
    model.set_teacher(teacher)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noise = {}
    for step in range(2):
        data, tgt = batch(rng)
        u = teacher_logits(torc, data)
        want_loss, want_kl, want_acc = distill_metrics(oracle_probs(orc, data, True, step), u, tgt, alpha, t)
        with distilled(u, alpha, t):
            res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        assert abs(want_loss - res["loss"]) > 100 * 2e-5 * res["loss"]               # not the plain loss, by far
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - want_loss) < 2e-5 * max(1, abs(want_loss))            # test_host_nic's bounds
        assert abs(got["distill_kl"] - want_kl) < 2e-5 * max(1, abs(want_kl)) and want_kl > 1e-3
        assert abs(got["accuracy"] - want_acc) < 1e-6
        for k, v in orc.p.items():
            if k == "attention/V/bias":                  # zero-gradient variable: Adam amplifies rounding noise
                continue
            if grads.get(k) is not None:                 # test_gpu_nic's rule: where the gradient is rounding noise
                noise[k] = noise.get(k, 0.0) + 1e-3 * (np.abs(grads[k]) < 1e-8)   # (|g| < 1e-8), Adam steps +-lr at random
            assert (np.abs(model.get_weight(k) - v) <= 3e-6 + 2e-4 * np.abs(v) + noise.get(k, 0.0)).all(), (step, k)
    # test_step reports the plain cross-entropy
    data, tgt = batch(rng)
    want = orc.test_step(data, tgt)[0]
    got = model.test_step((data, tgt)).as_floats()
    assert "distill_kl" not in got and abs(got["loss"] - want["loss"]) < 2e-5 * max(1, want["loss"])


def test_dense_student_under_an_attention_teacher_through_adapt(mock_backend):
    rng = np.random.default_rng(9)
    U2 = 2 * U
    model, orc = dense(rng)
    teacher, torc = attention(rng, units=U2, scale=2 * HEAD_SCALE)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(0.5, 2.0))
    data, tgt = batch(rng)
    model.set_teacher(teacher)
    with pytest.raises(ValueError, match="adapt"):                             # the teacher cannot stage the student's states
        model.train_step((data, tgt))

    def adapt(d):
        (x, cap, a0, c0), y = d
        return (x, cap, np.concatenate([a0, a0], 1), np.concatenate([c0, c0], 1)), y
    model.set_teacher(teacher, adapt=adapt)
    tdata = adapt((data, tgt))[0]
    want_loss, want_kl, _ = distill_metrics(oracle_probs(orc, data, True), teacher_logits(torc, tdata), tgt, 0.5, 2.0)
    got = model.train_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1, want_loss) and abs(got["distill_kl"] - want_kl) < 2e-5
    with pytest.raises(ValueError, match="captions"):
        model.set_teacher(teacher, adapt=lambda d: ((d[0][0], d[0][1][:, :-1]) + adapt(d)[0][2:], d[1]))
        model.train_step((data, tgt))


# ---------------------------------------------------------------------------------------------------- refusals
def _hook():
    hook = lambda m: None
    hook.world = 2
    return hook


REFUSED_AT_COMPILE = {
    "grad_sync": lambda rng: dense(rng, grad_sync=_hook())[0],
    "scheduled sampling": lambda rng: dense(rng, scheduled_sampling=SS.linear(0.5, 0.0))[0],
    "attention scheduled sampling": lambda rng: attention(rng, scheduled_sampling=SS.linear(0.5, 0.0))[0],
    "free running": lambda rng: attention(rng, teacher_forcing=False)[0],
    "ms2 S=2": lambda rng: attention(rng, MsNIC, None, n_subjects=2)[0],
    "fc": lambda rng: NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11),
}


@pytest.mark.parametrize("what", sorted(REFUSED_AT_COMPILE))
def test_refused_at_compile_and_at_set_teacher(what, mock_backend):
    rng = np.random.default_rng(1)
    model = REFUSED_AT_COMPILE[what](rng)
    with pytest.raises(NotImplementedError, match="distillation"):
        model.compile(Adam(1e-3), loss_obj())
    assert model.optimizer is None
    with pytest.raises(NotImplementedError, match="distillation"):
        model.set_teacher(dense(rng)[0])
    model.compile(Adam(1e-3), loss_obj(0.0))                                  # neutral: fine everywhere
    assert mock_backend.names == []


def test_think_and_tell_refuses(mock_backend):
    model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                None, T, device="cpu", seed=11)
    assert not model.SUPPORTS_DISTILLATION
    with pytest.raises(NotImplementedError, match="distillation"):
        model.compile(Adam(1e-3), loss_obj())
    with pytest.raises(NotImplementedError, match="distillation"):
        model.set_teacher(dense(np.random.default_rng(1))[0])
    assert model.optimizer is None and mock_backend.names == []


def test_refusals_of_a_compiled_model(mock_backend):
    rng = np.random.default_rng(2)
    data, tgt = batch(rng)
    # no teacher
    model, _ = dense(rng)
    model.compile(Adam(1e-3), loss_obj())
    with pytest.raises(RuntimeError, match="set_teacher"):
        model.train_step((data, tgt))
    # the student itself
    with pytest.raises(NotImplementedError, match="own teacher"):
        model.set_teacher(model)
    # gradient accumulation, at compile and assigned later
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        model.compile(Adam(1e-3, gradient_accumulation_steps=2), loss_obj())
    model.set_teacher(dense(rng)[0])
    model.optimizer.gradient_accumulation_steps = 2
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        model.train_step((data, tgt))
    model.optimizer.gradient_accumulation_steps = None
    # dp.attach
    with pytest.raises(NotImplementedError, match="distillation"):
        dp.attach(model, world=2, rank=0)
    # teachers that cannot teach
    for bad, match in ((attention(rng, LcNIC, None, n_subjects=2)[0], "n_subjects"),
                       (attention(rng, LcNIC, None, use_layer_norm=True)[0], "use_layer_norm"),
                       (attention(rng, LcNIC, None, teacher_forcing=False)[0], "teacher_forcing"),
                       (NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11), "teacher")):
        with pytest.raises(NotImplementedError, match=match):
            model.set_teacher(bad)
    # train_step_sam
    att, _ = attention(rng)
    att.compile(Adam(1e-3), loss_obj())
    att.set_teacher(dense(rng)[0])
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        att.train_step_sam((data, tgt))
    assert mock_backend.ds_calls == []


# ---------------------------------------------------------------------------------------------------- fit
def test_fit_two_epochs(mock_backend):
    rng = np.random.default_rng(7)
    model, _ = dense(rng)
    teacher, _ = attention(rng, scale=2 * HEAD_SCALE)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(0.5, 2.0))
    model.set_teacher(teacher)
    batches = [batch(rng) for _ in range(2)]
    before = teacher.arena.theta.clone()
    hist = model.fit(batches, epochs=2, verbose=0)
    assert len(mock_backend.ds_calls) == 4 and "softmax_cce" not in mock_backend.names
    assert len(hist["loss"]) == 2 and len(hist["distill_kl"]) == 2 and all(k > 0 for k in hist["distill_kl"])
    per_step = [reference(c["logits"], c["teacher"], c["target"], 0.5, 2.0, 1.0) for c in mock_backend.ds_calls]
    assert np.isclose(hist["loss"][0], np.mean([r["loss"].mean() for r in per_step[:2]]), rtol=1e-5)
    assert np.isclose(hist["distill_kl"][1], np.mean([r["kl"].mean() for r in per_step[2:]]), rtol=1e-5)
    assert torch.equal(teacher.arena.theta, before)
