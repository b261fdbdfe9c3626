"""Weight averaging (optimizers.MovingAverage / SWA) on the CPU through a mock backend that follows
tnt_weight_average_f32's header definition (tests/average_oracle.py): the wrappers, the place of the averaging launch in
every training route, the recursion over a run, the guard, swapping, saving, the callback, fit and the refusals."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import dp
from masters_thesis_amd import think_and_tell as TT
from masters_thesis_amd.callbacks import AverageModelCheckpoint, LearningRateScheduler, ModelCheckpoint
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical as SC
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import SGD, SWA, Adam, Average, MovingAverage
from average_oracle import EMA, AverageMockBackend, Recursion, plan, reference
from helpers import synth_batch, tiny_groups
from scst_oracle import SCSTMockBackend
from ss_att_oracle import SSAttMockBackend
from test_host_naive_attention import NaiveMockBackend

B, N, T, V, U, E = 5, 23, 6, 13, 16, 16
LC = dict(R=4, D=16, A=5, Et=12)
UPDATES = ("adam", "sgd", "dense_dw_adam", "adam_fin", "dense_dw_adam_fin")


class RecordingBackend(AverageMockBackend, SCSTMockBackend, SSAttMockBackend, NaiveMockBackend):
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


def dense(seed=1, **kw):
    rng = np.random.default_rng(seed)
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw)
    for name in model.trainable_names():
        model.set_weight(name, 0.3 * rng.standard_normal(model.keras_shapes[name]))
    return model


def attention(seed=1, cls=LcNIC, **kw):
    rng = np.random.default_rng(seed)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    model = cls(g, U, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11, **kw)
    for name in model.trainable_names():
        model.set_weight(name, 0.3 * rng.standard_normal(model.keras_shapes[name]))
    return model


def ema(opt=None, **kw):
    return MovingAverage(opt if opt is not None else Adam(1e-2, clipnorm=0.1), 0.5, **kw)


def batch(b=B, seed=3):
    return synth_batch(b, N, T, V, U, np.random.default_rng(seed))


def theta(model):
    return model.arena.theta.numpy().copy()


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_plan_follows_the_definition():
    assert plan(0, EMA, 0.9, False, 0, 1) == ("copy", None) and plan(1, EMA, 0.9, False, 0, 1) == ("copy", None)
    assert plan(3, EMA, 0.9, False, 3, 1) == ("copy", None) and plan(2, EMA, 0.9, False, 3, 1) == ("copy", None)
    assert plan(2, EMA, 0.5, False, 0, 1) == ("blend", 0.5)
    assert plan(4, EMA, 0.5, False, 2, 3) == ("skip", None) and plan(5, EMA, 0.5, False, 2, 3) == ("blend", 0.5)
    assert plan(2, EMA, 0.999, True, 0, 1) == ("blend", float(np.float32(1 - 2 / 11)))          # (1 + 1) / (10 + 1) wins
    assert plan(10 ** 6, EMA, 0.999, True, 0, 1) == ("blend", float(np.float32(1 - 0.999)))     # momentum wins
    assert plan(2, 1, 0.0, False, 0, 1) == ("blend", 0.5)                                       # SWA: n = 1 -> d = 1/2
    assert plan(1 + 7 * 3, 1, 0.0, False, 1, 3) == ("blend", float(np.float32(1 - 7 / 8)))
    w, e = np.float32([1.0, 2.0, 0.0]), np.float32([3.0, 2.0, 0.0])
    mode, out, bound = reference(w, e, 2, 1, 0.0, False, 0, 1)
    assert mode == "blend" and out.tolist() == [2.0, 2.0, 0.0] and (bound > 0).all()
    assert reference(w, e, 2, 1, 0.0, False, 0, 1, guard=5)[0] == "guard"
    # SWA over snapshots is their equal-weight mean
    rec = Recursion(np.float32([0.0]), 1, 0.0, False, 0, 1)
    for k in range(1, 6):
        rec.step(np.float32([k]))
    assert abs(rec.avg[0] - 3.0) <= rec.tol[0] and rec.modes == ["copy"] + ["blend"] * 4


# ---------------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_delegate_to_the_wrapped_descriptor():
    inner = Adam(1e-3, beta_1=0.8, beta_2=0.95, epsilon=1e-6, clipnorm=0.2)
    w = MovingAverage(inner, 0.9, start_step=3, dynamic_decay=True, every=2)
    assert (w.kind, w.lr, w.learning_rate, w.beta_1, w.beta_2, w.epsilon, w.clipnorm) == ("adam", 1e-3, 1e-3, 0.8, 0.95, 1e-6, 0.2)
    assert w.average == Average("ema", 0.9, True, 3, 2) and w.average.kind_id == 0
    assert (w.average.kind, w.average.momentum, w.average.dynamic, w.average.start_step, w.average.every) == ("ema", 0.9, True, 3, 2)
    w.lr = 0.5
    assert inner.lr == 0.5 and w.learning_rate == 0.5
    w.learning_rate = 0.25
    assert inner.lr == 0.25
    w.iterations += 2
    assert inner.iterations == 2 and w.iterations == 2
    s = SWA(SGD(0.1, momentum=0.9, clipnorm=1.0), start_averaging=4, average_period=5)
    assert (s.kind, s.lr, s.momentum, s.clipnorm) == ("sgd", 0.1, 0.9, 1.0)
    assert s.average == Average("swa", 0.0, False, 4, 5) and s.average.kind_id == 1
    assert SWA(Adam()).average == Average("swa", 0.0, False, 0, 10)
    assert MovingAverage(Adam()).average == Average("ema", 0.99, False, 0, 1)
    with pytest.raises(AttributeError):
        s.beta_1


def test_wrapper_validation():
    with pytest.raises(NotImplementedError):
        MovingAverage(Adam(), num_updates=100)
    for bad in (1.0, -0.1, float("nan"), "x", None, True):
        with pytest.raises(ValueError):
            MovingAverage(Adam(), bad)
    for bad in (-1, 1.5, "2", None, True):
        with pytest.raises(ValueError):
            MovingAverage(Adam(), start_step=bad)
        with pytest.raises(ValueError):
            SWA(Adam(), start_averaging=bad)
    for bad in (0, -3, 2.0, None, False):
        with pytest.raises(ValueError):
            MovingAverage(Adam(), every=bad)
        with pytest.raises(ValueError):
            SWA(Adam(), average_period=bad)
    for bad in (None, object(), MovingAverage(Adam())):
        with pytest.raises(ValueError):
            SWA(bad)


def test_learning_rate_scheduler_reaches_the_wrapped_optimizer(mock_backend):
    model = dense()
    inner = Adam(1e-2)
    model.compile(MovingAverage(inner, 0.5))
    cb = LearningRateScheduler(lambda epoch: 5e-3)
    cb.model = model
    cb.on_epoch_begin(0, {})
    assert inner.lr == 5e-3 and model.optimizer.lr == 5e-3
    model.train_step(batch())
    assert float(model.lr_dev[0]) == np.float32(5e-3)


# ---------------------------------------------------------------------------------------------------- one launch per step
def _tt(seed):
    return TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                               None, T, device="cpu", seed=11)


def _tt_batch(b):
    rng = np.random.default_rng(5)
    return rng.standard_normal((b, N)).astype(np.float32), None, rng.integers(1, V, (b, T)).astype(np.int32)


def _attr(model, **kw):
    for k, v in kw.items():
        setattr(model, k, v)
    return model


def _agc(model):
    model.enable_agc(0.02, 1e-3)
    return model


ROUTES = {
    "fused": lambda: (dense(), None, "train_step", batch()),
    "fused_update=False": lambda: (_attr(dense(), fused_update=False), None, "train_step", batch()),
    "fused_finalize=False": lambda: (_attr(dense(), fused_finalize=False), None, "train_step", batch()),
    "SGD": lambda: (dense(), SGD(0.01, momentum=0.9, clipnorm=0.1), "train_step", batch()),
    "AGC": lambda: (_agc(dense()), None, "train_step", batch()),
    "attention": lambda: (attention(), None, "train_step", batch()),
    "attention SGD": lambda: (attention(), SGD(0.01, momentum=0.9), "train_step", batch()),
    "train_step_sam": lambda: (attention(), None, "train_step_sam", batch()),
    "scheduled sampling": lambda: (dense(scheduled_sampling=SS.linear(0.5, 0.0)), None, "train_step", batch()),
    "attention scheduled sampling": lambda: (attention(scheduled_sampling=SS.linear(0.5, 0.0)), None, "train_step", batch()),
    "teacher_forcing=False": lambda: (attention(teacher_forcing=False), None, "train_step", batch()),
    "SCST": lambda: (dense(self_critical=SC(2, n_samples=2, baseline="mean", reward="bleu4")), None, "train_step", batch()),
    "NICfc": lambda: (NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11), None, "train_step", batch()),
    "ms_nic": lambda: (attention(cls=MsNIC, n_subjects=2), None, "train_step", batch(6)),
    "ThinkAndTell": lambda: (_tt(1), None, "train_step", _tt_batch(4)),
    "ThinkAndTell SAM": lambda: (_tt(1), None, "train_step_SAM", _tt_batch(4)),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_ends_in_one_averaging_launch(route, mock_backend):
    model, inner, method, data = ROUTES[route]()
    model.compile(ema(inner, start_step=1, every=2))
    for step in range(1, 4):
        mock_backend.names.clear()
        mock_backend.avg_calls.clear()
        getattr(model, method)(data).as_floats()
        names = mock_backend.names
        assert names.count("weight_average") == 1 and names[-1] == "weight_average", (route, step, names[-6:])
        assert max(i for i, n in enumerate(names) if n in UPDATES) < names.index("weight_average")
        (call,) = mock_backend.avg_calls
        # adam_t is the number of applied updates when the launch runs, whichever launch ticked it
        assert call["t"] == step and call["n"] == model.arena.total and call["guard"] == 0
        assert (call["kind"], call["momentum"], call["dynamic"], call["start_step"], call["every"]) == (0, 0.5, False, 1, 2)
        assert call["mode"] == ("copy", "skip", "blend")[step - 1]
    assert "swap" not in mock_backend.names


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_without_averaging_nothing_changes(kind, mock_backend):
    make = dense if kind == "dense" else attention
    runs = {}
    for name, opt in (("plain", lambda: Adam(1e-2, clipnorm=0.1)), ("averaged", lambda: ema(start_step=0))):
        model = make()
        model.compile(opt())
        mock_backend.names.clear()
        mets = [model.train_step(batch(seed=s)).as_floats() for s in (3, 4, 5)]
        runs[name] = (list(mock_backend.names), theta(model), model.opt_m.numpy().copy(), model.opt_v.numpy().copy(), mets, model)
    plain, averaged = runs["plain"], runs["averaged"]
    assert "weight_average" not in plain[0] and plain[5].opt_avg is None and plain[5].average is None
    assert [n for n in averaged[0] if n != "weight_average"] == plain[0] and averaged[0].count("weight_average") == 3
    for a, b in zip(plain[1:4], averaged[1:4]):
        assert np.array_equal(a, b)
    assert plain[4] == averaged[4]
    assert not np.array_equal(averaged[5].opt_avg.numpy(), averaged[1])          # and the average is not the last iterate


# ---------------------------------------------------------------------------------------------------- the recursion
@pytest.mark.parametrize("wrapper", ["ema", "dynamic", "swa"])
def test_seven_steps_follow_the_oracle_recursion(wrapper, mock_backend):
    model = dense()
    inner = Adam(1e-2, clipnorm=0.1)
    opt = {"ema": lambda: MovingAverage(inner, 0.75, start_step=2, every=2),
           "dynamic": lambda: MovingAverage(inner, 0.75, start_step=2, dynamic_decay=True, every=2),
           "swa": lambda: SWA(inner, start_averaging=2, average_period=2)}[wrapper]()
    model.compile(opt)
    av = opt.average
    rec = None
    for step in range(1, 8):
        model.train_step(batch(seed=step)).as_floats()
        if rec is None:
            rec = Recursion(np.zeros(model.arena.total, np.float32), av.kind_id, av.momentum, av.dynamic, av.start_step, av.every)
        want, tol = rec.step(theta(model))
        got = model.opt_avg.numpy().astype(np.float64)
        assert (np.abs(got - want) <= tol).all(), (step, np.abs(got - want).max())
        if rec.modes[-1] == "copy":
            assert np.array_equal(model.opt_avg.numpy(), theta(model))
    assert rec.modes == ["copy", "copy", "skip", "blend", "skip", "blend", "skip"]
    assert [c["t"] for c in mock_backend.avg_calls] == list(range(1, 8))
    name = "time_distributed_softmax/kernel"
    slot = model.get_optimizer_slot(name, "average")
    assert slot.shape == tuple(model.keras_shapes[name]) and not np.array_equal(slot, model.get_weight(name))
    e = model.arena.entries[name]
    assert np.array_equal(model._unpack(name, model.opt_avg[e.off:e.off + e.size].view(e.shape)), slot)
    # the padding between the variables is zero in both buffers
    used = np.zeros(model.arena.total, bool)
    for e in model.arena.entries.values():
        used[e.off:e.off + e.size] = True
    assert not model.opt_avg.numpy()[~used].any() and not theta(model)[~used].any() and (~used).any()


def test_a_guarded_step_leaves_the_average(mock_backend):
    model = dense()
    model.compile(ema(start_step=0))
    for s in (3, 4):
        model.train_step(batch(seed=s))
    before = (theta(model), model.opt_avg.numpy().copy(), int(model.adam_t[0]))
    word = torch.ones(1, dtype=torch.int32)
    model._guard_word = lambda: word                 # the persistent chain's error word, set
    mock_backend.avg_calls.clear()
    model.train_step(batch(seed=5))
    assert [c["guard"] for c in mock_backend.avg_calls] == [1] and mock_backend.avg_calls[0]["mode"] == "guard"
    assert np.array_equal(theta(model), before[0]) and np.array_equal(model.opt_avg.numpy(), before[1])
    assert int(model.adam_t[0]) == before[2]
    word.zero_()
    model.train_step(batch(seed=5))
    assert mock_backend.avg_calls[-1]["t"] == before[2] + 1 and mock_backend.avg_calls[-1]["mode"] == "blend"
    assert not np.array_equal(model.opt_avg.numpy(), before[1])


def test_recompile_with_another_setting_drops_the_graphs(mock_backend):
    model = dense()
    model.compile(ema())
    model.train_step(batch())
    assert model.opt_avg is not None
    for opt, same in ((ema(), True), (ema(every=3), False), (SWA(Adam(1e-2)), False), (Adam(1e-2), False), (Adam(1e-2), True)):
        model._graphs["sentinel"] = 1
        model.__dict__["_init_optimizer_state"] = lambda: None          # compile's own reset aside
        try:
            model.compile(opt)
        finally:
            del model.__dict__["_init_optimizer_state"]
        assert ("sentinel" in model._graphs) == same, opt
    model.compile(Adam(1e-2))
    assert model.opt_avg is None and model.average is None
    mock_backend.names.clear()
    model.train_step(batch())
    assert "weight_average" not in mock_backend.names
    model.compile(ema())                                                # the slot starts again as a copy of the weights
    assert np.array_equal(model.opt_avg.numpy(), theta(model)) and int(model.adam_t[0]) == 0


# ---------------------------------------------------------------------------------------------------- using the average
def trained(make=dense, steps=4, **kw):
    model = make()
    model.compile(ema(start_step=0, **kw))
    for s in range(steps):
        model.train_step(batch(seed=10 + s))
    return model


def test_swap_twice_is_the_identity(mock_backend):
    model = trained()
    w, a = theta(model), model.opt_avg.numpy().copy()
    ptrs = (model.arena.theta.data_ptr(), model.opt_avg.data_ptr())
    mock_backend.names.clear()
    model.swap_weights()
    assert mock_backend.names == ["swap"] and model._swapped
    assert np.array_equal(theta(model), a) and np.array_equal(model.opt_avg.numpy(), w)
    name = "lstm/kernel"
    assert np.array_equal(model.get_weight(name), model.get_optimizer_slot(name, "average"))       # the slot follows the swap
    model.swap_weights()
    assert not model._swapped and np.array_equal(theta(model), w) and np.array_equal(model.opt_avg.numpy(), a)
    assert ptrs == (model.arena.theta.data_ptr(), model.opt_avg.data_ptr())


def test_averaged_weights_restores_on_exception_and_refuses_training(mock_backend):
    model = trained()
    w, a = theta(model), model.opt_avg.numpy().copy()
    data = batch(seed=20)
    plain = model.test_step(data).as_floats()
    with model.averaged_weights() as m:
        assert m is model and np.array_equal(theta(model), a)
        inside = model.test_step(data).as_floats()
        mock_backend.names.clear()
        for method in ("train_step",):
            with pytest.raises(RuntimeError, match="swapped"):
                getattr(model, method)(data)
        assert not set(mock_backend.names) & set(UPDATES) and "weight_average" not in mock_backend.names
        with pytest.raises(RuntimeError):
            model.assign_average_vars()
        with pytest.raises(RuntimeError):
            with model.averaged_weights():
                pass
    assert inside["loss"] != plain["loss"]
    assert np.array_equal(theta(model), w) and np.array_equal(model.opt_avg.numpy(), a) and not model._swapped
    with pytest.raises(KeyError):
        with model.averaged_weights():
            raise KeyError("inside")
    assert np.array_equal(theta(model), w) and np.array_equal(model.opt_avg.numpy(), a) and not model._swapped
    att = trained(attention)
    att.swap_weights()
    for method in ("train_step", "train_step_sam"):
        with pytest.raises(RuntimeError, match="swapped"):
            getattr(att, method)(data)
    att.swap_weights()
    att.train_step(data)
    model.train_step(data)                                                       # and training goes on afterwards


def test_assign_average_vars(mock_backend):
    model = trained()
    a = model.opt_avg.numpy().copy()
    model.assign_average_vars()
    assert np.array_equal(theta(model), a) and np.array_equal(model.opt_avg.numpy(), a)


@pytest.mark.parametrize("ext", ["npz", "h5"])
def test_save_averaged_and_load_into_a_fresh_model(ext, tmp_path, mock_backend):
    model = trained()
    path = str(tmp_path / f"avg.{ext}")
    model.save_weights(path, averaged=True)
    fresh = dense(seed=9)
    fresh.load_weights(path)
    for name in model.trainable_names():
        assert np.array_equal(fresh.get_weight(name), model.get_optimizer_slot(name, "average")), name
    assert not np.array_equal(fresh.get_weight("lstm/kernel"), model.get_weight("lstm/kernel"))
    for name in model.keras_shapes:                       # BatchNorm moving statistics: as they are
        if "moving_" in name:
            assert np.array_equal(fresh.get_weight(name), model.get_weight(name)), name
    assert any("moving_" in n for n in model.keras_shapes)
    raw = str(tmp_path / f"raw.{ext}")
    model.save_weights(raw)
    fresh.load_weights(raw)
    assert np.array_equal(fresh.get_weight("lstm/kernel"), model.get_weight("lstm/kernel"))
    model.swap_weights()                                  # the same file while the average is swapped in
    again = str(tmp_path / f"again.{ext}")
    model.save_weights(again, averaged=True)
    model.swap_weights()
    fresh.load_weights(again)
    assert np.array_equal(fresh.get_weight("lstm/kernel"), model.get_optimizer_slot("lstm/kernel", "average"))


@pytest.mark.parametrize("update_weights", [False, True])
def test_checkpoint_callback_and_validation_averaged(update_weights, tmp_path, mock_backend):
    model = dense()
    model.compile(ema(start_step=0))
    train = [batch(seed=30 + s) for s in range(3)]
    val = [batch(seed=40)]
    path = str(tmp_path / "ck_{epoch}.npz")
    cb = AverageModelCheckpoint(update_weights, path, monitor="val_loss")
    assert isinstance(cb, ModelCheckpoint)
    hist = model.fit(train, epochs=1, validation_data=val, validation_averaged=True, callbacks=[cb], verbose=0)
    a = model.opt_avg.numpy().copy()
    assert not model._swapped
    assert np.array_equal(theta(model), a) == update_weights
    with model.averaged_weights():
        want = model.test_step(val[0]).as_floats()
    assert hist["val_loss"] == [want["loss"]] and hist["val_accuracy"] == [want["accuracy"]]
    fresh = dense(seed=9)
    fresh.load_weights(str(tmp_path / "ck_1.npz"))
    assert np.array_equal(fresh.get_weight("lstm/kernel"), model.get_optimizer_slot("lstm/kernel", "average"))
    if not update_weights:
        plain = model.test_step(val[0]).as_floats()
        assert plain["loss"] != want["loss"]
        hist2 = model.fit(train[:0], epochs=1, steps_per_epoch=0, validation_data=val, verbose=0)
        assert hist2["val_loss"] == [plain["loss"]]


# ---------------------------------------------------------------------------------------------------- refusals
def test_data_parallel_refuses(mock_backend):
    model = dense()
    model.compile(ema())
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    assert model.grad_sync is None
    other = dense()
    hook = lambda m: None
    hook.world = 2
    other.grad_sync = hook
    with pytest.raises(NotImplementedError, match="data-parallel"):
        other.compile(ema())
    assert other.optimizer is None and other.average is None
    other.compile(Adam(1e-2))
    assert mock_backend.names == []


def test_accessors_raise_without_averaging(tmp_path, mock_backend):
    model = dense()
    model.compile(Adam(1e-2))
    model.train_step(batch())
    mock_backend.names.clear()
    with pytest.raises(ValueError):
        model.get_optimizer_slot("lstm/kernel", "average")
    with pytest.raises(ValueError):
        model.swap_weights()
    with pytest.raises(ValueError):
        with model.averaged_weights():
            pass
    with pytest.raises(ValueError):
        model.assign_average_vars()
    with pytest.raises(ValueError):
        model.save_weights(str(tmp_path / "w.npz"), averaged=True)
    with pytest.raises(ValueError):
        model.fit([batch()], epochs=1, validation_data=[batch()], validation_averaged=True, verbose=0)
    cb = AverageModelCheckpoint(True, str(tmp_path / "c.npz"))
    cb.model = model
    with pytest.raises(ValueError):
        cb.on_epoch_end(0, {"val_loss": 1.0})
    assert mock_backend.names == [] and not list(tmp_path.iterdir())
    assert model.get_optimizer_slot("lstm/kernel", "m").shape == tuple(model.keras_shapes["lstm/kernel"])
    with pytest.raises(ValueError):
        class Bad(Adam):
            average = "ema"
        model.compile(Bad())
