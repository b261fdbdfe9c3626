"""Gradient accumulation (Adam / SGD gradient_accumulation_steps=) on the CPU through a mock backend that follows
tnt_grad_accumulate_f32's header definition (tests/accum_oracle.py): the descriptor, the launch sequence of a window, the
contract "k micro-steps on consecutive slices of a batch equal one step on the whole batch" at test_dp_gloo.py's sizes and
tolerances, the counters, the refusals and fit."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd import think_and_tell as TT
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import AttentionCoverage, DeviceGuardError, ScheduledSampling as SS, SelfCritical as SC
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import (SGD, SWA, Adam, AdamW, CategoricalCrossentropy, MovingAverage,
                                           check_gradient_accumulation_steps, schedules)
from accum_oracle import ADD, CLOSE, OPEN, AccumMockBackend, reference
from average_oracle import AverageMockBackend
from global_clip_oracle import GlobalClipMockBackend
from helpers import synth_batch, tiny_groups
from lr_schedule_oracle import LrScheduleMockBackend
from test_dp_gloo import DIMS, _make

D = DIMS
ADAM = dict(beta_2=0.98, epsilon=1e-8)
UPDATES = {"adam", "sgd", "adamw", "sgdw", "adam_gclip", "sgd_gclip", "adam_fin", "adamw_fin", "adam_fin_gclip", "dense_dw_adam",
           "dense_dw_adam_fin", "dense_dw_adamw", "dense_dw_adamw_fin", "dense_dw_adam_gclip", "dense_dw_adam_fin_gclip"}
PER_UPDATE = UPDATES | {"step_tick", "step_finalize", "lr_schedule", "weight_average", "global_sqnorm"}


class RecordingBackend(AccumMockBackend, GlobalClipMockBackend, LrScheduleMockBackend, AverageMockBackend):
    """the mock with the accumulation op; ``names`` logs every public call when it is called"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v):
            return v
        names = object.__getattribute__(self, "names")

        def logged(*a, **k):
            names.append(name)
            return v(*a, **k)
        return logged


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def batch(b=D["B"], seed=3):
    return synth_batch(b, D["N"], D["T"], D["V"], D["U"], np.random.default_rng(seed))


def slices(data, tgt, k):
    """the k consecutive slices of a batch"""
    n = tgt.shape[0] // k
    return [(tuple(a[j * n:(j + 1) * n] for a in data), tgt[j * n:(j + 1) * n]) for j in range(k)]


def theta(model):
    return model.arena.theta.numpy().copy()


# ---------------------------------------------------------------------------------------------------- the descriptor
def test_descriptor_validation():
    assert Adam(gradient_accumulation_steps=3).gradient_accumulation_steps == 3
    assert Adam().gradient_accumulation_steps is None and SGD().gradient_accumulation_steps is None
    assert Adam(gradient_accumulation_steps=1).gradient_accumulation_steps is None        # 1 is stored as None
    assert AdamW(gradient_accumulation_steps=np.int64(4)).gradient_accumulation_steps == 4
    assert SGD(0.1, gradient_accumulation_steps=2).gradient_accumulation_steps == 2
    assert check_gradient_accumulation_steps(None) is None and check_gradient_accumulation_steps(2) == 2
    for bad in (True, False, 2.0, "2", 0, -3, float("nan")):
        for make in (Adam, SGD, AdamW):
            with pytest.raises(ValueError, match="gradient_accumulation_steps"):
                make(gradient_accumulation_steps=bad)
    opt = Adam()
    opt.gradient_accumulation_steps = 5
    assert opt.gradient_accumulation_steps == 5
    with pytest.raises(ValueError):
        opt.gradient_accumulation_steps = 1.5
    assert opt.gradient_accumulation_steps == 5


def test_the_wrappers_delegate():
    for wrap in (lambda o: MovingAverage(o, 0.9), lambda o: SWA(o, 0, 2)):
        inner = Adam(gradient_accumulation_steps=3)
        w = wrap(inner)
        assert w.gradient_accumulation_steps == 3
        w.gradient_accumulation_steps = None
        assert inner.gradient_accumulation_steps is None
        with pytest.raises(ValueError):
            w.gradient_accumulation_steps = 0


def test_config_key():
    base = dict(optimizer="Adam", clipnorm=0.1, alpha=0.01)
    assert cfg.build_optimizer(base).gradient_accumulation_steps is None
    assert cfg.build_optimizer(dict(base, gradient_accumulation_steps=None)).gradient_accumulation_steps is None
    assert cfg.build_optimizer(dict(base, gradient_accumulation_steps=1)).gradient_accumulation_steps is None
    assert cfg.build_optimizer(dict(base, gradient_accumulation_steps=4)).gradient_accumulation_steps == 4
    assert cfg.build_optimizer(dict(base, optimizer="AdamW", gradient_accumulation_steps=2)).gradient_accumulation_steps == 2
    assert cfg.build_optimizer(dict(base, optimizer="SGD", gradient_accumulation_steps=8)).gradient_accumulation_steps == 8
    for bad in (0, -1, 2.5, "x", True):
        with pytest.raises(ValueError):
            cfg.build_optimizer(dict(base, gradient_accumulation_steps=bad))


def test_the_reference_follows_the_header_table():
    acc, grad = np.array([1, 2, np.nan], np.float32), np.array([10, 20, 30], np.float32)
    a, g, qa, qs, ds = reference(acc, grad, OPEN, 5.0, 7.0, 3)
    assert np.array_equal(a, grad) and np.array_equal(g, grad) and (qa, qs, ds) == (7.0, 7.0, 4)     # acc (NaN) is not read
    a, g, qa, qs, ds = reference(np.array([1, 2, 3], np.float32), grad, ADD, 5.0, 7.0, 0xFFFFFFFF)
    assert a.tolist() == [11, 22, 33] and np.array_equal(g, grad) and (qa, qs, ds) == (12.0, 7.0, 0)
    a, g, qa, qs, ds = reference(np.array([1, 2, 3], np.float32), grad, CLOSE, 5.0, 7.0, 9)
    assert a.tolist() == [1, 2, 3] and g.tolist() == [11, 22, 33] and (qa, qs, ds) == (5.0, 12.0, 9)
    a, g, qa, qs, ds = reference(np.array([1, 2, 3], np.float32), grad, ADD, 5.0, 7.0, 9, guard=2)
    assert a.tolist() == [1, 2, 3] and np.array_equal(g, grad) and (qa, qs, ds) == (5.0, 7.0, 9)
    a, g, qa, qs, ds = reference(np.zeros(0, np.float32), np.zeros(0, np.float32), ADD, None, None, None)
    assert a.size == 0 and (qa, qs, ds) == (None, None, None)
    # float32 adds, in the operand order acc + grad
    x, y = np.float32(1.0), np.float32(2.0 ** -24)
    assert reference([x], [y], ADD)[0][0] == np.float32(x + y) == np.float32(1.0)


# ---------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_with_k_unset_the_launch_names_are_unchanged(kind, mock_backend):
    runs = {}
    for name, opt in (("without", lambda: Adam(1e-3, **ADAM, clipnorm=0.1)),
                      ("none", lambda: Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=None)),
                      ("one", lambda: Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=1))):
        model = _make(kind, seed=100)
        model.compile(opt())
        mock_backend.names.clear()
        mets = [model.train_step(batch(seed=s)).as_floats() for s in (3, 4)]
        runs[name] = (list(mock_backend.names), theta(model), mets)
        assert model.acc_grad is None and model.acc_sq is None and model.accumulation_position == (0, 1)
    for name in ("none", "one"):
        assert runs[name][0] == runs["without"][0] and "grad_accumulate" not in runs[name][0]
        assert np.array_equal(runs[name][1], runs["without"][1]) and runs[name][2] == runs["without"][2]


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
@pytest.mark.parametrize("opt", ["adam", "sgd", "averaged schedule"])
def test_a_window_of_three_is_open_add_close(kind, opt, mock_backend):
    model = _make(kind, seed=100)
    sched = schedules.Warmup(schedules.CosineDecay(1e-3, 10), 2)
    model.compile({"adam": lambda: Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=3),
                   "sgd": lambda: SGD(0.01, momentum=0.9, gradient_accumulation_steps=3),
                   "averaged schedule": lambda: MovingAverage(Adam(sched, **ADAM, gradient_accumulation_steps=3), 0.5)}[opt]())
    for window in range(2):
        for j in range(3):
            mock_backend.names.clear()
            mock_backend.acc_calls.clear()
            model.train_step(batch(seed=10 * window + j)).as_floats()
            names = mock_backend.names
            (call,) = mock_backend.acc_calls
            assert names.count("grad_accumulate") == 1 and call["phase"] == j and call["n"] == model.arena.total
            assert call["guard"] == 0 and call["drop_step"] == 3 * window + j
            # the micro-step ran the dense Embedding backward, wrote the encoder gradient, nothing was deferred
            assert "embedding_bwd" in names and "embedding_bwd_sparse" not in names
            assert not {"stage_batch_map", "dense_fwd_stream_gram_stage", "softmax_cce_live"} & set(names)
            if j < 2:
                assert not PER_UPDATE & set(names), (j, sorted(PER_UPDATE & set(names)))
                assert names[-1] == "grad_accumulate"
                assert names.count("seg_sqnorm") == (1 if j == 0 else 0)            # the L2 metric: the opening micro-step
            else:
                i = names.index("grad_accumulate")
                assert not PER_UPDATE & set(names[:i]) and names[i + 1] == "seg_sqnorm"
                assert len(UPDATES & set(names[i:])) == 1 and names.count("step_tick") == 1
                assert names.count("lr_schedule") == names.count("weight_average") == (1 if opt == "averaged schedule" else 0)
            assert model.accumulation_position == ((j + 1) % 3, 3)
        assert model.iterations == window + 1 and model.optimizer.iterations == window + 1


# ---------------------------------------------------------------------------------------------------- the contract
def _optimizer(variant, k):
    if variant == "clipnorm":
        return Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=k)
    if variant == "global_clipnorm":
        return Adam(1e-3, **ADAM, global_clipnorm=0.05, gradient_accumulation_steps=k)
    if variant == "adamw":
        return AdamW(1e-3, weight_decay=0.01, **ADAM, clipnorm=0.1, gradient_accumulation_steps=k)
    if variant == "schedule":
        return Adam(schedules.Warmup(schedules.CosineDecay(1e-3, 4), 2, 1e-4), **ADAM, clipnorm=0.1, gradient_accumulation_steps=k)
    assert variant == "averaged"
    return MovingAverage(Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=k), 0.5, every=1)


CONTRACT = ([("clipnorm", 2), ("clipnorm", 3)] + [(v, 3) for v in ("global_clipnorm", "adamw", "schedule", "averaged")])


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
@pytest.mark.parametrize("variant,k", CONTRACT)
def test_k_micro_steps_equal_one_step_on_the_concatenated_batch(kind, variant, k, mock_backend):
    """norm="layer", no dropout, test_dp_gloo.py's sizes and tolerances; two windows"""
    acc, ref = _make(kind, seed=100), _make(kind, seed=100)
    acc.compile(_optimizer(variant, k))
    ref.compile(_optimizer(variant, None))
    rng = np.random.default_rng(7)
    for window in range(2):
        data, tgt = synth_batch(k * D["B"], D["N"], D["T"], D["V"], D["U"], rng)
        want = ref.train_step((data, tgt)).as_floats()
        got = [acc.train_step(mb).as_floats() for mb in slices(data, tgt, k)]
        assert abs(np.mean([m["loss"] for m in got]) - want["loss"]) < 1e-5
        assert abs(np.mean([m["accuracy"] for m in got]) - want["accuracy"]) < 1e-5
        # L2 is the term of the weights the micro-step's forward used: the window's, every micro-step
        assert all(abs(m["L2"] - want["L2"]) < 1e-6 * max(1.0, abs(want["L2"])) for m in got)
        if variant == "schedule":
            assert got[-1]["lr"] == want["lr"]
        a, r = acc.arena, ref.arena
        # every gradient (the window's mean, as get_gradient returns it behind the closing micro-step), the clip norms
        assert np.allclose(a.grad.numpy(), r.grad.numpy(), rtol=1e-4, atol=2e-6)
        assert np.allclose(a.sq_override.numpy(), r.sq_override.numpy(), rtol=1e-4)
        assert np.allclose(a.sq.numpy(), r.sq.numpy(), rtol=1e-4, atol=1e-12)
        if variant == "clipnorm":
            assert (np.sqrt(r.sq.numpy()) > 0.1).any()                          # the clip binds
        if variant == "global_clipnorm":
            assert acc.global_grad_norm() == pytest.approx(ref.global_grad_norm(), rel=1e-4) and ref.global_grad_norm() > 0.05
        for name, v in ref.get_weights_dict().items():
            if name == "attention/V/bias":
                continue
            assert np.allclose(acc.get_weight(name), v, rtol=1e-4, atol=2e-6), (window, name)
            if "moving_" not in name:
                assert np.allclose(acc.get_gradient(name), ref.get_gradient(name), rtol=1e-4, atol=2e-6), (window, name)
        if variant == "averaged":
            assert np.allclose(acc.opt_avg.numpy(), ref.opt_avg.numpy(), rtol=1e-4, atol=2e-6)
    assert acc.iterations == ref.iterations == 2


def test_a_micro_step_leaves_its_share_in_get_gradient(mock_backend):
    k = 2
    acc, ref = _make("nic", seed=100), _make("nic", seed=100)
    acc.compile(Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=k))
    ref.compile(Adam(1e-3, **ADAM, clipnorm=0.1))
    mb = batch(seed=5)
    acc.train_step(mb)
    ref.train_step(mb)
    for name in ("lstm/kernel", "emb_text/embeddings", "dense_img/kernel"):
        assert np.allclose(acc.get_gradient(name), ref.get_gradient(name) / k, rtol=1e-5, atol=1e-9), name


def test_micro_batches_of_different_sizes_give_the_mean_of_the_means(mock_backend):
    """the update is the mean of the k micro-batch gradients, whatever their sizes"""
    acc = _make("nic", seed=100)
    acc.compile(Adam(1e-3, **ADAM, clipnorm=None, gradient_accumulation_steps=2))
    grads = []
    for b, seed in ((4, 5), (3, 6)):
        one = _make("nic", seed=100)
        one.compile(Adam(1e-3, **ADAM, clipnorm=None))
        one.train_step(batch(b, seed))
        grads.append(one.arena.grad.numpy().copy())
        acc.train_step(batch(b, seed))
    assert np.allclose(acc.arena.grad.numpy(), (grads[0] + grads[1]) / 2, rtol=1e-5, atol=1e-9)
    assert acc.iterations == 1


# ---------------------------------------------------------------------------------------------------- counters
@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_counters(kind, mock_backend):
    model = _make(kind, seed=100)
    sched = schedules.Warmup(schedules.CosineDecay(1e-3, 10), 3, 1e-5)
    model.compile(Adam(sched, **ADAM, clipnorm=0.1, gradient_accumulation_steps=3))
    assert model.accumulation_position == (0, 3)
    lrs = []
    for i in range(7):
        before = theta(model)
        m = model.train_step(batch(seed=i)).as_floats()
        lrs.append(m["lr"])
        closed = i % 3 == 2
        assert model.iterations == model.optimizer.iterations == (i + 1) // 3 == int(model.adam_t[0])
        assert int(model.drop_step[0]) == i + 1
        assert model.accumulation_position == ((i + 1) % 3, 3)
        assert np.array_equal(theta(model), before) != closed
    # the lr metric is what the last applied update used: it moves once per window
    assert lrs[0] == lrs[1] == np.float32(sched(0)) and lrs[2] == np.float32(sched(0))
    assert lrs[3] == lrs[4] == lrs[2] and lrs[5] == np.float32(sched(1)) != lrs[2] and lrs[6] == lrs[5]


def test_reset_accumulation_drops_the_window(mock_backend):
    model, fresh = _make("nic", seed=100), _make("nic", seed=100)
    for m in (model, fresh):
        m.compile(Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=2))
    model.train_step(batch(seed=1))
    state = (theta(model), model.opt_m.numpy().copy(), model.opt_v.numpy().copy(), int(model.adam_t[0]))
    assert model.accumulation_position == (1, 2)
    model.reset_accumulation()
    assert model.accumulation_position == (0, 2)
    assert np.array_equal(theta(model), state[0]) and np.array_equal(model.opt_m.numpy(), state[1])
    assert np.array_equal(model.opt_v.numpy(), state[2]) and int(model.adam_t[0]) == state[3] == 0
    mock_backend.acc_calls.clear()
    for s in (2, 3):
        model.train_step(batch(seed=s))
        fresh.train_step(batch(seed=s))
    assert [c["phase"] for c in mock_backend.acc_calls] == [OPEN, OPEN, CLOSE, CLOSE]            # (the two models in turn)
    assert np.array_equal(theta(model), theta(fresh))                          # the dropped micro-batch left no trace


def test_a_guarded_micro_step_leaves_the_window_and_a_trip_reopens_it(mock_backend):
    model = _make("nic", seed=100)
    model.compile(Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=3))
    model.train_step(batch(seed=1))
    state = (theta(model), model.opt_m.numpy().copy(), model.opt_v.numpy().copy(), int(model.adam_t[0]),
             model.acc_grad.numpy().copy(), float(model.acc_sq[0]), int(model.drop_step[0]))
    word = torch.ones(1, dtype=torch.int32)
    model._guard_word = lambda: word                 # the persistent chain's error word, set
    mock_backend.acc_calls.clear()
    model.train_step(batch(seed=2))
    assert [(c["phase"], c["guard"]) for c in mock_backend.acc_calls] == [(ADD, 1)]
    assert np.array_equal(model.acc_grad.numpy(), state[4]) and float(model.acc_sq[0]) == state[5]
    assert int(model.drop_step[0]) == state[6]
    with pytest.raises(DeviceGuardError, match="discarded"):
        model._on_guard_trip(1)                      # what reading the guarded step's metrics does
    assert model.accumulation_position == (0, 3)
    assert np.array_equal(theta(model), state[0]) and np.array_equal(model.opt_m.numpy(), state[1])
    assert np.array_equal(model.opt_v.numpy(), state[2]) and int(model.adam_t[0]) == state[3]
    word.zero_()
    mock_backend.acc_calls.clear()
    for s in (3, 4, 5):
        model.train_step(batch(seed=s))
    assert [c["phase"] for c in mock_backend.acc_calls] == [OPEN, ADD, CLOSE] and model.iterations == 1
    plain = _make("nic", seed=100)
    plain.compile(Adam(1e-3, **ADAM, clipnorm=0.1))
    with pytest.raises(DeviceGuardError) as e:
        plain._on_guard_trip(1)
    assert "discarded" not in str(e.value)


# ---------------------------------------------------------------------------------------------------- changing k
def test_changing_k(mock_backend):
    model = _make("nic", seed=100)
    opt = Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=2)
    model.compile(opt)
    model.train_step(batch(seed=1))
    opt.gradient_accumulation_steps = 3
    with pytest.raises(RuntimeError, match="open window"):
        model.train_step(batch(seed=2))
    opt.gradient_accumulation_steps = 2
    model.train_step(batch(seed=2))                                          # closes the window
    assert model.accumulation_position == (0, 2) and model.iterations == 1
    model._graphs["sentinel"] = 1
    assert model._emb_state is not None
    opt.gradient_accumulation_steps = 3                                        # at j == 0: picked up
    mock_backend.acc_calls.clear()
    for s in (3, 4, 5):
        model.train_step(batch(seed=s))
        assert "sentinel" not in model._graphs
    assert [c["phase"] for c in mock_backend.acc_calls] == [OPEN, ADD, CLOSE] and model.iterations == 2
    # back to None: the accumulator goes, the Embedding backward's state restarts, the step is a fresh model's
    model._graphs["sentinel"] = 1
    old_state = model._emb_state
    opt.gradient_accumulation_steps = None
    fresh = _make("nic", seed=100)
    fresh.compile(Adam(1e-3, **ADAM, clipnorm=0.1))
    fresh.train_step(batch(seed=0))                                            # builds its state; then the model's goes in
    for name, v in model.get_weights_dict().items():
        fresh.set_weight(name, v)
    fresh.opt_m.copy_(model.opt_m); fresh.opt_v.copy_(model.opt_v); fresh.adam_t.copy_(model.adam_t)
    fresh.drop_step.copy_(model.drop_step)
    mock_backend.names.clear()
    got = model.train_step(batch(seed=6)).as_floats()
    names = [n for n in mock_backend.names if n != "embedding_bwd_parts"]      # (the size query of the rebuilt state)
    assert "sentinel" not in model._graphs and model._emb_state is not old_state
    assert model.acc_grad is None and model.acc_sq is None and "grad_accumulate" not in names
    mock_backend.names.clear()
    want = fresh.train_step(batch(seed=6)).as_floats()
    assert names == mock_backend.names and got == want
    assert np.array_equal(theta(model), theta(fresh)) and np.array_equal(model.arena.grad.numpy(), fresh.arena.grad.numpy())


# ---------------------------------------------------------------------------------------------------- refusals
N, U, E, V, T = 23, 16, 16, 13, 6
ACC = dict(gradient_accumulation_steps=2)


def dense(**kw):
    return NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw)


def attention(cls=LcNIC, **kw):
    g = (tiny_groups(N, 4, np.random.default_rng(1)), [16] * 4)
    return cls(g, U, 512, 12, 5, V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11, **kw)


def test_data_parallel_refuses(mock_backend):
    model = dense()
    model.compile(Adam(1e-3, **ACC))
    with pytest.raises(NotImplementedError, match="data parallel"):
        dp.attach(model, world=1, rank=0)
    assert model.grad_sync is None
    other = dense()
    hook = lambda m: None
    hook.world = 2
    other.grad_sync = hook
    for opt in (Adam(1e-3, **ACC), SGD(0.1, **ACC), MovingAverage(Adam(**ACC))):
        with pytest.raises(NotImplementedError, match="data parallel|data-parallel"):
            other.compile(opt)
    assert other.optimizer is None
    other.compile(Adam(1e-2, clipnorm=0.1))


def test_agc_refuses(mock_backend):
    model = dense()
    model.compile(Adam(1e-3, **ACC))
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc(0.02, 1e-3)
    model.enable_agc(None)
    other = dense()
    other.enable_agc(0.02, 1e-3)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.compile(Adam(1e-3, **ACC))
    # assigned behind compile, in front of the optimizer-state build: the build refuses
    opt = Adam(1e-3, clipnorm=0.1)
    other.compile(opt)
    opt.gradient_accumulation_steps = 2
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.train_step(synth_batch(4, N, T, V, U, np.random.default_rng(0)))
    # ... and behind a recorded step: the next step finds it
    opt.gradient_accumulation_steps = None
    third = dense()
    third.enable_agc(0.02, 1e-3)
    third.compile(opt)
    third.train_step(synth_batch(4, N, T, V, U, np.random.default_rng(0)))
    opt.gradient_accumulation_steps = 2
    with pytest.raises(NotImplementedError, match="enable_agc"):
        third.train_step(synth_batch(4, N, T, V, U, np.random.default_rng(0)))


def test_sam_refuses(mock_backend):
    model = attention()
    model.compile(Adam(1e-3, clipnorm=0.1, **ACC))
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam(synth_batch(4, N, T, V, U, np.random.default_rng(0)))


REFUSED = {
    "scheduled sampling": lambda: dense(scheduled_sampling=SS.linear(0.5, 0.0)),
    "attention scheduled sampling": lambda: attention(scheduled_sampling=SS.linear(0.5, 0.0)),
    "self critical": lambda: dense(self_critical=SC(2, n_samples=2, baseline="mean", reward="bleu4")),
    "teacher_forcing=False": lambda: attention(teacher_forcing=False),
    "attention_coverage": lambda: attention(attention_coverage=AttentionCoverage(0.5)),
    "n_subjects": lambda: attention(n_subjects=2),
    "ms_nic": lambda: attention(cls=MsNIC, n_subjects=2),
    "NICfc": lambda: NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11),
    "ThinkAndTell": lambda: TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0),
                                                TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0), None, T, device="cpu", seed=11),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_unsupported_models_and_modes_refuse(what, mock_backend):
    model = REFUSED[what]()
    for opt in (Adam(1e-3, **ACC), SGD(0.1, **ACC), SWA(Adam(**ACC))):
        with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
            model.compile(opt)
    assert model.optimizer is None and mock_backend.names == []
    model.compile(Adam(1e-3, gradient_accumulation_steps=1))                 # 1 is off


def test_normalise_weights_refuses(mock_backend):
    model = dense()
    with pytest.raises(NotImplementedError, match="normalise"):
        model.compile(Adam(1e-3, **ACC), CategoricalCrossentropy(class_weight={0: 0.0}, normalise="weights"))
    model.compile(Adam(1e-3, **ACC), CategoricalCrossentropy(class_weight={0: 0.0}, normalise="count"))
    model.set_class_weight({0: 0.5})
    # assigned behind compile: the optimizer-state build refuses
    other = dense()
    opt = Adam(1e-3)
    other.compile(opt, CategoricalCrossentropy(class_weight={0: 0.0}, normalise="weights"))
    opt.gradient_accumulation_steps = 2
    with pytest.raises(NotImplementedError, match="normalise"):
        other.train_step(synth_batch(4, N, T, V, U, np.random.default_rng(0)))


# ---------------------------------------------------------------------------------------------------- fit
def test_fit_carries_an_open_window_over_the_epoch_boundary(mock_backend):
    model = _make("nic", seed=100)
    model.compile(Adam(1e-3, **ADAM, clipnorm=0.1, gradient_accumulation_steps=3))
    batches = [batch(seed=s) for s in range(4)]
    hist = model.fit(batches, epochs=2, verbose=0)                             # 8 micro-steps: steps_per_epoch counts them
    assert [c["phase"] for c in mock_backend.acc_calls] == [OPEN, ADD, CLOSE, OPEN, ADD, CLOSE, OPEN, ADD]
    assert model.iterations == 2 and model.accumulation_position == (2, 3) and int(model.drop_step[0]) == 8
    assert len(hist["loss"]) == 2 and set(hist) == {"loss", "L2", "accuracy"}
    model.train_step(batches[0])
    assert model.iterations == 3 and model.accumulation_position == (0, 3)
