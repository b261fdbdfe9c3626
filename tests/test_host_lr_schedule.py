"""Learning-rate schedules (optimizers.schedules) on the CPU through a mock backend that follows tnt_lr_schedule_f32's
header definition (tests/lr_schedule_oracle.py): the descriptors, the place of the schedule's launch in every training
route, the float path left as it was, the guard, recompiling, the callbacks, set_iterations, the config key and two
data-parallel ranks."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import optimizers, schedules
from masters_thesis_amd.callbacks import LearningRateScheduler, ReduceLROnPlateau
from masters_thesis_amd.optimizers import SGD, Adam, MovingAverage
from masters_thesis_amd.schedules import (CosineDecay, CosineDecayRestarts, ExponentialDecay, InverseTimeDecay,
                                          PiecewiseConstantDecay, PolynomialDecay, Warmup)
import lr_schedule_oracle as O
from lr_schedule_oracle import LrScheduleMockBackend
from lr_schedule_cases import CASES
from average_oracle import AverageMockBackend
from scst_oracle import SCSTMockBackend
from ss_att_oracle import SSAttMockBackend
from test_host_average import ROUTES, attention, batch, dense, theta
from test_host_naive_attention import NaiveMockBackend

HERE = os.path.dirname(os.path.abspath(__file__))
READERS = ("step_tick", "span_sqnorm_lr", "dense_gram_norm", "step_finalize", "adam_fin", "sgd")      # of lr_dev


class RecordingBackend(LrScheduleMockBackend, AverageMockBackend, SCSTMockBackend, SSAttMockBackend, NaiveMockBackend):
    """every mock op of the training routes, the schedule's among them, with the name of every public call logged in
    ``names`` when it is called (a ``hasattr`` probe of the model's is no call)"""

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


def sched():
    return Warmup(CosineDecay(1e-2, 4, alpha=0.1), 2)


SCHED_PARAMS = O.pack(O.COSINE, [1e-2, 4, 0.1], w=2)

# ---------------------------------------------------------------------------------------------------- the descriptors
@pytest.mark.parametrize("case", sorted(CASES))
def test_descriptor_parameters_and_values_equal_the_oracle(case):
    make, want = CASES[case]
    s = make()
    assert s.params() == want and len(want) == 16
    for step in list(range(0, 40)) + [2 ** 31 + 5]:
        got = s(step)
        assert isinstance(got, float) and got == float(O.lr32(want, step)), (case, step, got, O.lr64(want, step))
    assert s == make() and hash(s) == hash(make()) and s != CosineDecay(0.5, 3)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError):
            s(bad)


def test_the_oracle_follows_the_definition():
    assert O.lr64(O.pack(O.EXPONENTIAL, [0.1, 5, 0.5, 0]), 10) == 0.1 * 0.25
    assert O.lr64(O.pack(O.EXPONENTIAL, [0.1, 5, 0.5, 1]), 9) == 0.1 * 0.5
    assert O.lr64(O.pack(O.INVERSE_TIME, [0.3, 5, 1.0, 0]), 5) == 0.15
    assert O.lr64(O.pack(O.COSINE, [1.0, 4, 0.0]), 0) == 1.0 and O.lr64(O.pack(O.COSINE, [1.0, 4, 0.25]), 9) == 0.25
    assert abs(O.lr64(O.pack(O.COSINE, [1.0, 4, 0.0]), 2) - 0.5) < 1e-15
    r = O.pack(O.RESTARTS, [1.0, 4, 2.0, 0.5, 0.0])         # periods 4, 8, 16: restarts at 4 and 12, each half as high
    assert [O.lr64(r, s) for s in (0, 4, 12)] == [1.0, 0.5, 0.25] and abs(O.lr64(r, 8) - 0.25) < 1e-15
    r1 = O.pack(O.RESTARTS, [1.0, 4, 1.0, 0.5, 0.0])
    assert [O.lr64(r1, s) for s in (0, 4, 8, 13)][:3] == [1.0, 0.5, 0.25]
    p = O.pack(O.POLYNOMIAL, [1.0, 4, 0.0, 1.0, 0])
    assert [O.lr64(p, s) for s in (0, 1, 4, 9)] == [1.0, 0.75, 0.0, 0.0]
    pc = O.pack(O.POLYNOMIAL, [1.0, 4, 0.0, 1.0, 1])         # cycle: D' = 4, 4, 8, 8, 12
    assert [O.lr64(pc, s) for s in (0, 4, 5, 8, 9)] == [1.0, 0.0, 1 - 5 / 8, 0.0, 1 - 9 / 12]
    pw = O.pack_piecewise([3, 5], [1.0, 0.5, 0.25])
    assert [O.lr64(pw, s) for s in (0, 3, 4, 5, 6, 100)] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25]
    w = O.pack(O.CONSTANT, [0.4], w=4, start=0.2)
    assert [O.lr64(w, s) for s in (0, 2, 4, 50)] == [0.2, 0.2 + 0.2 * 2 / 4, 0.4, 0.4]
    wp = O.pack_piecewise([3, 5], [1.0, 0.5, 0.25], w=2)
    assert [O.lr64(wp, s) for s in (0, 1, 2, 5, 6, 7, 8)] == [0.0, 0.5, 1.0, 1.0, 0.5, 0.5, 0.25]
    assert math.isnan(O.lr64([9.0] + [0.0] * 15, 3)) and math.isnan(O.lr64([0.5] + [0.0] * 15, 3))
    assert O.lr64(O.pack(O.CONSTANT, [0.4]), -7) == 0.4


def test_constructor_refusals():
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -1e-3, "x", None, True, 1e39):
        for make in (lambda v: ExponentialDecay(v, 5, 0.5), lambda v: InverseTimeDecay(v, 5, 0.5), lambda v: CosineDecay(v, 5),
                     lambda v: CosineDecayRestarts(v, 5), lambda v: PolynomialDecay(v, 5), lambda v: PolynomialDecay(0.1, 5, v),
                     lambda v: PiecewiseConstantDecay([3], [0.1, v]), lambda v: Warmup(v, 3), lambda v: Warmup(0.1, 3, v)):
            with pytest.raises(ValueError):
                make(bad)
    for bad in (0, -2, 2.0, 1.5, None, "3", True, 2 ** 31):
        for make in (lambda v: ExponentialDecay(0.1, v, 0.5), lambda v: InverseTimeDecay(0.1, v, 0.5), lambda v: CosineDecay(0.1, v),
                     lambda v: CosineDecayRestarts(0.1, v), lambda v: PolynomialDecay(0.1, v), lambda v: Warmup(0.1, v),
                     lambda v: PiecewiseConstantDecay([v], [0.1, 0.2]), lambda v: PiecewiseConstantDecay([1, v], [0.1, 0.2, 0.3])):
            with pytest.raises(ValueError):
                make(bad)
    for bad in (0.0, -0.5, nan, inf):
        with pytest.raises(ValueError):
            ExponentialDecay(0.1, 5, bad)
    for bad in (-0.5, nan, inf):
        with pytest.raises(ValueError):
            InverseTimeDecay(0.1, 5, bad)
    for bad in (-0.1, 1.1, nan):
        with pytest.raises(ValueError):
            CosineDecay(0.1, 5, alpha=bad)
        with pytest.raises(ValueError):
            CosineDecayRestarts(0.1, 5, alpha=bad)
    for bad in (0.5, 1.01, nan, inf):                        # t_mul: 1, or at least 1.05 (the subtraction loop's length)
        with pytest.raises(ValueError):
            CosineDecayRestarts(0.1, 5, t_mul=bad)
    CosineDecayRestarts(0.1, 5, t_mul=1.05)
    for bad in (0.0, -1.0, nan, inf):
        with pytest.raises(ValueError):
            CosineDecayRestarts(0.1, 5, m_mul=bad)
        with pytest.raises(ValueError):
            PolynomialDecay(0.1, 5, power=bad)
    for b, v in (([], [0.1]), ([3, 3], [1, 2, 3]), ([5, 3], [1, 2, 3]), ([3], [1]), ([3], [1, 2, 3]), (list(range(1, 9)), [0.1] * 9),
                 (3, [1, 2]), ([3], None)):
        with pytest.raises(ValueError):
            PiecewiseConstantDecay(b, v)
    with pytest.raises(ValueError):
        Warmup(Warmup(0.1, 3), 3)
    with pytest.raises(ValueError):                          # the warm-up's fields take the seventh boundary's place
        Warmup(PiecewiseConstantDecay(list(range(1, 8)), [0.1] * 8), 3)
    Warmup(PiecewiseConstantDecay(list(range(1, 7)), [0.1] * 7), 3)


def test_optimizers_hold_a_schedule():
    s = sched()
    for opt in (Adam(s, clipnorm=0.1), Adam(learning_rate=s), SGD(s, momentum=0.9), Adam(lr=s)):
        assert opt.learning_rate is s and opt.lr is s and optimizers.optimizer_schedule(opt) is s
        opt.learning_rate = 0.25
        assert opt.lr == 0.25 and opt.learning_rate == 0.25 and optimizers.optimizer_schedule(opt) is None
        opt.lr = s
        assert opt.learning_rate is s
    w = MovingAverage(Adam(s))
    assert w.learning_rate is s and optimizers.optimizer_schedule(w) is s
    assert optimizers.schedules is schedules and optimizers.optimizer_schedule(Adam(1e-3)) is None
    with pytest.raises((TypeError, ValueError)):
        Adam("fast")


# ---------------------------------------------------------------------------------------------------- one launch per step
def _compile(model, inner, s):
    if inner is None:
        inner = Adam(s, clipnorm=0.1)
    else:
        inner.learning_rate = s
    model.compile(inner)
    return inner


ALL_ROUTES = dict(ROUTES)
ALL_ROUTES["SGD plain"] = lambda: (dense(), SGD(0.01), "train_step", batch())


@pytest.mark.parametrize("route", sorted(ALL_ROUTES))
def test_every_route_computes_the_rate_once_in_front_of_its_first_reader(route, mock_backend):
    model, inner, method, data = ALL_ROUTES[route]()
    _compile(model, inner, sched())
    assert model.lr_schedule == sched()
    for step in range(1, 5):
        mock_backend.names.clear()
        mock_backend.lr_calls.clear()
        got = getattr(model, method)(data).as_floats()
        names = mock_backend.names
        assert names.count("lr_schedule") == 1, (route, step, names)
        readers = [i for i, n in enumerate(names) if n in READERS]
        assert readers and names.index("lr_schedule") < min(readers), (route, step, names)
        want = float(O.lr32(SCHED_PARAMS, step - 1))
        assert mock_backend.lr_calls == [dict(s=step - 1, lr=want)]
        assert got["lr"] == want and float(model.lr_dev[0]) == want and model.iterations == step, (route, step, got)
    assert model.lr_params.dtype == torch.float64 and model.lr_params.tolist() == SCHED_PARAMS


@pytest.mark.parametrize("kind", ["dense", "attention"])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_a_float_learning_rate_leaves_the_step_as_it_was(kind, opt, mock_backend):
    """the float path issues no schedule launch, holds no parameter buffer and writes lr_dev from the host as before; fed
    the scheduled run's rates it gives that run's names (less the schedule's launch) and that run's bits"""
    make = dense if kind == "dense" else attention
    new = (lambda lr: Adam(lr, clipnorm=0.1)) if opt == "adam" else (lambda lr: SGD(lr, momentum=0.9, clipnorm=0.1))

    def state(m):
        return [theta(m), m.opt_m.numpy().copy(), None if m.opt_v is None else m.opt_v.numpy().copy(), int(m.adam_t[0]),
                int(m.drop_step[0]), m.lr_dev.numpy().copy(), m.lr_t_dev.numpy().copy()]

    scheduled = make()
    scheduled.compile(new(sched()))
    mock_backend.names.clear()
    runs = []
    for s in (3, 4, 5):
        mets = scheduled.train_step(batch(seed=s)).as_floats()
        runs.append((mets, state(scheduled)))
    names_s = list(mock_backend.names)
    plain = make()
    o = new(0.5)
    plain.compile(o)
    assert plain.lr_schedule is None and plain.lr_params is None
    mock_backend.names.clear()
    for s, (mets, st) in zip((3, 4, 5), runs):
        o.lr = mets["lr"]
        got = plain.train_step(batch(seed=s)).as_floats()
        assert {k: v for k, v in mets.items() if k in got} == got and set(mets) - set(got) <= {"lr"}
        for a, b in zip(state(plain), st):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    names_p = list(mock_backend.names)
    assert plain.lr_schedule is None and plain.lr_params is None
    assert "lr_schedule" not in names_p and names_s.count("lr_schedule") == 3
    assert [n for n in names_s if n != "lr_schedule"] == names_p
    assert mock_backend.lr_calls == [dict(s=i, lr=float(O.lr32(SCHED_PARAMS, i))) for i in range(3)]


def test_a_guarded_step_leaves_the_counter_and_the_next_rate(mock_backend):
    model = dense()
    model.compile(Adam(sched(), clipnorm=0.1))
    lrs = [model.train_step(batch(seed=s)).as_floats()["lr"] for s in (3, 4)]
    assert lrs == [float(O.lr32(SCHED_PARAMS, s)) for s in (0, 1)]
    before = (theta(model), model.iterations)
    word = torch.ones(1, dtype=torch.int32)
    model._guard_word = lambda: word                 # the persistent chain's error word, set
    mock_backend.lr_calls.clear()
    model.train_step(batch(seed=5))
    assert np.array_equal(theta(model), before[0]) and model.iterations == before[1] == 2
    word.zero_()
    got = model.train_step(batch(seed=5)).as_floats()
    assert [c["s"] for c in mock_backend.lr_calls] == [2, 2]           # the same value computed again
    assert got["lr"] == float(O.lr32(SCHED_PARAMS, 2)) and model.iterations == 3


def test_recompiling_with_another_schedule_drops_the_graphs(mock_backend):
    model = dense()
    model.compile(Adam(sched(), clipnorm=0.1))
    model.train_step(batch())
    other = Warmup(CosineDecay(1e-2, 4, alpha=0.1), 3)
    for opt, same in ((Adam(sched()), True), (Adam(other), False), (Adam(other), True), (Adam(1e-2), False), (Adam(1e-2), True),
                      (SGD(ExponentialDecay(0.1, 3, 0.5)), False)):
        model._graphs["sentinel"] = 1
        model.__dict__["_init_optimizer_state"] = lambda: None          # compile's own reset aside
        try:
            model.compile(opt)
        finally:
            del model.__dict__["_init_optimizer_state"]
        assert ("sentinel" in model._graphs) == same, opt
    model.compile(Adam(other))                                          # seeds lr_dev with schedule(0), counter at 0
    assert float(model.lr_dev[0]) == other(0) and model.iterations == 0 and model.lr_params.tolist() == other.params()


def test_assigning_a_float_replaces_the_schedule_and_records_again(mock_backend):
    model = dense()
    opt = Adam(sched(), clipnorm=0.1)
    model.compile(opt)
    model.train_step(batch())
    model._graphs["sentinel"] = 1
    opt.learning_rate = 0.125
    mock_backend.names.clear()
    got = model.train_step(batch()).as_floats()
    assert "sentinel" not in model._graphs and "lr_schedule" not in mock_backend.names
    assert model.lr_schedule is None and model.lr_params is None and float(model.lr_dev[0]) == 0.125 and "lr" not in got
    model._graphs["sentinel"] = 1
    opt.learning_rate = 0.25                                            # a float for a float: the host write, as ever
    model.train_step(batch())
    assert "sentinel" in model._graphs and float(model.lr_dev[0]) == 0.25
    opt.learning_rate = sched()                                         # and back: at the counter's value, not at 0
    got = model.train_step(batch()).as_floats()
    assert "sentinel" not in model._graphs and got["lr"] == float(O.lr32(SCHED_PARAMS, 3))


# ---------------------------------------------------------------------------------------------------- callbacks
def test_callbacks_refuse_an_optimizer_that_holds_a_schedule(mock_backend):
    model = dense()
    model.compile(Adam(sched()))
    for cb in (LearningRateScheduler(lambda e: 1e-3), ReduceLROnPlateau("loss")):
        with pytest.raises(TypeError, match="schedule"):
            cb.set_model(model)
        cb.model = model
        with pytest.raises(TypeError, match="schedule"):
            cb.on_train_begin()
        with pytest.raises(TypeError, match="schedule"):
            model.fit([batch()], epochs=1, callbacks=[cb], verbose=0)
    assert model.iterations == 0
    model.compile(Adam(1e-2))
    for cb in (LearningRateScheduler(lambda e: 1e-3), ReduceLROnPlateau("loss")):
        cb.set_model(model)
        cb.on_train_begin()


def test_reduce_lr_on_plateau_arithmetic():
    class M:
        optimizer = Adam(1.0)
    cb = ReduceLROnPlateau("loss", factor=0.5, patience=2, min_delta=0.1, min_lr=0.2, cooldown=1, mode="min")
    cb.set_model(M)
    cb.on_train_begin()
    seen = []
    # keras's rule per epoch: a cooldown epoch is counted down and clears the wait; a gain of more than min_delta clears
    # it too; otherwise, outside the cooldown, the wait grows and at ``patience`` the rate drops (never below min_lr).
    # epoch 0 best; 1, 2 no gain -> 0.5; 3 (cooldown ends), 4 -> 0.25; 5; 6 gain; 7, 8 -> max(0.125, 0.2); then at min_lr
    losses = [1.0, 0.95, 0.95, 0.95, 0.95, 0.95, 0.5, 0.45, 0.45, 0.45, 0.45, 0.45, 0.45, 0.45, 0.45]
    for e, v in enumerate(losses):
        logs = {"loss": v}
        cb.on_epoch_end(e, logs)
        seen.append(M.optimizer.lr)
        assert "lr" in logs
    assert seen == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.25, 0.25] + [0.2] * 7
    up = ReduceLROnPlateau("val_accuracy", factor=0.1, patience=1, min_delta=0.0)
    M.optimizer = SGD(1.0)
    up.set_model(M)
    up.on_train_begin()
    for e, v in enumerate([0.5, 0.6, 0.6, 0.7]):
        up.on_epoch_end(e, {"val_accuracy": v})
    assert M.optimizer.lr == 0.1 and up.sign == -1
    up.on_epoch_end(9, {"loss": 1.0})                                   # the monitor is missing: nothing happens
    assert M.optimizer.lr == 0.1
    for bad in (dict(factor=1.0), dict(factor=-0.1), dict(mode="best"), dict(patience=-1), dict(min_lr=-1.0), dict(cooldown=-1)):
        with pytest.raises(ValueError):
            ReduceLROnPlateau(**bad)


# ---------------------------------------------------------------------------------------------------- the counter
def test_set_iterations_moves_the_schedule_and_leaves_the_dropout_counter(mock_backend):
    model = dense()
    with pytest.raises(RuntimeError):
        model.set_iterations(3)
    assert model.iterations == 0
    model.compile(Adam(sched(), clipnorm=0.1))
    for s in (3, 4, 5):
        model.train_step(batch(seed=s))
    drop = int(model.drop_step[0])
    assert model.iterations == 3 and drop == 3
    model.set_iterations(0)
    assert model.iterations == 0 and int(model.drop_step[0]) == drop
    got = model.train_step(batch(seed=6)).as_floats()
    assert got["lr"] == sched()(0) == 0.0 and model.iterations == 1 and int(model.drop_step[0]) == drop + 1
    model.set_iterations(40)
    assert model.train_step(batch(seed=7)).as_floats()["lr"] == sched()(40) == float(np.float32(1e-3))
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError):
            model.set_iterations(bad)


# ---------------------------------------------------------------------------------------------------- config.yaml
def test_config_key():
    base = dict(optimizer="Adam", clipnorm=0.1, alpha=0.01)
    plain = cfg.build_optimizer(base)
    assert plain.lr == 0.0001 and (plain.beta_2, plain.clipnorm) == (0.98, 0.1)
    assert cfg.build_optimizer(dict(base, optimizer="SGD")).lr == 0.01
    c = dict(base, lr_schedule=dict(kind="CosineDecay", initial_learning_rate=1e-2, decay_steps=4, alpha=0.1, warmup_steps=2))
    opt = cfg.build_optimizer(c)
    assert opt.learning_rate == sched() and (opt.beta_2, opt.clipnorm) == (0.98, 0.1)
    assert c["lr_schedule"]["kind"] == "CosineDecay"                    # the mapping is not consumed
    sgd = cfg.build_optimizer(dict(base, optimizer="SGD", lr_schedule=dict(kind="ExponentialDecay", initial_learning_rate=0.1,
                                                                           decay_steps=3, decay_rate=0.5, staircase=True)))
    assert sgd.kind == "sgd" and sgd.learning_rate == ExponentialDecay(0.1, 3, 0.5, staircase=True)
    pw = schedules.from_config(dict(kind="PiecewiseConstantDecay", boundaries=[3, 5], values=[1.0, 0.5, 0.25], warmup_steps=4,
                                    warmup_start=0.125))
    assert pw == Warmup(PiecewiseConstantDecay([3, 5], [1.0, 0.5, 0.25]), 4, 0.125)
    for bad in (dict(kind="LinearCosineDecay"), dict(initial_learning_rate=0.1), dict(kind="CosineDecay", decay_steps=4),
                dict(kind="CosineDecay", initial_learning_rate=0.1, decay_steps=4, beta=1), "CosineDecay",
                dict(kind="Warmup", after=0.3, warmup_steps=7), dict(kind="CosineDecay", initial_learning_rate=0.1, decay_steps=0)):
        with pytest.raises(ValueError):
            schedules.from_config(bad)


# ---------------------------------------------------------------------------------------------------- two ranks over gloo
def _worker(rank, world, port, kind, q):
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import masters_thesis_amd.ops as ops
    from masters_thesis_amd import dp
    from masters_thesis_amd.optimizers import Adam
    from test_dp_gloo import DIMS, _global_batch, _make
    ops.set_backend(RecordingBackend())
    model = _make(kind, seed=100 + rank)
    model.compile(Adam(sched(), beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    dp.attach(model)
    rng = np.random.default_rng(7)
    lrs, counts = [], []
    for step in range(3):
        data, tgt = _global_batch(rng, world)
        sl = slice(rank * DIMS["B"], (rank + 1) * DIMS["B"])
        ops.backend().names.clear()
        m = model.train_step((tuple(a[sl] for a in data), tgt[sl]))
        lrs.append(m.as_floats()["lr"])
        names = ops.backend().names
        counts.append((names.count("lr_schedule"), names.index("lr_schedule") < min(i for i, n in enumerate(names) if n in READERS)))
    q.put((rank, lrs, counts, type(model.grad_sync).__name__, model.iterations, model.get_weights_dict()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_two_ranks_follow_the_schedule(kind):
    world, port = 2, 37500 + (os.getpid() % 2000)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, kind, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, *rest = q.get(timeout=120)
        res[r] = rest
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [float(O.lr32(SCHED_PARAMS, s)) for s in (0, 1, 2)]
    for r in range(world):
        lrs, counts, sync, its, _ = res[r]
        assert lrs == want and counts == [(1, True)] * 3 and its == 3, (r, lrs, counts)
        assert sync == {"nic": "PipelinedDenseSync", "lcnic": "PipelinedAttentionSync"}[kind]      # through _tick
    for k in res[0][4]:
        assert np.array_equal(res[0][4][k], res[1][4][k]), k
