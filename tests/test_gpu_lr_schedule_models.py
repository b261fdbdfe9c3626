"""Learning-rate schedules through the models on the GPU: nic.NIC and lc_nic.NIC at the tiny sizes of
tests/test_gpu_average_models.py, eager, as a recorded launch plan and as a hipGraph, compiled with
Adam(Warmup(CosineDecay(1e-2, 4, alpha=0.1), 2), clipnorm=0.1).

Six training steps cross warm-up, record / capture and replay, the end of the warm-up (2) and the end of the decay (6):
what is under test is the schedule launch's place in front of the step's first reader of lr_dev and the device-side
counter it reads there.  The ``lr`` metric of step k must be the oracle's value at k - 1 applied updates, inside the bound
of tests/test_gpu_lr_schedule.py for a kind that calls cos (one float32 spacing).  A twin model compiled with a float
learning rate, whose ``optimizer.lr`` is set before each step to the float32 the first model reported, runs the same
kernels on the same lr bits: its parameters, moments and metrics must be bit-identical after every step."""
import numpy as np
import pytest
import torch

import lr_schedule_oracle as O
from test_gpu_average_models import RUNNERS, batches, build

pytestmark = pytest.mark.gpu

PARAMS = O.pack(O.COSINE, [1e-2, 4, 0.1], w=2)


def sched():
    from masters_thesis_amd.schedules import CosineDecay, Warmup
    return Warmup(CosineDecay(1e-2, 4, alpha=0.1), 2)


def adam(lr):
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=lr, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def sgd(lr):
    from masters_thesis_amd.optimizers import SGD
    return SGD(learning_rate=lr, momentum=0.9, clipnorm=0.1)


def follows(lr, s):
    """the bound of a kind that calls cos: equal or adjacent float32 values"""
    want = O.lr32(PARAMS, s)
    return abs(float(np.float32(lr)) - float(want)) <= float(np.spacing(want))


def same_state(a, b):
    torch.cuda.synchronize()
    ok = torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m)
    if a.opt_v is not None:
        ok = ok and torch.equal(a.opt_v, b.opt_v)
    return ok and torch.equal(a.lr_dev, b.lr_dev) and torch.equal(a.lr_t_dev, b.lr_t_dev) and torch.equal(a.adam_t, b.adam_t)


def twin_steps(model, twin, opt, data):
    """the scheduled model and its float twin over ``data``; returns the lr metrics"""
    lrs = []
    for step, d in enumerate(data, 1):
        got = model.train_step(d).as_floats()
        assert follows(got["lr"], step - 1), (step, got["lr"], float(O.lr32(PARAMS, step - 1)))
        assert model.iterations == step
        opt.lr = got["lr"]
        want = twin.train_step(d).as_floats()
        assert {k: v for k, v in got.items() if k in want} == want and set(got) - set(want) <= {"lr"}, (step, got, want)
        assert same_state(model, twin), step
        lrs.append(got["lr"])
    return lrs


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_six_steps_follow_the_schedule_and_the_float_twin(kind, runner):
    model, twin = build(kind, **RUNNERS[runner]), build(kind, **RUNNERS[runner])
    model.compile(adam(sched()))
    opt = adam(0.5)
    twin.compile(opt)
    lrs = twin_steps(model, twin, opt, batches(6))
    assert lrs[0] == 0.0                                     # warmup_start + (a0 - warmup_start) * 0 / w, whatever a0
    assert len(set(lrs)) == 6 and lrs[2] == max(lrs)
    if RUNNERS[runner]["use_graph"]:
        assert model._graphs and set(model._graphs) == set(twin._graphs), "the step was never recorded / captured"
    assert twin.lr_params is None and model.lr_params.tolist() == PARAMS
    # back to 0 applied updates: the schedule starts again, Adam's bias correction with it
    model.set_iterations(0)
    twin.set_iterations(0)
    assert model.iterations == 0
    opt.lr = 0.0
    d = batches(7)[6]
    got, want = model.train_step(d).as_floats(), twin.train_step(d).as_floats()
    assert got["lr"] == sched()(0) == 0.0 and model.iterations == 1
    assert {k: v for k, v in got.items() if k in want} == want and same_state(model, twin)


@pytest.mark.parametrize("runner", sorted(RUNNERS))
def test_sgd_on_the_dense_model(runner):
    model, twin = build("dense", **RUNNERS[runner]), build("dense", **RUNNERS[runner])
    model.compile(sgd(sched()))
    opt = sgd(0.5)
    twin.compile(opt)
    twin_steps(model, twin, opt, batches(6))


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_with_a_weight_average(kind):
    from masters_thesis_amd.optimizers import MovingAverage
    model, twin = build(kind), build(kind)
    model.compile(MovingAverage(adam(sched()), 0.5, start_step=1, every=2))
    opt = MovingAverage(adam(0.5), 0.5, start_step=1, every=2)
    twin.compile(opt)
    twin_steps(model, twin, opt, batches(6))
    torch.cuda.synchronize()
    assert torch.equal(model.opt_avg, twin.opt_avg) and not torch.equal(model.opt_avg, model.arena.theta)


def test_assigning_a_float_records_the_step_again():
    model, twin = build("dense"), build("dense")
    o, opt = adam(sched()), adam(0.5)
    model.compile(o)
    twin.compile(opt)
    data = batches(8)
    twin_steps(model, twin, opt, data[:4])
    o.learning_rate = opt.lr = 2.5e-3
    for d in data[4:]:
        got, want = model.train_step(d).as_floats(), twin.train_step(d).as_floats()
        assert got == want and "lr" not in got and same_state(model, twin)
    assert float(model.lr_dev.item()) == float(np.float32(2.5e-3)) and model.lr_schedule is None
