"""Weight averaging through the models on the GPU: nic.NIC and lc_nic.NIC at tiny sizes (B = 5, N = 23, T = 6, V = 13,
U = 16), eager, as a recorded launch plan and as a hipGraph.

Six training steps cross warm-up, record / capture and replay: what is under test is the averaging launch's place behind
the update and the device-side counter it reads there.  After every step the slot must equal the float64 recursion of
tests/average_oracle.py fed with the device's own parameter snapshots, inside the sum of the per-launch bounds derived
there (a copy is bitwise), and the weights, the moments and the metrics must be the bits of the same run without averaging.
Decoding and evaluating inside ``averaged_weights()`` must give what a fresh model gives whose weights were set from the
``average`` slot -- with the decode replayed from a graph captured before the swap --, and training afterwards must not
notice the detour."""
import numpy as np
import pytest
import torch

import test_gpu_nic as TN
import test_gpu_lcnic as TL
from average_oracle import Recursion
from helpers import synth_batch

pytestmark = pytest.mark.gpu

DIMS_NIC = (5, 23, 6, 13, 16, 16)                        # B, N, T, V, U, E
DIMS_LC = (5, 23, 4, 16, 5, 16, 12, 13, 6)               # B, N, R, D, A, U, Et, V, T
B, N, T, V, U = 5, 23, 6, 13, 16
RUNNERS = {"eager": dict(use_graph=False), "plan": dict(use_graph=True), "graph": dict(use_graph=True, plan_step=False)}


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-2, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def wrappers():
    from masters_thesis_amd.optimizers import SWA, MovingAverage
    return {"ema": lambda: MovingAverage(adam(), 0.5, start_step=1, every=2), "swa": lambda: SWA(adam(), 1, 2)}


def build(kind, use_graph=True, plan_step=True, seed=9):
    rng = np.random.default_rng(seed)
    if kind == "dense":
        m, _ = TN.build(rng, (0.1, 0.2, 0.2), DIMS_NIC, use_graph=use_graph)
    else:
        m, _ = TL.build(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), DIMS_LC, use_graph=use_graph)
    m.plan_step = plan_step
    return m


def batches(n, seed=10):
    rng = np.random.default_rng(seed)
    return [synth_batch(B, N, T, V, U, rng) for _ in range(n)]


def decode(m, data):
    x, cap, a0, c0 = data
    out = m.greedy_predict(x, a0, c0, cap[:, 0], T)
    return [np.asarray(o) for o in (out if isinstance(out, tuple) else (out,))]


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("wrapper", ["ema", "swa"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_six_steps_follow_the_oracle_recursion(kind, wrapper, runner):
    opt = wrappers()[wrapper]()
    model, plain = build(kind, **RUNNERS[runner]), build(kind, **RUNNERS[runner])
    model.compile(opt)
    plain.compile(adam())
    av = opt.average
    rec = None
    for step, data in enumerate(batches(6), 1):
        got, want = model.train_step(data).as_floats(), plain.train_step(data).as_floats()
        assert got == want, (step, got, want)
        torch.cuda.synchronize()
        assert torch.equal(model.arena.theta, plain.arena.theta), step
        assert torch.equal(model.opt_m, plain.opt_m) and torch.equal(model.opt_v, plain.opt_v), step
        assert int(model.adam_t.item()) == step
        theta = model.arena.theta.cpu().numpy()
        if rec is None:
            rec = Recursion(np.zeros_like(theta), av.kind_id, av.momentum, av.dynamic, av.start_step, av.every)
        ref, tol = rec.step(theta)
        slot = model.opt_avg.cpu().numpy()
        if rec.modes[-1] == "copy":
            assert np.array_equal(slot.view(np.uint32), theta.view(np.uint32)), step
        else:
            err = np.abs(slot.astype(np.float64) - ref)
            assert (err <= tol).all(), (step, rec.modes[-1], float((err / np.maximum(tol, 1e-300)).max()))
    assert rec.modes == ["copy", "skip", "blend", "skip", "blend", "skip"]
    assert not torch.equal(model.opt_avg, model.arena.theta)
    assert plain.opt_avg is None
    if RUNNERS[runner]["use_graph"]:
        assert model._graphs and set(model._graphs) == set(plain._graphs), "the step was never recorded / captured"
    name = "time_distributed_softmax/kernel"
    e = model.arena.entries[name]
    assert np.array_equal(model.get_optimizer_slot(name, "average"),
                          model._unpack(name, model.opt_avg[e.off:e.off + e.size].view(e.shape)))


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_decode_and_evaluate_with_the_averaged_weights(kind):
    from masters_thesis_amd.optimizers import MovingAverage
    model = build(kind)
    model.compile(MovingAverage(adam(), 0.5, start_step=1, every=1))
    data = batches(5)
    for d in data[:4]:
        model.train_step(d)
    probe = data[4]
    raw = [decode(model, probe[0]) for _ in range(3)]                    # warm-up, capture, replay: with the raw weights
    raw_eval = [model.test_step(probe).as_floats() for _ in range(3)][-1]
    assert all(np.array_equal(a, b) for a, b in zip(raw[0], raw[2]))
    fresh = build(kind)                                                  # the same voxel groups; every weight is set below
    fresh.compile(adam())
    for name in model.keras_shapes:
        fresh.set_weight(name, model.get_optimizer_slot(name, "average") if name in model.arena.entries else model.get_weight(name))
    want, want_eval = decode(fresh, probe[0]), fresh.test_step(probe).as_floats()
    with model.averaged_weights():
        inside = decode(model, probe[0])                                 # the graph captured before the swap, replayed
        inside_eval = model.test_step(probe).as_floats()
    assert len(inside) == len(want) and all(np.array_equal(a, b) for a, b in zip(inside, want))
    assert inside_eval == want_eval
    # and the averaged weights are not the raw ones (the probabilities differ even where the argmax ids agree)
    assert any(not np.array_equal(a, b) for a, b in zip(inside, raw[2])) and inside_eval != raw_eval
    after = decode(model, probe[0])
    assert all(np.array_equal(a, b) for a, b in zip(after, raw[2])) and model.test_step(probe).as_floats() == raw_eval
    with pytest.raises(RuntimeError):
        with model.averaged_weights():
            model.train_step(probe)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_training_goes_on_as_without_the_detour(kind):
    from masters_thesis_amd.optimizers import MovingAverage
    a, b = build(kind), build(kind)
    for m in (a, b):
        m.compile(MovingAverage(adam(), 0.5, start_step=1, every=2))
    data = batches(6)
    for d in data[:3]:
        assert a.train_step(d).as_floats() == b.train_step(d).as_floats()
    with a.averaged_weights():
        decode(a, data[5][0])
        a.test_step(data[5])
    a.swap_weights()
    a.swap_weights()
    for step, d in enumerate(data[3:5]):
        assert a.train_step(d).as_floats() == b.train_step(d).as_floats(), step
    torch.cuda.synchronize()
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_avg, b.opt_avg)
    assert torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
