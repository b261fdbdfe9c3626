"""Decoupled weight decay through the models on the GPU: a small nic.NIC with the encoder's fused update on (E = 512:
tnt_dense_dw_adamw_fin_f32 + tnt_adamw_fin_f32) and a small lc_nic.NIC (tnt_adamw_fin_f32), compiled with
AdamW(weight_decay=0.05) and the biases excluded.

Oracle parity: three train_steps against the float64 oracle step followed by the restated update
(tests/weight_decay_oracle.AdamWState), with the loss and weight tolerances of test_gpu_nic.py / test_gpu_lcnic.py.
Replay: the same steps as a recorded launch plan and as a hipGraph give the bits of the eager run.  No decay:
Adam(weight_decay=0) gives the bits of Adam().  Composition: under MovingAverage the update is the unwrapped one's, and
under Warmup(CosineDecay) the decay uses the scheduled rate -- there the decay is 0.5, which moves a weight by 1.2e-3
relative over the four steps, twelve times the 1e-4 tolerance."""
import numpy as np
import pytest
import torch

import lr_schedule_oracle as LO
import test_gpu_lcnic as TL
import test_gpu_nic as TN
from helpers import synth_batch
from oracle import models as M
from weight_decay_oracle import AdamWState, decay_of

pytestmark = pytest.mark.gpu

DIMS_NIC = (5, 23, 6, 13, 16, 512)                       # B, N, T, V, U, E: E = 512 switches the encoder's fused update on
DIMS_LC = (5, 23, 4, 16, 5, 16, 12, 13, 6)               # B, N, R, D, A, U, Et, V, T
B, N, T, V, U = 5, 23, 6, 13, 16
RUNNERS = {"eager": dict(use_graph=False), "plan": dict(use_graph=True), "graph": dict(use_graph=True, plan_step=False)}
ADAM = dict(beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def build(kind, use_graph=True, plan_step=True, seed=9):
    rng = np.random.default_rng(seed)
    if kind == "dense":
        m, orc = TN.build(rng, (0.1, 0.2, 0.2), DIMS_NIC, use_graph=use_graph)
    else:
        m, orc = TL.build(rng, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2), DIMS_LC, use_graph=use_graph)
    m.plan_step = plan_step
    return m, orc


def adamw(lr=1e-3, wd=0.05):
    from masters_thesis_amd.optimizers import AdamW
    opt = AdamW(lr, wd, **ADAM)
    opt.exclude_from_weight_decay(var_names=["bias"])
    return opt


def batches(n, seed=10):
    rng = np.random.default_rng(seed)
    return [synth_batch(B, N, T, V, U, rng) for _ in range(n)]


def state_of(m):
    torch.cuda.synchronize()
    return [m.arena.theta.clone(), m.opt_m.clone(), m.opt_v.clone(), m.adam_t.clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_weights(kind, model, orc, step, noisy_el=None, grads=None):
    for k, v in orc.p.items():
        if kind == "attention" and k == "attention/V/bias":           # zero-gradient variable (test_gpu_lcnic)
            continue
        w = model.get_weight(k)
        tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()
        if kind == "dense" and grads is not None and grads.get(k) is not None:      # test_gpu_nic's zero-gradient elements
            noisy = noisy_el.setdefault(k, np.zeros(v.shape, bool))
            noisy |= np.abs(grads[k]) < 1e-8
            tol = tol + 1e-3 * (step + 1) * noisy
        assert (np.abs(w - v) <= tol).all(), (step, k, np.abs(w - v).max())


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_three_steps_match_the_oracle(kind):
    model, orc = build(kind)
    model.compile(adamw())
    state = AdamWState(orc.p, decay_of(orc.p, 0.05, substrings=["bias"]), lr=1e-3, clipnorm=0.1)
    noisy = {}
    for step, (data, tgt) in enumerate(batches(3)):
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2") + (("attention",) if kind == "attention" else ()):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        check_weights(kind, model, orc, step, noisy, grads)
    tab = model.seg_wd.cpu().numpy()
    for n, e in model.arena.entries.items():
        assert tab[e.seg] == (0.0 if "bias" in n else np.float32(0.05)), n
    if kind == "dense":
        assert model._enc_grad_stale is not None                       # the encoder's fused update ran
    model.check_device_errors()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_and_graph_replays_are_the_eager_bits(kind):
    models = {r: build(kind, **kw)[0] for r, kw in RUNNERS.items()}
    for m in models.values():
        m.compile(adamw())
    for step, d in enumerate(batches(4)):                               # eager, record / capture, replay, replay
        mets = {r: m.train_step(d).as_floats() for r, m in models.items()}
        states = {r: state_of(m) for r, m in models.items()}
        for r in ("plan", "graph"):
            assert mets[r] == mets["eager"], (step, r, mets[r], mets["eager"])
            assert same(states[r], states["eager"]), (step, r)
    assert models["plan"]._graphs and models["graph"]._graphs, "the step was never recorded / captured"


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_zero_decay_is_plain_adam(kind, runner):
    from masters_thesis_amd.optimizers import Adam
    a, b = build(kind, **RUNNERS[runner])[0], build(kind, **RUNNERS[runner])[0]
    a.compile(Adam(1e-3, weight_decay=0, **ADAM))
    b.compile(Adam(1e-3, **ADAM))
    for step, d in enumerate(batches(3)):
        assert a.train_step(d).as_floats() == b.train_step(d).as_floats(), step
        assert same(state_of(a), state_of(b)), step
    assert a.seg_wd is None
    # ... and a decaying twin is not: the comparison above can tell
    c = build(kind, **RUNNERS[runner])[0]
    c.compile(adamw())
    for d in batches(3):
        c.train_step(d)
    assert not torch.equal(c.arena.theta, b.arena.theta)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_under_a_weight_average_the_update_is_the_unwrapped_one(kind):
    from masters_thesis_amd.optimizers import MovingAverage
    model, plain = build(kind)[0], build(kind)[0]
    model.compile(MovingAverage(adamw(), 0.5, start_step=1))
    plain.compile(adamw())
    assert model.optimizer.weight_decay == 0.05
    for step, d in enumerate(batches(3)):
        assert model.train_step(d).as_floats() == plain.train_step(d).as_floats(), step
        assert same(state_of(model), state_of(plain)), step
    torch.cuda.synchronize()
    assert not torch.equal(model.opt_avg, model.arena.theta) and float(model.opt_avg.abs().max()) > 0


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_the_decay_uses_the_scheduled_rate(kind, runner):
    """AdamW(learning_rate=Warmup(CosineDecay(1e-3, 4, alpha=0.1), 2), weight_decay=0.5): the oracle takes the step's ``lr``
    metric for both its Adam update and its decay, lr * wd; the rates stay at or below 1e-3, so test_gpu_nic's weight
    tolerance (2 % of an Adam step at 1e-3) applies as it stands"""
    from masters_thesis_amd.schedules import CosineDecay, Warmup
    params = LO.pack(LO.COSINE, [1e-3, 4, 0.1], w=2)
    model, orc = build(kind, **RUNNERS[runner])
    model.compile(adamw(Warmup(CosineDecay(1e-3, 4, alpha=0.1), 2), 0.5))
    state = AdamWState(orc.p, decay_of(orc.p, 0.5, substrings=["bias"]), lr=0.0, clipnorm=0.1)
    noisy, lrs = {}, []
    for step, (data, tgt) in enumerate(batches(4)):
        got = model.train_step((data, tgt)).as_floats()
        want = LO.lr32(params, step)
        assert abs(got["lr"] - float(want)) <= float(np.spacing(want)), (step, got["lr"], want)
        state.lr = got["lr"]
        lrs.append(got["lr"])
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]) + 1e-7, (step, got, res)
        check_weights(kind, model, orc, step, noisy, grads)
    assert lrs[0] == 0.0 and max(lrs) <= float(np.float32(1e-3)) and len(set(lrs)) == 4      # the float32 nearest 1e-3
