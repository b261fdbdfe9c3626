"""Global-norm gradient clipping through the models on the GPU: the tiny nic.NIC of test_gpu_weight_decay_models with the
encoder's fused update on (E = 512, where NIC._enc_update_fused holds: tnt_global_sqnorm_f32 in its fin form, then
tnt_dense_dw_adam_fin_gclip_f32 and tnt_adam_fin_gclip_f32 read the same word) and the tiny lc_nic.NIC
(tnt_adam_fin_gclip_f32), compiled with global_clipnorm.

Oracle parity: three train_steps against the float64 oracle step behind tf.clip_by_global_norm
(tests/global_clip_oracle.GlobalClip), with the loss and weight tolerances of test_gpu_nic.py / test_gpu_lcnic.py; every
step asserts from the oracle's norm that the threshold clips by a factor of 2 at least.  Replay: the same steps as a
recorded launch plan and as a hipGraph give the bits of the eager run.  Composition: AdamW under Warmup(CosineDecay).
global_grad_norm() is the oracle's norm.  A model compiled with clipnorm is untouched by the feature: the bits of a
twin whose descriptor had global_clipnorm set and taken back before the first step."""
import numpy as np
import pytest
import torch

import lr_schedule_oracle as LO
from global_clip_oracle import GlobalClip
from oracle import models as M
from test_gpu_weight_decay_models import RUNNERS, batches, build, check_weights, same, state_of
from weight_decay_oracle import AdamWState, decay_of

pytestmark = pytest.mark.gpu

C = 0.02
ADAM = dict(beta_1=0.9, beta_2=0.98, epsilon=1e-8)


def adam(lr=1e-3, **kw):
    from masters_thesis_amd.optimizers import Adam
    return Adam(lr, **ADAM, **kw)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_three_steps_match_the_oracle(kind):
    model, orc = build(kind)
    model.compile(adam(global_clipnorm=C))
    with pytest.raises(RuntimeError):
        model.global_grad_norm()
    state = GlobalClip(AdamWState(orc.p, {}, lr=1e-3, clipnorm=None), C)
    noisy, norms = {}, []
    for step, (data, tgt) in enumerate(batches(3)):
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        assert state.norm >= 2 * C, (step, state.norm)
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2") + (("attention",) if kind == "attention" else ()):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        check_weights(kind, model, orc, step, noisy, grads)
        norms.append(model.global_grad_norm())
        print(f"step {step}: global norm kernel {norms[-1]:.8g} oracle {state.norm:.8g}")
        assert abs(norms[-1] - state.norm) <= 1e-4 * state.norm, (step, norms[-1], state.norm)
    assert len(set(norms)) == 3
    if kind == "dense":
        assert model._enc_grad_stale is not None                       # the encoder's fused update ran
    model.check_device_errors()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_and_graph_replays_are_the_eager_bits(kind):
    models = {r: build(kind, **kw)[0] for r, kw in RUNNERS.items()}
    for m in models.values():
        m.compile(adam(global_clipnorm=C))
    for step, d in enumerate(batches(4)):                               # eager, record / capture, replay, replay
        mets = {r: m.train_step(d).as_floats() for r, m in models.items()}
        states = {r: state_of(m) + [m.gsq.clone()] for r, m in models.items()}
        for r in ("plan", "graph"):
            assert mets[r] == mets["eager"], (step, r, mets[r], mets["eager"])
            assert same(states[r], states["eager"]), (step, r)
    assert models["plan"]._graphs and models["graph"]._graphs, "the step was never recorded / captured"


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_a_clipnorm_model_is_untouched(kind, runner):
    a, b = build(kind, **RUNNERS[runner])[0], build(kind, **RUNNERS[runner])[0]
    a.compile(adam(clipnorm=0.1))
    opt = adam(global_clipnorm=C)
    b.compile(opt)
    opt.global_clipnorm = None                                          # taken back before the first step
    opt.clipnorm = 0.1
    for step, d in enumerate(batches(3)):
        assert a.train_step(d).as_floats() == b.train_step(d).as_floats(), step
        assert same(state_of(a), state_of(b)), step
    with pytest.raises(RuntimeError):
        b.global_grad_norm()
    # ... and a globally clipped twin is not: the comparison above can tell
    c = build(kind, **RUNNERS[runner])[0]
    c.compile(adam(global_clipnorm=C))
    for d in batches(3):
        c.train_step(d)
    assert not torch.equal(c.arena.theta, a.arena.theta)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_adamw_under_a_schedule_with_global_clipping(kind):
    """AdamW(learning_rate=Warmup(CosineDecay(1e-3, 4, alpha=0.1), 2), weight_decay=0.5, global_clipnorm=C): decay and
    global clipping compose in the one gclip launch; the oracle takes the step's ``lr`` metric for its Adam update and
    its decay"""
    from masters_thesis_amd.optimizers import AdamW
    from masters_thesis_amd.schedules import CosineDecay, Warmup
    params = LO.pack(LO.COSINE, [1e-3, 4, 0.1], w=2)
    model, orc = build(kind)
    opt = AdamW(Warmup(CosineDecay(1e-3, 4, alpha=0.1), 2), 0.5, **ADAM, global_clipnorm=C)
    opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)
    state = GlobalClip(AdamWState(orc.p, decay_of(orc.p, 0.5, substrings=["bias"]), lr=0.0, clipnorm=None), C)
    noisy = {}
    for step, (data, tgt) in enumerate(batches(4)):
        got = model.train_step((data, tgt)).as_floats()
        want = LO.lr32(params, step)
        assert abs(got["lr"] - float(want)) <= float(np.spacing(want)), (step, got["lr"], want)
        state.lr = got["lr"]
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        assert state.norm >= 2 * C
        assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]) + 1e-7, (step, got, res)
        assert abs(model.global_grad_norm() - state.norm) <= 1e-4 * state.norm
        check_weights(kind, model, orc, step, noisy, grads)
    assert model.seg_wd is not None
