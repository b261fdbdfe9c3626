"""Layer freezing and learning-rate multipliers through the models on the GPU: the tiny nic.NIC and lc_nic.NIC of
test_gpu_weight_decay_models (tnt_span_sqnorm_lrmul_f32 with the lr job, tnt_adam_fin_lrmul_f32; under global_clipnorm
tnt_global_sqnorm_lrmul_f32 in its fin form) with the decoder frozen, the encoder kernel frozen and a mixed table.

Oracle parity: three train_steps against the float64 oracle (tests/finetune_oracle.FinetuneState), with the loss and
weight tolerances of test_gpu_global_clip_models for the same comparison; a frozen variable and its moments are compared
bit for bit.  Replay: the same steps as a recorded launch plan and as a hipGraph give the bits of the eager run, across an
in-place table rewrite.  Gradual unfreezing and the transfer journey of test_host_finetune run on the device."""
import numpy as np
import pytest
import torch

from finetune_oracle import FinetuneState
from oracle import models as M
from test_gpu_weight_decay_models import DIMS_NIC, RUNNERS, batches, build, check_weights, same, state_of

pytestmark = pytest.mark.gpu

ADAM = dict(beta_1=0.9, beta_2=0.98, epsilon=1e-8)
C = 0.02
DECODER = ("emb_text", "lstm", "time_distributed_softmax")
TABLES = {
    "decoder": lambda names: {n: 0.0 for n in names if n.split("/")[0] in DECODER},
    "encoder": lambda names: {n: 0.0 for n in names if n.startswith(("dense_img/", "dense_in/")) and n.endswith("/kernel")},
    "mixed": lambda names: {"lstm/recurrent_kernel": 0.0, "time_distributed_softmax/bias": 0.0, "lstm/kernel": 0.1,
                            "emb_text/embeddings": 10.0, "time_distributed_softmax/kernel": 0.5},
}


def adam(lr=1e-3, **kw):
    from masters_thesis_amd.optimizers import Adam
    return Adam(lr, **ADAM, **kw)


def table_for(model, which):
    tab = TABLES[which](list(model.arena.entries))
    if which == "mixed" and "dense_img/kernel" in model.arena.entries:
        tab["dense_img/kernel"] = 2.0       # the encoder's fused update at a scalar multiplier (tnt_dense_dw_adam_fin_lrmul_f32)
    assert tab and set(tab) <= set(model.arena.entries), tab
    return tab


def frozen_state(model, names):
    """(weight, m, v) per variable; the moments are zeros until the first step has built the optimizer state"""
    slot = lambda n, k: np.zeros(model.keras_shapes[n], np.float32) if model.opt_m is None else model.get_optimizer_slot(n, k)
    return {n: (model.get_weight(n), slot(n, "m"), slot(n, "v")) for n in names}


def assert_held(model, held):
    for n, want in held.items():
        for got, w in zip(frozen_state(model, [n])[n], want):
            assert np.array_equal(got, w), n


@pytest.mark.parametrize("clip", ["clipnorm", "global"])
@pytest.mark.parametrize("which", sorted(TABLES))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_three_steps_match_the_oracle(kind, which, clip):
    model, orc = build(kind)
    gc = clip == "global"
    model.compile(adam(**(dict(global_clipnorm=C) if gc else dict(clipnorm=0.1))))
    tab = table_for(model, which)
    model.set_lr_multipliers(tab)
    state = FinetuneState(orc.p, lr=1e-3, mul=tab, **(dict(global_clipnorm=C) if gc else dict(clipnorm=0.1)))
    frozen = [n for n, m in tab.items() if m == 0.0]
    held = frozen_state(model, frozen)
    noisy = {}
    for step, (data, tgt) in enumerate(batches(3)):
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2") + (("attention",) if kind == "attention" else ()):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        check_weights(kind, model, orc, step, noisy, {k: (None if k in frozen else g) for k, g in grads.items()})
        if gc:
            assert abs(model.global_grad_norm() - state.norm) <= 1e-4 * state.norm, (step, model.global_grad_norm(), state.norm)
    assert_held(model, held)
    assert model.seg_lrm is not None and model.iterations == 3
    if kind == "dense" and which != "encoder":
        assert model._enc_grad_stale is not None                       # the encoder's fused update ran under the table
    for n in frozen:
        with pytest.raises(ValueError, match="frozen"):
            model.get_gradient(n)
    model.check_device_errors()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_and_graph_replays_are_the_eager_bits_across_a_table_rewrite(kind):
    models = {r: build(kind, **kw)[0] for r, kw in RUNNERS.items()}
    for m in models.values():
        m.compile(adam(clipnorm=0.1))
        m.set_lr_multipliers(table_for(m, "mixed"))
    for step, d in enumerate(batches(6)):                               # eager, record / capture, replay ...
        if step == 4:                                                   # ... a rewrite in place, and two more replays
            for m in models.values():
                m.set_lr_multipliers({"lstm/kernel": 2.0, "emb_text/embeddings": 0.25})
        mets = {r: m.train_step(d).as_floats() for r, m in models.items()}
        states = {r: state_of(m) for r, m in models.items()}
        for r in ("plan", "graph"):
            assert mets[r] == mets["eager"], (step, r, mets[r], mets["eager"])
            assert same(states[r], states["eager"]), (step, r)
    assert models["plan"]._graphs and models["graph"]._graphs, "the step was never recorded / captured"


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_gradual_unfreezing_matches_the_oracle(kind):
    """freeze the decoder, two steps, unfreeze it at 0.1, two steps"""
    model, orc = build(kind)
    model.compile(adam(clipnorm=0.1))
    model.freeze(*DECODER)
    tab = table_for(model, "decoder")
    state = FinetuneState(orc.p, lr=1e-3, mul=tab, clipnorm=0.1)
    held = frozen_state(model, list(tab))
    noisy = {}
    for step, (data, tgt) in enumerate(batches(4)):
        if step == 2:
            assert_held(model, held)
            model.unfreeze(*DECODER, multiplier=0.1)
            state.mul = {n: 0.1 for n in tab}
        res, grads, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]) + 1e-7, (step, got, res)
        check_weights(kind, model, orc, step, noisy, {k: (None if step < 2 and k in tab else g) for k, g in grads.items()})
    assert model.iterations == 4 and not np.array_equal(model.get_weight("lstm/kernel"), held["lstm/kernel"][0])


def test_transfer_to_another_subject(tmp_path):
    """train A, save; B has another voxel count: load what fits, freeze the decoder, train the encoder"""
    from masters_thesis_amd.nic import NIC
    A, _ = build("dense")
    A.compile(adam(clipnorm=0.1))
    for d in batches(3):
        A.train_step(d)
    path = tmp_path / "subject_a.npz"
    A.save_weights(path)
    Bn, N, T, V, U, E = DIMS_NIC
    N2 = N + 9
    Bm = NIC(N2, U, E, V, T, 0.1, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cuda:0", seed=12)
    before = {n: Bm.get_weight(n) for n in Bm.keras_shapes}
    Bm.load_weights(path, by_name=True, skip_mismatch=True)
    assert np.array_equal(Bm.get_weight("dense_img/kernel"), before["dense_img/kernel"])
    Bm.compile(adam(clipnorm=0.1), freeze=list(DECODER))
    decoder = [n for n in Bm.arena.entries if n.split("/")[0] in DECODER]
    rng = np.random.default_rng(8)
    from helpers import synth_batch
    for _ in range(3):
        m = Bm.train_step(synth_batch(Bn, N2, T, V, U, rng)).as_floats()
        assert np.isfinite(m["loss"])
    for n in decoder:
        assert np.array_equal(Bm.get_weight(n), A.get_weight(n)), n
    for n in ("dense_img/kernel", "dense_img/bias", "batch_norm/gamma"):
        assert not np.array_equal(Bm.get_weight(n), before[n]), n
    assert torch.isfinite(Bm.arena.theta).all()
    Bm.check_device_errors()
