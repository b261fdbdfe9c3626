"""Gradient accumulation (gradient_accumulation_steps=k) through the real HIP kernels: nic.NIC and lc_nic.NIC against the
accumulating float64 oracle step (tests/accum_oracle.py ``AccumStep``) over three windows, so that every phase's recording
runs eager, captured and replayed.  Tolerances: test_train_parity's of tests/test_gpu_nic.py (noisy-element term
included) and of tests/test_gpu_lcnic.py, unchanged, with the update index in the place of the step index."""
import numpy as np
import pytest
import torch

from oracle import models as M
from accum_oracle import AccumStep
from helpers import synth_batch
from test_gpu_lcnic import DIMS as LC_DIMS, build as build_lc
from test_gpu_nic import DIMS as NIC_DIMS, build as build_nic

pytestmark = pytest.mark.gpu

ADAM = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)
RATES = {"nic": {"none": (0, 0, 0), "dropout": (0.1, 0.2, 0.2)},
         "lcnic": {"none": (0,) * 6, "dropout": (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)}}


def _dims(kind, dims):
    """(B, N, T, V, U) of a dims tuple of either model"""
    if kind == "nic":
        B, N, T, V, U, E = dims
    else:
        B, N, R, D, A, U, Et, V, T = dims
    return B, N, T, V, U


def _check_weights(kind, model, orc, update, grads, noisy_el, what):
    for k, v in orc.p.items():
        if kind == "lcnic" and k == "attention/V/bias":        # zero-gradient variable: Adam amplifies rounding noise
            continue
        w = model.get_weight(k)
        tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()
        if kind == "nic" and k in grads and grads[k] is not None:
            noisy = noisy_el.setdefault(k, np.zeros(v.shape, bool))
            noisy |= np.abs(grads[k]) < 1e-8
            tol = tol + 1e-3 * (update + 1) * noisy
        assert (np.abs(w - v) <= tol).all(), (what, update, k, np.abs(w - v).max())


def _check_metrics(kind, got, res, what):
    keys = ("loss", "L2") + (("attention",) if kind == "lcnic" else ())
    for k in keys:
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + (1e-7 if kind == "lcnic" else 0.0), (what, k, got[k], res[k])
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6, what


def _run(kind, dims, rates, norm, k, windows=3, plain_too=False):
    from masters_thesis_amd.optimizers import Adam
    rng = np.random.default_rng(61)
    build = build_nic if kind == "nic" else build_lc
    B, N, T, V, U = _dims(kind, dims)
    model, orc = build(rng, rates, dims, norm)
    model.compile(Adam(**ADAM, gradient_accumulation_steps=k))
    step = AccumStep(orc, M.AdamState(orc.p, lr=1e-3, clipnorm=0.1), k, seed=11)
    if plain_too:       # the contract: one plain step of the oracle on the concatenated batch
        _, whole = build(np.random.default_rng(61), rates, dims, norm)
        whole_opt = M.AdamState(whole.p, lr=1e-3, clipnorm=0.1)
    noisy_el, noisy_whole = {}, {}
    for window in range(windows):       # every phase's recording: eager, capture, replay
        batches = [synth_batch(B, N, T, V, U, rng) for _ in range(k)]
        for j, (data, tgt) in enumerate(batches):
            res = step.micro_step(data, tgt)
            got = model.train_step((data, tgt)).as_floats()
            _check_metrics(kind, got, res, (window, j))
            assert model.accumulation_position == ((j + 1) % k, k)
        assert model.iterations == window + 1 and int(model.drop_step[0]) == (window + 1) * k
        _check_weights(kind, model, orc, window, step.last_grads, noisy_el, "accumulating oracle")
        # behind the closing micro-step get_gradient is what the update consumed (without the L2 term the oracle's carries)
        name = "lstm/recurrent_kernel"
        g = step.last_grads[name]
        assert np.abs(model.get_gradient(name) - g).max() <= 1e-4 * np.abs(g).max() + 1e-9
        if plain_too:
            data = tuple(np.concatenate([b[0][i] for b in batches]) for i in range(4))
            tgt = np.concatenate([b[1] for b in batches])
            _, grads, _ = whole.train_step(data, tgt, whole_opt, M.DropCtx(seed=11, step=window, training=True))
            _check_weights(kind, model, whole, window, grads, noisy_whole, "plain oracle step on the concatenated batch")
    torch.cuda.synchronize()
    if model.use_graph:
        recorded = {key[3]: type(v).__name__ for key, v in model._graphs.items() if key[0] == "train_acc"}
        assert recorded == {0: "CUDAGraph", 1: "CUDAGraph", 2: "CUDAGraph"} if k > 2 else recorded == {0: "CUDAGraph", 2: "CUDAGraph"}
    model.check_device_errors()
    return model


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_layer_norm_no_dropout_is_the_plain_step_on_the_concatenated_batch(kind):
    dims = (NIC_DIMS if kind == "nic" else LC_DIMS)[0]
    _run(kind, dims, RATES[kind]["none"], "layer", 3, plain_too=True)


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_batch_norm_and_dropout_are_per_micro_batch(kind):
    """pins the per-micro-batch BatchNorm statistics (moving statistics included: they are among the compared weights) and
    the per-micro-step mask stream"""
    dims = (NIC_DIMS if kind == "nic" else LC_DIMS)[0]
    _run(kind, dims, RATES[kind]["dropout"], "batch", 3)


def test_dense_model_at_real_widths():
    _run("nic", NIC_DIMS[1], RATES["nic"]["dropout"], "batch", 2)


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_with_the_persistent_chains(kind):
    """512 LSTM units, where the persistent chains run and the launch takes their error word as its guard: two windows of
    k = 2 at the sizes of smoke()'s 512-unit check, against the accumulating oracle within that check's bound (the same
    kernels at the same sizes: 2e-5 + 2e-4 max|w| on the weights, 1e-4 relative on the loss)"""
    from masters_thesis_amd.optimizers import Adam
    dims = (16, 3000, 6, 301, 512, 64) if kind == "nic" else (16, 3000, 40, 32, 32, 512, 64, 301, 6)
    B, N, T, V, U = _dims(kind, dims)
    rng = np.random.default_rng(63)
    model, orc = (build_nic if kind == "nic" else build_lc)(rng, RATES[kind]["dropout"], dims)
    model.compile(Adam(**ADAM, gradient_accumulation_steps=2))
    step = AccumStep(orc, M.AdamState(orc.p, lr=1e-3, clipnorm=0.1), 2, seed=11)
    for window in range(2):
        for j in range(2):
            data, tgt = synth_batch(B, N, T, V, U, rng)
            res = step.micro_step(data, tgt)
            got = model.train_step((data, tgt)).as_floats()
            assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]), (window, j, got, res)
        assert model.iterations == window + 1
        for k, v in orc.p.items():
            if kind == "lcnic" and k == "attention/V/bias":
                continue
            assert np.abs(model.get_weight(k) - v).max() <= 2e-5 + 2e-4 * np.abs(v).max(), (window, k)
    model.check_device_errors()
    if model.__dict__.get("_seq_lstm"):         # (off where the device census refuses the chains)
        assert model._guard_word() is not None


@pytest.mark.parametrize("kind", ["nic", "lcnic"])
def test_with_k_unset_every_bit_is_as_without_the_argument(kind):
    from masters_thesis_amd.optimizers import Adam
    dims = (NIC_DIMS if kind == "nic" else LC_DIMS)[1]
    build = build_nic if kind == "nic" else build_lc
    B, N, T, V, U = _dims(kind, dims)
    models = []
    for kw in ({}, dict(gradient_accumulation_steps=None)):
        model, _ = build(np.random.default_rng(62), RATES[kind]["dropout"], dims)
        model.compile(Adam(**ADAM, **kw))
        models.append(model)
    rng = np.random.default_rng(6)
    for _ in range(3):
        data, tgt = synth_batch(B, N, T, V, U, rng)
        a, b = (m.train_step((data, tgt)).as_floats() for m in models)
        assert a == b
    torch.cuda.synchronize()
    a, b = models
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    assert sorted(map(str, a._graphs)) == sorted(map(str, b._graphs)) and b.acc_grad is None
