"""Label smoothing through the models on the GPU: one train_step and one test_step of nic.NIC and lc_nic.NIC at the tiny
golden sizes of tests/test_gpu_nic.py / tests/test_gpu_lcnic.py (their DIMS[0], their build()), dropout off, eps = 0.1,
against the float64 oracle with the smoothed loss substituted (smooth_oracle.smoothed); the per-subject losses of
lc_nic with S = 2; and a scheduled-sampling step whose dlogits are checked against the kernel reference on the step's
own logits.  The tolerances are the ones those two files apply to the unsmoothed step."""
import numpy as np
import pytest
import torch

from oracle import models as M
from oracle import ops as O
from helpers import synth_batch, tiny_groups
import test_gpu_nic as TN
import test_gpu_lcnic as TL
from test_gpu_head import near_clip
from test_gpu_smooth import grad_bound
from smooth_oracle import reference, smooth_cce_from_probs, smoothed

pytestmark = pytest.mark.gpu

EPS = 0.1
LAM_NIC = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}       # test_gpu_nic.py
LAM_LC = {"attention/W1/kernel": 0.001, "attention/W2/kernel": 0.001, "lstm/kernel": 3e-5,             # test_gpu_lcnic.py
          "time_distributed_nonlinear/kernel": 1e-5, "time_distributed_softmax/kernel": 1e-5}


def loss_obj(eps=EPS):
    from masters_thesis_amd.optimizers import CategoricalCrossentropy
    return CategoricalCrossentropy(from_logits=False, reduction="none", label_smoothing=eps)


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def sharpen(model, orc, scale=8.0):
    """at initialisation p is near uniform, where smoothing changes almost nothing: scale the vocabulary kernel"""
    k = "time_distributed_softmax/kernel"
    orc.p[k] = orc.p[k] * scale
    model.set_weight(k, orc.p[k])


def differs(orc, data, tgt):
    """the comparison below can tell the smoothed step from the plain one: the head-bias gradients of the two oracle
    steps differ by far more than the gradient tolerance.  (The LOSS barely moves at random targets: -log p_y and the
    class mean of -log p_v have the same expectation.)"""
    k = "time_distributed_softmax/bias"
    out, cache = orc.forward(data, True, M.DropCtx(seed=11, step=0, training=True))
    probs = out[0] if isinstance(out, tuple) else out          # the attention model returns (probs, attention)
    plain, _ = orc.backward(probs, cache, tgt)
    with smoothed(EPS):
        smooth, _ = orc.backward(probs, cache, tgt)
    assert np.abs(plain[k] - smooth[k]).max() > 100 * 2e-4 * np.abs(smooth[k]).max()


def test_dense_train_and_test_step_match_the_smoothed_oracle():
    rng = np.random.default_rng(31)
    dims = TN.DIMS[0]
    B, N, T, V, U, E = dims
    model, orc = TN.build(rng, (0, 0, 0), dims, use_graph=False)
    sharpen(model, orc)
    model.compile(adam(), loss_obj())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    differs(orc, data, tgt)
    with smoothed(EPS):
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    got = model.train_step((data, tgt)).as_floats()
    # test_gpu_nic.test_train_parity: loss 1e-4 relative, accuracy 1e-6; test_forward_gradients_greedy: gradients 1e-4 of
    # the largest + 1e-9; test_train_parity: weights 2e-2 * lr + 1e-4 of the largest (+ 1e-3 where the gradient is noise)
    assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]), (got, res)
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    for k in orc.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM_NIC.get(k, 0.0) * w0[k]
        assert np.abs(g - grads[k]).max() <= 1e-4 * np.abs(grads[k]).max() + 1e-9, k
    for k, v in orc.p.items():
        tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()
        if k in grads and grads[k] is not None:
            tol = tol + 1e-3 * (np.abs(grads[k]) < 1e-8)
        assert (np.abs(model.get_weight(k) - v) <= tol).all(), (k, np.abs(model.get_weight(k) - v).max())
    data, tgt = synth_batch(B, N, T, V, U, rng)
    with smoothed(EPS):
        want, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want["loss"]) <= 1e-4 * abs(want["loss"]), (got, want)


def test_attention_train_and_test_step_match_the_smoothed_oracle():
    rng = np.random.default_rng(51)
    dims = TL.DIMS[0]
    B, N, R, D, A, U, Et, V, T = dims
    model, orc = TL.build(rng, (0,) * 6, dims, use_graph=False)
    sharpen(model, orc)
    model.compile(adam(), loss_obj())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    differs(orc, data, tgt)
    with smoothed(EPS):
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    got = model.train_step((data, tgt)).as_floats()
    # test_gpu_lcnic.test_train_parity: metrics 1e-4 relative + 1e-7, weights 2e-2 * lr + 1e-4 of the largest (not
    # attention/V/bias); test_forward_gradients_greedy: gradients 2e-4 of the largest + 1e-9
    for k in ("loss", "L2", "attention"):
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    for k in orc.trainable():
        if k == "attention/V/bias":
            assert np.abs(model.get_gradient(k)).max() < 1e-5
            continue
        l = 0.01 if k.startswith("dense_in") and k.endswith("kernel") else LAM_LC.get(k, 0.0)
        g = model.get_gradient(k) + 2 * l * w0[k]
        assert np.abs(g - grads[k]).max() <= 2e-4 * np.abs(grads[k]).max() + 1e-9, (k, np.abs(g - grads[k]).max())
    for k, v in orc.p.items():
        if k == "attention/V/bias":
            continue
        assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), k
    data, tgt = synth_batch(B, N, T, V, U, rng)
    with smoothed(EPS):
        want, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want["loss"]) <= 1e-4 * abs(want["loss"]) + 1e-7, (got, want)


def test_per_subject_losses_are_the_smoothed_ones():
    from masters_thesis_amd.ms_nic import NIC
    from oracle.models_ms import MsLcNIC
    rng = np.random.default_rng(61)
    B, N, R, D, A, U, Et, V, T = TL.DIMS[0]
    S = 2
    g = (tiny_groups(N, R, rng), [D] * R)
    args = (g, U, 512, Et, A, V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    orc = MsLcNIC(*args, n_subjects=S).init_params(rng)
    model = NIC(*args, n_subjects=S, seed=11, use_graph=False)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    sharpen(model, orc)
    model.compile(adam(), loss_obj())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = synth_batch(S * B, N, T, V, U, rng)
    with smoothed(EPS):
        res, _, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    got = model.train_step((data, tgt)).as_floats()
    for k in ("loss", "lossA", "lossB"):
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert abs(res["lossA"] - res["lossB"]) > 1e-3 * res["loss"]          # two subjects, two different numbers


def test_scheduled_sampling_step_with_smoothing():
    """one scheduled-sampling step with eps = 0.1: the head launch is the smoothed one, and the dlogits it wrote are the
    kernel reference (tests/test_gpu_smooth.py's bound) of the logits the step itself produced"""
    import masters_thesis_amd.ops as ops
    from masters_thesis_amd.model_base import ScheduledSampling
    from masters_thesis_amd.nic import NIC
    rng = np.random.default_rng(71)
    B, N, T, V, U, E = 3, 37, 4, 11, 16, 8
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, seed=11, use_graph=False,
                scheduled_sampling=ScheduledSampling.linear(0.5, 0.0))
    orc = M.NICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    sharpen(model, orc, 4.0)
    model.compile(adam(), loss_obj())
    data, tgt = synth_batch(B, N, T, V, U, rng)
    be = ops.backend()
    seen = []
    real = be.softmax_cce_smooth

    def spy(logits, target, probs, loss_row, correct_row, dlogits, rows, Vv, ld, gscale, eps):
        x = logits.view(-1)[:rows * ld].clone()
        real(logits, target, probs, loss_row, correct_row, dlogits, rows, Vv, ld, gscale, eps)
        torch.cuda.synchronize()
        seen.append(dict(x=x.cpu().numpy().reshape(rows, ld)[:, :Vv], y=target.cpu().numpy()[:rows].astype(np.int64),
                         dl=dlogits.view(-1)[:rows * ld].cpu().numpy().reshape(rows, ld)[:, :Vv].copy(),
                         loss=loss_row.cpu().numpy()[:rows].copy(), gscale=gscale, eps=eps, rows=rows))
    be.softmax_cce_smooth = spy
    try:
        got = model.train_step((data, tgt)).as_floats()
    finally:
        del be.softmax_cce_smooth
    (c,) = seen
    assert c["rows"] == T * B and c["eps"] == EPS and c["gscale"] == 1.0 / (T * B)
    assert np.array_equal(c["y"].reshape(T, B).T, tgt)
    e32, g32 = float(np.float32(EPS)), float(np.float32(c["gscale"]))
    ref = reference(c["x"], c["y"], g32, e32)
    assert not near_clip(ref["p"]).any(), "the step's own probabilities sit on a clip bound: change the seed"
    assert (np.abs(c["dl"].astype(np.float64) - ref["grad"]) <= grad_bound(ref, g32)).all()
    want = smooth_cce_from_probs(ref["p"], c["y"], e32).mean()
    assert abs(got["loss"] - want) <= 1e-4 * abs(want)
    assert np.isfinite(list(got.values())).all()
