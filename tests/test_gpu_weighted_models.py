"""Token weights, the focal factor and the weight-sum normalisation through the models on the GPU: one train_step and one
test_step of nic.NIC and lc_nic.NIC at the tiny golden sizes of tests/test_gpu_nic.py / tests/test_gpu_lcnic.py (their
DIMS[0], their build()), dropout off, inverse-sqrt weights from data.token_class_weights with pad_weight 0, gamma 2 and
normalise="weights", against the float64 oracle with the weighted gradient substituted (weighted_oracle.weighted) and the
loss / accuracy of weighted_oracle.weighted_metrics on the oracle's own probabilities; the per-subject metrics of lc_nic
with S = 2 under "count"; a scheduled-sampling step whose dlogits are checked against the kernel reference on the step's
own logits; a recorded launch plan and a captured hipGraph against the eager step, with set_class_weight between two
replays.  The tolerances are the ones tests/test_gpu_nic.py and tests/test_gpu_lcnic.py apply to the plain step."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch, tiny_groups
import test_gpu_nic as TN
import test_gpu_lcnic as TL
from test_gpu_head import near_clip
from test_gpu_weighted import check_outputs
from weighted_oracle import reference, weighted, weighted_metrics, wt_loss

pytestmark = pytest.mark.gpu

GAMMA = 2.0
LAM_NIC = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}       # test_gpu_nic.py
LAM_LC = {"attention/W1/kernel": 0.001, "attention/W2/kernel": 0.001, "lstm/kernel": 3e-5,             # test_gpu_lcnic.py
          "time_distributed_nonlinear/kernel": 1e-5, "time_distributed_softmax/kernel": 1e-5}
DIMS_REPLAY_NIC = (6, 200, 6, 101, 32, 32)               # B, N, T, V, U, E: test_gpu_unlikelihood_models.py's capture sizes
DIMS_REPLAY_LC = (6, 200, 8, 16, 16, 32, 32, 101, 6)     # B, N, R, D, A, U, Et, V, T


def loss_obj(cw, gamma=GAMMA, normalise="weights"):
    from masters_thesis_amd.optimizers import CategoricalCrossentropy
    return CategoricalCrossentropy(from_logits=False, reduction="none", class_weight=cw, focal_gamma=gamma, normalise=normalise)


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def sharpen(model, orc, scale=8.0):
    """at initialisation p is near uniform, where the focal factor is the same in every row: scale the vocabulary kernel"""
    k = "time_distributed_softmax/kernel"
    orc.p[k] = orc.p[k] * scale
    model.set_weight(k, orc.p[k])


def padded_batch(B, N, T, V, U, rng):
    """synth_batch with captions of 1 .. T - 2 words over the ids 1 .. V - 1, the rest padding"""
    (x, cap, a0, c0), _ = synth_batch(B, N, T, V, U, rng)
    for b in range(B):
        n = int(rng.integers(1, T - 1))
        cap[b, 1:1 + n] = rng.integers(1, V, n)
        cap[b, 1 + n:] = 0
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    assert (tgt == 0).sum() >= B and (tgt != 0).sum() >= B
    return (x, cap, a0, c0), tgt


def corpus_weights(V, rng, T=6):
    """inverse-sqrt weights of a skewed synthetic corpus: a few frequent words, pad_weight 0"""
    from masters_thesis_amd.data import token_class_weights
    caps = np.minimum(rng.geometric(0.15, (64, T)), V - 1)
    caps[:, T - 2:] = 0
    w = token_class_weights(caps, V, scheme="inverse_sqrt", pad_weight=0.0)
    assert w[0] == 0 and w[1:].min() > 0 and w[1:].max() > 1.5 * w[1:].min()
    return w


def oracle_step(orc, opt, data, tgt, cw, gamma, norm):
    """(metrics of the weighted loss, gradients) of the patched float64 training step"""
    out, cache = orc.forward(data, True, M.DropCtx(seed=11, step=0, training=True))
    probs = out[0] if isinstance(out, tuple) else out          # the attention model returns (probs, attention)
    loss, acc = weighted_metrics(probs, tgt, cw, gamma, norm)
    plain = orc.backward(probs, cache, tgt)[0]
    with weighted(cw, gamma, norm):
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=0, training=True))
    # the comparison can tell the step from the plain one: the loss and the head-bias gradient move far past the
    # tolerances below
    k = "time_distributed_softmax/bias"
    assert abs(loss - res["loss"]) > 100 * 1e-4 * res["loss"]
    assert np.abs(plain[k] - grads[k]).max() > 100 * 2e-4 * np.abs(grads[k]).max()
    res = dict(res)
    res["loss"], res["accuracy"] = loss, acc
    return res, grads


def oracle_test_metrics(orc, data, tgt, cw, gamma, norm):
    out = orc.test_step(data, tgt)[1]
    return weighted_metrics(out[0] if isinstance(out, tuple) else out, tgt, cw, gamma, norm)


def test_dense_train_and_test_step_match_the_weighted_oracle():
    rng = np.random.default_rng(31)
    dims = TN.DIMS[0]
    B, N, T, V, U, E = dims
    model, orc = TN.build(rng, (0, 0, 0), dims, use_graph=False)
    sharpen(model, orc)
    w = corpus_weights(V, rng)
    model.compile(adam(), loss_obj(w))
    cw = w.astype(np.float64)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = padded_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    res, grads = oracle_step(orc, opt, data, tgt, cw, GAMMA, True)
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
    data, tgt = padded_batch(B, N, T, V, U, rng)
    want_loss, want_acc = oracle_test_metrics(orc, data, tgt, cw, GAMMA, True)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want_loss) <= 1e-4 * abs(want_loss), (got, want_loss)
    assert abs(got["accuracy"] - want_acc) < 1e-6


def test_attention_train_and_test_step_match_the_weighted_oracle():
    rng = np.random.default_rng(51)
    dims = TL.DIMS[0]
    B, N, R, D, A, U, Et, V, T = dims
    model, orc = TL.build(rng, (0,) * 6, dims, use_graph=False)
    sharpen(model, orc)
    w = corpus_weights(V, rng)
    model.compile(adam(), loss_obj(w))
    cw = w.astype(np.float64)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    data, tgt = padded_batch(B, N, T, V, U, rng)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    res, grads = oracle_step(orc, opt, data, tgt, cw, GAMMA, True)
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
    data, tgt = padded_batch(B, N, T, V, U, rng)
    want_loss, want_acc = oracle_test_metrics(orc, data, tgt, cw, GAMMA, True)
    got = model.test_step((data, tgt)).as_floats()
    assert abs(got["loss"] - want_loss) <= 1e-4 * abs(want_loss) + 1e-7, (got, want_loss)
    assert abs(got["accuracy"] - want_acc) < 1e-6


def test_per_subject_metrics_under_count():
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
    w = corpus_weights(V, rng)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        model.compile(adam(), loss_obj(w, normalise="weights"))
    model.compile(adam(), loss_obj(w, normalise="count"))
    cw = w.astype(np.float64)
    data, tgt = padded_batch(S * B, N, T, V, U, rng)
    (probs, _), _ = orc.forward(data, True, M.DropCtx(seed=11, step=0, training=True))
    got = model.train_step((data, tgt)).as_floats()
    want = {"loss": weighted_metrics(probs, tgt, cw, GAMMA, False)}
    for q in range(S):
        want["AB"[q]] = weighted_metrics(probs[q * B:(q + 1) * B], tgt[q * B:(q + 1) * B], cw, GAMMA, False)
    assert abs(got["loss"] - want["loss"][0]) <= 1e-4 * want["loss"][0] + 1e-7        # the model reports accuracy per subject
    for tag in "AB":
        assert abs(got["loss" + tag] - want[tag][0]) <= 1e-4 * want[tag][0] + 1e-7, (tag, got, want)
        assert abs(got["accuracy" + tag] - want[tag][1]) < 1e-6, (tag, got, want)
    assert abs(want["A"][0] - want["B"][0]) > 1e-3 * want["loss"][0]          # two subjects, two different numbers


def test_scheduled_sampling_step_with_token_weights():
    """one scheduled-sampling step: the head launch is the weighted one, and the loss_row / dlogits it wrote are the kernel
    reference (tests/test_gpu_weighted.py's bounds) of the logits the step itself produced"""
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
    w = corpus_weights(V, rng)
    model.compile(adam(), loss_obj(w))
    data, tgt = padded_batch(B, N, T, V, U, rng)
    be = ops.backend()
    seen, names = [], []
    real, plain = be.softmax_cce_weighted, be.softmax_cce

    def spy(logits, target, cw, probs, loss_row, correct_row, dlogits, rows, Vv, ld, gscale, gamma, normalise):
        x = logits.view(-1)[:rows * ld].clone()
        real(logits, target, cw, probs, loss_row, correct_row, dlogits, rows, Vv, ld, gscale, gamma, normalise)
        torch.cuda.synchronize()
        seen.append(dict(x=x.cpu().numpy().reshape(rows, ld)[:, :Vv], y=target.cpu().numpy()[:rows].astype(np.int64),
                         dl=dlogits.view(-1)[:rows * ld].cpu().numpy().reshape(rows, ld), cw=cw.cpu().numpy().copy(),
                         loss=loss_row.cpu().numpy()[:rows].copy(), corr=correct_row.cpu().numpy()[:rows].copy(),
                         gscale=gscale, gamma=gamma, normalise=normalise, rows=rows))

    def no_plain(*a, **k):
        names.append("softmax_cce")
        return plain(*a, **k)
    be.softmax_cce_weighted, be.softmax_cce = spy, no_plain
    try:
        got = model.train_step((data, tgt)).as_floats()
    finally:
        del be.softmax_cce_weighted, be.softmax_cce
    (c,) = seen
    assert names == []
    assert c["rows"] == T * B and c["gamma"] == GAMMA and c["normalise"] and c["gscale"] == 1.0 / (T * B)
    assert np.array_equal(c["cw"], w) and np.array_equal(c["y"].reshape(T, B).T, tgt)
    g32 = float(np.float32(c["gscale"]))
    ref = reference(c["x"], c["y"], w, g32, GAMMA, True)
    assert not near_clip(ref["py"]).any(), "the step's own probabilities sit on a clip bound: change the seed"
    check_outputs(dict(loss=c["loss"], corr=c["corr"], dl=c["dl"], gscale=g32), ref, GAMMA, True, True, "scheduled sampling")
    want = wt_loss(ref["p"], c["y"], w.astype(np.float64), GAMMA, True).mean()
    assert abs(got["loss"] - want) <= 1e-4 * abs(want)
    assert np.isfinite(list(got.values())).all()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_replay_graph_replay_and_eager_step_are_bit_identical(kind):
    """eager / a recorded launch plan / a captured hipGraph over eager -> record or capture -> replay -> replay, then
    set_class_weight on all three and two more replays: the same launches, the same bits, nothing recorded again; a
    fourth, eager model that keeps the first weights shows that the new ones change the step"""
    models = []
    for use_graph, plan in ((False, True), (True, True), (True, False), (False, True)):
        rng = np.random.default_rng(9)
        if kind == "dense":
            m, orc = TN.build(rng, (0, 0, 0), DIMS_REPLAY_NIC, use_graph=use_graph)
            B, N, T, V, U, E = DIMS_REPLAY_NIC
        else:
            m, orc = TL.build(rng, (0,) * 6, DIMS_REPLAY_LC, use_graph=use_graph)
            B, N, R, D, A, U, Et, V, T = DIMS_REPLAY_LC
        sharpen(m, orc)
        m.plan_step = plan
        models.append(m)
    wrng = np.random.default_rng(10)
    w1, w2 = corpus_weights(V, wrng), corpus_weights(V, wrng)[::-1].copy()
    w2[0], w2[V - 1] = 0.0, w1[1]
    for m in models:
        m.compile(adam(), loss_obj(w1))
    eager, planned, graphed, kept = models
    rng = np.random.default_rng(11)
    keys = None
    for step in range(6):
        if step == 4:
            keys = [set(m._graphs) for m in (planned, graphed)]
            bufs = [m.cw_dev.data_ptr() for m in models]
            for m in (eager, planned, graphed):
                m.set_class_weight(w2)
            assert [m.cw_dev.data_ptr() for m in models] == bufs
        data, tgt = padded_batch(B, N, T, V, U, rng)
        ra, rb, rc, rd = (m.train_step((data, tgt)).as_floats() for m in models)
        assert ra == rb == rc, (step, ra, rb, rc)
        assert (ra == rd) == (step < 4), (step, ra, rd)
    torch.cuda.synchronize()
    assert [set(m._graphs) for m in (planned, graphed)] == keys, "set_class_weight recorded / captured the step again"
    assert any(isinstance(v, tuple) for v in planned._graphs.values()), "the second model did not replay a launch plan"
    assert any(isinstance(v, torch.cuda.CUDAGraph) for v in graphed._graphs.values()), "the third model did not replay a graph"
    assert not any(isinstance(v, tuple) for v in graphed._graphs.values())
    for m in (planned, graphed):
        assert torch.equal(eager.arena.theta, m.arena.theta) and torch.equal(eager.opt_m, m.opt_m)
        assert torch.equal(eager.opt_v, m.opt_v)
    assert not torch.equal(eager.arena.theta, kept.arena.theta)
