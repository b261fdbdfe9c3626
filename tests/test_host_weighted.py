"""Token weights, the focal factor and the weight-sum normalisation on the CPU through a mock backend that follows
tnt_softmax_cce_weighted_f32's header definition (tests/weighted_oracle.py): the float64 gradient against finite
differences of the float64 loss, a training and an evaluation step of both models against the oracle models with the
weighted loss, the launches with and without the feature, set_class_weight, the refusals, the config keys,
CategoricalFocalCrossentropy, fit(class_weight=) and data.token_class_weights."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd import think_and_tell as TT, show_and_tell as SAT
from masters_thesis_amd.data import token_class_weights
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical as SC
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import (Adam, CategoricalCrossentropy, CategoricalFocalCrossentropy, check_class_weight,
                                           check_focal_gamma, check_normalise, loss_class_weight, loss_focal_gamma,
                                           loss_normalise)
from oracle import models as M
from helpers import synth_batch, tiny_groups
from smooth_oracle import SmoothMockBackend
from ss_att_oracle import SSAttMockBackend
from test_host_naive_attention import NaiveMockBackend
from unlikelihood_oracle import UnlikelihoodMockBackend
from weighted_oracle import (LO, WeightedMockBackend, reference, terms, weighted, weighted_metrics, wt_correct, wt_grad,
                             wt_loss)

B, N, T, V, U, E = 5, 23, 6, 13, 16, 16
LC = dict(R=4, D=16, A=5, Et=12)
HEAD_SCALE = 8.0       # on the vocabulary kernel: at initialisation p is near uniform, where the focal factor is flat


class RecordingBackend(WeightedMockBackend, UnlikelihoodMockBackend, SmoothMockBackend, SSAttMockBackend, NaiveMockBackend):
    """the mock with every public call's name logged in ``names``"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if not name.startswith("_") and callable(v) and name not in ("names",):
            object.__getattribute__(self, "names").append(name)
        return v


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def loss_obj(**kw):
    return CategoricalCrossentropy(from_logits=False, reduction="none", **kw)


def dense(rng, **kw):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw)
    orc = M.NICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    orc.p["time_distributed_softmax/kernel"] *= HEAD_SCALE
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def attention(rng, cls=LcNIC, orc_cls=M.LcNIC, **kw):
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    args = (g, U, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    model = cls(*args, device="cpu", seed=11, **kw)
    orc = orc_cls(*args).init_params(rng) if orc_cls is not None else None
    if orc is not None:
        orc.p["time_distributed_softmax/kernel"] *= HEAD_SCALE
    for k, v in (orc.p.items() if orc is not None else ()):
        model.set_weight(k, v)
    return model, orc


def padded_batch(b, rng):
    """synth_batch with captions of 2 .. T - 1 words, the rest padding: about a third of the targets are id 0"""
    data, tgt = synth_batch(b, N, T, V, U, rng)
    x, cap, a0, c0 = data
    for i in range(b):
        n = int(rng.integers(2, T))
        cap[i, 1:1 + n] = rng.integers(1, V, n)
        cap[i, 1 + n:] = 0
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    assert (tgt == 0).sum() >= b and (tgt != 0).sum() >= 2 * b
    return (x, cap, a0, c0), tgt


def some_weights(rng, pad=0.0):
    w = rng.uniform(0.25, 2.0, V).astype(np.float32)
    w[0] = pad
    return w


def call_loss(c):
    p = M.O.softmax(c["logits"])
    return wt_loss(p, c["target"], c["cw"], c["gamma"], c["normalise"]).mean()


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
def test_gradient_against_central_differences(gamma, normalise):
    rng = np.random.default_rng(12)
    rows, Vv = 7, 13
    x = rng.standard_normal((rows, Vv)) * 2
    tg = rng.integers(1, Vv, rows)
    cw = rng.uniform(0.2, 3.0, Vv)
    cw[tg[2]] = 0.0                                          # a zero weight on a present target
    tg[4] = Vv + 3                                           # y outside [0, V): weight 1, p_y = 0, no gradient
    tg[5] = 0
    x[5, 0] = x[5].max() - 40.0                              # the target clipped low: constant loss, zero gradient row
    p = M.O.softmax(x)
    t = terms(p, tg, cw, gamma, normalise)
    assert t["w"][2] == 0 and t["w"][4] == 1 and t["my"][4] == 0 and t["my"][5] == 0 and t["py"][5] < LO
    keep = np.ones(rows, bool); keep[[4, 5]] = False
    assert (t["py"][keep] > 1e-5).all() and (t["py"][keep] < 1 - 1e-5).all()     # out of the clip bands, also at x +- h
    if normalise:
        assert np.isclose(t["k"], rows / t["w"].sum()) and t["k"] != 1.0
    gscale, h = 0.37, 1e-6
    g = wt_grad(p, tg, cw, gscale, gamma, normalise)
    fd = np.zeros_like(x)
    for r in range(rows):
        for v in range(Vv):
            xp, xm = x.copy(), x.copy()
            xp[r, v] += h; xm[r, v] -= h
            lp = wt_loss(M.O.softmax(xp), tg, cw, gamma, normalise).sum()
            lm = wt_loss(M.O.softmax(xm), tg, cw, gamma, normalise).sum()
            fd[r, v] = gscale * (lp - lm) / (2 * h)
    assert np.abs(g - fd).max() < 1e-8, np.abs(g - fd).max()
    assert np.abs(g).max() > 0.05 and (g[[2, 4, 5]] == 0).all()
    ref = reference(x.astype(np.float32), tg, cw.astype(np.float32), gscale, gamma, normalise)
    x32 = x.astype(np.float32).astype(np.float64)
    assert np.allclose(ref["loss"], wt_loss(M.O.softmax(x32), tg, cw.astype(np.float32).astype(np.float64), gamma, normalise))
    # the mean of loss_row is sum(w l) / rows resp. sum(w l) / sum(w)
    l = t["f"] * t["ce"]
    want = (t["w"] * l).sum() / (t["w"].sum() if normalise else rows)
    assert np.isclose(wt_loss(p, tg, cw, gamma, normalise).mean(), want)


def test_neutral_settings_are_the_plain_oracle_steps():
    rng = np.random.default_rng(13)
    rows, Vv = 6, 9
    x = rng.standard_normal((rows, Vv)) * 2
    tg = rng.integers(0, Vv, rows)
    p = M.O.softmax(x)
    for cw, normalise in ((None, False), (None, True), (np.ones(Vv), False), (np.ones(Vv), True)):
        assert np.abs(wt_loss(p, tg, cw, 0.0, normalise) - M.O.cce_from_probs(p, tg)).max() < 1e-15
        assert np.abs(wt_grad(p, tg, cw, 0.3, 0.0, normalise) - M.O.cce_softmax_bwd(p, tg, np.full(rows, 0.3))).max() < 1e-15
        assert np.array_equal(wt_correct(p, tg, cw, 0.0, normalise), (p.argmax(-1) == tg).astype(np.float64))


def test_every_weight_zero_gives_zero_and_nothing_non_finite():
    rng = np.random.default_rng(14)
    rows, Vv = 5, 7
    p = M.O.softmax(rng.standard_normal((rows, Vv)))
    tg = rng.integers(0, 3, rows)
    cw = np.ones(Vv); cw[:3] = 0.0
    for gamma in (0.0, 2.0):
        t = terms(p, tg, cw, gamma, True)
        assert t["W"] == 0 and t["k"] == 0
        for out in (wt_loss(p, tg, cw, gamma, True), wt_correct(p, tg, cw, gamma, True), wt_grad(p, tg, cw, 1.0, gamma, True)):
            assert (out == 0).all() and np.isfinite(out).all()


def test_focal_factor_values():
    p = np.array([[0.25, 0.75], [0.9, 0.1]])
    tg = np.array([0, 0])
    l = wt_loss(p, tg, None, 2.0, False)
    assert np.allclose(l, [0.75 ** 2 * -np.log(0.25), 0.1 ** 2 * -np.log(0.9)])
    l = wt_loss(p, tg, np.array([0.25, 1.0]), 2.0, False)             # keras CategoricalFocalCrossentropy(alpha=0.25)
    assert np.allclose(l, [0.25 * 0.75 ** 2 * -np.log(0.25), 0.25 * 0.1 ** 2 * -np.log(0.9)])


def test_mock_op_follows_the_restatement(mock_backend):
    rng = np.random.default_rng(10)
    rows, Vv = 8, 11
    ld = Vv + 3
    x = rng.standard_normal((rows, Vv))
    tg = rng.integers(0, 4, rows)
    cw = rng.uniform(0.5, 2, Vv).astype(np.float32); cw[0] = 0
    buf = torch.full((rows, ld), 7.0)
    buf[:, :Vv] = torch.tensor(x, dtype=torch.float32)
    x32 = buf[:, :Vv].numpy().copy()
    loss, corr = torch.zeros(rows), torch.zeros(rows)
    mock_backend.softmax_cce_weighted(buf, torch.tensor(tg, dtype=torch.int32), torch.tensor(cw), None, loss, corr, buf, rows, Vv,
                                      ld, 0.25, 2.0, True)
    ref = reference(x32, tg, cw, 0.25, 2.0, True)
    assert np.allclose(loss.numpy(), ref["loss"], rtol=1e-6) and np.allclose(corr.numpy(), ref["corr"], rtol=1e-6)
    assert np.allclose(buf[:, :Vv].numpy(), ref["grad"], rtol=1e-6, atol=1e-9) and (buf[:, Vv:] == 7.0).all()
    assert (tg == 0).any() and (loss.numpy()[tg == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------- the loss object
def test_loss_object_and_checks():
    l = CategoricalCrossentropy()
    assert l.class_weight is None and l.focal_gamma == 0.0 and l.normalise == "count"
    l = loss_obj(class_weight={3: 0.5, 0: 0}, focal_gamma=2, normalise="weights")
    assert l.class_weight == {3: 0.5, 0: 0.0} and l.focal_gamma == 2.0 and l.normalise == "weights"
    w = loss_class_weight(l, 6)
    assert w.dtype == np.float32 and w.tolist() == [0, 1, 1, 0.5, 1, 1]                # missing ids weigh 1
    assert loss_class_weight(loss_obj(class_weight=[1, 2, 3]), 3).tolist() == [1, 2, 3]
    assert loss_class_weight(None) is None and loss_class_weight(object(), 5) is None
    assert loss_focal_gamma(None) == 0.0 and loss_focal_gamma(object()) == 0.0 and loss_focal_gamma(l) == 2.0
    assert loss_normalise(None) == "count" and loss_normalise(object()) == "count" and loss_normalise(l) == "weights"
    assert check_focal_gamma(1) == 1.0 and check_normalise("count") == "count"
    for bad in (-0.1, float("nan"), float("inf"), float("-inf"), "x", None):
        with pytest.raises(ValueError):
            loss_obj(focal_gamma=bad)
        with pytest.raises(ValueError):
            check_focal_gamma(bad)
    for bad in ("mean", "Weights", None, 1, True):
        with pytest.raises(ValueError):
            loss_obj(normalise=bad)
    for bad in ({1: -1.0}, {1: float("nan")}, {1: float("inf")}, {-1: 1.0}, {1.5: 1.0}, {"a": 1.0}, {1: "x"}, {True: 1.0},
                [1.0, -2.0], [1.0, float("nan")], [float("inf")], [], [[1.0, 2.0]], "abc", 3.0):
        with pytest.raises(ValueError):
            loss_obj(class_weight=bad)
    with pytest.raises(ValueError):
        check_class_weight({7: 1.0}, 7)                      # an id outside the vocabulary
    with pytest.raises(ValueError):
        check_class_weight([1.0, 2.0], 3)                    # a length other than V


def test_categorical_focal_crossentropy(mock_backend):
    l = CategoricalFocalCrossentropy()
    assert (l.alpha, l.gamma, l.focal_gamma, l.normalise, l.label_smoothing, l.unlikelihood) == (0.25, 2.0, 2.0, "count", 0, 0)
    assert loss_class_weight(l, 4).tolist() == [0.25] * 4
    l = CategoricalFocalCrossentropy(alpha=0.5, gamma=1.5)
    assert loss_class_weight(l, 3).tolist() == [0.5] * 3 and l.focal_gamma == 1.5
    for kw in (dict(alpha=-1), dict(alpha=float("nan")), dict(gamma=-1), dict(gamma=float("nan")), dict(alpha="x")):
        with pytest.raises(ValueError):
            CategoricalFocalCrossentropy(**kw)
    with pytest.raises(NotImplementedError):
        CategoricalFocalCrossentropy(from_logits=True)
    rng = np.random.default_rng(21)
    model, _ = dense(rng)
    model.compile(Adam(1e-3, clipnorm=0.1), CategoricalFocalCrossentropy(alpha=0.25, gamma=2.0))
    assert model.focal_gamma == 2.0 and model.class_weight.tolist() == [0.25] * V and model.loss_normalise == "count"
    data, tgt = padded_batch(B, rng)
    got = model.train_step((data, tgt)).as_floats()
    (c,) = mock_backend.wt_calls
    p = M.O.softmax(c["logits"])
    py = p[np.arange(T * B), c["target"]]
    want = (0.25 * (1 - py) ** 2 * -np.log(py)).mean()       # keras's formula
    assert abs(got["loss"] - want) <= 2e-6 * max(1.0, want)


def test_compile_reads_the_loss_object(mock_backend):
    model, _ = dense(np.random.default_rng(1))
    assert model.class_weight is None and model.cw_dev is None and model.focal_gamma == 0.0 and model.loss_normalise == "count"
    for loss in (None, object(), CategoricalCrossentropy()):
        model.compile(Adam(1e-3), loss)
        assert model.class_weight is None and model.cw_dev is None and not model._token_weights_on()
    model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0, 2: 3.0}, focal_gamma=0.5, normalise="weights"))
    want = np.ones(V, np.float32); want[0] = 0; want[2] = 3
    assert np.array_equal(model.class_weight, want) and np.array_equal(model.cw_dev.numpy(), want)
    assert model.cw_dev.dtype == torch.float32 and model.cw_dev.shape == (V,)
    assert model.focal_gamma == 0.5 and model.loss_normalise == "weights" and model._token_weights_on()

    class Bad:
        focal_gamma = float("nan")
    with pytest.raises(ValueError):
        model.compile(Adam(1e-3), Bad())
    with pytest.raises(ValueError):
        model.compile(Adam(1e-3), loss_obj(class_weight={V: 1.0}))
    with pytest.raises(ValueError):
        model.compile(Adam(1e-3), loss_obj(class_weight=np.ones(V + 1)))
    assert mock_backend.names == []


# ---------------------------------------------------------------------------------------------------- neutral settings
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_neutral_settings_issue_todays_calls(kind, mock_backend):
    make = dense if kind == "dense" else attention
    logs = []
    for loss in ("absent", None, CategoricalCrossentropy(), loss_obj(class_weight=None, focal_gamma=0.0, normalise="count")):
        rng = np.random.default_rng(2)
        model, _ = make(rng)
        if loss == "absent":
            model.compile(Adam(1e-3, clipnorm=0.1))
        else:
            model.compile(Adam(1e-3, clipnorm=0.1), loss)
        data, tgt = padded_batch(B, rng)
        mock_backend.names.clear()
        m1 = model.train_step((data, tgt)).as_floats()
        m2 = model.test_step((data, tgt)).as_floats()
        logs.append((list(mock_backend.names), m1, m2))
    assert all(l == logs[0] for l in logs[1:])
    assert "softmax_cce_weighted" not in logs[0][0] and logs[0][0].count("softmax_cce") == 2
    assert mock_backend.wt_calls == []


# ---------------------------------------------------------------------------------------------------- the feature
SETTINGS = {
    "weights": dict(class_weight="w", focal_gamma=0.0, normalise="count"),
    "focal": dict(class_weight=None, focal_gamma=2.0, normalise="count"),
    "normalised": dict(class_weight={0: 0.0}, focal_gamma=0.0, normalise="weights"),
    "all": dict(class_weight="w", focal_gamma=0.5, normalise="weights"),
    "mode only": dict(class_weight=None, focal_gamma=0.0, normalise="weights"),
}


def settings(name, rng):
    kw = dict(SETTINGS[name])
    if kw["class_weight"] == "w":
        kw["class_weight"] = some_weights(rng)
    return kw


@pytest.mark.parametrize("kind", ["dense", "attention"])
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_one_weighted_launch_where_the_plain_one_was(kind, name, mock_backend):
    """the launch log of the step is the neutral step's with softmax_cce replaced by softmax_cce_weighted, and nothing else"""
    logs = {}
    for on in (False, True):
        rng = np.random.default_rng(3)
        model, _ = (dense if kind == "dense" else attention)(rng)
        kw = settings(name, rng)
        model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(**kw) if on else None)
        data, tgt = padded_batch(B, rng)
        mock_backend.names.clear()
        mock_backend.wt_calls.clear()
        model.train_step((data, tgt))
        model.test_step((data, tgt))
        logs[on] = list(mock_backend.names)
    assert "softmax_cce_live" not in logs[True] and logs[True].count("softmax_cce_weighted") == 2
    assert "softmax_cce" not in logs[True] and logs[False].count("softmax_cce") == 2
    assert [n if n != "softmax_cce_weighted" else "softmax_cce" for n in logs[True]] == logs[False]
    train, test = mock_backend.wt_calls
    assert train["want_grad"] and not train["want_probs"] and train["gscale"] == 1.0 / (T * B)
    assert test["want_probs"] and not test["want_grad"] and test["gscale"] == 0.0
    for c in (train, test):
        assert (c["rows"], c["V"], c["gamma"], c["normalise"]) == (T * B, V, kw["focal_gamma"], kw["normalise"] == "weights")
        assert (c["cw"] is None) == (kw["class_weight"] is None)
        assert np.array_equal(c["target"].reshape(T, B).T, tgt)


@pytest.mark.parametrize("kind", ["dense", "attention"])
@pytest.mark.parametrize("world", [1, 2])
def test_gscale_carries_the_world_size(kind, world, mock_backend):
    rng = np.random.default_rng(4)
    kw = {}
    if world > 1:
        hook = lambda m: None
        hook.world = world
        kw["grad_sync"] = hook
    model, _ = (dense if kind == "dense" else attention)(rng, **kw)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(class_weight=some_weights(rng), focal_gamma=2.0))
    data, tgt = padded_batch(B, rng)
    got = model.train_step((data, tgt)).as_floats()
    (c,) = mock_backend.wt_calls
    assert c["gscale"] == 1.0 / (T * B * world) and not c["normalise"]
    want = call_loss(c)
    assert abs(got["loss"] - want) <= 2e-6 * max(1.0, want)


@pytest.mark.parametrize("kind", ["dense", "attention"])
@pytest.mark.parametrize("name", ["all", "normalised", "focal"])
def test_train_and_test_step_match_the_weighted_oracle(kind, name, mock_backend):
    rng = np.random.default_rng(5)
    model, orc = (dense if kind == "dense" else attention)(rng)
    kw = settings(name, rng)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), loss_obj(**kw))
    cw, gamma, norm = model.class_weight, kw["focal_gamma"], kw["normalise"] == "weights"
    cw = None if cw is None else cw.astype(np.float64)
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noise = {}
    for step in range(2):
        data, tgt = padded_batch(B, rng)
        out = orc.forward(data, True, M.DropCtx(seed=11, step=step, training=True))[0]
        probs = out[0] if isinstance(out, tuple) else out
        want_loss, want_acc = weighted_metrics(probs, tgt, cw, gamma, norm)
        with weighted(cw, gamma, norm):
            res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        assert abs(want_loss - res["loss"]) > 100 * 2e-5 * res["loss"]               # not the plain loss, by far
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - want_loss) < 2e-5 * max(1, abs(want_loss))            # test_host_nic's bounds
        assert abs(got["accuracy"] - want_acc) < 1e-6
        if name == "normalised":         # class_weight {0: 0}, "weights": the means over the non-padding positions
            pt = probs.transpose(1, 0, 2).reshape(T * B, V)
            yt = tgt.T.reshape(-1)
            live = yt != 0
            assert abs(got["loss"] - M.O.cce_from_probs(pt[live], yt[live]).mean()) < 2e-5 * max(1, want_loss)
            assert abs(got["accuracy"] - (pt[live].argmax(-1) == yt[live]).mean()) < 1e-6
        for k, v in orc.p.items():
            if k == "attention/V/bias":                  # zero-gradient variable: Adam amplifies rounding noise
                continue
            if grads.get(k) is not None:                 # test_gpu_nic's rule: where the gradient is rounding noise
                noise[k] = noise.get(k, 0.0) + 1e-3 * (np.abs(grads[k]) < 1e-8)   # (|g| < 1e-8), Adam steps +-lr at random
            assert (np.abs(model.get_weight(k) - v) <= 3e-6 + 2e-4 * np.abs(v) + noise.get(k, 0.0)).all(), (step, k)
    data, tgt = padded_batch(B, rng)
    out = orc.test_step(data, tgt)[1]
    want_loss, want_acc = weighted_metrics(out[0] if isinstance(out, tuple) else out, tgt, cw, gamma, norm)
    got = model.test_step((data, tgt)).as_floats()                      # the same objective in the evaluation form
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1, abs(want_loss)) and abs(got["accuracy"] - want_acc) < 1e-6


def test_dense_model_leaves_the_compact_head(mock_backend):
    model, _ = dense(np.random.default_rng(5))
    model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}))
    data, tgt = padded_batch(B, np.random.default_rng(5))
    model.train_step((data, tgt))
    # every other condition of the compact head granted, the feature alone turns it off
    be = mock_backend
    model._seq_lstm, model.seq_xch = True, object()
    for name in ("stage_batch_map", "softmax_cce_live", "gemm3"):
        if not hasattr(be, name):
            setattr(be, name, lambda *a, **k: None)
    for name in ("head_pos", "head_w", "head_tgt", "head_live"):
        if name not in model.__dict__:
            setattr(model, name, None)
    assert model._head_map_bufs(B, T) is None
    model.set_class_weight(None)
    assert model._head_map_bufs(B, T) is not None
    model.focal_gamma = 2.0
    assert model._head_map_bufs(B, T) is None
    model.focal_gamma, model.loss_normalise = 0.0, "weights"
    assert model._head_map_bufs(B, T) is None
    model.loss_normalise = "count"
    assert model._head_map_bufs(B, T) is not None


# ---------------------------------------------------------------------------------------------------- graphs, the buffer
def test_recompile_with_another_setting_drops_the_graphs(mock_backend):
    rng = np.random.default_rng(5)
    model, _ = dense(rng)
    w = some_weights(rng)
    model.compile(Adam(1e-3), loss_obj(class_weight=w, focal_gamma=2.0))
    for loss, same in ((loss_obj(class_weight=w * 2, focal_gamma=2.0), True),               # other weights: the same launch
                       (loss_obj(class_weight=w, focal_gamma=1.0), False),
                       (loss_obj(class_weight=w, focal_gamma=1.0, normalise="weights"), False),
                       (loss_obj(focal_gamma=1.0, normalise="weights"), False),             # the weights go
                       (loss_obj(class_weight={1: 2.0}, focal_gamma=1.0, normalise="weights"), False),
                       (None, False)):
        model._graphs["sentinel"] = 1
        model.compile(Adam(1e-3), loss)
        assert ("sentinel" in model._graphs) == same, loss and vars(loss)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_set_class_weight_rewrites_the_buffer_in_place(kind, mock_backend):
    """what a recorded plan or a captured graph holds is the buffer's address: new weights reach the next replay because
    they are written into that buffer, and nothing is recorded again"""
    rng = np.random.default_rng(6)
    model, _ = (dense if kind == "dense" else attention)(rng)
    w1, w2 = some_weights(rng), some_weights(rng, pad=0.5)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(class_weight=w1, normalise="weights"))
    data, tgt = padded_batch(B, rng)
    model.train_step((data, tgt))
    buf, ptr = model.cw_dev, model.cw_dev.data_ptr()
    model._graphs["sentinel"] = "recorded with w1"
    model.set_class_weight(w2)
    assert model.cw_dev is buf and buf.data_ptr() == ptr and np.array_equal(buf.numpy(), w2)
    assert model._graphs.get("sentinel") == "recorded with w1"
    model.set_class_weight({1: 4.0, 0: 0.0})
    w3 = np.ones(V, np.float32); w3[1] = 4; w3[0] = 0
    assert model.cw_dev is buf and np.array_equal(buf.numpy(), w3) and "sentinel" in model._graphs
    mock_backend.wt_calls.clear()
    got = model.train_step((data, tgt)).as_floats()
    (c,) = mock_backend.wt_calls
    assert c["cw_tensor"] is buf and np.array_equal(c["cw"], w3.astype(np.float64))
    assert abs(got["loss"] - call_loss(c)) <= 2e-6 * max(1.0, call_loss(c))
    # weights <-> no weights is another launch: the recordings go ("weights" keeps the weighted head without them)
    model.set_class_weight(None)
    assert model._graphs == {} and model.cw_dev is None and model.class_weight is None and model._token_weights_on()
    model._graphs["sentinel"] = 1
    model.set_class_weight(w1)
    assert model._graphs == {} and np.array_equal(model.cw_dev.numpy(), w1)
    for bad in ({V: 1.0}, np.ones(V - 1), {1: -1.0}, [float("nan")] * V):
        with pytest.raises(ValueError):
            model.set_class_weight(bad)
    assert np.array_equal(model.cw_dev.numpy(), w1)


def test_fit_class_weight(mock_backend):
    rng = np.random.default_rng(7)
    model, _ = dense(rng)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batches = [padded_batch(B, rng) for _ in range(2)]
    hist = model.fit(batches, epochs=1, verbose=0, class_weight={0: 0.0, 3: 2.0})
    want = np.ones(V, np.float32); want[0] = 0; want[3] = 2
    assert np.array_equal(model.class_weight, want)
    assert len(mock_backend.wt_calls) == 2 and all(np.array_equal(c["cw"], want) and not c["normalise"]
                                                   for c in mock_backend.wt_calls)      # from the first step on
    assert "softmax_cce" not in mock_backend.names
    assert np.isclose(hist["loss"][0], np.mean([call_loss(c) for c in mock_backend.wt_calls]), rtol=1e-5)
    mock_backend.wt_calls.clear()
    model.fit(batches, epochs=1, verbose=0)                  # None leaves the weights as they are
    assert len(mock_backend.wt_calls) == 2 and np.array_equal(model.class_weight, want)
    with pytest.raises(ValueError):
        model.fit(batches, epochs=1, verbose=0, class_weight={V + 2: 1.0})


# ---------------------------------------------------------------------------------------------------- inherited paths
PATHS = {
    "ms2 S=2": lambda rng: (attention(rng, MsNIC, None, n_subjects=2)[0], "train_step", 6),
    "scheduled sampling": lambda rng: (dense(rng, scheduled_sampling=SS.linear(0.5, 0.0))[0], "train_step", B),
    "attention scheduled sampling": lambda rng: (attention(rng, scheduled_sampling=SS.linear(0.5, 0.0))[0], "train_step", B),
    "train_step_sam": lambda rng: (attention(rng)[0], "train_step_sam", B),
    "free running": lambda rng: (attention(rng, teacher_forcing=False)[0], "train_step", B),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_paths_through_loss_metrics_inherit_the_feature(path, mock_backend):
    rng = np.random.default_rng(6)
    model, method, b = PATHS[path](rng)
    w = some_weights(rng)
    mode = "count" if path == "ms2 S=2" else "weights"
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(class_weight=w, focal_gamma=2.0, normalise=mode))
    data, tgt = padded_batch(b, rng)
    mock_backend.names.clear()
    got = getattr(model, method)((data, tgt)).as_floats()
    n = 2 if method == "train_step_sam" else 1            # SAM: the loss at w and at w + e(w)
    assert mock_backend.names.count("softmax_cce_weighted") == n and "softmax_cce" not in mock_backend.names
    assert len(mock_backend.wt_calls) == n
    for c in mock_backend.wt_calls:
        assert c["gamma"] == 2.0 and c["want_grad"] and c["normalise"] == (mode == "weights") and np.array_equal(c["cw"], w)
        assert np.array_equal(c["target"].reshape(T, b).T, tgt)
    wants = [call_loss(c) for c in mock_backend.wt_calls]
    assert any(abs(got["loss"] - x) <= 2e-6 * max(1.0, x) for x in wants), (got["loss"], wants)
    if path == "ms2 S=2":                                  # the per-subject metrics read loss_row / correct_row
        (c,) = mock_backend.wt_calls
        p = M.O.softmax(c["logits"])
        rows = wt_loss(p, c["target"], c["cw"], 2.0, False).reshape(T, b)
        hits = wt_correct(p, c["target"], c["cw"], 2.0, False).reshape(T, b)
        for q in range(2):
            want = rows[:, q * 3:(q + 1) * 3].mean()
            assert abs(got["loss" + "AB"[q]] - want) <= 2e-6 * max(1.0, want), (q, got, want)
            assert abs(got["accuracy" + "AB"[q]] - hits[:, q * 3:(q + 1) * 3].mean()) < 1e-6


# ---------------------------------------------------------------------------------------------------- refusals
ACTIVE = [dict(class_weight={0: 0.0}), dict(focal_gamma=2.0), dict(normalise="weights")]


@pytest.mark.parametrize("kw", ACTIVE)
@pytest.mark.parametrize("other", [dict(label_smoothing=0.1), dict(unlikelihood=1.0)])
def test_refused_together_with_smoothing_or_unlikelihood(kw, other, mock_backend):
    model, _ = dense(np.random.default_rng(1))
    with pytest.raises(ValueError, match="one head kernel"):
        model.compile(Adam(1e-3), loss_obj(**kw, **other))
    assert model.optimizer is None and not model._token_weights_on() and model.label_smoothing == 0.0
    model.compile(Adam(1e-3), loss_obj(**other))
    with pytest.raises(ValueError, match="one head kernel"):
        model.set_class_weight({0: 0.0})
    assert model.class_weight is None
    model.compile(Adam(1e-3), loss_obj(**kw))
    assert mock_backend.names == []


@pytest.mark.parametrize("kw", ACTIVE)
def test_self_critical_refuses_before_any_launch(kw, mock_backend):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, self_critical=SC(2))
    with pytest.raises(ValueError, match="self_critical"):
        model.compile(Adam(1e-3), loss_obj(**kw))
    assert model.optimizer is None and not model._token_weights_on()
    model.compile(Adam(1e-3), loss_obj())
    with pytest.raises(ValueError, match="self_critical"):
        model.set_class_weight({0: 0.0})
    assert mock_backend.names == []


@pytest.mark.parametrize("kw", ACTIVE)
@pytest.mark.parametrize("kind", ["think_and_tell", "show_and_tell", "fc"])
def test_models_with_another_loss_refuse(kind, kw, mock_backend):
    if kind == "show_and_tell":
        model = SAT.CaptionGenerator(SAT.Encoder(E), SAT.Decoder(E, U, V), None, T, device="cpu", seed=11)
    elif kind == "think_and_tell":
        model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                    None, T, device="cpu", seed=11)
    else:
        model = NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    assert not model.SUPPORTS_TOKEN_WEIGHTS
    with pytest.raises(NotImplementedError, match="caption head"):
        model.compile(Adam(1e-3), loss_obj(**kw))
    assert model.optimizer is None
    model.compile(Adam(1e-3), loss_obj())
    model.compile(Adam(1e-3))
    with pytest.raises(NotImplementedError, match="caption head"):
        model.set_class_weight({0: 0.0})
    with pytest.raises(NotImplementedError, match="caption head"):
        model.fit([], epochs=0, verbose=0, class_weight={0: 0.0})
    assert mock_backend.names == []


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_weights_normalisation_is_refused_under_data_parallel(kind, mock_backend):
    hook = lambda m: None
    hook.world = 2
    model, _ = (dense if kind == "dense" else attention)(np.random.default_rng(1), grad_sync=hook)
    with pytest.raises(NotImplementedError, match="per rank"):
        model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}, normalise="weights"))
    with pytest.raises(NotImplementedError, match="per rank"):
        model.compile(Adam(1e-3), loss_obj(normalise="weights"))
    assert model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}, focal_gamma=2.0))            # "count" works
    # dp.attach on a model compiled with it refuses before it touches the process group or the model
    model, _ = (dense if kind == "dense" else attention)(np.random.default_rng(1))
    model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}, normalise="weights"))
    seed = model.seed
    with pytest.raises(NotImplementedError, match="per rank"):
        dp.attach(model, world=2, rank=1)
    assert model.grad_sync is None and model.dp_world == 1 and model.seed == seed
    assert mock_backend.names == []


def test_weights_normalisation_is_refused_with_several_subjects(mock_backend):
    model, _ = attention(np.random.default_rng(1), MsNIC, None, n_subjects=2)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}, normalise="weights"))
    assert model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(class_weight={0: 0.0}, focal_gamma=2.0))            # "count" works
    assert mock_backend.names == []


# ---------------------------------------------------------------------------------------------------- config
def _config(**extra):
    c = dict(top_k=V - 1, units=U, embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], max_length=T,
             dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
             input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", clipnorm=0.1, alpha=1e-4)
    c.update(extra)
    return c


def test_build_model_config_keys(mock_backend):
    rng = np.random.default_rng(8)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    m = cfg.build_model(_config(), g, device="cpu")
    assert m.class_weight is None and m.focal_gamma == 0.0 and m.loss_normalise == "count" and not m._token_weights_on()
    m = cfg.build_model(_config(class_weight={0: 0.0, 5: 2.5}, focal_gamma=1.5, loss_normalise="weights"), g, device="cpu")
    want = np.ones(V, np.float32); want[0] = 0; want[5] = 2.5
    assert np.array_equal(m.class_weight, want) and m.focal_gamma == 1.5 and m.loss_normalise == "weights"
    assert m.loss.focal_gamma == 1.5 and m.label_smoothing == 0.0 and m.unlikelihood == 0.0
    for bad in (dict(focal_gamma=-1.0), dict(loss_normalise="mean"), dict(class_weight={0: -1.0}), dict(class_weight={V: 1.0}),
                dict(focal_gamma=2.0, label_smoothing=0.1), dict(class_weight={0: 0.0}, unlikelihood=1.0)):
        with pytest.raises(ValueError):
            cfg.build_model(_config(**bad), g, device="cpu")
    with pytest.raises(NotImplementedError):
        cfg.build_model(_config(focal_gamma=2.0), None, mode="fc", input_size=N, device="cpu")
    assert mock_backend.names == []


# ---------------------------------------------------------------------------------------------------- token_class_weights
def test_token_class_weights_on_a_hand_counted_corpus():
    # counts: id 0 (pad) x5, id 1 x4, id 2 x1, id 3 x9, id 4 never, id 5 x1
    caps = np.array([[1, 3, 3, 3, 0], [1, 3, 3, 2, 0], [1, 3, 3, 5, 0], [1, 3, 3, 0, 0]])
    Vv = 6
    n = np.array([5, 4, 1, 9, 1, 1], np.float64)                          # the unseen class counts as 1
    cnt = np.array([5, 4, 1, 9, 0, 1], np.float64)
    tokens = 15.0
    for scheme, raw in (("inverse", 1 / n), ("inverse_sqrt", 1 / np.sqrt(n)), ("effective", (1 - 0.9) / (1 - 0.9 ** n))):
        w = token_class_weights(caps, Vv, scheme=scheme, beta=0.9, mean_one=False, pad_weight=0.125)
        assert w.dtype == np.float32 and w.shape == (Vv,)
        want = raw.copy(); want[0] = 0.125
        assert np.allclose(w, want, rtol=1e-6) and w[0] == 0.125
        assert w[4] == w[2] == w[5]                                       # unseen: the weight of count 1
        assert w[3] < w[1] < w[2]                                         # frequent words weigh less
        w1 = token_class_weights(caps, Vv, scheme=scheme, beta=0.9)
        s = tokens / (cnt[1:] * raw[1:]).sum()
        want = raw * s; want[0] = 0.0
        assert np.allclose(w1, want, rtol=1e-6) and w1[0] == 0.0          # pad_weight defaults to 0
        assert np.isclose((cnt[1:] * w1[1:].astype(np.float64)).sum() / tokens, 1.0, rtol=1e-6)    # corpus-token mean 1
        assert np.array_equal(w1, token_class_weights(caps.copy(), Vv, scheme=scheme, beta=0.9))    # deterministic
    assert np.array_equal(token_class_weights(caps, Vv), token_class_weights(caps, Vv, scheme="inverse_sqrt"))
    # clip, in the scaled units
    w = token_class_weights(caps, Vv, scheme="inverse", clip=(0.5, 2.0))
    full = token_class_weights(caps, Vv, scheme="inverse")
    assert np.allclose(w[1:], np.clip(full[1:], 0.5, 2.0)) and w[0] == 0 and w.max() == 2.0 and w[1:].min() == 0.5
    assert full.max() > 2.0 and full[1:].min() < 0.5
    # any integer shape / dtype; no non-pad token: nothing to scale by
    assert np.array_equal(token_class_weights(caps.reshape(-1).astype(np.int32), Vv), token_class_weights(caps, Vv))
    assert token_class_weights(np.zeros((2, 3), np.int64), 3).tolist() == [0.0, 1.0, 1.0]
    for bad in (dict(scheme="log"), dict(beta=1.0), dict(beta=0.0), dict(pad_weight=-1.0), dict(pad_weight=float("nan")),
                dict(clip=(2.0, 1.0)), dict(clip=(-1.0, 1.0))):
        with pytest.raises(ValueError):
            token_class_weights(caps, Vv, **{"scheme": "effective", **bad})
    with pytest.raises(ValueError):
        token_class_weights(caps, 5)                                      # id 5 outside the vocabulary
    with pytest.raises(ValueError):
        token_class_weights(caps.astype(np.float32), Vv)
    with pytest.raises(ValueError):
        token_class_weights(caps, 0)
    check_class_weight(token_class_weights(caps, Vv), Vv)                 # what the loss object accepts
