"""The attention coverage penalty on the CPU through a mock backend that follows tnt_attention_coverage_f32's header
definition (tests/coverage_oracle.py): the float64 restatement against central differences, the chain backward with a
rider against central differences of a scalar, validation and the config key, the launch sequence with the feature on and
off, the capture key, every refusal, the ``coverage`` metric of train_step / test_step / fit, and a training step of
lc_nic.NIC against the oracle model that differentiates CE + L2 + weight * coverage."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import AttentionCoverage, ScheduledSampling as SS
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from oracle import ops as O
from helpers import synth_batch, tiny_groups
import coverage_oracle as CO
import lc_chain_oracle as C

B, N, T, V, U = 5, 23, 6, 13, 16
LC = dict(R=4, D=16, A=5, Et=12)


class RecordingBackend(CO.CoverageMockBackend):
    """the mock with every public call logged in ``calls`` as (name, args, kwargs)"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v) or name in ("calls", "cov_calls"):
            return v
        calls = object.__getattribute__(self, "calls")

        def logged(*a, **k):
            calls.append((name, a, k))
            return v(*a, **k)
        return logged

    @property
    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def attention(rng, cls=LcNIC, rates=(0,) * 6, coverage=None, with_arg=True, **kw):
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    args = (g, U, 512, LC["Et"], LC["A"], V, T, *rates, 0.01, 0.001, 3e-5, 1e-5)
    if with_arg:
        kw["attention_coverage"] = coverage
    model = cls(*args, device="cpu", seed=11, **kw)
    orc = CO.CoverageLcNIC(*args).init_params(rng)
    orc.coverage = (coverage.weight, coverage.axis) if coverage is not None else None
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("axis", CO.AXES)
def test_value_and_gradient_against_central_differences(axis):
    rng = np.random.default_rng(3)
    Tt, Bb, Rr, w = 4, 3, 5, 0.7
    alpha = rng.random((Tt, Bb, Rr))
    alpha /= alpha.sum(-1, keepdims=True)
    s = CO.sums(alpha, axis)
    assert s.shape == ((Bb, Rr) if axis == "time" else (Tt, Rr))
    want = sum((1 - s[i, r]) ** 2 for i in range(s.shape[0]) for r in range(Rr)) / (s.shape[0] * Rr)
    assert np.isclose(CO.coverage(alpha, axis), want, rtol=1e-14)
    g, h = CO.coverage_grad(alpha, w, axis), 1e-6
    fd = np.zeros_like(alpha)
    for idx in np.ndindex(alpha.shape):
        ap, am = alpha.copy(), alpha.copy()
        ap[idx] += h; am[idx] -= h
        fd[idx] = w * (CO.coverage(ap, axis) - CO.coverage(am, axis)) / (2 * h)
    assert np.abs(g - fd).max() <= 1e-8 * np.abs(g).max()
    e = CO.ext_rows(alpha, w, axis)
    assert np.array_equal(CO.ext_view(e, *CO.strides(axis, Rr), Tt, Bb, Rr), g)


def test_batch_axis_value_is_the_attention_metric():
    rng = np.random.default_rng(4)
    alpha = rng.random((4, 3, 5))
    orc = M.LcNIC.__new__(M.LcNIC)
    probs, y = np.full((3, 4, 2), 0.5), np.zeros((3, 4), np.int64)
    assert CO.coverage(alpha, "batch") == orc.metrics(probs, alpha[..., None], y)[2]
    assert CO.coverage(alpha, "time") != CO.coverage(alpha, "batch")


def test_chain_backward_with_a_rider_against_central_differences():
    """chain_bwd_ext's gradients are those of sum(dout * hs[1:]) + sum(ext * alpha) (ext an arbitrary constant [T][B][R]);
    with ext = 0 it is lc_chain_oracle.chain_bwd"""
    rng = np.random.default_rng(8)
    Tt, Bb, Rr, D, A, Uu = 3, 2, 5, 4, 4, 8
    n = lambda *s, sc=1.0: rng.standard_normal(s) * sc
    i = dict(F=n(Bb, Rr, D), P=n(Bb, Rr, A), W2=n(Uu, A, sc=0.4), b2=n(A, sc=0.1), v=n(A), bv=n(1), xz=n(Tt, Bb, Uu, 4, sc=0.5),
             Wc=n(D, Uu, 4, sc=0.5), Ur=n(Uu, Uu, 4, sc=0.4), zb=n(Uu, 4, sc=0.1), h0=n(Bb, Uu, sc=0.5), c0=n(Bb, Uu, sc=0.5))
    dout, ext = n(Tt, Bb, Uu), n(Tt, Bb, Rr)

    def scalar(**over):
        f = C.chain_fwd(**{**i, **over})
        return (dout * f["hs"][1:]).sum() + (ext * f["alpha"]).sum(), f
    _, f = scalar()
    args = (i["F"], i["P"], i["W2"], i["v"], i["Wc"], i["Ur"], f["qpre"], f["alpha"], f["gates"], f["cs"], dout)
    got = CO.chain_bwd_ext(*args, ext)
    plain, zero = C.chain_bwd(*args), CO.chain_bwd_ext(*args, np.zeros_like(ext))
    for k in plain:
        assert np.array_equal(plain[k], zero[k]), k
    assert np.abs(got["dP"] - plain["dP"]).max() > 1e-3
    h = 1e-6
    for name, key in (("P", "dP"), ("F", "dF"), ("xz", "dz"), ("h0", "dh0"), ("c0", "dc0")):
        fd = np.zeros_like(i[name])
        for idx in list(np.ndindex(i[name].shape))[::3]:
            p_, m_ = i[name].copy(), i[name].copy()
            p_[idx] += h; m_[idx] -= h
            fd[idx] = (scalar(**{name: p_})[0] - scalar(**{name: m_})[0]) / (2 * h)
        mask = fd != 0
        assert mask.any() and np.abs(got[key][mask] - fd[mask]).max() <= 1e-6 * np.abs(fd).max(), name


@pytest.mark.parametrize("axis", CO.AXES)
def test_oracle_model_gradient_against_central_differences(axis):
    """CoverageLcNIC.backward differentiates scalar_loss = CE + L2 + weight * coverage"""
    rng = np.random.default_rng(21)
    _, orc = attention(rng, coverage=AttentionCoverage(3.0, axis))
    data, tgt = synth_batch(B, N, T, V, U, rng, dtype=np.float64)
    drop = M.DropCtx(seed=11, step=0, training=True)
    (probs, attn), cache = orc.forward(data, training=True, drop=drop)
    grads, _ = orc.backward(probs, cache, tgt)
    orc.coverage, plain = None, None
    plain, _ = orc.backward(probs, cache, tgt)
    orc.coverage = (3.0, axis)
    h = 1e-6
    for k in ("attention/V/kernel", "attention/W2/bias", "attention/W1/bias", "lstm/bias", "dense_in/1/bias"):
        w0 = orc.p[k]
        assert np.abs(grads[k] - plain[k]).max() > 1e-6, k              # the term reaches this variable
        for idx in list(np.ndindex(w0.shape))[:4]:
            vals = []
            for sgn in (1, -1):
                w = w0.copy(); w[idx] += sgn * h
                orc.p[k] = w
                vals.append(orc.scalar_loss(data, tgt, drop))
            orc.p[k] = w0
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(grads[k][idx] - fd) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (k, idx, grads[k][idx], fd)


# ---------------------------------------------------------------------------------------------------- the public surface
def test_validation_and_config_key():
    c = AttentionCoverage(0.5)
    assert (c.weight, c.axis, c.axis_id, c.key) == (0.5, "time", 0, ("coverage", 0.5, "time"))
    assert AttentionCoverage(1, "batch").axis_id == 1 and AttentionCoverage(1, "batch") == AttentionCoverage(1.0, "batch")
    assert c.coef(6, 5, 4) == 2 * 0.5 / (5 * 4) and AttentionCoverage(0.5, "batch").coef(6, 5, 4) == 2 * 0.5 / (6 * 4)
    assert c.strides(4) == (0, 4) and AttentionCoverage(0.5, "batch").strides(4) == (4, 0)
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            AttentionCoverage(bad)
    for bad in ("t", 0, None, "Time"):
        with pytest.raises(ValueError, match="axis"):
            AttentionCoverage(1.0, bad)
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="AttentionCoverage"):
        attention(rng, coverage=None, with_arg=False, attention_coverage=0.5)
    assert attention(rng, coverage=AttentionCoverage(0.0))[0].attention_coverage is None     # weight 0: the plain model
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    base = dict(units=U, embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], top_k=V - 1, max_length=T,
                dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
                input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3, clipnorm=0.1,
                decay=0)
    try:
        plain = cfg.build_model(base, g, device="cpu")
    except (KeyError, ValueError, TypeError) as e:           # the optimizer keys of this library's config
        pytest.fail(f"config without the key does not build: {e!r}")
    assert plain.attention_coverage is None
    m = cfg.build_model({**base, "attention_coverage": {"weight": 0.25, "axis": "batch"}}, g, device="cpu")
    assert m.attention_coverage == AttentionCoverage(0.25, "batch")
    assert cfg.build_model({**base, "attention_coverage": {"weight": 0.25}}, g, device="cpu").attention_coverage.axis == "time"
    for bad in ({"axis": "time"}, {"weight": 1, "axes": "time"}, 0.5, {"weight": -1}):
        with pytest.raises(ValueError):
            cfg.build_model({**base, "attention_coverage": bad}, g, device="cpu")
    with pytest.raises(TypeError):                           # the dense models and NICfc do not take the argument
        NIC(N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", attention_coverage=c)
    with pytest.raises(TypeError):
        NICfc(N, U, 512, 16, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", attention_coverage=c)


def test_every_refusal(mock_backend):
    rng = np.random.default_rng(2)
    c = AttentionCoverage(0.5)
    for kw, what in ((dict(teacher_forcing=False, rates=(0, 0, 0, 0, 0, 0)), "teacher_forcing"),
                     (dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                     (dict(use_layer_norm=True), "use_layer_norm"),
                     (dict(grad_sync=lambda m: None), "data-parallel")):
        with pytest.raises(NotImplementedError, match=what):
            attention(rng, coverage=c, **kw)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        attention(rng, cls=MsNIC, coverage=c)
    model, _ = attention(rng, coverage=c)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batch = synth_batch(B, N, T, V, U, rng)
    with pytest.raises(NotImplementedError, match="alpha_mse"):
        model.train_step_sam(batch)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    model.grad_sync = lambda m: None                          # attached behind the constructor's back
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.train_step(batch)
    assert mock_backend.names == []                          # nothing was launched by any of them
    # weight 0 refuses nothing
    attention(rng, coverage=AttentionCoverage(0.0), use_layer_norm=True)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    MsNIC(g, U, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu",
          attention_coverage=AttentionCoverage(0.0))


# ---------------------------------------------------------------------------------------------------- launches
def norm(x):
    """a call argument by value; a tensor by shape and dtype (two models own different buffers)"""
    import torch
    if isinstance(x, torch.Tensor):
        return ("tensor", tuple(x.shape), str(x.dtype))
    if isinstance(x, (tuple, list)):
        return tuple(norm(y) for y in x)
    if isinstance(x, dict):
        return tuple(sorted((k, norm(v)) for k, v in x.items()))
    return x


@pytest.mark.parametrize("rates", [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)])
def test_feature_off_launches_what_a_model_without_the_argument_does(mock_backend, rates):
    """None and weight 0: the same backend methods with the same arguments (tensors compared by shape and dtype, each model
    owning its buffers) and the same metrics as a model built without the keyword, in train_step and test_step"""
    logs = []
    for kw in (dict(with_arg=False), dict(coverage=None), dict(coverage=AttentionCoverage(0.0, "batch"))):
        rng = np.random.default_rng(6)
        model, _ = attention(rng, rates=rates, **kw)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = synth_batch(B, N, T, V, U, rng)
        mock_backend.calls.clear()
        m1 = model.train_step(batch).as_floats()
        m2 = model.test_step(batch).as_floats()
        assert "coverage" not in m1 and "coverage" not in m2
        assert not hasattr(model, "cov_ext")
        logs.append(([(n, norm(a), norm(k_)) for n, a, k_ in mock_backend.calls], m1, m2))
    assert all(l == logs[0] for l in logs[1:])
    assert "attention_coverage" not in [c[0] for c in logs[0][0]]
    assert all("ext" not in dict(c[2]) for c in logs[0][0])


@pytest.mark.parametrize("axis", CO.AXES)
def test_feature_on_adds_exactly_one_launch_in_front_of_the_chain(mock_backend, axis):
    logs = {}
    for on in (False, True):
        rng = np.random.default_rng(6)
        model, _ = attention(rng, coverage=AttentionCoverage(0.5, axis) if on else None)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = synth_batch(B, N, T, V, U, rng)
        mock_backend.calls.clear()
        model.train_step(batch)
        logs[on] = list(mock_backend.calls)
    names = {k: [c[0] for c in v] for k, v in logs.items()}
    assert names[True].count("attention_coverage") == 1 and "attention_coverage" not in names[False]
    k = names[True].index("attention_coverage")
    assert names[True][:k] + names[True][k + 1:] == names[False]
    # behind the last forward step and the loss, in front of the first backward step of the chain
    assert max(i for i, n in enumerate(names[True]) if n == "attention_step_fwd") < k
    assert max(i for i, n in enumerate(names[True]) if n == "softmax_cce") < k
    first_bwd = min(i for i, n in enumerate(names[True]) if n in ("lstm_step_bwd", "attention_step_bwd"))
    assert k < first_bwd
    R = LC["R"]
    call = mock_backend.cov_calls[0]
    rows = B if axis == "time" else T
    assert (call["T"], call["B"], call["R"], call["axis"]) == (T, B, R, axis) and call["want_ext"] and call["want_out"]
    assert np.isclose(call["coef"], 2 * 0.5 / (rows * R), rtol=1e-12)
    steps = [c for c in logs[True] if c[0] == "attention_step_bwd"]
    assert len(steps) == T
    ts, bs = CO.strides(axis, R)
    ext0 = call["ext_tensor"]
    for j, c in enumerate(steps):                            # the chain runs i = T-1 .. 0
        i = T - 1 - j
        assert c[2]["ext_bs"] == bs and c[2]["ext"].data_ptr() == ext0.data_ptr() + 4 * i * ts
    assert all("ext" not in c[2] for c in logs[False] if c[0] == "attention_step_bwd")


def test_capture_key_carries_weight_and_axis(mock_backend, monkeypatch):
    rng = np.random.default_rng(6)
    keys = {}
    for name, cov in (("off", None), ("a", AttentionCoverage(0.5)), ("b", AttentionCoverage(0.25)),
                      ("c", AttentionCoverage(0.5, "batch"))):
        model, _ = attention(rng, coverage=cov)
        model.compile(Adam(1e-3, clipnorm=0.1))
        seen = []
        real_step, real_cap = model._run_step, model._run_captured
        monkeypatch.setattr(model, "_run_step", lambda run, key, fn, s=seen, r=real_step: (s.append(key), r(run, key, fn))[1])
        monkeypatch.setattr(model, "_run_captured", lambda key, fn, s=seen, r=real_cap: (s.append(key), r(key, fn))[1])
        batch = synth_batch(B, N, T, V, U, rng)
        model.train_step(batch)
        model.test_step(batch)
        keys[name] = seen
    assert keys["off"] == [("train", B, T), ("test", B, T)]
    assert keys["a"] == [("train", B, T, "coverage", 0.5, "time"), ("test", B, T, "coverage", 0.5, "time")]
    assert len({tuple(map(tuple, v)) for v in keys.values()}) == 4


# ---------------------------------------------------------------------------------------------------- steps against the oracle
@pytest.mark.parametrize("rates", [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)])
@pytest.mark.parametrize("axis", CO.AXES)
def test_train_and_test_step_against_the_oracle(mock_backend, axis, rates):
    rng = np.random.default_rng(31)
    weight = 5.0
    model, orc = attention(rng, rates=rates, coverage=AttentionCoverage(weight, axis))
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(2):
        data, tgt = synth_batch(B, N, T, V, U, rng)
        res, grads, (_, attn) = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert set(got) == {"loss", "L2", "accuracy", "attention", "coverage", "lr"}
        for k in ("loss", "L2", "attention", "coverage"):
            assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        if axis == "batch":
            assert abs(got["coverage"] - got["attention"]) <= 4 * 2.0 ** -24 * got["attention"]     # float32 rounding
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k)
    # the term moved the update: the plain oracle lands elsewhere
    theta = model.arena.theta.clone()
    mock_backend.cov_calls.clear()
    data, tgt = synth_batch(B, N, T, V, U, rng)
    res, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert set(got) == {"loss", "L2", "accuracy", "attention", "coverage"}
    for k in ("loss", "attention", "coverage"):
        assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert len(mock_backend.cov_calls) == 1 and not mock_backend.cov_calls[0]["want_ext"]        # the value-only form
    assert (model.arena.theta == theta).all()


@pytest.mark.parametrize("axis", CO.AXES)
def test_the_term_reaches_the_gradient(axis):
    """the oracle's gradient of attention/V/kernel with and without the term differ by far more than any tolerance here"""
    rng = np.random.default_rng(31)
    _, orc = attention(rng, coverage=AttentionCoverage(5.0, axis))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    (probs, attn), cache = orc.forward(data, training=True, drop=M.DropCtx(seed=11, step=0, training=True))
    on, _ = orc.backward(probs, cache, tgt)
    orc.coverage = None
    off, _ = orc.backward(probs, cache, tgt)
    k = "attention/V/kernel"
    assert np.abs(on[k] - off[k]).max() >= 100 * 2e-4 * np.abs(on[k]).max()


def test_fit_history_has_coverage(mock_backend):
    rng = np.random.default_rng(9)
    model, _ = attention(rng, coverage=AttentionCoverage(0.5))
    model.compile(Adam(1e-3, clipnorm=0.1))
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(2)]
    hist = model.fit(batches, epochs=2, verbose=0)
    assert len(hist["coverage"]) == 2 and len(mock_backend.cov_calls) == 4
    per_step = [CO.coverage(c["alpha"], "time") for c in mock_backend.cov_calls]
    assert np.isclose(hist["coverage"][0], np.mean(per_step[:2]), rtol=1e-5)
    plain, _ = attention(rng, coverage=None)
    plain.compile(Adam(1e-3, clipnorm=0.1))
    assert "coverage" not in plain.fit(batches, epochs=1, verbose=0)
