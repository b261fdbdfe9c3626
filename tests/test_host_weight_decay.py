"""Decoupled weight decay (Adam / SGD ``weight_decay=``, ``AdamW``) on the CPU through a mock backend that follows the
header definition (tests/weight_decay_oracle.py): the restatement against torch.optim.AdamW, the descriptors, the
exclusions, the per-variable table, the decaying call in the plain one's place in every update route of both caption
models, three training steps against the float64 oracle, the scheduled rate, set_weight_decay, the refusals and the
config keys.

The model-level tolerance is the existing host tests' (rtol 2e-4): three steps at lr = 1e-3 decay a weight by
3e-3 * wd relative, so these tests use wd = 0.5 (1.5e-3, seven times the tolerance) -- an update that ignored the decay
would fail them."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import SGD, SWA, Adam, AdamW, MovingAverage, check_weight_decay, weight_decay_table
from masters_thesis_amd.schedules import CosineDecay
from oracle import models as M
from oracle import ops as O
import lr_schedule_oracle as LO
from average_oracle import AverageMockBackend
from helpers import synth_batch, tiny_groups
from lr_schedule_oracle import LrScheduleMockBackend
from weight_decay_oracle import AdamWState, SGDWState, WeightDecayMockBackend, adamw_update, decay_of, sgdw_update

WD = 0.5
PLAIN = ("adam", "sgd", "dense_dw_adam")
DECAYING = {"adam": "adamw", "sgd": "sgdw", "dense_dw_adam": "dense_dw_adamw"}


class RecordingBackend(WeightDecayMockBackend, LrScheduleMockBackend, AverageMockBackend):
    """the mock with the decaying ops, the schedule's and the averaging launch; ``names`` logs every public call when it
    is called (a ``hasattr`` probe of the model's is no call)"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v):
            return v
        names = object.__getattribute__(self, "names")

        def logged(*a, **k):
            names.append(name)
            return v(*a, **k)
        return logged


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_torch_adamw():
    """float64, 5 steps, eps = 1e-30 and v bounded away from 0: keras puts eps outside the bias correction and torch
    inside it, so the two are compared where eps cannot matter; agreement 1e-12 relative"""
    rng = np.random.default_rng(3)
    lr, wd, b1, b2, eps = 1e-2, 0.3, 0.9, 0.98, 1e-30
    w0 = rng.standard_normal(50)
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    th, m, v = w0.copy(), np.zeros(50), np.zeros(50)
    plain = (w0.copy(), np.zeros(50), np.zeros(50))
    for t in range(1, 6):
        g = rng.standard_normal(50) + np.sign(rng.standard_normal(50)) * 0.5          # |g| >= ~0: v grows from the first step
        g = np.where(np.abs(g) < 0.1, 0.1, g)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        th, m, v = adamw_update(th, m, v, g, t, lr, wd, b1, b2, eps)
        assert v.min() >= 1e-4
        got, want = th, p.detach().numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (t, np.abs(got - want).max())
        # weight_decay = 0 is the plain oracle, bit for bit
        zero = adamw_update(*plain, g, t, lr, 0.0, b1, b2, eps)
        plain = O.adam_update(*plain, g, t, lr, b1, b2, eps)
        for a, b in zip(zero, plain):
            assert np.array_equal(a, b)
    th2, mo = sgdw_update(w0, np.zeros(50), g, 0.1, 0.0, 0.9)
    ref = O.sgd_momentum_update(w0, np.zeros(50), g, 0.1, 0.9)
    assert np.array_equal(th2, ref[0]) and np.array_equal(mo, ref[1])
    th3, _ = sgdw_update(w0, np.zeros(50), g, 0.1, 0.25, 0.9)
    assert np.allclose(th3, ref[0] - 0.025 * w0, rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------- the descriptors
def test_descriptor_validation():
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), True, False, "0.1", [0.1]):
        for make in (lambda v: Adam(weight_decay=v), lambda v: SGD(weight_decay=v), lambda v: AdamW(weight_decay=v)):
            with pytest.raises(ValueError):
                make(bad)
        with pytest.raises(ValueError):
            check_weight_decay(bad)
    assert Adam().weight_decay is None and SGD().weight_decay is None and Adam(weight_decay=0).weight_decay == 0.0
    assert Adam(weight_decay=np.float32(0.25)).weight_decay == 0.25 and SGD(0.1, weight_decay=1).weight_decay == 1.0
    with pytest.raises(ValueError):
        AdamW(weight_decay=None)
    o = Adam()
    o.weight_decay = 0.1
    assert o.weight_decay == 0.1
    with pytest.raises(ValueError):
        o.weight_decay = -1


def test_adamw_defaults_and_the_wrappers():
    a = AdamW()
    assert (a.kind, a.lr, a.weight_decay, a.beta_1, a.beta_2, a.epsilon, a.clipnorm) == ("adam", 0.001, 0.004, 0.9, 0.999, 1e-7, None)
    b = AdamW(1e-2, 0.1, beta_2=0.98, clipnorm=0.1)
    assert (b.lr, b.weight_decay, b.beta_2, b.clipnorm) == (1e-2, 0.1, 0.98, 0.1) and isinstance(b, Adam)
    for w in (MovingAverage(b, 0.5), SWA(b)):
        assert w.weight_decay == 0.1
        w.weight_decay = 0.2
        assert b.weight_decay == 0.2
        w.exclude_from_weight_decay(var_names=["bias"])
        assert weight_decay_table(w, ["k", "k/bias"]) == [0.2, 0.0]
        b.weight_decay = 0.1
    assert MovingAverage(SGD(0.1, weight_decay=0.3)).weight_decay == 0.3 and MovingAverage(Adam()).weight_decay is None


def test_exclude_from_weight_decay():
    names = ["dense/kernel", "dense/bias", "bn/gamma", "bn/beta", "lstm/kernel", "lstm/bias"]
    o = AdamW(weight_decay=0.1)
    assert weight_decay_table(o, names) == [0.1] * 6                        # keras's rule: everything decays
    o.exclude_from_weight_decay(var_names=["bias", "bn/"])                  # substrings
    assert weight_decay_table(o, names) == [0.1, 0, 0, 0, 0.1, 0]
    o.exclude_from_weight_decay(var_list=["lstm/kernel", "dense"])          # exact names: "dense" names no variable
    assert weight_decay_table(o, names) == [0.1, 0.1, 0.1, 0.1, 0, 0.1]     # ... and each call replaces the earlier one
    o.exclude_from_weight_decay(var_list=["dense/kernel"], var_names=["lstm"])
    assert weight_decay_table(o, names) == [0, 0.1, 0.1, 0.1, 0, 0]
    o.exclude_from_weight_decay(var_names=["/"])
    assert weight_decay_table(o, names) is None                             # nothing left to decay: the plain launches
    assert weight_decay_table(Adam(), names) is None and weight_decay_table(Adam(weight_decay=0.0), names) is None
    for bad in ("bias", [1], [None]):
        with pytest.raises(ValueError):
            o.exclude_from_weight_decay(var_names=bad)
        with pytest.raises(ValueError):
            o.exclude_from_weight_decay(var_list=bad)


def test_exclusions_raise_once_the_model_has_built_its_state():
    model = dense()
    opt = AdamW(1e-3, WD, clipnorm=0.1)
    opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)                                                      # not built yet: still allowed
    opt.exclude_from_weight_decay(var_names=["bias", "gamma"])
    model.train_step(batch())
    with pytest.raises(ValueError, match="before"):
        opt.exclude_from_weight_decay(var_names=["beta"])
    wrapped = MovingAverage(AdamW(1e-3, WD))
    model.compile(wrapped)                                                  # a built model builds the state in compile
    with pytest.raises(ValueError, match="before"):
        wrapped.exclude_from_weight_decay(var_list=["lstm/bias"])


# ---------------------------------------------------------------------------------------------------- models
B, N, T, V, U = 5, 23, 6, 13, 16
LC = dict(B=4, N=41, R=5, D=16, A=6, U=16, Et=12, V=13, T=5)
ADAM = dict(beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def dense(E=10, seed=21, **attrs):
    rng = np.random.default_rng(seed)
    model = NIC(N, U, E, V, T, 0, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    orc = M.NICDense(N, U, E, V, T, 0, 0.2, 0.2, 0.01, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    for k, v in attrs.items():
        setattr(model, k, v)
    model.orc, model.dims = orc, (B, N, T, V, U)
    return model


def attention(seed=41, **attrs):
    rng = np.random.default_rng(seed)
    d = LC
    g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
    rates = (0, 0.2, 0, 0.2, 0, 0)
    model = LcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11)
    orc = M.LcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *rates, 0.01, 0.001, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    for k, v in attrs.items():
        setattr(model, k, v)
    model.orc, model.dims = orc, (d["B"], d["N"], d["T"], d["V"], d["U"])
    return model


def batch(model=None, seed=3):
    dims = model.dims if model is not None else (B, N, T, V, U)
    return synth_batch(*dims, np.random.default_rng(seed))


@pytest.mark.parametrize("make", [dense, attention])
def test_the_table_holds_the_value_except_for_the_excluded(make):
    model = make()
    opt = AdamW(1e-3, 0.25, **ADAM)
    opt.exclude_from_weight_decay(var_names=["bias", "gamma", "beta"])
    model.compile(opt)
    assert model.seg_wd is None                                             # built with the optimizer state
    model.train_step(batch(model))
    names = list(model.arena.entries)
    assert names == model.trainable_names() or set(names) == set(model.trainable_names())
    tab = model.seg_wd.numpy()
    assert tab.dtype == np.float32 and tab.shape == (model.arena.nseg,)
    excluded = [n for n in names if any(s in n for s in ("bias", "gamma", "beta"))]
    assert excluded and len(excluded) < len(names)
    for n, e in model.arena.entries.items():
        assert tab[e.seg] == (0.0 if n in excluded else np.float32(0.25)), n
    assert np.array_equal(model.seg_wd_host, tab)
    plain = make()
    plain.compile(Adam(1e-3, weight_decay=0, **ADAM))
    plain.train_step(batch(plain))
    assert plain.seg_wd is None and plain.seg_wd_host is None


# every update route the mock offers: the fused step with its finalize launch (the mock has no tnt_adam_fin_f32, as in the
# other host tests), the unfused sequence, SGD, and the encoder's fused update (E = 512) in the first two
ROUTES = {
    "dense fused": (lambda: dense(), "adam", ["adam"]),
    "dense fused_update=False": (lambda: dense(fused_update=False), "adam", ["adam"]),
    "dense SGD": (lambda: dense(), "sgd", ["sgd"]),
    "dense SGD fused_update=False": (lambda: dense(fused_update=False), "sgd", ["sgd"]),
    "dense encoder update": (lambda: dense(E=512), "adam", ["adam", "dense_dw_adam"]),
    "dense encoder update off": (lambda: dense(E=512, fuse_enc_update=False), "adam", ["adam"]),
    "attention fused": (lambda: attention(), "adam", ["adam"]),
    "attention fused_update=False": (lambda: attention(fused_update=False), "adam", ["adam"]),
    "attention SGD": (lambda: attention(), "sgd", ["sgd"]),
}


def optimizer(kind, wd, lr=1e-3):
    if kind == "adam":
        return Adam(lr, weight_decay=wd, **ADAM) if wd != "absent" else Adam(lr, **ADAM)
    return SGD(lr, momentum=0.9, clipnorm=0.1, weight_decay=wd) if wd != "absent" else SGD(lr, momentum=0.9, clipnorm=0.1)


def updates(names):
    return [n for n in names if n in PLAIN or n in DECAYING.values()]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_issues_the_decaying_call_where_the_plain_one_was(route, mock_backend):
    make, kind, plain_calls = ROUTES[route]
    runs = {}
    for wd in ("absent", None, 0, WD):
        model = make()
        opt = optimizer(kind, wd)
        if wd == WD:
            opt.exclude_from_weight_decay(var_names=["bias"])
        model.compile(opt)
        mock_backend.names.clear()
        for s in (3, 4):
            model.train_step(batch(model, seed=s))
        runs[wd] = (list(mock_backend.names), model.arena.theta.numpy().copy())
    base_names, base_theta = runs["absent"]
    assert updates(base_names) == plain_calls * 2, (route, updates(base_names))
    for wd in (None, 0):                                     # no decay: launch for launch and bit for bit today's step
        assert runs[wd][0] == base_names and np.array_equal(runs[wd][1], base_theta), (route, wd)
    names = runs[WD][0]
    assert [DECAYING.get(n, n) for n in base_names] == names, (route, names)
    assert updates(names) == [DECAYING[n] for n in plain_calls] * 2
    assert not np.array_equal(runs[WD][1], base_theta)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_three_steps_match_the_float64_oracle(route, mock_backend):
    make, kind, _ = ROUTES[route]
    model = make()
    opt = optimizer(kind, WD)
    opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)
    orc = model.orc
    wd = decay_of(orc.p, WD, substrings=["bias"])
    state = (AdamWState(orc.p, wd, lr=1e-3, clipnorm=0.1) if kind == "adam" else
             SGDWState(orc.p, wd, lr=1e-3, momentum=0.9, clipnorm=0.1))
    rng = np.random.default_rng(5)
    for step in range(3):
        data, tgt = synth_batch(*model.dims, rng)
        res, _, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) < 3e-5 * max(1, abs(res["loss"])), (step, got, res)
        assert abs(got["L2"] - res["L2"]) < 3e-5 * max(1, abs(res["L2"]))              # the decay is no part of the metric
        for k, v in orc.p.items():
            w = model.get_weight(k)
            atol = 3e-3 * (step + 1) if k == "attention/V/bias" else (2e-5 if k == "dense_img/bias" else 3e-6)
            assert np.allclose(w, v, rtol=2e-4, atol=atol), (route, step, k, np.abs(w - v).max())
    assert [c["name"] for c in mock_backend.wd_calls if c["name"] != "dense_dw_adamw"] == [DECAYING[kind]] * 3


def test_sgdw_follows_the_definition(mock_backend):
    """one SGD step of the dense model with and without decay from the same state: theta differs by lr * wd * theta_before
    on the decayed variables and not at all on the excluded ones; the momentum is the same"""
    a, b = dense(), dense()
    a.compile(SGD(1e-2, momentum=0.9, clipnorm=0.1))
    ob = SGD(1e-2, momentum=0.9, clipnorm=0.1, weight_decay=WD)
    ob.exclude_from_weight_decay(var_names=["bias"])
    b.compile(ob)
    before = {k: b.get_weight(k).astype(np.float64) for k in b.trainable_names()}
    a.train_step(batch(a))
    b.train_step(batch(b))
    for k, w0 in before.items():
        wa, wb = a.get_weight(k).astype(np.float64), b.get_weight(k).astype(np.float64)
        want = wa - (float(np.float32(1e-2)) * (0.0 if "bias" in k else WD)) * w0
        assert np.allclose(wb, want, rtol=1e-6, atol=1e-7), (k, np.abs(wb - want).max())
        assert ("bias" in k) == bool(np.array_equal(wa, wb)), k
    assert torch.equal(a.opt_m, b.opt_m)
    assert [c["name"] for c in mock_backend.wd_calls] == ["sgdw"]


# ---------------------------------------------------------------------------------------------------- the scheduled rate
def test_the_decay_follows_the_scheduled_rate(mock_backend):
    sched = CosineDecay(1e-2, 4, alpha=0.1)
    params = LO.pack(LO.COSINE, [1e-2, 4, 0.1])
    model = dense()
    opt = AdamW(sched, WD, **ADAM)
    opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)
    orc = model.orc
    state = AdamWState(orc.p, decay_of(orc.p, WD, substrings=["bias"]), lr=1e-2, clipnorm=0.1)
    rng = np.random.default_rng(5)
    rates = []
    for step in range(4):
        data, tgt = synth_batch(*model.dims, rng)
        state.lr = float(LO.lr32(params, step))
        rates.append(state.lr)
        orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        mock_backend.names.clear()
        got = model.train_step((data, tgt)).as_floats()
        assert got["lr"] == state.lr
        names = mock_backend.names
        assert names.index("lr_schedule") < names.index("adamw")
        for k, v in orc.p.items():
            w = model.get_weight(k)
            assert np.allclose(w, v, rtol=2e-4, atol=2e-5 if k == "dense_img/bias" else 3e-6), (step, k, np.abs(w - v).max())
    assert [c["lr"] for c in mock_backend.wd_calls] == rates and len(set(rates)) == 4


# ---------------------------------------------------------------------------------------------------- set_weight_decay
def test_set_weight_decay_rewrites_the_table_in_place(mock_backend):
    model = dense()
    with pytest.raises(RuntimeError):
        model.set_weight_decay(0.1)
    opt = AdamW(1e-3, WD, **ADAM)
    opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)
    model.train_step(batch(model))
    buf, ptr = model.seg_wd, model.seg_wd.data_ptr()
    model._graphs["sentinel"] = 1
    model.set_weight_decay(0.125)
    assert model.seg_wd is buf and model.seg_wd.data_ptr() == ptr and "sentinel" in model._graphs       # no re-record
    assert opt.weight_decay == 0.125
    mock_backend.wd_calls.clear()
    model.train_step(batch(model, seed=4))
    tab = mock_backend.wd_calls[0]["wd"]
    assert sorted(set(tab)) == [0.0, 0.125] and tab == model.seg_wd_host.tolist()
    for bad in (-1.0, float("nan"), "x", True):
        with pytest.raises(ValueError):
            model.set_weight_decay(bad)
    model.set_weight_decay(0)                                # decay off: the plain launches again, recorded again
    assert model.seg_wd is None and "sentinel" not in model._graphs
    mock_backend.names.clear()
    model.train_step(batch(model, seed=5))
    assert "adam" in mock_backend.names and "adamw" not in mock_backend.names
    model._graphs["sentinel"] = 1
    model.set_weight_decay(0.25)                             # and on again
    assert "sentinel" not in model._graphs and float(model.seg_wd.max()) == 0.25
    # the encoder's fused update takes its variable's decay as a scalar argument: a new value is recorded again
    enc = dense(E=512)
    enc.compile(AdamW(1e-3, WD, **ADAM))
    enc.train_step(batch(enc))
    assert "dense_dw_adamw" in mock_backend.names
    enc._graphs["sentinel"] = 1
    enc.set_weight_decay(0.125)
    assert "sentinel" not in enc._graphs
    mock_backend.wd_calls.clear()
    enc.train_step(batch(enc, seed=4))
    assert [c["wd"] for c in mock_backend.wd_calls if c["name"] == "dense_dw_adamw"] == [[0.125]]


# ---------------------------------------------------------------------------------------------------- refusals
def test_data_parallel_refuses(mock_backend):
    model = dense()
    model.compile(AdamW(1e-3, WD))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    assert model.grad_sync is None
    other = dense()
    hook = lambda m: None
    hook.world = 2
    other.grad_sync = hook
    for opt in (AdamW(1e-3, WD), SGD(0.1, weight_decay=0.1), MovingAverage(AdamW())):
        with pytest.raises(NotImplementedError, match="data-parallel"):
            other.compile(opt)
    assert other.optimizer is None
    other.compile(Adam(1e-2, weight_decay=0))                # no decay: compiles as before
    assert other.optimizer.weight_decay == 0.0


def test_sam_refuses(mock_backend):
    model = attention()
    model.compile(AdamW(1e-3, WD, **ADAM))
    model.train_step(batch(model))
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam(batch(model))
    plain = attention()
    plain.compile(Adam(1e-3, weight_decay=0.0, **ADAM))
    plain.train_step_sam(batch(plain))


def test_agc_refuses(mock_backend):
    model = dense()
    model.compile(AdamW(1e-3, WD, **ADAM))
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc(0.02, 1e-3)
    model.enable_agc(None)
    other = dense()
    other.enable_agc(0.02, 1e-3)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.compile(AdamW(1e-3, WD, **ADAM))
    other.compile(Adam(1e-3, **ADAM))
    other.train_step(batch(other))
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.set_weight_decay(0.1)
    assert other.seg_wd is None


# ---------------------------------------------------------------------------------------------------- config.yaml
def test_config_keys():
    base = dict(optimizer="Adam", clipnorm=0.1, alpha=0.01)
    plain = cfg.build_optimizer(base)
    assert plain.weight_decay is None and weight_decay_table(plain, ["a"]) is None and type(plain) is Adam
    o = cfg.build_optimizer(dict(base, weight_decay=0.05, weight_decay_exclude=["bias", "gamma"]))
    assert type(o) is Adam and o.weight_decay == 0.05 and (o.lr, o.beta_2, o.clipnorm) == (0.0001, 0.98, 0.1)
    assert weight_decay_table(o, ["k", "k/bias", "bn/gamma"]) == [0.05, 0.0, 0.0]
    w = cfg.build_optimizer(dict(base, optimizer="AdamW"))
    assert type(w) is AdamW and w.weight_decay == 0.004 and (w.lr, w.beta_2, w.epsilon, w.clipnorm) == (0.0001, 0.98, 10.0e-9, 0.1)
    w = cfg.build_optimizer(dict(base, optimizer="AdamW", weight_decay=0.1, weight_decay_exclude=["bias"]))
    assert w.weight_decay == 0.1 and weight_decay_table(w, ["k", "b/bias"]) == [0.1, 0.0]
    s = cfg.build_optimizer(dict(base, optimizer="SGD", weight_decay=0.2))
    assert s.kind == "sgd" and s.weight_decay == 0.2 and s.lr == 0.01
    for bad in (dict(weight_decay=-1), dict(weight_decay="x"), dict(weight_decay_exclude="bias"), dict(weight_decay_exclude=7)):
        with pytest.raises(ValueError):
            cfg.build_optimizer(dict(base, **bad))
