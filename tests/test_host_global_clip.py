"""Global-norm gradient clipping (Adam / AdamW / SGD ``global_clipnorm=``) on the CPU through a mock backend that follows
the header definition (tests/global_clip_oracle.py): the restatement against torch.nn.utils.clip_grad_norm_, the
descriptors, the gclip call in the plain one's place on every update route of both caption models with exactly one
reduction launch in front of the first update, three training steps against the float64 oracle, global_grad_norm(),
the refusals and the config keys.

The model-level tolerance is the existing host tests' (rtol 2e-4).  Every parity test asserts from the oracle's own norm
that the threshold clips by at least a factor of 2.  An update that ignored global_clipnorm -- the constructor used to
swallow the argument -- takes SGD steps at least twice too large, and leaves Adam's first moment at least twice too
large (test_the_moments_show_the_global_scale, bound 1e-5): both miss by orders of magnitude."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.optimizers import SGD, SWA, Adam, AdamW, MovingAverage, check_global_clipnorm
from oracle import models as M
from average_oracle import AverageMockBackend
from global_clip_oracle import GlobalClip, GlobalClipMockBackend, clip_by_global_norm
from helpers import synth_batch
from lr_schedule_oracle import LrScheduleMockBackend
from test_host_weight_decay import ADAM as ADAM_CLIP, WD, attention, batch, dense
from weight_decay_oracle import AdamWState, SGDWState, decay_of

ADAM = {k: v for k, v in ADAM_CLIP.items() if k != "clipnorm"}
GCLIP = {"adam": "adam_gclip", "sgd": "sgd_gclip", "dense_dw_adam": "dense_dw_adam_gclip"}
UPDATES = set(GCLIP) | set(GCLIP.values()) | {"adamw", "sgdw", "dense_dw_adamw"}


class RecordingBackend(GlobalClipMockBackend, LrScheduleMockBackend, AverageMockBackend):
    """the mock with the gclip ops; ``names`` logs every public call when it is called"""

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
def test_restatement_equals_torch_clip_grad_norm():
    """float64; torch scales by c / (norm + 1e-6) clamped to 1, the definition by c / max(norm, c): at a norm of about 1
    the two agree to the 1e-6 torch adds to the norm, relative"""
    rng = np.random.default_rng(7)
    shapes = [(5, 7), (13,), (1,), (4, 3, 2)]
    raw = [rng.standard_normal(s) for s in shapes]
    total = np.sqrt(sum((g * g).sum() for g in raw))
    grads = {str(i): g / total * 1.25 for i, g in enumerate(raw)}               # global norm 1.25
    for c in (0.5, 0.1, 1.0, 1.25, 3.0):
        ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads.values()]
        for p, g in zip(ps, grads.values()):
            p.grad = torch.tensor(g, dtype=torch.float64)
        tn = float(torch.nn.utils.clip_grad_norm_(ps, c))
        got, norm = clip_by_global_norm(grads, c)
        assert abs(norm - 1.25) < 1e-12 and abs(tn - 1.25) < 1e-12
        for p, g in zip(ps, got.values()):
            want = p.grad.numpy()
            assert np.abs(g - want).max() <= 1e-6 * np.abs(want).max(), (c, np.abs(g - want).max())
        if c >= 1.25:                                                            # inside the ball: untouched, exactly
            for g0, g1 in zip(grads.values(), got.values()):
                assert np.array_equal(g0, g1)
    # an IndexedSlices norm replaces the dense one in the global norm
    got, norm = clip_by_global_norm(grads, 0.5, sparse_norms={"1": 2.0})
    want = np.sqrt(1.25 ** 2 - (grads["1"] ** 2).sum() + 4.0)
    assert abs(norm - want) < 1e-12 and np.allclose(got["0"], grads["0"] * 0.5 / want, rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------- the descriptors
MAKERS = (lambda **k: Adam(**k), lambda **k: SGD(**k), lambda **k: AdamW(**k))


def test_descriptor_validation():
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), True, False, "5.0", [5.0]):
        for make in MAKERS:
            with pytest.raises(ValueError):
                make(global_clipnorm=bad)
        with pytest.raises(ValueError):
            check_global_clipnorm(bad)
    for make in MAKERS:
        assert make().global_clipnorm is None and make(global_clipnorm=5).global_clipnorm == 5.0
        assert make(global_clipnorm=np.float32(0.25)).global_clipnorm == 0.25
        o = make()
        o.global_clipnorm = 2.5
        assert o.global_clipnorm == 2.5
        for bad in (-1, "x", True, float("nan")):
            with pytest.raises(ValueError):
                o.global_clipnorm = bad
        o.global_clipnorm = None
        assert o.global_clipnorm is None


def test_clipnorm_and_global_clipnorm_exclude_each_other():
    for make in MAKERS:
        with pytest.raises(ValueError, match="both"):
            make(clipnorm=0.1, global_clipnorm=5.0)
        o = make(clipnorm=0.1)
        with pytest.raises(ValueError, match="both"):
            o.global_clipnorm = 5.0
        assert o.global_clipnorm is None and o.clipnorm == 0.1


def test_clipvalue_is_refused_not_swallowed():
    for make in MAKERS:
        with pytest.raises(NotImplementedError, match="IndexedSlices"):
            make(clipvalue=0.5)
        assert make(clipvalue=None).global_clipnorm is None


def test_the_wrappers_delegate():
    b = Adam(1e-3, global_clipnorm=5.0)
    for w in (MovingAverage(b, 0.5), SWA(b)):
        assert w.global_clipnorm == 5.0
        w.global_clipnorm = 2.0
        assert b.global_clipnorm == 2.0
        with pytest.raises(ValueError):
            w.global_clipnorm = -1
        b.global_clipnorm = 5.0
    assert MovingAverage(SGD(0.1)).global_clipnorm is None


# ---------------------------------------------------------------------------------------------------- routes
# every update route the mock offers (it has no tnt_adam_fin_f32, as in the other host tests)
ROUTES = {
    "dense fused": (lambda: dense(), "adam", ["adam"]),
    "dense fused_update=False": (lambda: dense(fused_update=False), "adam", ["adam"]),
    "dense SGD": (lambda: dense(), "sgd", ["sgd"]),
    "dense SGD fused_update=False": (lambda: dense(fused_update=False), "sgd", ["sgd"]),
    "dense encoder update": (lambda: dense(E=512), "adam", ["adam", "dense_dw_adam"]),
    "attention fused": (lambda: attention(), "adam", ["adam"]),
    "attention fused_update=False": (lambda: attention(fused_update=False), "adam", ["adam"]),
    "attention SGD": (lambda: attention(), "sgd", ["sgd"]),
}
C = 0.02          # the global threshold of the model tests: the tests assert that it clips by a factor of 2 at least


def optimizer(kind, gclip, lr=1e-3, wd=None):
    clip = dict(global_clipnorm=gclip) if gclip is not None else dict(clipnorm=0.1)
    if kind == "adam":
        return Adam(lr, weight_decay=wd, **ADAM, **clip)
    return SGD(lr, momentum=0.9, weight_decay=wd, **clip)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_issues_the_gclip_call_where_the_plain_one_was(route, mock_backend):
    make, kind, plain_calls = ROUTES[route]
    runs = {}
    for gclip in (None, C):
        model = make()
        model.compile(optimizer(kind, gclip))
        mock_backend.names.clear()
        for s in (3, 4):
            model.train_step(batch(model, seed=s))
        runs[gclip] = list(mock_backend.names)
    base, names = runs[None], runs[C]
    assert [n for n in base if n in UPDATES] == plain_calls * 2 and "global_sqnorm" not in base
    assert [GCLIP.get(n, n) for n in base] == [n for n in names if n != "global_sqnorm"], (route, names)
    # exactly one reduction per step, in front of the step's first update call and behind the launch that filed the norms
    ups = [i for i, n in enumerate(names) if n in UPDATES]
    reds = [i for i, n in enumerate(names) if n == "global_sqnorm"]
    per_step = len(plain_calls)
    assert len(reds) == 2 and len(ups) == 2 * per_step
    for k, r in enumerate(reds):
        assert names[r + 1] in UPDATES or names[r + 1] in ("lr_schedule", "step_tick"), (route, names[r - 1:r + 3])
        assert r < ups[k * per_step] and (k == 0 or r > ups[k * per_step - 1])
        since = names[(ups[k * per_step - 1] if k else 0):r]          # the step so far (the mock's step_finalize calls step_tick)
        assert "step_finalize" in since or "seg_sqnorm" in since, (route, since[-4:])


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
@pytest.mark.parametrize("make", [dense, attention, lambda: dense(E=512), lambda: dense(fused_update=False)],
                         ids=["dense", "attention", "dense-encoder-update", "dense-unfused"])
def test_three_steps_match_the_float64_oracle(make, kind, mock_backend):
    model = make()
    wd = WD if kind == "adamw" else None
    opt = optimizer("sgd" if kind == "sgd" else "adam", C, wd=wd)
    if wd:
        opt.exclude_from_weight_decay(var_names=["bias"])
    model.compile(opt)
    with pytest.raises(RuntimeError):
        model.global_grad_norm()
    orc = model.orc
    tab = decay_of(orc.p, wd or 0.0, substrings=["bias"])
    inner = (SGDWState(orc.p, tab, lr=1e-3, momentum=0.9, clipnorm=None) if kind == "sgd" else
             AdamWState(orc.p, tab, lr=1e-3, clipnorm=None))
    state = GlobalClip(inner, C)
    rng = np.random.default_rng(5)
    for step in range(3):
        data, tgt = synth_batch(*model.dims, rng)
        res, _, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        assert state.norm >= 2 * C, (step, state.norm)                      # the threshold is active, by a factor >= 2
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) < 3e-5 * max(1, abs(res["loss"])), (step, got, res)
        assert abs(model.global_grad_norm() - state.norm) <= 2e-4 * state.norm, (step, model.global_grad_norm(), state.norm)
        for k, v in orc.p.items():
            w = model.get_weight(k)
            atol = 3e-3 * (step + 1) if k == "attention/V/bias" else (2e-5 if k == "dense_img/bias" else 3e-6)
            assert np.allclose(w, v, rtol=2e-4, atol=atol), (kind, step, k, np.abs(w - v).max())
    calls = mock_backend.gclip_calls
    assert calls and all(c["c"] == C for c in calls) and len({c["gsq"] for c in calls}) == 3
    assert abs(np.sqrt(calls[-1]["gsq"]) - state.norm) <= 2e-4 * state.norm


def test_the_moments_show_the_global_scale(mock_backend):
    """one Adam step from zero moments: m = (1 - beta_1) * cs * g for EVERY variable with the one cs, so m of the globally
    clipped model is the unclipped model's m times cs exactly (to float32 rounding) -- per-variable clipping, or none,
    misses this by the factor the test asserts"""
    a, b = dense(), dense()
    a.compile(Adam(1e-3, **ADAM))                                            # no clipping at all
    b.compile(Adam(1e-3, **ADAM, global_clipnorm=C))
    a.train_step(batch(a))
    b.train_step(batch(b))
    cs = C / max(b.global_grad_norm(), C)
    assert cs <= 0.5
    ma, mb = a.opt_m.numpy().astype(np.float64), b.opt_m.numpy().astype(np.float64)
    assert np.abs(ma).max() > 0 and np.allclose(mb, ma * cs, rtol=1e-5, atol=1e-12)


def test_assigning_the_threshold_drops_the_recordings(mock_backend):
    model = dense()
    opt = Adam(1e-3, **ADAM, global_clipnorm=C)
    model.compile(opt)
    model.train_step(batch(model))
    model._graphs["sentinel"] = 1
    model.train_step(batch(model, seed=4))
    assert "sentinel" in model._graphs                                       # nothing assigned: the recordings stay
    opt.global_clipnorm = 2 * C
    mock_backend.gclip_calls.clear()
    model.train_step(batch(model, seed=5))
    assert "sentinel" not in model._graphs and {c["c"] for c in mock_backend.gclip_calls} == {2 * C}
    model._graphs["sentinel"] = 1
    opt.global_clipnorm = None                                               # off: the plain launches again
    mock_backend.names.clear()
    model.train_step(batch(model, seed=6))
    assert "sentinel" not in model._graphs and "adam" in mock_backend.names and "global_sqnorm" not in mock_backend.names


# ---------------------------------------------------------------------------------------------------- refusals
def test_data_parallel_refuses(mock_backend):
    model = dense()
    model.compile(Adam(1e-3, global_clipnorm=5.0))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    assert model.grad_sync is None
    other = dense()
    hook = lambda m: None
    hook.world = 2
    other.grad_sync = hook
    for opt in (Adam(1e-3, global_clipnorm=5.0), SGD(0.1, global_clipnorm=1.0), MovingAverage(Adam(global_clipnorm=5.0))):
        with pytest.raises(NotImplementedError, match="data-parallel"):
            other.compile(opt)
    assert other.optimizer is None
    other.compile(Adam(1e-2, clipnorm=0.1))


def test_sam_refuses(mock_backend):
    model = attention()
    model.compile(Adam(1e-3, **ADAM, global_clipnorm=C))
    model.train_step(batch(model))
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam(batch(model))
    plain = attention()
    plain.compile(Adam(1e-3, **ADAM_CLIP))
    plain.train_step_sam(batch(plain))


def test_agc_refuses(mock_backend):
    model = dense()
    model.compile(Adam(1e-3, **ADAM, global_clipnorm=C))
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc(0.02, 1e-3)
    model.enable_agc(None)
    other = dense()
    other.enable_agc(0.02, 1e-3)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.compile(Adam(1e-3, **ADAM, global_clipnorm=C))
    opt = Adam(1e-3, **ADAM_CLIP)
    other.compile(opt)
    other.train_step(batch(other))
    opt.clipnorm = None
    opt.global_clipnorm = C                                                  # assigned behind a recorded step: found by the next
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.train_step(batch(other))


# ---------------------------------------------------------------------------------------------------- config.yaml
def test_config_keys():
    base = dict(optimizer="Adam", clipnorm=0.1, alpha=0.01)
    plain = cfg.build_optimizer(base)
    assert plain.global_clipnorm is None and plain.clipnorm == 0.1
    for conf in (dict(optimizer="Adam", alpha=0.01, global_clipnorm=5.0), dict(base, clipnorm=None, global_clipnorm=5.0)):
        o = cfg.build_optimizer(conf)
        assert type(o) is Adam and o.global_clipnorm == 5.0 and o.clipnorm is None and (o.lr, o.beta_2) == (0.0001, 0.98)
    w = cfg.build_optimizer(dict(optimizer="AdamW", alpha=0.01, global_clipnorm=2, weight_decay=0.1))
    assert type(w) is AdamW and w.global_clipnorm == 2.0 and w.weight_decay == 0.1
    s = cfg.build_optimizer(dict(optimizer="SGD", alpha=0.01, global_clipnorm=1.5))
    assert s.kind == "sgd" and s.global_clipnorm == 1.5 and s.lr == 0.01
    with pytest.raises(ValueError, match="both"):
        cfg.build_optimizer(dict(base, global_clipnorm=5.0))
    for bad in (-1, 0, "x", float("nan")):
        with pytest.raises(ValueError):
            cfg.build_optimizer(dict(optimizer="Adam", alpha=0.01, global_clipnorm=bad))
