"""Unlikelihood training on the CPU through a mock backend that follows tnt_softmax_cce_unlikely_f32's header definition
(tests/unlikelihood_oracle.py): the candidate-set rules, the float64 gradient against finite differences of the float64
loss, the launches of a step of both models with and without the feature, the compact head, the refusals, the config key
and evaluate.repeat_rate."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import evaluate
from masters_thesis_amd import think_and_tell as TT, show_and_tell as SAT
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical as SC
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam, CategoricalCrossentropy, check_unlikelihood, loss_unlikelihood
from oracle import models as M
from helpers import synth_batch, tiny_groups
from smooth_oracle import SmoothMockBackend
from ss_att_oracle import SSAttMockBackend
from test_host_naive_attention import NaiveMockBackend
from unlikelihood_oracle import (LO, UnlikelihoodMockBackend, candidates, candidate_mask, reference, ul_grad, ul_loss, ul_mean,
                                 unlikely)

B, N, T, V, U, E = 5, 23, 6, 13, 16, 16
LC = dict(R=4, D=16, A=5, Et=12)
HEAD_SCALE = 8.0       # on the vocabulary kernel: at initialisation p is near uniform


class RecordingBackend(UnlikelihoodMockBackend, SmoothMockBackend, SSAttMockBackend, NaiveMockBackend):
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


def loss_obj(alpha, **kw):
    return CategoricalCrossentropy(from_logits=False, reduction="none", unlikelihood=alpha, **kw)


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


def repeating_batch(b, rng):
    """synth_batch with words repeated inside each caption, so that most rows have candidates"""
    data, tgt = synth_batch(b, N, T, V, U, rng)
    x, cap, a0, c0 = data
    for i in range(b):
        cap[i, 1:T] = rng.integers(3, 6, T - 1)              # three words: repeats from the third position on
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    return (x, cap, a0, c0), tgt


def expected_loss(call):
    p = M.O.softmax(call["logits"])
    return ul_loss(p, call["target"], call["B"], call["T"], call["alpha"])[0].mean()


# ---------------------------------------------------------------------------------------------------- candidate sets
def test_candidate_set_rules():
    Vv = 10
    # caption 0: a duplicate (4 twice), the row's own target among the prefix (t = 3: target 4), a 0 inside the prefix,
    # ids >= V and < 0; caption 1: padding behind the end keeps the candidates
    cap0 = [4, 7, 4, 4, 0, 12, -3, 5]
    cap1 = [3, 5, 2, 0, 0, 0, 0, 0]
    Tq = len(cap0)
    tg = np.stack([cap0, cap1], 1).reshape(-1)               # t-major: row t * 2 + b
    C = candidates(tg, 2, Tq, Vv)
    c0, c1 = C[0::2], C[1::2]
    assert c0[0] == [] and c1[0] == []                       # t = 0
    assert c0[1] == [4]
    assert c0[2] == [7]                                      # target 4 is in the prefix {4, 7}: dropped
    assert c0[3] == [7]                                      # prefix 4, 7, 4: the duplicate counts once, the target goes
    assert c0[4] == [4, 7]                                   # a padding position keeps its candidates
    assert c0[5] == [4, 7]                                   # the 0 in the prefix is no candidate
    assert c0[6] == [4, 7]                                   # nor is 12 >= V
    assert c0[7] == [4, 7]                                   # nor -3
    assert c1[3] == [2, 3, 5] and c1[7] == [2, 3, 5]
    m = candidate_mask(tg, 2, Tq, Vv)
    assert m.shape == (2 * Tq, Vv) and m[2 * 4 + 0].nonzero()[0].tolist() == [4, 7] and not m[:2].any()
    # loss: a duplicate in the prefix counts once
    tg = np.array([4, 7, 4, 4, 0])                           # caption 0's valid front alone
    p = np.full((5, Vv), 1.0 / Vv)
    _, ce, ul = ul_loss(p, tg, 1, 5, 1.0)
    assert np.allclose(ul[3], -np.log(0.9)) and np.allclose(ul[4], -2 * np.log(0.9)) and ul[0] == 0


def test_gradient_against_central_differences():
    rng = np.random.default_rng(12)
    Bq, Tq, Vv = 3, 5, 9
    tg = rng.integers(1, 5, (Tq, Bq))                        # few words: many repeats
    tg[3, 1] = 0                                             # a padding position
    tg = tg.reshape(-1)
    x = rng.standard_normal((Tq * Bq, Vv)) * 2
    assert sum(len(c) for c in candidates(tg, Bq, Tq, Vv)) > 10
    gscale, h = 0.37, 1e-6
    for alpha in (0.0, 0.5, 2.0):
        p = M.O.softmax(x)
        assert (p > 1e-5).all() and (p < 1 - 1e-5).all()     # out of every clip band, also at x +- h
        g = ul_grad(p, tg, Bq, Tq, gscale, alpha)
        fd = np.zeros_like(x)
        for r in range(x.shape[0]):
            for v in range(Vv):
                xp, xm = x.copy(), x.copy()
                xp[r, v] += h; xm[r, v] -= h
                lp = ul_loss(M.O.softmax(xp), tg, Bq, Tq, alpha)[0].sum()
                lm = ul_loss(M.O.softmax(xm), tg, Bq, Tq, alpha)[0].sum()
                fd[r, v] = gscale * (lp - lm) / (2 * h)
        assert np.abs(g - fd).max() < 1e-8, (alpha, np.abs(g - fd).max())
        ref = reference(x.astype(np.float32), tg, Bq, Tq, gscale, alpha)
        assert np.allclose(ref["loss"], ul_loss(M.O.softmax(x.astype(np.float32).astype(np.float64)), tg, Bq, Tq, alpha)[0])
    # alpha = 0 and rows without candidates: the plain oracle steps
    plain = M.O.cce_softmax_bwd(p, tg, np.full(Tq * Bq, gscale))
    assert np.abs(ul_grad(p, tg, Bq, Tq, gscale, 0.0) - plain).max() < 1e-15
    assert np.abs(ul_grad(p, tg, Bq, Tq, gscale, 2.0)[:Bq] - plain[:Bq]).max() < 1e-15
    assert np.abs(ul_loss(p, tg, Bq, Tq, 0.0)[0] - M.O.cce_from_probs(p, tg)).max() < 1e-15


def test_saturated_candidate_and_target_clip():
    """m_c = 0 where 1 - p_c < 1e-7: loss term -log(1e-7), q_c = 0; m_y = 0 where the clip of ce is active"""
    Bq, Tq, Vv = 1, 2, 6
    tg = np.array([3, 2])
    x = np.zeros((2, Vv)); x[1, 3] = 40.0
    p = M.O.softmax(x)
    loss, ce, ul = ul_loss(p, tg, Bq, Tq, 0.5)
    assert np.isclose(ul[1], -np.log(LO)) and np.isclose(ce[1], -np.log(LO))
    assert (ul_grad(p, tg, Bq, Tq, 1.0, 0.5)[1] == 0).all()  # target clipped, the one candidate saturated


def test_mock_op_follows_the_restatement(mock_backend):
    rng = np.random.default_rng(10)
    Bq, Tq, Vv = 2, 4, 11
    rows, ld = Bq * Tq, Vv + 3
    x = rng.standard_normal((rows, Vv))
    tg = rng.integers(1, 4, rows)
    buf = torch.full((rows, ld), 7.0)
    buf[:, :Vv] = torch.tensor(x, dtype=torch.float32)
    x32 = buf[:, :Vv].numpy().copy()
    loss, corr = torch.zeros(rows), torch.zeros(rows)
    mock_backend.softmax_cce_unlikely(buf, torch.tensor(tg, dtype=torch.int32), None, loss, corr, buf, Bq, Tq, Vv, ld, 0.25, 0.5)
    ref = reference(x32, tg, Bq, Tq, 0.25, 0.5)
    assert np.allclose(loss.numpy(), ref["loss"], rtol=1e-6) and np.array_equal(corr.numpy(), ref["amax"] == tg)
    assert np.allclose(buf[:, :Vv].numpy(), ref["grad"], rtol=1e-6, atol=1e-9) and (buf[:, Vv:] == 7.0).all()
    assert (ref["ul"][Bq:] > 0).any()


# ---------------------------------------------------------------------------------------------------- the loss object
def test_loss_object_and_checks():
    assert CategoricalCrossentropy().unlikelihood == 0.0
    assert loss_obj(1.0).unlikelihood == 1.0 and loss_obj(0).unlikelihood == 0.0 and loss_obj(7.5).unlikelihood == 7.5
    assert check_unlikelihood(2) == 2.0 and loss_unlikelihood(None) == 0.0 and loss_unlikelihood(object()) == 0.0
    assert loss_unlikelihood(loss_obj(0.5)) == 0.5
    for bad in (-0.1, float("nan"), float("inf"), float("-inf"), "x", None):
        with pytest.raises(ValueError):
            loss_obj(bad)
        with pytest.raises(ValueError):
            check_unlikelihood(bad)


def test_compile_reads_the_loss_object(mock_backend):
    model, _ = dense(np.random.default_rng(1))
    assert model.unlikelihood == 0.0
    model.compile(Adam(1e-3), None)
    assert model.unlikelihood == 0.0
    model.compile(Adam(1e-3), object())
    assert model.unlikelihood == 0.0
    model.compile(Adam(1e-3), loss_obj(1.0))
    assert model.unlikelihood == 1.0

    class Bad:
        unlikelihood = float("inf")
    with pytest.raises(ValueError):
        model.compile(Adam(1e-3), Bad())
    assert mock_backend.names == []


# ---------------------------------------------------------------------------------------------------- alpha = 0
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_alpha_zero_issues_todays_calls(kind, mock_backend):
    make = dense if kind == "dense" else attention
    logs = []
    for loss in ("absent", None, CategoricalCrossentropy(), loss_obj(0.0)):
        rng = np.random.default_rng(2)
        model, _ = make(rng)
        if loss == "absent":
            model.compile(Adam(1e-3, clipnorm=0.1))
        else:
            model.compile(Adam(1e-3, clipnorm=0.1), loss)
        data, tgt = repeating_batch(B, rng)
        mock_backend.names.clear()
        m1 = model.train_step((data, tgt)).as_floats()
        m2 = model.test_step((data, tgt)).as_floats()
        logs.append((list(mock_backend.names), m1, m2))
    assert all(l == logs[0] for l in logs[1:])
    assert "softmax_cce_unlikely" not in logs[0][0] and logs[0][0].count("softmax_cce") == 2
    assert mock_backend.ul_calls == []


# ---------------------------------------------------------------------------------------------------- alpha > 0
@pytest.mark.parametrize("kind", ["dense", "attention"])
@pytest.mark.parametrize("world", [1, 2])
def test_one_unlikelihood_launch_per_step(kind, world, mock_backend):
    rng = np.random.default_rng(3)
    kw = {}
    if world > 1:
        hook = lambda m: None
        hook.world = world
        kw["grad_sync"] = hook
    model, orc = (dense if kind == "dense" else attention)(rng, **kw)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(1.0))
    for step in range(2):
        data, tgt = repeating_batch(B, rng)
        mock_backend.names.clear()
        mock_backend.ul_calls.clear()
        got = model.train_step((data, tgt)).as_floats()
        assert mock_backend.names.count("softmax_cce_unlikely") == 1
        assert "softmax_cce" not in mock_backend.names and "softmax_cce_live" not in mock_backend.names
        (call,) = mock_backend.ul_calls
        assert (call["B"], call["T"], call["V"], call["alpha"]) == (B, T, V, 1.0) and call["want_grad"] and not call["want_probs"]
        assert call["gscale"] == 1.0 / (T * B * world)
        assert np.array_equal(call["target"].reshape(T, B).T, tgt)
        want = expected_loss(call)
        plain = M.O.cce_from_probs(M.O.softmax(call["logits"]), call["target"]).mean()
        assert want > plain + 0.05                                      # the captions repeat: the term is there
        assert abs(got["loss"] - want) <= 2e-6 * max(1.0, want), (got["loss"], want)
    mock_backend.names.clear()
    mock_backend.ul_calls.clear()
    got = model.test_step((data, tgt)).as_floats()                      # the same objective in the evaluation form
    assert mock_backend.names.count("softmax_cce_unlikely") == 1 and "softmax_cce" not in mock_backend.names
    (call,) = mock_backend.ul_calls
    assert call["want_probs"] and not call["want_grad"] and call["gscale"] == 0.0 and call["alpha"] == 1.0
    want = expected_loss(call)
    assert abs(got["loss"] - want) <= 2e-6 * max(1.0, want)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_train_step_matches_the_patched_oracle(kind, mock_backend):
    rng = np.random.default_rng(4)
    model, orc = (dense if kind == "dense" else attention)(rng)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), loss_obj(1.0))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noise = {}
    for step in range(2):
        data, tgt = repeating_batch(B, rng)
        out = orc.forward(data, True, M.DropCtx(seed=11, step=step, training=True))[0]
        extra = 1.0 * ul_mean(out[0] if isinstance(out, tuple) else out, tgt)
        assert extra > 0.05
        with unlikely(1.0):
            res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        want = res["loss"] + extra
        assert abs(got["loss"] - want) < 2e-5 * max(1, abs(want))                       # test_host_nic's bounds
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        for k, v in orc.p.items():
            if k == "attention/V/bias":                  # zero-gradient variable: Adam amplifies rounding noise
                continue
            if grads.get(k) is not None:                 # test_gpu_nic's rule: where the gradient is rounding noise
                noise[k] = noise.get(k, 0.0) + 1e-3 * (np.abs(grads[k]) < 1e-8)   # (|g| < 1e-8), Adam steps +-lr at random
            assert (np.abs(model.get_weight(k) - v) <= 3e-6 + 2e-4 * np.abs(v) + noise.get(k, 0.0)).all(), (step, k)


def test_dense_model_leaves_the_compact_head(mock_backend):
    model, _ = dense(np.random.default_rng(5))
    model.compile(Adam(1e-3), loss_obj(1.0))
    data, tgt = repeating_batch(B, np.random.default_rng(5))
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
    model.unlikelihood = 0.0
    assert model._head_map_bufs(B, T) is not None
    model.unlikelihood = 1.0
    assert model._head_map_bufs(B, T) is None


def test_recompile_with_another_alpha_drops_the_graphs(mock_backend):
    rng = np.random.default_rng(5)
    model, _ = dense(rng)
    model.compile(Adam(1e-3), loss_obj(1.0))
    data, tgt = repeating_batch(B, rng)
    model.train_step((data, tgt))
    model._graphs["sentinel"] = "captured with alpha = 1"
    model.compile(Adam(1e-3), loss_obj(0.5))
    assert model._graphs == {} and model.unlikelihood == 0.5
    mock_backend.ul_calls.clear()
    model.train_step((data, tgt))
    assert [c["alpha"] for c in mock_backend.ul_calls] == [0.5]
    model._graphs["sentinel"] = 1
    model.compile(Adam(1e-3), None)
    assert model._graphs == {} and model.unlikelihood == 0.0


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
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(1.0))
    data, tgt = repeating_batch(b, rng)
    mock_backend.names.clear()
    got = getattr(model, method)((data, tgt)).as_floats()
    n = 2 if method == "train_step_sam" else 1            # SAM: the loss at w and at w + e(w)
    assert mock_backend.names.count("softmax_cce_unlikely") == n
    assert len(mock_backend.ul_calls) == n and all(c["alpha"] == 1.0 and c["want_grad"] for c in mock_backend.ul_calls)
    assert "softmax_cce" not in mock_backend.names
    # the prefix is the ground truth in the targets, whatever was fed
    assert all(np.array_equal(c["target"].reshape(T, b).T, tgt) and (c["B"], c["T"]) == (b, T) for c in mock_backend.ul_calls)
    wants = [expected_loss(c) for c in mock_backend.ul_calls]
    assert any(abs(got["loss"] - w) <= 2e-6 * max(1.0, w) for w in wants), (got["loss"], wants)
    if path == "ms2 S=2":                                  # the per-subject losses read loss_row
        (c,) = mock_backend.ul_calls
        rows = ul_loss(M.O.softmax(c["logits"]), c["target"], b, T, 1.0)[0].reshape(T, b)
        for q in range(2):
            want = rows[:, q * 3:(q + 1) * 3].mean()
            assert abs(got["loss" + "AB"[q]] - want) <= 2e-6 * max(1.0, want), (q, got, want)


def test_agc_step_inherits_the_feature(mock_backend):
    rng = np.random.default_rng(8)
    model, _ = dense(rng)
    model.enable_agc(0.02, 1e-3)
    model.compile(Adam(1e-3, clipnorm=0.1), loss_obj(1.0))
    data, tgt = repeating_batch(B, rng)
    mock_backend.names.clear()
    model.train_step((data, tgt))
    assert mock_backend.names.count("softmax_cce_unlikely") == 1 and "softmax_cce" not in mock_backend.names


# ---------------------------------------------------------------------------------------------------- refusals
def test_refused_together_with_label_smoothing(mock_backend):
    model, _ = dense(np.random.default_rng(1))
    with pytest.raises(ValueError, match="label_smoothing"):
        model.compile(Adam(1e-3), loss_obj(1.0, label_smoothing=0.1))
    assert model.unlikelihood == 0.0 and model.label_smoothing == 0.0 and model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(0.0, label_smoothing=0.1))
    model.compile(Adam(1e-3), loss_obj(1.0))
    assert mock_backend.names == []


def test_self_critical_refuses_before_any_launch(mock_backend):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, self_critical=SC(2))
    with pytest.raises(ValueError, match="unlikelihood"):
        model.compile(Adam(1e-3), loss_obj(1.0))
    assert model.unlikelihood == 0.0 and model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(0.0))
    assert mock_backend.names == []


@pytest.mark.parametrize("kind", ["think_and_tell", "show_and_tell", "fc"])
def test_models_with_another_loss_refuse(kind, mock_backend):
    if kind == "show_and_tell":
        model = SAT.CaptionGenerator(SAT.Encoder(E), SAT.Decoder(E, U, V), None, T, device="cpu", seed=11)
    elif kind == "think_and_tell":
        model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                    None, T, device="cpu", seed=11)
    else:
        model = NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    with pytest.raises(NotImplementedError, match="unlikelihood"):
        model.compile(Adam(1e-3), loss_obj(1.0))
    assert model.optimizer is None
    model.compile(Adam(1e-3), loss_obj(0.0))
    model.compile(Adam(1e-3))
    assert mock_backend.names == []


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_more_than_64_loss_positions_is_refused_at_the_first_step(kind, mock_backend):
    rng = np.random.default_rng(9)
    Tl = 65
    if kind == "dense":
        model = NIC(N, U, E, V, Tl, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    else:
        g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
        model = LcNIC(g, U, 512, LC["Et"], LC["A"], V, Tl, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11)
    model.compile(Adam(1e-3), loss_obj(1.0))                 # compile does not know the caption length yet
    data, tgt = synth_batch(2, N, Tl, V, U, rng)
    mock_backend.names.clear()
    with pytest.raises(ValueError, match="64"):
        model.train_step((data, tgt))
    with pytest.raises(ValueError, match="64"):
        model.test_step((data, tgt))
    assert mock_backend.names == [] and mock_backend.ul_calls == []          # refused in front of every launch


# ---------------------------------------------------------------------------------------------------- config, evaluate
def _config(**extra):
    c = dict(top_k=V - 1, units=U, embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], max_length=T,
             dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
             input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", clipnorm=0.1, alpha=1e-4)
    c.update(extra)
    return c


def test_build_model_config_key(mock_backend):
    rng = np.random.default_rng(8)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    assert cfg.build_model(_config(), g, device="cpu").unlikelihood == 0.0
    m = cfg.build_model(_config(unlikelihood=1.0), g, device="cpu")
    assert m.unlikelihood == 1.0 and m.loss.unlikelihood == 1.0 and m.label_smoothing == 0.0
    with pytest.raises(ValueError):
        cfg.build_model(_config(unlikelihood=-1.0), g, device="cpu")
    with pytest.raises(ValueError):
        cfg.build_model(_config(unlikelihood=1.0, label_smoothing=0.1), g, device="cpu")
    with pytest.raises(NotImplementedError):
        cfg.build_model(_config(unlikelihood=1.0), None, mode="fc", input_size=N, device="cpu")
    assert mock_backend.names == []


def test_repeat_rate():
    rr = evaluate.repeat_rate
    assert rr([]) == 0.0 and rr([[]]) == 0.0
    assert rr([["a", "dog", "on", "grass"]]) == 0.0
    assert rr([["a", "dog", "a", "dog", "a"]]) == 3 / 5            # positions 2, 3, 4 repeat
    assert rr([["a", "a"], ["b", "c", "d", "b"]]) == 2 / 6
    assert rr(np.array([[3, 4, 3, 5], [6, 6, 6, 6]])) == 4 / 8     # id arrays
    assert rr([(1, 2), (1, 2)]) == 0.0                            # the same words in two captions repeat nothing
