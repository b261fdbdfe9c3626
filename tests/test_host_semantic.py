"""The sentence-embedding target (nic.NIC(semantic=SemanticTarget(...))) on the CPU through a mock backend that follows the
header text of tnt_cosine_loss_f32 / tnt_row_inv_norm_f32 / tnt_cosine_topk_f32 (tests/semantic_oracle.py): the float64
restatement and the oracle model against central differences, validation and the config key, every refusal, semantic=None
against the model built without the argument (arena offsets, launch list, a fifth input ignored), the launch order with the
term on, three training steps / test_step / predict_embedding against the oracle model under two optimizer combinations, the
checkpoint round trips, the generators' fifth element, and the ranks of semantic_identification."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp, evaluate
from masters_thesis_amd.data import DataGenerator, SyntheticGenerator, Tokenizer
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical, SemanticTarget
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam, AdamW, CategoricalCrossentropy
from oracle import models as M
from helpers import synth_batch, tiny_groups
import semantic_oracle as SO
from distill_oracle import DistillMockBackend
from finetune_oracle import FinetuneMockBackend

B, N, T, V, U, E, G = 5, 23, 6, 13, 16, 12, 7


class RecordingBackend(SO.SemanticMockBackend, FinetuneMockBackend, DistillMockBackend):
    """the mock with every public call logged in ``calls`` as (name, args, kwargs)"""

    def __init__(self):
        self.calls = []
        super().__init__()

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v) or name == "calls":
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


def dense(rng, rates=(0, 0, 0), sem=SemanticTarget(G, 0.7, 0.02), with_arg=True, **kw):
    args = (N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5)
    if with_arg:
        kw["semantic"] = sem
    model = NIC(*args, device="cpu", seed=11, **kw)
    if sem is not None:
        orc = SO.SemanticNIC(*args).configure(sem.dim, sem.weight, sem.reg)
    else:
        orc = M.NICDense(*args)
    orc.init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def batch5(rng, dtype=np.float32, zero_row=None):
    data, tgt = synth_batch(B, N, T, V, U, rng, dtype=dtype)
    g = rng.standard_normal((B, G)).astype(dtype)
    if zero_row is not None:
        g[zero_row] = 0
    return data + (g,), tgt


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_against_central_differences():
    """cosine_loss's dz is the gradient of gscale * sum_b loss_b in z, above and below the epsilon, and through z = x W +
    bias the gradients of W, bias and x follow"""
    rng = np.random.default_rng(3)
    Bb, Ee, Gg, gscale = 4, 5, 6, 0.3
    x, W, bias = rng.standard_normal((Bb, Ee)), rng.standard_normal((Ee, Gg)) * 0.5, rng.standard_normal(Gg) * 0.1
    g = rng.standard_normal((Bb, Gg))
    g[1] = 0                                         # a missing embedding: cos = 0, loss = 1, no gradient
    i = dict(x=x, W=W, bias=bias)

    def scalar(**over):
        a = {**i, **over}
        return gscale * SO.cosine_loss(a["x"] @ a["W"] + a["bias"], g)[0].sum()
    loss, cos, dz = SO.cosine_loss(x @ W + bias, g, gscale)
    assert cos[1] == 0 and loss[1] == 1 and not dz[1].any()
    zn, gn = (x @ W + bias) / np.linalg.norm(x @ W + bias, axis=1)[:, None], g / np.maximum(np.linalg.norm(g, axis=1), 1e-6)[:, None]
    assert np.allclose(cos, (zn * gn).sum(1))
    got = dict(x=dz @ W.T, W=x.T @ dz, bias=dz.sum(0))
    h = 1e-6
    for name in ("x", "W", "bias"):
        fd = np.zeros_like(i[name])
        for idx in np.ndindex(i[name].shape):
            p_, m_ = i[name].copy(), i[name].copy()
            p_[idx] += h; m_[idx] -= h
            fd[idx] = (scalar(**{name: p_}) - scalar(**{name: m_})) / (2 * h)
        assert np.abs(got[name] - fd).max() <= 1e-7 * max(np.abs(fd).max(), 1.0), name
    # below the epsilon the normaliser is the constant 1e-6: cos = z . gn / 1e-6 is linear in z
    z0 = np.full((1, Gg), 1e-9)
    _, c0, d0 = SO.cosine_loss(z0, g[:1], 1.0)
    gn0 = g[0] / np.linalg.norm(g[0])
    assert np.allclose(d0[0], -gn0 / 1e-6, rtol=1e-12) and np.isclose(c0[0], (z0[0] * gn0).sum() / 1e-6)
    _, _, dzero = SO.cosine_loss(np.zeros((1, Gg)), g[:1], 1.0)
    assert np.isfinite(dzero).all() and np.allclose(dzero[0], -gn0 / 1e-6)
    assert np.allclose(SO.row_inv_norm(np.array([[3.0, 4.0], [0.0, 0.0]])), [0.2, 1e6])


def test_selection_order_of_the_restatement():
    nan, inf = np.nan, np.inf
    c = np.array([[1.0, nan, 3.0, -inf, 3.0, inf, -0.0, 0.0, nan]], np.float32)
    idx, val = SO.topk(c, 9)
    assert idx.tolist() == [[5, 2, 4, 0, 6, 7, 3, 1, 8]]
    assert np.signbit(val[0, 4]) and not np.signbit(val[0, 5])
    S = np.array([[3.0, 1e-30]], np.float32)
    got = SO.similarity_f32(S, np.array([1e-20], np.float32), np.array([1e20, 1e20], np.float32))
    assert got[0, 0] == np.float32(np.float32(np.float32(3.0) * np.float32(1e-20)) * np.float32(1e20))
    assert got[0, 1] == 0.0                         # (S * qinv) underflows first: the order of the two products is visible


def test_oracle_model_gradient_against_central_differences():
    """SemanticNIC.backward differentiates scalar_loss = CE + L2 + weight * semantic, with the feature Dropout on"""
    rng = np.random.default_rng(21)
    _, orc = dense(rng, rates=(0.1, 0.2, 0.2))
    data, tgt = batch5(rng, np.float64, zero_row=2)
    drop = M.DropCtx(seed=11, step=0, training=True)
    probs, cache = orc.forward(data, training=True, drop=drop)
    grads, _ = orc.backward(probs, cache, tgt)
    plain, _ = M.NICDense.backward(orc, probs, cache, tgt)
    h = 1e-6
    for k in SO.NAMES + ("batch_norm/gamma", "batch_norm/beta", "dense_img/bias", "dense_img/kernel", "lstm/kernel"):
        w0 = orc.p[k]
        for idx in list(np.ndindex(w0.shape))[:4]:
            vals = []
            for sgn in (1, -1):
                w = w0.copy(); w[idx] += sgn * h
                orc.p[k] = w
                vals.append(orc.scalar_loss(data, tgt, drop))
            orc.p[k] = w0
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(grads[k][idx] - fd) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (k, idx, grads[k][idx], fd)
    # the term is visible where the GPU test looks, and nowhere behind the feature row
    assert np.abs(grads["batch_norm/gamma"] - plain["batch_norm/gamma"]).max() > 1e-6
    assert np.array_equal(grads["lstm/kernel"], plain["lstm/kernel"])


# ---------------------------------------------------------------------------------------------------- the public surface
def test_validation_and_config_key():
    s = SemanticTarget()
    assert (s.dim, s.weight, s.reg) == (512, 1.0, 0.0)
    assert SemanticTarget(8, 0.5, 0.1) == SemanticTarget(8, 0.5, 0.1) and SemanticTarget(8, 0.5) != SemanticTarget(8, 0.6)
    for bad in (0, 2049, -3, 1.5, "8", None, True):
        with pytest.raises(ValueError, match="dim"):
            SemanticTarget(bad)
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            SemanticTarget(8, bad)
        with pytest.raises(ValueError, match="reg"):
            SemanticTarget(8, 1.0, bad)
    assert SemanticTarget(2048, 0).weight == 0
    with pytest.raises(ValueError, match="SemanticTarget"):
        NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", semantic=True)
    base = dict(units=U, embedding_features=512, embedding_text=E, attn_units=5, top_k=V - 1, max_length=T,
                dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
                input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3, clipnorm=0.1,
                decay=0)
    assert cfg.build_model(base, None, mode="dense", input_size=N, device="cpu").semantic is None
    m = cfg.build_model({**base, "semantic": {"dim": G, "weight": 0.25, "reg": 0.5}}, None, mode="dense", input_size=N,
                        device="cpu")
    assert m.semantic == SemanticTarget(G, 0.25, 0.5) and m.arena.entries["guse_out/kernel"].l2 == 0.5
    assert m.arena.entries["guse_out/bias"].l2 == 0
    assert cfg.build_model({**base, "semantic": {}}, None, mode="dense", input_size=N, device="cpu").semantic == SemanticTarget()
    for bad in ({"l2": 1.0}, 0.5, "yes", {"dim": 0}, True):
        with pytest.raises(ValueError):
            cfg.build_model({**base, "semantic": bad}, None, mode="dense", input_size=N, device="cpu")
    g = (tiny_groups(N, 4, np.random.default_rng(1)), [16] * 4)
    for mode, kw in (("attention", {}), ("fc", dict(input_size=N))):
        with pytest.raises(NotImplementedError, match="semantic"):
            cfg.build_model({**base, "semantic": {"dim": G}}, g, mode=mode, device="cpu", **kw)


def test_layer_shapes_and_initialisation():
    rng = np.random.default_rng(1)
    args = (N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5)
    on, off = NIC(*args, device="cpu", seed=11, semantic=SemanticTarget(G, 1.0, 0.5)), NIC(*args, device="cpu", seed=11)
    assert list(on.layers_spec)[-1] == "guse_out" and list(on.layers_spec)[:-1] == list(off.layers_spec)
    assert on.layers_spec["guse_out"] == ["kernel", "bias"]
    assert on.keras_shapes["guse_out/kernel"] == (E, G) and on.keras_shapes["guse_out/bias"] == (G,)
    k = on.get_weight("guse_out/kernel")
    lim = np.sqrt(6.0 / (E + G))
    assert k.shape == (E, G) and np.abs(k).max() <= lim and np.abs(k).max() > 0.7 * lim and abs(k.mean()) < 0.3 * lim
    assert not on.get_weight("guse_out/bias").any() and on.get_layer("guse_out").trainable
    # the rows are padded to a multiple of 4 as the head's are, and the pad holds zeros
    e = on.arena.entries["guse_out/kernel"]
    assert on.ldG == 8 and tuple(e.shape) == (E, 8) and not on.arena.p("guse_out/kernel").view(E, 8)[:, G:].any()
    # the model without the layer keeps its arena and its initial values; the two variables sit behind every entry
    assert list(on.arena.entries)[:-2] == list(off.arena.entries) and tuple(list(on.arena.entries)[-2:]) == SO.NAMES
    for n, ent in off.arena.entries.items():
        assert (on.arena.entries[n].off, on.arena.entries[n].seg) == (ent.off, ent.seg), n
        assert np.array_equal(on.get_weight(n), off.get_weight(n)), n
    assert on.count_params() == off.count_params() + E * G + G
    data, tgt = batch5(rng)
    l2 = lambda m: m.test_step((data, tgt)).as_floats()["L2"]
    want = 0.5 * (on.get_weight("guse_out/kernel").astype(np.float64) ** 2).sum()
    assert abs((l2(on) - l2(off)) - want) <= 1e-5 * want


def test_every_refusal(mock_backend):
    rng = np.random.default_rng(2)
    s = SemanticTarget(G)
    for kw, what in ((dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                     (dict(self_critical=SelfCritical(end_id=2)), "self_critical"),
                     (dict(grad_sync=lambda m: None), "data-parallel")):
        with pytest.raises(NotImplementedError, match=what):
            NIC(N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", semantic=s, **kw)
    # constructors that do not know the keyword refuse it by name
    with pytest.raises(TypeError, match="semantic"):
        NICfc(N, U, 16, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", semantic=s)
    g = (tiny_groups(N, 4, np.random.default_rng(100)), [16] * 4)
    with pytest.raises(TypeError, match="semantic"):
        LcNIC(g, U, 512, E, 5, V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", semantic=s)
    model, _ = dense(rng)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batch = batch5(rng)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc()
    model.enable_agc(None)                                   # switching it off is no request for it
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    model.grad_sync = lambda m: None                          # attached behind the constructor's back
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.train_step(batch)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.test_step(batch)
    model.grad_sync = None
    for call in (lambda: model.freeze("lstm"), lambda: model.set_lr_multipliers({"guse_out": 0.5}),
                 lambda: model.compile(Adam(1e-3), freeze=["emb_text"])):
        with pytest.raises(NotImplementedError, match="semantic"):
            call()
    acc, _ = dense(rng)
    with pytest.raises(NotImplementedError, match="semantic"):
        acc.compile(Adam(1e-3, clipnorm=0.1, gradient_accumulation_steps=2))
        acc.train_step(batch)
    student, _ = dense(rng)
    teacher, _ = dense(rng, sem=None)
    with pytest.raises(NotImplementedError, match="semantic"):
        student.set_teacher(teacher)
    with pytest.raises(NotImplementedError, match="semantic"):
        student.compile(Adam(1e-3), CategoricalCrossentropy(distillation=dict(alpha=0.5, temperature=2.0)))
        student.train_step(batch)
    # the fifth input: missing or wrongly shaped raises in front of every launch
    model.compile(Adam(1e-3, clipnorm=0.1))
    for bad in (batch[0][:4], batch[0][:4] + (batch[0][4][:, :-1],), batch[0][:4] + (batch[0][4][:-1],),
                batch[0][:4] + (None,)):
        for step in (model.train_step, model.test_step):
            with pytest.raises(ValueError, match="guse"):
                step((bad, batch[1]))
    assert mock_backend.names == []                          # nothing was launched by any of them
    plain, _ = dense(rng, sem=None)
    with pytest.raises(ValueError, match="semantic"):
        plain.predict_embedding(batch[0][0])


# ---------------------------------------------------------------------------------------------------- launches
def norm(x):
    """a call argument by value; a tensor by shape and dtype (two models own different buffers)"""
    if isinstance(x, torch.Tensor):
        return ("tensor", tuple(x.shape), str(x.dtype))
    if isinstance(x, (tuple, list)):
        return tuple(norm(y) for y in x)
    if isinstance(x, dict):
        return tuple(sorted((k, norm(v)) for k, v in x.items()))
    return x


@pytest.mark.parametrize("rates", [(0, 0, 0), (0.1, 0.2, 0.2)])
def test_none_is_the_model_without_the_argument(mock_backend, rates):
    """the same arena offsets, the same backend methods with the same arguments (tensors by shape and dtype) and the same
    metrics, in train_step, test_step and a greedy decode; the batch carries a fifth input, which is ignored"""
    logs = []
    for kw in (dict(with_arg=False), dict(with_arg=True)):
        rng = np.random.default_rng(6)
        model, _ = dense(rng, rates=rates, sem=None, **kw)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = batch5(rng)
        mock_backend.calls.clear()
        m1 = model.train_step(batch).as_floats()
        m2 = model.test_step(batch).as_floats()
        x, _, a0, c0 = batch[0][:4]
        probs = model.greedy_predict(x, a0, c0, np.ones(B, np.int64), 3)
        assert not hasattr(model, "sem_g") and model.semantic is None and "semantic" not in m1 and "semantic" not in m2
        offs = [(n, e.off, e.seg) for n, e in model.arena.entries.items()]
        logs.append(([(n, norm(a), norm(k_)) for n, a, k_ in mock_backend.calls], m1, m2, probs.tolist(), offs,
                     model.arena.total, sorted(map(str, model._graphs))))
    assert logs[1] == logs[0]
    names = [c[0] for c in logs[0][0]]
    assert "cosine_loss" not in names


@pytest.mark.parametrize("rates", [(0, 0, 0), (0.1, 0.2, 0.2)])
def test_feature_on_launch_order(mock_backend, rates):
    """on top of the plain step: the product and the loss launch behind the encoder tail (the launch that writes the feature
    rows), the layer's gradient behind the loss launch, and the accumulating dx product between the writer of dXin and the
    tail backward; everything else is the plain step's list"""
    logs = {}
    for on in (False, True):
        rng = np.random.default_rng(6)
        model, _ = dense(rng, rates=rates, sem=SemanticTarget(G, 0.7) if on else None)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = batch5(rng)
        model.train_step(batch)
        mock_backend.calls.clear()
        model.train_step(batch)
        logs[on] = list(mock_backend.calls)
    names = {k: [c[0] for c in v] for k, v in logs.items()}
    calls = logs[True]
    kl = names[True].index("cosine_loss")
    assert names[True].count("cosine_loss") == 1 and names[True][kl - 1] == "gemm"
    fwd = calls[kl - 1]
    assert fwd[1][2].data_ptr() == model.sem_z.data_ptr() and fwd[1][3:6] == (B, G, E)
    assert fwd[1][0].data_ptr() == model._route.xin_used.data_ptr() and fwd[2]["bias"] is not None
    tail = max(i for i, n in enumerate(names[True][:kl]) if n.startswith("enc_tail_fwd") or n in ("batchnorm_fwd", "bn_fwd"))
    assert tail < kl - 1
    la = calls[kl][1]
    assert la[0].data_ptr() == la[4].data_ptr() == model.sem_z.data_ptr() and la[2].data_ptr() == model.sem_g.data_ptr()
    assert la[7].data_ptr() == model.met[6:7].data_ptr() and la[8:10] == (B, G) and la[10] == pytest.approx(0.7 / B)
    # dW (x^T dz, then the bias gradient's column sums), and dx accumulated into dXin[:B]
    dw = [i for i, c in enumerate(calls) if c[0] == "gemm" and c[1][2].data_ptr() == model.arena.g("guse_out/kernel").data_ptr()]
    assert len(dw) == 1 and dw[0] > kl and calls[dw[0]][2].get("transA") and names[True][dw[0] + 1] == "colsum"
    assert calls[dw[0] + 1][1][1].data_ptr() == model.arena.g("guse_out/bias").data_ptr()
    dx = [i for i, c in enumerate(calls) if c[0] == "gemm" and c[2].get("accumulate")]
    assert len(dx) == 1 and calls[dx[0]][1][2].data_ptr() == model.dXin.data_ptr() and calls[dx[0]][1][3:6] == (B, E, G)
    writer = [i for i, c in enumerate(calls) if c[0] == "gemm" and not c[2].get("accumulate")
              and c[1][2].data_ptr() == model.dXin.data_ptr()]
    reader = [i for i, n in enumerate(names[True]) if n.startswith("enc_tail_bwd") or n in ("batchnorm_bwd", "bn_bwd")]
    assert len(writer) == 1 and reader and writer[0] < dx[0] < min(reader)
    extra = {kl - 1, kl, dw[0], dw[0] + 1, dx[0]}
    assert [n for i, n in enumerate(names[True]) if i not in extra] == names[False]
    # the step key tells the two apart
    assert any("semantic" in k for k in model._graphs if isinstance(k, tuple)) or not model._graphs
    # test_step: the product and the loss launch alone, no gradient
    mock_backend.calls.clear()
    model.test_step(batch)
    assert mock_backend.names.count("cosine_loss") == 1 and not any(c[2].get("accumulate") for c in mock_backend.calls)
    assert [c for c in mock_backend.calls if c[0] == "cosine_loss"][0][1][4] is None


# ---------------------------------------------------------------------------------------------------- against the oracle
OPTIMIZERS = {
    "adam-clipnorm": (lambda: Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), None),
    "adamw-global": (lambda: AdamW(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, weight_decay=0.05,
                                   global_clipnorm=0.05), (0.05, 0.05)),
}


def oracle_update(orc, opt, grads, sparse, decoupled):
    """AdamState.apply, or (``decoupled`` = (weight_decay, global_clipnorm)) the AdamW + global-norm form: one norm over every
    gradient -- the Embedding by its un-merged rows, as the per-variable clip does -- and theta -= lr * wd * theta"""
    if decoupled is None:
        opt.apply(orc.p, grads, sparse)
        return
    wd, gclip = decoupled
    sq = sum(sparse[k] ** 2 if k in sparse else (g * g).sum() for k, g in grads.items())
    scale = gclip / max(np.sqrt(sq), gclip)
    w0 = {k: orc.p[k].copy() for k in grads}
    clip, opt.clipnorm = opt.clipnorm, None
    opt.apply(orc.p, {k: g * scale for k, g in grads.items()})
    opt.clipnorm = clip
    for k in grads:
        orc.p[k] = orc.p[k] - opt.lr * wd * w0[k]


@pytest.mark.parametrize("rates", [(0, 0, 0), (0.1, 0.2, 0.2)])
@pytest.mark.parametrize("opt_name", sorted(OPTIMIZERS))
def test_three_training_steps_against_the_oracle(mock_backend, rates, opt_name):
    rng = np.random.default_rng(31)
    model, orc = dense(rng, rates=rates)
    make, decoupled = OPTIMIZERS[opt_name]
    model.compile(make())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    lam = lambda k: model.arena.entries[k].l2
    for step in range(3):
        data, tgt = batch5(rng, zero_row=1 if step == 1 else None)
        w0 = {k: v.copy() for k, v in orc.p.items()}
        drop = M.DropCtx(seed=11, step=step, training=True)
        probs, cache = orc.forward(data, training=True, drop=drop)
        ce, acc = orc.metrics(probs, tgt)
        res = dict(loss=ce, L2=orc.l2_loss(), accuracy=acc, semantic=orc.semantic(cache))
        grads, sparse = orc.backward(probs, cache, tgt)
        oracle_update(orc, opt, grads, sparse, decoupled)
        orc.p["batch_norm/moving_mean"], orc.p["batch_norm/moving_variance"] = cache["new_mm"], cache["new_mv"]
        got = model.train_step((data, tgt)).as_floats()
        assert set(got) == {"loss", "L2", "accuracy", "semantic"}
        for k in ("loss", "L2", "semantic"):
            assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) <= 1e-6
        for k in M.NICDense.TRAINABLE + list(SO.NAMES):
            g = model.get_gradient(k) + 2 * lam(k) * w0[k]
            assert np.abs(g - grads[k]).max() <= 2e-5 * np.abs(grads[k]).max() + 1e-9, (step, k, np.abs(g - grads[k]).max())
        for k, v in orc.p.items():
            assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k)
    theta = model.arena.theta.clone()
    data, tgt = batch5(rng)
    res, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert set(got) == {"loss", "L2", "accuracy", "semantic"}
    for k in ("loss", "L2", "semantic"):
        assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert (model.arena.theta == theta).all()
    # predict_embedding: the inference encoder and the one product; no decoder step
    mock_backend.calls.clear()
    z = model.predict_embedding(data[0])
    want = orc.embed(data[0].astype(np.float64))
    assert tuple(z.shape) == (B, G) and z.dtype == torch.float32
    assert np.abs(z.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert not any(n.startswith(("lstm", "embedding", "softmax")) for n in mock_backend.names), mock_backend.names
    assert mock_backend.names.count("gemm") == 2


def test_weight_zero_reports_the_value_and_leaves_the_step_alone(mock_backend):
    """weight 0: the metric is reported, the term's gradient is zero and every shared variable moves as in the plain model"""
    rng = np.random.default_rng(41)
    on, _ = dense(rng, sem=SemanticTarget(G, 0.0))
    off, _ = dense(np.random.default_rng(41), sem=None)
    for k in off.keras_shapes:
        off.set_weight(k, on.get_weight(k))
    on.compile(Adam(1e-3, clipnorm=0.1)); off.compile(Adam(1e-3, clipnorm=0.1))
    data, tgt = batch5(rng)
    got = on.train_step((data, tgt)).as_floats()
    off.train_step((data[:4], tgt))
    assert 0 < got["semantic"] < 2 and not on.get_gradient("guse_out/kernel").any()
    for k in off.keras_shapes:
        assert np.array_equal(on.get_weight(k), off.get_weight(k)), k


# ---------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("ext", ["npz", "h5"])
def test_checkpoint_round_trip_and_old_checkpoint(tmp_path, ext):
    model, _ = dense(np.random.default_rng(71))
    path = str(tmp_path / f"w.{ext}")
    model.save_weights(path)
    other, _ = dense(np.random.default_rng(72))
    assert not np.array_equal(other.get_weight("guse_out/kernel"), model.get_weight("guse_out/kernel"))
    other.load_weights(path)
    for k in model.keras_shapes:
        assert np.array_equal(other.get_weight(k), model.get_weight(k)), k
    # a checkpoint of the model without the layer: everything else loads, the layer keeps its initialisation
    plain, _ = dense(np.random.default_rng(73), sem=None)
    old = str(tmp_path / f"old.{ext}")
    plain.save_weights(old)
    fresh = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, semantic=SemanticTarget(G))
    init = {k: fresh.get_weight(k).copy() for k in SO.NAMES}
    fresh.load_weights(old, by_name=True, skip_mismatch=True)
    for k in plain.keras_shapes:
        assert np.array_equal(fresh.get_weight(k), plain.get_weight(k)), k
    for k in SO.NAMES:
        assert np.array_equal(fresh.get_weight(k), init[k]), k
    # and the other way round: the plain model ignores the layer of a new checkpoint
    plain.load_weights(path, by_name=True, skip_mismatch=True)
    assert np.array_equal(plain.get_weight("lstm/kernel"), model.get_weight("lstm/kernel"))


# ---------------------------------------------------------------------------------------------------- generators
def test_generators_fifth_element():
    for idx in (0, 3):
        a = SyntheticGenerator(4, B, N, U, T, V, seed=9)[idx]
        b = SyntheticGenerator(4, B, N, U, T, V, seed=9, guse_dim=G)[idx]
        assert len(a[0]) == 4 and len(b[0]) == 5
        for x, y in zip(a[0], b[0][:4]):                    # every existing array keeps its bits
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert np.array_equal(a[1], b[1])
        g = b[0][4]
        assert g.shape == (B, G) and g.dtype == np.float32 and np.allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-6)
        assert np.array_equal(g, SyntheticGenerator(4, B, N, U, T, V, seed=9, guse_dim=G)[idx][0][4])
    assert not np.array_equal(SyntheticGenerator(4, B, N, U, T, V, seed=9, guse_dim=G)[0][0][4],
                              SyntheticGenerator(4, B, N, U, T, V, seed=9, guse_dim=G)[1][0][4])
    assert not np.array_equal(SyntheticGenerator(4, B, N, U, T, V, seed=9, guse_dim=G)[0][0][4],
                              SyntheticGenerator(4, B, N, U, T, V, seed=10, guse_dim=G)[0][0][4])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="guse_dim"):
            SyntheticGenerator(4, B, N, U, T, V, guse_dim=bad)
    tok = Tokenizer(num_words=V, oov_token="<unk>")
    pairs = [(f"k{i}", f"<start> a cat {i % 3} <end>", i) for i in range(6)]
    tok.fit_on_texts([p[1] for p in pairs])
    betas = lambda key, row: np.full(N, row[2], np.float32)
    guse = lambda key, row: np.arange(G, dtype=np.float64) + row[2]
    kw = dict(shuffle=False, training=True, one_hot=False)
    plain = DataGenerator(pairs, 3, tok, U, T, V, betas, N, **kw)[1]
    with5 = DataGenerator(pairs, 3, tok, U, T, V, betas, N, load_guse=guse, **kw)[1]
    assert len(plain[0]) == 4 and len(with5[0]) == 5
    for x, y in zip(plain[0], with5[0][:4]):
        assert np.array_equal(x, y)
    g = with5[0][4]
    assert g.shape == (3, G) and g.dtype == np.float32 and np.array_equal(g[:, 0], [3, 4, 5])


# ---------------------------------------------------------------------------------------------------- retrieval
def test_identification_ranks_on_a_hand_made_matrix():
    sims = np.array([[0.9, 0.9, 0.1, 0.5, 0.9],        # own 0: ties do not count (strictly above)
                     [0.2, 0.8, 0.8, 0.3, 0.1],        # own {0, 3}: best own 0.3; rows 1 and 2 are above
                     [0.5, 0.4, 0.3, 0.2, 0.6],        # own {2, 4}: best own 0.6 is the maximum
                     [0.7, 0.1, 0.7, 0.7, 0.2]], np.float32)   # own [1]: all four others are above
    own = [0, {0, 3}, (2, 4), [1]]
    rank, best = evaluate.semantic_ranks(sims, own)
    assert rank.tolist() == [0, 2, 0, 4] and np.allclose(best, [0.9, 0.3, 0.6, 0.1])
    # an index named twice is one row
    assert evaluate.semantic_ranks(sims, [0, [3, 0, 3], (2, 4), [1]])[0].tolist() == [0, 2, 0, 4]
    for bad in ([0, 1, 2], [0, 1, 2, 5], [0, 1, 2, []], [0, 1, 2, -1]):
        with pytest.raises(ValueError):
            evaluate.semantic_ranks(sims, bad)


def test_retrieval_and_identification_through_the_mock(mock_backend):
    rng = np.random.default_rng(81)
    model, orc = dense(rng)
    Mb = 11
    bank_rows = rng.standard_normal((Mb, G)).astype(np.float32)
    bank_rows[4] = bank_rows[2]                       # a duplicate: the tie goes to the smaller index
    bank = evaluate.SemanticBank(bank_rows, device="cpu")
    assert len(bank) == Mb and np.allclose(bank.inv.numpy(), SO.row_inv_norm(bank_rows), rtol=1e-6)
    assert mock_backend.names == ["row_inv_norm"]
    x = rng.standard_normal((B, N)).astype(np.float32)
    z = orc.embed(x.astype(np.float64))
    want = (z / np.linalg.norm(z, axis=1)[:, None]) @ (bank_rows / np.linalg.norm(bank_rows, axis=1)[:, None]).T
    idx, sim, sims = evaluate.semantic_retrieve(model, x, bank, k=3, return_sims=True)
    assert idx.shape == (B, 3) and idx.dtype == np.int32 and sim.dtype == np.float32 and sims.shape == (B, Mb)
    assert np.abs(sims - want).max() <= 1e-5
    wi, _ = SO.topk(sims, 3)
    assert np.array_equal(idx, wi) and np.array_equal(sim, np.take_along_axis(sims, idx.astype(np.int64), 1))
    assert len(evaluate.semantic_retrieve(model, x, bank, k=3)) == 2
    # queries given directly: the same answer without a model
    q = model.predict_embedding(x)
    i2, s2 = evaluate.semantic_retrieve(q, None, bank, k=3)
    assert np.array_equal(i2, idx) and np.array_equal(s2, sim)
    res = evaluate.semantic_identification(model, x, bank, [int(i) for i in idx[:, 0]])
    assert res["rank"].tolist() == [0] * B and res["top1"] == 1.0 and res["top5"] == 1.0 and res["mrr"] == 1.0
    assert abs(res["mean_cos"] - float(sim[:, 0].mean())) <= 1e-6
    res = evaluate.semantic_identification(model, x, bank, [int(i) for i in idx[:, 2]])
    assert (res["rank"] <= 2).all() and res["rank"].max() >= 1 and res["top1"] < 1.0
    for bad in (0, 65, Mb + 1, 1.5):
        with pytest.raises(ValueError, match="k must"):
            evaluate.semantic_retrieve(model, x, bank, k=bad)
    with pytest.raises(ValueError, match="SemanticBank"):
        evaluate.semantic_retrieve(model, x, bank_rows)
    with pytest.raises(ValueError, match="queries"):
        evaluate.semantic_retrieve(np.zeros((2, G + 1), np.float32), None, bank)
