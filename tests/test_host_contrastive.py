"""The contrastive sentence-embedding loss (nic.NIC(semantic=SemanticTarget(..., loss="contrastive"))) on the CPU through a mock
backend that follows the header text of tnt_contrastive_loss_f32 (tests/contrastive_oracle.py): the float64 restatement against
central differences of its own scalar and against torch autograd of an independent few-line statement; validation and the
config key; SemanticTarget() and loss="cosine" against today's object (equality, hash, plan keys, arena, launch list, buffers);
with loss="contrastive" the launch order, three training steps / test_step against the oracle model under Adam and AdamW,
weight 0; and every refusal that ``semantic`` has."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.model_base import ScheduledSampling as SS, SelfCritical, SemanticTarget
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam, AdamW, CategoricalCrossentropy
from oracle import models as M
from helpers import synth_batch
import semantic_oracle as SO
import contrastive_oracle as CO
from distill_oracle import DistillMockBackend
from finetune_oracle import FinetuneMockBackend

B, N, T, V, U, E, G = 5, 23, 6, 13, 16, 12, 7
OPTIONS = [(0.0, True), (0.0, False), (2.0, True), (2.0, False)]          # (soft_inv_t, symmetric)
CONTRASTIVE = dict(loss="contrastive", temperature=0.5, symmetric=True, soft_temperature=0.8)


class RecordingBackend(CO.ContrastiveMockBackend, SO.SemanticMockBackend, FinetuneMockBackend, DistillMockBackend):
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


def dense(rng, rates=(0, 0, 0), sem=SemanticTarget(G, 0.7, 0.02, **CONTRASTIVE), **kw):
    args = (N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5)
    model = NIC(*args, device="cpu", seed=11, semantic=sem, **kw)
    if sem is None:
        orc = M.NICDense(*args)
    elif sem.loss == "contrastive":
        orc = CO.ContrastiveNIC(*args).configure(sem.dim, sem.weight, sem.reg)
        orc.configure_loss(sem.temperature, sem.symmetric, sem.soft_temperature)
    else:
        orc = SO.SemanticNIC(*args).configure(sem.dim, sem.weight, sem.reg)
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
def torch_statement(z, g, inv_t, soft_inv_t, symmetric, weight):
    """weight * loss and its gradient in z by autograd: an independent statement with F.normalize and F.cross_entropy on
    probability targets (rows of z above the epsilon)"""
    z = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(g, dtype=torch.float64)
    valid = (g * g).sum(1) > 1e-12
    zn, gn = F.normalize(z[valid], dim=1, eps=1e-6), F.normalize(g[valid], dim=1, eps=1e-6)
    L = zn @ gn.T * inv_t
    Q = torch.softmax(gn @ gn.T * soft_inv_t, 1) if soft_inv_t > 0 else torch.eye(len(L), dtype=torch.float64)
    lr, lc = F.cross_entropy(L, Q, reduction="sum"), F.cross_entropy(L.T, Q, reduction="sum")
    loss = (0.5 * (lr + lc) if symmetric else lr) / max(int(valid.sum()), 1)
    (weight * loss).backward()
    return float(loss.detach()), z.grad.numpy()


def inputs(Bb, Gg, seed, zero_row=None, twins=None):
    rng = np.random.default_rng(seed)
    z, g = rng.standard_normal((Bb, Gg)), rng.standard_normal((Bb, Gg))
    if zero_row is not None:
        g[zero_row] = 0
    if twins is not None:
        g[twins[1]] = g[twins[0]]
    return z, g


@pytest.mark.parametrize("soft_inv_t,symmetric", OPTIONS)
@pytest.mark.parametrize("shape", [(2, 3), (5, 7), (6, 16)])
@pytest.mark.parametrize("kind", ["plain", "zero_row", "twins"])
def test_restatement_against_central_differences_and_autograd(shape, soft_inv_t, symmetric, kind):
    Bb, Gg = shape
    z, g = inputs(Bb, Gg, 7 * Bb + Gg, zero_row=1 if kind == "zero_row" else None, twins=(0, Bb - 1) if kind == "twins" else None)
    inv_t, weight = 1.0 / 0.3, 0.6
    loss_row, hit, loss, top1, dz = CO.contrastive_loss(z, g, inv_t, soft_inv_t, symmetric, weight)
    scalar = lambda zz: weight * CO.contrastive_loss(zz, g, inv_t, soft_inv_t, symmetric, weight)[2]
    h = 1e-6
    fd = np.zeros_like(z)
    for idx in np.ndindex(z.shape):
        p_, m_ = z.copy(), z.copy()
        p_[idx] += h; m_[idx] -= h
        fd[idx] = (scalar(p_) - scalar(m_)) / (2 * h)
    assert np.abs(dz - fd).max() <= 1e-7 * max(np.abs(fd).max(), 1.0)
    want_loss, want_dz = torch_statement(z, g, inv_t, soft_inv_t, symmetric, weight)
    assert abs(loss - want_loss) <= 1e-12 * max(abs(want_loss), 1.0)
    assert np.abs(dz - want_dz).max() <= 1e-12 * max(np.abs(want_dz).max(), 1.0)
    valid = (g * g).sum(1) > 1e-12
    Bv = int(valid.sum())
    assert np.isclose(loss, loss_row.sum() / Bv) and top1 == hit.sum() / Bv
    if kind == "zero_row":
        assert Bv == Bb - 1 and loss_row[1] == 0 and hit[1] == 0 and not dz[1].any()
    if kind == "twins":                     # equal logits in the two columns: the first wins, the last row cannot hit
        assert hit[Bb - 1] == 0
    if kind == "twins" and soft_inv_t > 0:  # ... and equal Q
        L, _, _, gn, _, _ = CO.logits(z, g, inv_t)
        assert np.array_equal(L[:, 0], L[:, Bb - 1])


def test_restatement_edges():
    """B = 1 and Bv = 0: loss 0, gradient 0, finite; a z row below the epsilon: the constant normaliser 1e-6"""
    z, g = inputs(1, 4, 1)
    for soft, sym in OPTIONS:
        lrow, hit, loss, top1, dz = CO.contrastive_loss(z, g, 10.0, soft, sym, 1.0)
        assert abs(loss) <= 1e-15 and top1 == 1 and np.abs(dz).max() <= 1e-12
    z, g = inputs(4, 5, 2)
    lrow, hit, loss, top1, dz = CO.contrastive_loss(z, np.zeros_like(g), 10.0, 0.0, True, 1.0)
    assert loss == 0 and top1 == 0 and not dz.any() and not lrow.any() and not hit.any()
    z[2] = 1e-9
    _, _, _, _, dz = CO.contrastive_loss(z, g, 2.0, 0.0, True, 1.0)
    scalar = lambda zz: CO.contrastive_loss(zz, g, 2.0, 0.0, True, 1.0)[2]
    for j in range(5):                      # zn = 1e6 z there: a step of 1e-11 in z is one of 1e-5 in zn
        p_, m_ = z.copy(), z.copy()
        p_[2, j] += 1e-11; m_[2, j] -= 1e-11
        fd = (scalar(p_) - scalar(m_)) / 2e-11
        assert abs(dz[2, j] - fd) <= 1e-6 * max(abs(fd), 1.0), (j, dz[2, j], fd)
    assert np.isfinite(dz).all() and np.abs(dz[2]).max() > 1e3


def test_oracle_model_gradient_against_central_differences():
    """ContrastiveNIC.backward differentiates scalar_loss = CE + L2 + weight * semantic, with the feature Dropout on"""
    rng = np.random.default_rng(21)
    _, orc = dense(rng, rates=(0.1, 0.2, 0.2))
    data, tgt = batch5(rng, np.float64, zero_row=2)
    drop = M.DropCtx(seed=11, step=0, training=True)
    probs, cache = orc.forward(data, training=True, drop=drop)
    grads, _ = orc.backward(probs, cache, tgt)
    h = 1e-6
    for k in SO.NAMES + ("batch_norm/gamma", "dense_img/bias", "dense_img/kernel"):
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


# ---------------------------------------------------------------------------------------------------- the public surface
def test_validation_and_config_key():
    s = SemanticTarget()
    assert (s.dim, s.weight, s.reg, s.loss, s.temperature, s.symmetric, s.soft_temperature) == (512, 1.0, 0.0, "cosine", 0.07, True, None)
    c = SemanticTarget(8, 0.5, 0.1, "contrastive", 0.2, False, 0.4)
    assert (c.loss, c.temperature, c.symmetric, c.soft_temperature) == ("contrastive", 0.2, False, 0.4)
    assert c == SemanticTarget(8, 0.5, 0.1, loss="contrastive", temperature=0.2, symmetric=False, soft_temperature=0.4)
    assert hash(c) == hash(SemanticTarget(8, 0.5, 0.1, "contrastive", 0.2, False, 0.4))
    for other in (dict(temperature=0.3), dict(symmetric=True), dict(soft_temperature=None), dict(soft_temperature=0.5)):
        kw = dict(temperature=0.2, symmetric=False, soft_temperature=0.4, **{})
        kw.update(other)
        assert c != SemanticTarget(8, 0.5, 0.1, "contrastive", **kw)
    assert c != SemanticTarget(8, 0.5, 0.1) and "contrastive" in repr(c) and "0.4" in repr(c)
    assert eval(repr(c)) == c and eval(repr(s)) == s
    for bad in ("clip", "", None, 1, True):
        with pytest.raises(ValueError, match="loss"):
            SemanticTarget(8, loss=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="temperature"):
            SemanticTarget(8, loss="contrastive", temperature=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="soft_temperature"):
            SemanticTarget(8, loss="contrastive", soft_temperature=bad)
    for bad in (0, 1, None, "yes", 1.0):
        with pytest.raises(ValueError, match="symmetric"):
            SemanticTarget(8, loss="contrastive", symmetric=bad)
    base = dict(units=U, embedding_features=512, embedding_text=E, attn_units=5, top_k=V - 1, max_length=T,
                dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
                input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3, clipnorm=0.1,
                decay=0)
    key = {"dim": G, "weight": 0.25, "loss": "contrastive", "temperature": 0.1, "symmetric": False, "soft_temperature": 0.3}
    m = cfg.build_model({**base, "semantic": key}, None, mode="dense", input_size=N, device="cpu")
    assert m.semantic == SemanticTarget(G, 0.25, 0.0, "contrastive", 0.1, False, 0.3)
    m = cfg.build_model({**base, "semantic": {"dim": G, "loss": "contrastive"}}, None, mode="dense", input_size=N, device="cpu")
    assert m.semantic == SemanticTarget(G, loss="contrastive", temperature=0.07, symmetric=True, soft_temperature=None)
    for bad in ({"loss": "clip"}, {"temperature": 0, "loss": "contrastive"}, {"temp": 0.1}, {"symmetric": 1}):
        with pytest.raises(ValueError):
            cfg.build_model({**base, "semantic": bad}, None, mode="dense", input_size=N, device="cpu")


def test_default_loss_is_todays_object():
    """SemanticTarget() equals and hashes as the three-argument object did, and under "cosine" the contrastive fields
    are normalised away"""
    a = SemanticTarget(8, 0.5, 0.1)
    assert hash(a) == hash(("semantic", 8, 0.5, 0.1)) and hash(SemanticTarget()) == hash(("semantic", 512, 1.0, 0.0))
    assert repr(a) == "SemanticTarget(dim=8, weight=0.5, reg=0.1)"
    b = SemanticTarget(8, 0.5, 0.1, loss="cosine", temperature=0.5, symmetric=False, soft_temperature=2.0)
    assert a == b and hash(a) == hash(b) and repr(a) == repr(b)
    assert (b.temperature, b.symmetric, b.soft_temperature) == (0.07, True, None)
    assert SemanticTarget.from_config({"dim": 8, "weight": 0.5, "reg": 0.1, "temperature": 0.9}) == a
    assert len({a, b, SemanticTarget(8, 0.5, 0.1, loss="contrastive")}) == 2


def norm(x):
    """a call argument by value; a tensor by shape and dtype (two models own different buffers)"""
    if isinstance(x, torch.Tensor):
        return ("tensor", tuple(x.shape), str(x.dtype))
    if isinstance(x, (tuple, list)):
        return tuple(norm(y) for y in x)
    if isinstance(x, dict):
        return tuple(sorted((k, norm(v)) for k, v in x.items()))
    return x


TODAY = ["sem_g", "sem_z", "sem_loss", "sem_cos"]
NEW = ["sem_work", "sem_hit", "sem_out"]


def test_cosine_keeps_launches_buffers_and_keys(mock_backend):
    """loss="cosine", spelt out with other contrastive fields, against today's three-argument object: the same backend calls
    with the same arguments, metrics, arena, plan keys and buffers; no contrastive_loss, no new buffer"""
    logs = []
    for sem in (SemanticTarget(G, 0.7, 0.02), SemanticTarget(G, 0.7, 0.02, loss="cosine", temperature=0.5, symmetric=False,
                                                             soft_temperature=1.5)):
        rng = np.random.default_rng(6)
        model, _ = dense(rng, rates=(0.1, 0.2, 0.2), sem=sem)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = batch5(rng)
        mock_backend.calls.clear()
        m1 = model.train_step(batch).as_floats()
        m2 = model.test_step(batch).as_floats()
        assert set(m1) == set(m2) == {"loss", "L2", "accuracy", "semantic"}
        assert all(hasattr(model, n) for n in TODAY) and not any(hasattr(model, n) for n in NEW)
        offs = [(n, e.off, e.seg) for n, e in model.arena.entries.items()]
        logs.append(([(n, norm(a), norm(k_)) for n, a, k_ in mock_backend.calls], m1, m2, offs, model.arena.total,
                     sorted(map(str, model._graphs)), model.get_weight("guse_out/kernel").tolist()))
    assert logs[1] == logs[0]
    names = [c[0] for c in logs[0][0]]
    assert "contrastive_loss" not in names and names.count("cosine_loss") == 2
    assert all("contrastive" not in k for k in logs[0][5])


@pytest.mark.parametrize("rates", [(0, 0, 0), (0.1, 0.2, 0.2)])
def test_contrastive_launch_order(mock_backend, rates):
    """the cosine step's list with tnt_contrastive_loss_f32 in the cosine launch's place and the two-word launch that files
    its means in met[6] / met[5] behind it; dz in place of sem_z; the layer's products unchanged"""
    logs, models = {}, {}
    for name, sem in (("cosine", SemanticTarget(G, 0.7)), ("contrastive", SemanticTarget(G, 0.7, **CONTRASTIVE))):
        rng = np.random.default_rng(6)
        model, _ = dense(rng, rates=rates, sem=sem)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = batch5(rng)
        model.train_step(batch)
        mock_backend.calls.clear()
        model.train_step(batch)
        logs[name], models[name] = list(mock_backend.calls), model
    names = {k: [c[0] for c in v] for k, v in logs.items()}
    model, calls = models["contrastive"], logs["contrastive"]
    kc, kl = names["cosine"].index("cosine_loss"), names["contrastive"].index("contrastive_loss")
    assert kc == kl and "cosine_loss" not in names["contrastive"] and names["contrastive"].count("contrastive_loss") == 1
    assert names["contrastive"][kl - 1] == "gemm" and calls[kl - 1][1][2].data_ptr() == model.sem_z.data_ptr()
    la = calls[kl][1]
    assert la[0].data_ptr() == la[4].data_ptr() == model.sem_z.data_ptr() and la[2].data_ptr() == model.sem_g.data_ptr()
    assert la[5].data_ptr() == model.sem_work.data_ptr() and model.sem_work.numel() == ops.contrastive_work_floats(B, True)
    assert la[6].data_ptr() == model.sem_loss.data_ptr() and la[7].data_ptr() == model.sem_hit.data_ptr()
    assert la[7].dtype == torch.int32 and la[8].data_ptr() == model.sem_out.data_ptr()
    assert la[9:11] == (B, G) and la[11:] == (pytest.approx(2.0), pytest.approx(1.25), True, pytest.approx(0.7))
    mv = calls[kl + 1]
    assert mv[0] == "sum2" and mv[1][4:] == (1, 1.0)
    assert mv[1][0].data_ptr() == model.sem_out[0:1].data_ptr() and mv[1][1].data_ptr() == model.met[6:7].data_ptr()
    assert mv[1][2].data_ptr() == model.sem_out[1:2].data_ptr() and mv[1][3].data_ptr() == model.met[5:6].data_ptr()
    assert names["contrastive"][kl + 2:kl + 4] == ["sum", "sum"]        # (the mock's sum2 is two logged sums)
    rest = [n for i, n in enumerate(names["contrastive"]) if i not in (kl, kl + 1, kl + 2, kl + 3)]
    assert rest == [n for i, n in enumerate(names["cosine"]) if i != kc]
    # the layer's gradient products read dz from sem_z, as under the cosine loss
    dw = [c for c in calls if c[0] == "gemm" and c[1][2].data_ptr() == model.arena.g("guse_out/kernel").data_ptr()]
    dx = [c for c in calls if c[0] == "gemm" and c[2].get("accumulate")]
    assert len(dw) == 1 and dw[0][1][1].data_ptr() == model.sem_z.data_ptr()
    assert len(dx) == 1 and dx[0][1][0].data_ptr() == model.sem_z.data_ptr()
    # plan / graph keys differ between the two losses of otherwise equal models
    keys = {k: {str(g) for g in m._graphs} for k, m in models.items()}
    assert not keys["cosine"] & keys["contrastive"] or not keys["cosine"]
    assert model._semantic_key() != models["cosine"]._semantic_key()
    # hard targets: the smaller workspace; test_step: no gradient
    hard, _ = dense(np.random.default_rng(6), sem=SemanticTarget(G, loss="contrastive"))
    mock_backend.calls.clear()
    got = hard.test_step(batch5(np.random.default_rng(7))).as_floats()
    assert set(got) == {"loss", "L2", "accuracy", "semantic", "semantic_top1"}
    c = [c for c in mock_backend.calls if c[0] == "contrastive_loss"]
    assert len(c) == 1 and c[0][1][4] is None and c[0][1][12] == 0.0
    assert hard.sem_work.numel() == ops.contrastive_work_floats(B, False) == 5 * B + B * B
    assert not any(k.get("accumulate") for _, _, k in mock_backend.calls)


# ---------------------------------------------------------------------------------------------------- against the oracle
OPTIMIZERS = {
    "adam-clipnorm": (lambda: Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), None),
    "adamw-global": (lambda: AdamW(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, weight_decay=0.05,
                                   global_clipnorm=0.05), (0.05, 0.05)),
}
VARIANTS = {"soft-symmetric": CONTRASTIVE, "hard-one-way": dict(loss="contrastive", temperature=0.07, symmetric=False)}


def oracle_update(orc, opt, grads, sparse, decoupled):
    """AdamState.apply, or (``decoupled`` = (weight_decay, global_clipnorm)) the AdamW + global-norm form, as
    tests/test_host_semantic.py states it"""
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


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("opt_name", sorted(OPTIMIZERS))
def test_three_training_steps_against_the_oracle(mock_backend, opt_name, variant):
    rng = np.random.default_rng(31)
    model, orc = dense(rng, rates=(0.1, 0.2, 0.2), sem=SemanticTarget(G, 0.7, 0.02, **VARIANTS[variant]))
    make, decoupled = OPTIMIZERS[opt_name]
    model.compile(make())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    lam = lambda k: model.arena.entries[k].l2
    names = {"loss", "L2", "accuracy", "semantic", "semantic_top1"}
    for step in range(3):
        data, tgt = batch5(rng, zero_row=1 if step == 1 else None)
        w0 = {k: v.copy() for k, v in orc.p.items()}
        drop = M.DropCtx(seed=11, step=step, training=True)
        probs, cache = orc.forward(data, training=True, drop=drop)
        ce, acc = orc.metrics(probs, tgt)
        res = dict(loss=ce, L2=orc.l2_loss(), accuracy=acc, semantic=orc.semantic(cache), semantic_top1=orc.top1(cache))
        grads, sparse = orc.backward(probs, cache, tgt)
        oracle_update(orc, opt, grads, sparse, decoupled)
        orc.p["batch_norm/moving_mean"], orc.p["batch_norm/moving_variance"] = cache["new_mm"], cache["new_mv"]
        got = model.train_step((data, tgt)).as_floats()
        assert set(got) == names
        for k in ("loss", "L2", "semantic"):
            assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) <= 1e-6 and got["semantic_top1"] == pytest.approx(res["semantic_top1"], abs=1e-6)
        for k in M.NICDense.TRAINABLE + list(SO.NAMES):
            g = model.get_gradient(k) + 2 * lam(k) * w0[k]
            assert np.abs(g - grads[k]).max() <= 2e-5 * np.abs(grads[k]).max() + 1e-9, (step, k, np.abs(g - grads[k]).max())
        for k, v in orc.p.items():
            assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k)
    theta = model.arena.theta.clone()
    data, tgt = batch5(rng)
    res, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    assert set(got) == names
    for k in ("loss", "L2", "semantic"):
        assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert got["semantic_top1"] == pytest.approx(res["semantic_top1"], abs=1e-6)
    assert (model.arena.theta == theta).all()
    z = model.predict_embedding(data[0])
    want = orc.embed(data[0].astype(np.float64))
    assert np.abs(z.numpy() - want).max() <= 1e-5 * np.abs(want).max()


def test_weight_zero_reports_the_value_and_leaves_the_step_alone(mock_backend):
    rng = np.random.default_rng(41)
    on, _ = dense(rng, sem=SemanticTarget(G, 0.0, **CONTRASTIVE))
    off, _ = dense(np.random.default_rng(41), sem=None)
    for k in off.keras_shapes:
        off.set_weight(k, on.get_weight(k))
    on.compile(Adam(1e-3, clipnorm=0.1)); off.compile(Adam(1e-3, clipnorm=0.1))
    data, tgt = batch5(rng)
    got = on.train_step((data, tgt)).as_floats()
    off.train_step((data[:4], tgt))
    assert got["semantic"] > 0 and 0 <= got["semantic_top1"] <= 1 and not on.get_gradient("guse_out/kernel").any()
    for k in off.keras_shapes:
        assert np.array_equal(on.get_weight(k), off.get_weight(k)), k


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_refusal(mock_backend):
    rng = np.random.default_rng(2)
    s = SemanticTarget(G, **CONTRASTIVE)
    for kw, what in ((dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                     (dict(self_critical=SelfCritical(end_id=2)), "self_critical"),
                     (dict(grad_sync=lambda m: None), "data-parallel")):
        with pytest.raises(NotImplementedError, match=what):
            NIC(N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", semantic=s, **kw)
    model, _ = dense(rng)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batch = batch5(rng)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    model.grad_sync = lambda m: None
    for step in (model.train_step, model.test_step):
        with pytest.raises(NotImplementedError, match="data-parallel"):
            step(batch)
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
    model.compile(Adam(1e-3, clipnorm=0.1))
    for bad in (batch[0][:4], batch[0][:4] + (batch[0][4][:, :-1],), batch[0][:4] + (batch[0][4][:-1],),
                batch[0][:4] + (None,)):
        for step in (model.train_step, model.test_step):
            with pytest.raises(ValueError, match="guse"):
                step((bad, batch[1]))
    assert mock_backend.names == []                          # nothing was launched by any of them
