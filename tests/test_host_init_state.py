"""The learned initial LSTM state (lc_nic.NIC(init_state=LearnedInitState(...))) on the CPU through a mock backend that follows
the header text of tnt_init_state_fwd_f32 / tnt_init_state_bwd_f32 (tests/init_state_oracle.py): the float64 restatement and
the oracle model against central differences, validation and the config key, every refusal, init_state=None against the model
built without the argument (arena offsets, launch list), the launch order with the feature on, a training step / test step /
greedy / beam decode / score_captions / learn_init_state against the oracle model, the guided, consensus, constrained and
sampled decodes and a teacher (each starts from the state of the rows it stages), one optimizer combination (AdamW + global
clipping), frozen layers, and the .npz / .h5 round trips with an old checkpoint."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import LearnedInitState, ScheduledSampling as SS
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch, tiny_groups
import init_state_oracle as IO
from distill_oracle import DistillMockBackend
from finetune_oracle import FinetuneMockBackend
from score_oracle import ScoreMockBackend
from test_host_guidance import GuidanceMockBackend

B, N, T, V, U = 5, 23, 6, 13, 16
LC = dict(R=4, D=16, A=5, Et=12)


class RecordingBackend(IO.InitMockBackend, FinetuneMockBackend, DistillMockBackend, ScoreMockBackend, GuidanceMockBackend):
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


def attention(rng, cls=LcNIC, rates=(0,) * 6, init=LearnedInitState(), with_arg=True, scale=3.0, **kw):
    g = (tiny_groups(N, LC["R"], np.random.default_rng(100)), [LC["D"]] * LC["R"])
    args = (g, U, 512, LC["Et"], LC["A"], V, T, *rates, 0.01, 0.001, 3e-5, 1e-5)
    if with_arg:
        kw["init_state"] = init
    model = cls(*args, device="cpu", seed=11, **kw)
    orc = (IO.InitLcNIC if init is not None else M.LcNIC)(*args)
    if init is not None:
        orc.reg = init.reg
        orc.init_params(rng, scale=scale)
    else:
        orc.init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_against_central_differences():
    """init_bwd's gradients are those of sum(dh0 * h0) + sum(dc0 * c0) with dh0, dc0 arbitrary constants"""
    rng = np.random.default_rng(3)
    Bb, R, D, Uu = 3, 5, 4, 6
    F, Wh, Wc = rng.standard_normal((Bb, R, D)), rng.standard_normal((D, Uu)) * 0.5, rng.standard_normal((D, Uu)) * 0.5
    bh, bc = rng.standard_normal(Uu) * 0.1, rng.standard_normal(Uu) * 0.1
    dh0, dc0 = rng.standard_normal((Bb, Uu)), rng.standard_normal((Bb, Uu))
    i = dict(F=F, Wh=Wh, bh=bh, Wc=Wc, bc=bc)

    def scalar(**over):
        h0, c0, _ = IO.init_fwd(**{**i, **over})
        return (dh0 * h0).sum() + (dc0 * c0).sum()
    h0, c0, m = IO.init_fwd(**i)
    assert np.allclose(m, F.sum(1) / R) and np.allclose(h0, np.tanh(m @ Wh + bh))
    got = IO.init_bwd(dh0, dc0, h0, c0, m, Wh, Wc, R)
    got["dF"] = np.broadcast_to(got["dF_row"][:, None, :], F.shape)
    h = 1e-6
    for name, key in (("F", "dF"), ("Wh", "dWh"), ("bh", "dbh"), ("Wc", "dWc"), ("bc", "dbc")):
        fd = np.zeros_like(i[name])
        for idx in np.ndindex(i[name].shape):
            p_, m_ = i[name].copy(), i[name].copy()
            p_[idx] += h; m_[idx] -= h
            fd[idx] = (scalar(**{name: p_}) - scalar(**{name: m_})) / (2 * h)
        assert np.abs(got[key] - fd).max() <= 1e-7 * np.abs(fd).max(), name


def test_oracle_model_gradient_against_central_differences():
    """InitLcNIC.backward differentiates scalar_loss = CE + L2 with the decoder started from the learned state"""
    rng = np.random.default_rng(21)
    _, orc = attention(rng, init=LearnedInitState(0.01))
    data, tgt = synth_batch(B, N, T, V, U, rng, dtype=np.float64)
    drop = M.DropCtx(seed=11, step=0, training=True)
    (probs, attn), cache = orc.forward(data, training=True, drop=drop)
    grads, _ = orc.backward(probs, cache, tgt)
    h = 1e-6
    for k in IO.NAMES + ("input_bn/gamma", "dense_in/1/bias", "attention/W2/kernel", "lstm/recurrent_kernel"):
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
    # the ablations differ from it: the branch is visible where the GPU test looks
    orc.branch_dF = False
    off, _ = orc.backward(probs, cache, tgt)
    assert np.abs(off["input_bn/gamma"] - grads["input_bn/gamma"]).max() > 1e-6
    assert np.array_equal(off["hidden_init/kernel"], grads["hidden_init/kernel"])


# ---------------------------------------------------------------------------------------------------- the public surface
def test_validation_and_config_key():
    s = LearnedInitState()
    assert s.reg == 0.0 and LearnedInitState(0.5) == LearnedInitState(0.5) and LearnedInitState(0.5) != s
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="L2 coefficient"):
            LearnedInitState(bad)
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="LearnedInitState"):
        attention(rng, with_arg=False, init_state=True)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    base = dict(units=U, embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], top_k=V - 1, max_length=T,
                dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0, dropout_out=0,
                input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3, clipnorm=0.1,
                decay=0)
    assert cfg.build_model(base, g, device="cpu").init_state is None
    assert cfg.build_model({**base, "learn_init_state": False}, g, device="cpu").init_state is None
    assert cfg.build_model({**base, "learn_init_state": True}, g, device="cpu").init_state == LearnedInitState(0.0)
    m = cfg.build_model({**base, "learn_init_state": {"reg": 0.25}}, g, device="cpu")
    assert m.init_state == LearnedInitState(0.25) and m.arena.entries["carry_init/kernel"].l2 == 0.25
    assert m.arena.entries["hidden_init/bias"].l2 == 0
    for bad in ({"l2": 1.0}, 0.5, "yes", {"reg": -1}):
        with pytest.raises(ValueError):
            cfg.build_model({**base, "learn_init_state": bad}, g, device="cpu")
    with pytest.raises(TypeError):                           # the dense model does not take the argument
        NIC(N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", init_state=s)


def test_layers_shapes_and_initialisation():
    rng = np.random.default_rng(1)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    args = (g, U, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    on, off = LcNIC(*args, device="cpu", seed=11, init_state=LearnedInitState(0.5)), LcNIC(*args, device="cpu", seed=11)
    D = LC["D"]
    assert list(on.layers_spec)[-2:] == ["hidden_init", "carry_init"]
    assert list(on.layers_spec)[:-2] == list(off.layers_spec)
    for nm in IO.LAYERS:
        assert on.layers_spec[nm] == ["kernel", "bias"]
        assert on.keras_shapes[f"{nm}/kernel"] == (D, U) and on.keras_shapes[f"{nm}/bias"] == (U,)
        k = on.get_weight(f"{nm}/kernel")
        lim = np.sqrt(6.0 / (D + U))
        assert np.abs(k).max() <= lim and np.abs(k).max() > 0.7 * lim and abs(k.mean()) < 0.2 * lim      # glorot_uniform
        assert not on.get_weight(f"{nm}/bias").any()
        assert on.get_layer(nm).trainable
    assert not np.array_equal(on.get_weight("hidden_init/kernel"), on.get_weight("carry_init/kernel"))
    # the model without the layers keeps its arena and its initial values; the four variables sit behind every entry
    assert list(on.arena.entries)[:-4] == list(off.arena.entries) and tuple(list(on.arena.entries)[-4:]) == IO.NAMES
    for n, e in off.arena.entries.items():
        assert (on.arena.entries[n].off, on.arena.entries[n].seg) == (e.off, e.seg), n
        assert np.array_equal(on.get_weight(n), off.get_weight(n)), n
    assert on.count_params() == off.count_params() + 2 * (D * U + U)
    # the L2 metric includes the two kernels (and nothing else of the two layers)
    batch = synth_batch(B, N, T, V, U, rng)
    l2 = lambda m: m.test_step(batch).as_floats()["L2"]
    want = 0.5 * sum((on.get_weight(f"{nm}/kernel").astype(np.float64) ** 2).sum() for nm in IO.LAYERS)
    assert abs((l2(on) - l2(off)) - want) <= 1e-5 * want


def test_every_refusal(mock_backend):
    rng = np.random.default_rng(2)
    s = LearnedInitState()
    for kw, what in ((dict(use_layer_norm=True), "use_layer_norm"), (dict(n_subjects=2), "n_subjects"),
                     (dict(teacher_forcing=False), "teacher_forcing"),
                     (dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                     (dict(grad_sync=lambda m: None), "data-parallel")):
        with pytest.raises(NotImplementedError, match=what):
            attention(rng, init=s, **kw)
    with pytest.raises(NotImplementedError, match="n_subjects"):
        attention(rng, cls=MsNIC, init=s)
    model, _ = attention(rng, init=s)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batch = synth_batch(B, N, T, V, U, rng)
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam(batch)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc()
    model.enable_agc(None)                                   # switching it off is no request for it
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    model.grad_sync = lambda m: None                          # attached behind the constructor's back
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.train_step(batch)
    model.grad_sync = None
    acc, _ = attention(rng, init=s)
    with pytest.raises(NotImplementedError, match="init_state"):
        acc.compile(Adam(1e-3, clipnorm=0.1, gradient_accumulation_steps=2))
        acc.train_step(batch)
    assert mock_backend.names == []                          # nothing was launched by any of them
    plain, _ = attention(rng, init=None)
    with pytest.raises(ValueError, match="init_state"):
        plain.learn_init_state(batch[0][0])


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
def test_none_is_the_model_without_the_argument(mock_backend, rates):
    """the same arena offsets, the same backend methods with the same arguments (tensors by shape and dtype) and the same
    metrics, in train_step, test_step and a greedy decode"""
    logs = []
    for kw in (dict(with_arg=False), dict(init=None)):
        rng = np.random.default_rng(6)
        model, _ = attention(rng, rates=rates, **{"init": None, **kw})
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = synth_batch(B, N, T, V, U, rng)
        mock_backend.calls.clear()
        m1 = model.train_step(batch).as_floats()
        m2 = model.test_step(batch).as_floats()
        x, _, a0, c0 = batch[0]
        words = model.greedy_predict(x, a0, c0, np.ones(B, np.int64), 3, return_s=False)[0]
        assert not hasattr(model, "fmean") and model.init_state is None
        offs = [(n, e.off, e.seg) for n, e in model.arena.entries.items()]
        logs.append(([(n, norm(a), norm(k_)) for n, a, k_ in mock_backend.calls], m1, m2, words.tolist(), offs,
                     model.arena.total))
    assert logs[1] == logs[0]
    names = [c[0] for c in logs[0][0]]
    assert "init_state_fwd" not in names and "init_state_bwd" not in names


def test_feature_on_launch_order(mock_backend):
    """on top of the plain step: one forward launch at the end of the encoder (behind the hoisted W1 product, in front of the
    first decoder step), and behind the chain one dh0 product and the backward launch, in front of the launch that finishes
    dF; the init backward receives the per-step route's dh_att / dc and the model's dF"""
    logs = {}
    for on in (False, True):
        rng = np.random.default_rng(6)
        model, _ = attention(rng, init=LearnedInitState() if on else None)
        model.compile(Adam(1e-3, clipnorm=0.1))
        batch = synth_batch(B, N, T, V, U, rng)
        mock_backend.calls.clear()
        model.train_step(batch)
        logs[on] = list(mock_backend.calls)
    names = {k: [c[0] for c in v] for k, v in logs.items()}
    assert names[True].count("init_state_fwd") == 1 and names[True].count("init_state_bwd") == 1
    kf, kb = names[True].index("init_state_fwd"), names[True].index("init_state_bwd")
    rest = [n for i, n in enumerate(names[True]) if i not in (kf, kb, kb - 1)]
    assert names[True][kb - 1] == "gemm" and rest == names[False]
    assert kf < names[True].index("attention_step_fwd")
    assert max(i for i, n in enumerate(names[True]) if n in ("lstm_step_bwd", "attention_step_bwd")) < kb - 1
    finish = [i for i, n in enumerate(names[True]) if n in ("attention_front_bwd", "act_bwd") and i > kb]
    assert finish, "the launch that finishes dF runs behind the init backward"
    fa, ba = logs[True][kf][1], logs[True][kb][1]
    assert fa[0].data_ptr() == model.F.data_ptr() and fa[6].data_ptr() == model.Hs.data_ptr()
    assert fa[7].data_ptr() == model.Cs.data_ptr() and fa[8:] == (B, LC["R"], LC["D"], U)
    assert ba[0].data_ptr() == model.dh_att.data_ptr() and ba[1].data_ptr() == model.dc.data_ptr()
    assert ba[11].data_ptr() == model.dF.data_ptr() and all(t is not None for t in ba[7:11])
    # test_step: the forward launch alone
    mock_backend.calls.clear()
    model.test_step(batch)
    assert mock_backend.names.count("init_state_fwd") == 1 and "init_state_bwd" not in mock_backend.names


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("rates", [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)])
def test_train_and_test_step_against_the_oracle(mock_backend, rates):
    rng = np.random.default_rng(31)
    model, orc = attention(rng, rates=rates, init=LearnedInitState(0.02))
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    lam = lambda k: model.arena.entries[k].l2
    for step in range(2):
        data, tgt = synth_batch(B, N, T, V, U, rng)
        data = (data[0], data[1], rng.standard_normal((B, U)).astype(np.float32), data[3])      # a0 is ignored
        w0 = {k: v.copy() for k, v in orc.p.items()}
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert set(got) == {"loss", "L2", "accuracy", "attention", "lr"}
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        if step == 0:
            for k in orc.trainable():
                if k == "attention/V/bias":
                    continue
                g = model.get_gradient(k) + 2 * lam(k) * w0[k]
                assert np.abs(g - grads[k]).max() <= 2e-5 * np.abs(grads[k]).max() + 1e-9, (k, np.abs(g - grads[k]).max())
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            assert np.abs(model.get_weight(k) - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k)
    theta = model.arena.theta.clone()
    data, tgt = synth_batch(B, N, T, V, U, rng)
    res, _ = orc.test_step(data, tgt)
    got = model.test_step((data, tgt)).as_floats()
    for k in ("loss", "L2", "attention"):
        assert abs(got[k] - res[k]) <= 1e-5 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert (model.arena.theta == theta).all()


def test_the_branch_reaches_the_gradients():
    """the oracle's gradients with and without the branch differ by far more than any tolerance here"""
    rng = np.random.default_rng(31)
    _, orc = attention(rng)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    (probs, attn), cache = orc.forward(data, training=True, drop=M.DropCtx(seed=11, step=0, training=True))
    on, _ = orc.backward(probs, cache, tgt)
    orc.branch_dF = False
    off, _ = orc.backward(probs, cache, tgt)
    k = "input_bn/gamma"
    assert np.abs(on[k] - off[k]).max() >= 100 * 2e-4 * np.abs(on[k]).max()


def test_decodes_and_learn_init_state_against_the_oracle(mock_backend):
    rng = np.random.default_rng(41)
    model, orc = attention(rng)
    data, _ = synth_batch(B, N, T, V, U, rng)
    x = data[0]
    junk = rng.standard_normal((B, U)).astype(np.float32)          # a0 / c0: shape-checked, values unused
    h0, c0 = model.learn_init_state(x)
    wh, wc = orc.learn_init_state(x)
    assert h0.shape == c0.shape == (B, U) and np.abs(h0 - wh).max() <= 1e-6 and np.abs(c0 - wc).max() <= 1e-6
    assert np.abs(wh).max() > 0.05                                # not the zero state
    start = np.ones(B, np.int64)
    words, probs, alpha, _ = model.greedy_predict(x, junk, junk, start, T, return_s=False)
    w_o, p_o, a_o, _ = orc.greedy_predict(x, None, None, start, T)
    assert np.array_equal(words, w_o) and np.abs(probs - p_o).max() <= 1e-5 and np.abs(alpha - a_o).max() <= 1e-5
    plain = M.LcNIC.greedy_predict(orc, x, np.zeros((B, U)), np.zeros((B, U)), start, T)
    assert np.abs(plain[1] - p_o).max() > 1e-3                    # the zero state decodes something else
    seqs, scores = model.beam_search(x, junk, junk, start, T, beam_width=3)
    s_o, sc_o, margin = orc.beam_search(x, None, None, start, T, k=3)
    ok = margin > 1e-4
    assert ok.any() and np.array_equal(seqs[ok], s_o[ok]) and np.abs(scores[ok] - sc_o[ok]).max() <= 1e-4
    with pytest.raises(Exception):
        model.greedy_predict(x, junk[:, :U - 1], junk, start, T)     # still shape-checked
    # score_captions gathers the learned state to its decoder rows: two candidates per scan against the oracle's
    # teacher-forced inference forward
    caps = rng.integers(1, V, (B, 2, T))
    lp, length = model.score_captions(x, junk, junk, caps)
    assert (np.asarray(length) == T - 1).all()
    for c in range(2):
        (p_tf, _), _ = orc.forward((x, caps[:, c, :-1], None, None), training=False)
        want = np.log(np.take_along_axis(p_tf, caps[:, c, 1:, None], axis=2)[:, :, 0]).sum(axis=1)
        assert np.abs(np.asarray(lp)[:, c] - want).max() <= 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("kind", ["guidance", "consensus", "constraints", "sample", "beam-guidance"])
def test_every_decode_starts_from_the_state_of_the_rows_it_stages(mock_backend, kind):
    """the decodes share _encode: whatever rows a decode stages (a null scan per scan under guidance, G members under
    consensus, k beams per scan) each get the state of their own features -- the one init forward launch of the decode sits
    behind the encoder, covers every staged row, and what it wrote is init_fwd of the staged features"""
    from masters_thesis_amd.model_base import Guidance, Consensus, DecodeConstraints
    rng = np.random.default_rng(43)
    model, orc = attention(rng)
    x = synth_batch(4, N, T, V, U, rng)[0][0]
    z = np.zeros((4, U), np.float32)
    start = np.ones(4, np.int64)
    seen = {}
    real = IO.InitMockBackend.init_state_fwd

    def spy(self, F, Wh, bh, Wc, bc, fmean, h0, c0, Bn, R, D, Un):
        real(self, F, Wh, bh, Wc, bc, fmean, h0, c0, Bn, R, D, Un)
        f64 = lambda t, *s: IO.flat(t)[:int(np.prod(s))].reshape(*s).astype(np.float64)
        seen["rows"], seen["F"], seen["h0"] = Bn, f64(F, Bn, R, D), f64(h0, Bn, Un).copy()
    mock_backend.__class__.init_state_fwd = spy
    try:
        mock_backend.calls.clear()
        if kind == "guidance":
            model.greedy_predict(x, z, z, start, 3, return_s=False, guidance=Guidance(1.5))
            rows = 8
        elif kind == "consensus":
            model.greedy_predict(x, z, z, start[:2], 3, return_s=False, consensus=Consensus(2))
            rows = 4
        elif kind == "constraints":
            model.greedy_predict(x, z, z, start, 3, return_s=False, constraints=DecodeConstraints(no_repeat_ngram_size=2))
            rows = 4
        elif kind == "sample":
            model.sample_predict(x, z, z, start, 3, return_s=False, top_k=3, sample_step=1)
            rows = 4
        else:
            model.beam_search(x, z, z, start, 3, beam_width=2, guidance=Guidance(1.5))
            rows = 16
    finally:
        del mock_backend.__class__.init_state_fwd
    names = mock_backend.names
    assert names.count("init_state_fwd") == 1 and seen["rows"] == rows
    assert names.index("init_state_fwd") < names.index("attention_step_fwd")
    p = orc.p
    want = IO.init_fwd(seen["F"], p["hidden_init/kernel"], p["hidden_init/bias"], p["carry_init/kernel"], p["carry_init/bias"])[0]
    assert np.abs(seen["h0"] - want).max() <= 1e-6
    if "guidance" in kind:                                   # the null scans' rows start from another state than the scans'
        half = rows // 2
        assert np.abs(seen["h0"][:half] - seen["h0"][half:]).max() > 1e-3


def test_a_teacher_with_the_layers_starts_from_its_own_state(mock_backend):
    """set_teacher: the teacher's captured inference forward goes through _encode, so a teacher built with init_state hands
    the student the logits of the decoder started from the learned state (the oracle's), not from the batch's zeros"""
    from masters_thesis_amd.optimizers import CategoricalCrossentropy, Distillation
    rng = np.random.default_rng(81)
    teacher, t_orc = attention(rng)
    student, _ = attention(np.random.default_rng(82), init=None)
    student.compile(Adam(1e-3, clipnorm=0.1),
                    CategoricalCrossentropy(from_logits=False, reduction="none", distillation=Distillation(0.5, 2.0)))
    student.set_teacher(teacher)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    mock_backend.calls.clear()
    got = student.train_step((data, tgt)).as_floats()
    assert "distill_kl" in got and mock_backend.names.count("init_state_fwd") == 1 and "init_state_bwd" not in mock_backend.names
    (_, _), cache = t_orc.forward(data, training=False)
    logits = teacher.logits[:, :V].numpy().reshape(T, B, V).transpose(1, 0, 2)
    assert np.abs(logits - cache["logits"]).max() <= 1e-4 * np.abs(cache["logits"]).max()


def test_adamw_with_global_clipping_reaches_the_new_variables(mock_backend):
    """one arena-wide optimizer combination: decoupled weight decay and a global clip norm reach the four new variables
    through the tables like every other"""
    rng = np.random.default_rng(51)
    model, orc = attention(rng, init=LearnedInitState(0.02))
    twin, _ = attention(np.random.default_rng(51), init=LearnedInitState(0.02))
    model.compile(Adam(learning_rate=1e-3, beta_2=0.98, epsilon=1e-8, weight_decay=0.1, global_clipnorm=0.05))
    twin.compile(Adam(learning_rate=1e-3, beta_2=0.98, epsilon=1e-8))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    w0 = {k: model.get_weight(k).astype(np.float64) for k in IO.NAMES}
    model.train_step((data, tgt)); twin.train_step((data, tgt))
    for k in IO.NAMES:                                   # the same gradients, another update
        assert np.array_equal(model.get_gradient(k), twin.get_gradient(k))
    for k in IO.NAMES:
        moved, plain = model.get_weight(k) - w0[k], twin.get_weight(k) - w0[k]
        assert np.abs(moved).max() > 0 and not np.array_equal(moved, plain), k
        assert np.abs(moved).max() <= 1.2e-3 + 1e-3 * 0.1 * np.abs(w0[k]).max()
    k = "hidden_init/kernel"
    decay = -1e-3 * 0.1 * w0[k]
    adam_part = model.get_weight(k) - w0[k] - decay
    assert np.abs(adam_part).max() <= 1.01e-3            # |Adam step| <= lr at step 1; the rest is the decoupled decay


def test_frozen_layers_keep_their_bits_and_skip_their_products(mock_backend):
    rng = np.random.default_rng(61)
    model, _ = attention(rng)
    model.compile(Adam(1e-3, clipnorm=0.1))
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(3)]
    model.train_step(batches[0])
    model.freeze("hidden_init", "carry_init")
    assert not model.get_layer("hidden_init").trainable and not model.get_layer("carry_init").trainable
    held = {k: (model.get_weight(k).copy(), model.get_optimizer_slot(k, "m").copy(), model.get_optimizer_slot(k, "v").copy())
            for k in IO.NAMES}
    other = model.get_weight("input_bn/gamma").copy()
    mock_backend.calls.clear()
    model.train_step(batches[1])
    call = [c for c in mock_backend.calls if c[0] == "init_state_bwd"]
    assert len(call) == 1 and all(t is None for t in call[0][1][7:11]) and call[0][1][11] is not None
    for k, (w, m, v) in held.items():
        assert np.array_equal(model.get_weight(k), w) and np.array_equal(model.get_optimizer_slot(k, "m"), m)
        assert np.array_equal(model.get_optimizer_slot(k, "v"), v)
    assert not np.array_equal(model.get_weight("input_bn/gamma"), other)
    # one layer frozen: all four gradients are formed, the table freezes the one
    model.unfreeze("carry_init")
    model.set_lr_multipliers({"carry_init": 0.5})
    mock_backend.calls.clear()
    model.train_step(batches[2])
    call = [c for c in mock_backend.calls if c[0] == "init_state_bwd"]
    assert all(t is not None for t in call[0][1][7:11])
    assert np.array_equal(model.get_weight("hidden_init/kernel"), held["hidden_init/kernel"][0])
    assert not np.array_equal(model.get_weight("carry_init/kernel"), held["carry_init/kernel"][0])


# ---------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("ext", ["npz", "h5"])
def test_checkpoint_round_trip_and_old_checkpoint(tmp_path, ext):
    rng = np.random.default_rng(71)
    model, _ = attention(rng)
    path = str(tmp_path / f"w.{ext}")
    model.save_weights(path)
    other, _ = attention(np.random.default_rng(72))
    assert not np.array_equal(other.get_weight("hidden_init/kernel"), model.get_weight("hidden_init/kernel"))
    other.load_weights(path)
    for k in model.keras_shapes:
        assert np.array_equal(other.get_weight(k), model.get_weight(k)), k
    # a checkpoint of the model without the layers: everything else loads, the two layers keep their initialisation
    plain, _ = attention(np.random.default_rng(73), init=None)
    old = str(tmp_path / f"old.{ext}")
    plain.save_weights(old)
    g = (tiny_groups(N, LC["R"], np.random.default_rng(100)), [LC["D"]] * LC["R"])
    fresh = LcNIC(g, U, 512, LC["Et"], LC["A"], V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11,
                  init_state=LearnedInitState())
    init = {k: fresh.get_weight(k).copy() for k in IO.NAMES}
    fresh.load_weights(old, by_name=True, skip_mismatch=True)
    for k in plain.keras_shapes:
        assert np.array_equal(fresh.get_weight(k), plain.get_weight(k)), k
    for k in IO.NAMES:
        assert np.array_equal(fresh.get_weight(k), init[k]), k
    # and the other way round: the plain model ignores the two layers of a new checkpoint
    plain.load_weights(path, by_name=True, skip_mismatch=True)
    assert np.array_equal(plain.get_weight("lstm/kernel"), model.get_weight("lstm/kernel"))
