"""lc_nic.NIC(init_state=LearnedInitState(...)) on the GPU against the float64 oracle model whose decoder starts from the
state its own region features predict (tests/init_state_oracle.py: InitLcNIC), on both routes of the backward chain:
  per-step   a tiny model with U = 16 (dc and dh_att as step 0's kernels leave them, one dh0 product)
  chain      U = 512, B = 5, R = 129, T = 3 (tnt_lc_seq_bwd_init_f32 stores dc0, two dh0 products; asserted: _lc_seq_bwd_ok())
with the tolerances tests/test_gpu_lcnic.py applies to the plain step: loss, L2, attention 1e-4 relative + 1e-7, gradients
2e-4 of the variable's largest gradient + 1e-9 (dropout-free, as there), post-Adam weights 2e-2 * lr + 1e-4 of the
variable's largest weight.  Three steps cover eager, record and replay.  ``SCALE`` multiplies the Glorot limit of the two
kernels' initial values so that the branch is far above the tolerance of the gradients it is checked in (asserted on the CPU,
in the oracle, in every case): input_bn/gamma with and without the branch's share of dF, and attention/W2/kernel with the
learned against a zero h0, each differ by at least 100 gradient tolerances.
Then: plan, hipGraph and eager steps bit-identical; greedy, beam (width 3) and score_captions against the oracle; test_step
changes no weight; frozen hidden_init + carry_init keep weights and moments bit for bit while the rest trains;
init_state=None is the model built without the argument, bit for bit, on both routes."""
import numpy as np
import pytest
import torch

import init_state_oracle as IO
from oracle import models as M
from helpers import synth_batch, tiny_groups

pytestmark = pytest.mark.gpu

# route -> (B, N, R, D, A, U, Et, V, T)
DIMS = {"per-step": (3, 37, 4, 16, 3, 16, 8, 11, 4), "chain": (5, 700, 129, 32, 32, 512, 64, 101, 3)}
SCALE = {"per-step": 1.0, "chain": 3.0}
DROP = (0.0, 0.2, 0.2, 0.2, 0.2, 0.2)
GTOL = 2e-4
REG = 0.002


def build(rng, dims, rates=(0,) * 6, on=True, with_arg=True, scale=1.0, **kw):
    from masters_thesis_amd.lc_nic import NIC
    from masters_thesis_amd.model_base import LearnedInitState
    B, N, R, D, A, U, Et, V, T = dims
    g = (tiny_groups(N, R, rng), [D] * R)
    args = (g, U, 512, Et, A, V, T, *rates, 0.01, 0.001, 3e-5, 1e-5)
    if with_arg:
        kw["init_state"] = LearnedInitState(REG) if on else None
    model = NIC(*args, seed=11, **kw)
    if on:
        orc = IO.InitLcNIC(*args)
        orc.reg = REG
        orc.init_params(rng, scale=scale)
    else:
        orc = M.LcNIC(*args).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


@pytest.mark.parametrize("route,rates", [("per-step", (0,) * 6), ("chain", (0,) * 6), ("chain", DROP)],
                         ids=["per-step", "chain", "chain-dropout"])
def test_train_step_against_the_oracle(route, rates):
    rng = np.random.default_rng(61)
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    model, orc = build(rng, dims, rates, scale=SCALE[route])
    model.compile(adam())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    lam = lambda k: model.arena.entries[k].l2
    for step in range(3):                      # eager, record / capture, replay
        data, tgt = synth_batch(B, N, T, V, U, rng)
        w0 = {k: v.copy() for k, v in orc.p.items()}
        if step == 0:                          # the branch is far above the tolerance of the gradients it is checked in
            (probs, attn), cache = orc.forward(data, training=True, drop=M.DropCtx(seed=11, step=0, training=True))
            full, _ = orc.backward(probs, cache, tgt)
            orc.branch_dF = False
            no_dF, _ = orc.backward(probs, cache, tgt)
            orc.branch_dF, orc.zero_h0 = True, True
            (p0, a0_), c0_ = orc.forward(data, training=True, drop=M.DropCtx(seed=11, step=0, training=True))
            zero_h, _ = orc.backward(p0, c0_, tgt)
            orc.zero_h0 = False
            for k, other in (("input_bn/gamma", no_dF), ("attention/W2/kernel", zero_h)):
                moved = np.abs(full[k] - other[k]).max()
                print(f"\n[{route}] the branch moves d {k} by {moved / (GTOL * np.abs(full[k]).max()):.0f} tolerances")
                assert moved >= 100 * GTOL * np.abs(full[k]).max(), (k, moved, np.abs(full[k]).max())
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        if step == 0:
            assert model._lc_seq_bwd_ok() == (route == "chain")
        assert set(got) == {"loss", "L2", "accuracy", "attention", "lr"}
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        if step == 0 and not any(rates):
            for k in orc.trainable():
                if k == "attention/V/bias":
                    continue
                g = model.get_gradient(k) + 2 * lam(k) * w0[k]
                assert np.abs(g - grads[k]).max() <= GTOL * np.abs(grads[k]).max() + 1e-9, (k, np.abs(g - grads[k]).max(),
                                                                                            np.abs(grads[k]).max())
        for k, v in orc.p.items():
            if k == "attention/V/bias":
                continue
            w = model.get_weight(k)
            assert np.abs(w - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k, np.abs(w - v).max())
    model.check_device_errors()


def _run(model, batches):
    out = [model.train_step(b).as_floats() for b in batches]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_plan_graph_and_eager_steps_are_bit_identical(route):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(5)
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(4)]
    models = []
    for kind in ("plan", "graph", "eager"):
        m, _ = build(np.random.default_rng(62), dims, DROP, scale=SCALE[route], use_graph=kind != "eager")
        if kind == "graph":
            m.plan_step = False
        m.compile(adam())
        models.append((m, _run(m, batches)))
    (a, ra), (b, rb), (c, rc) = models
    assert ra == rb == rc
    assert any(isinstance(v, tuple) for v in a._graphs.values()), "the first model did not replay a launch plan"
    assert any(isinstance(v, torch.cuda.CUDAGraph) for v in b._graphs.values()), "the second model did not replay a graph"
    assert not c._graphs
    for m in (b, c):
        assert torch.equal(a.arena.theta, m.arena.theta)
        assert torch.equal(a.opt_m, m.opt_m) and torch.equal(a.opt_v, m.opt_v)


@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_decodes_and_scores_against_the_oracle(route):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(63)
    model, orc = build(rng, dims, scale=SCALE[route])
    data, _ = synth_batch(B, N, T, V, U, rng)
    x = data[0]
    junk = rng.standard_normal((B, U)).astype(np.float32)          # a0 / c0: shape-checked, values unused
    start = np.ones(B, np.int64)
    h0, c0 = model.learn_init_state(x)
    wh, wc = orc.learn_init_state(x)
    assert np.abs(h0 - wh).max() <= 1e-5 and np.abs(c0 - wc).max() <= 1e-5 and np.abs(wh).max() > 0.05
    ww, wp, wa, _ = orc.greedy_predict(x, None, None, start, T)
    gw, gp, ga, _ = model.greedy_predict(x, junk, junk, start, T, U, None)
    assert np.array_equal(gw, ww)
    assert np.abs(gp - wp).max() <= 1e-4 and np.abs(ga - wa).max() <= 1e-4 * wa.max()
    plain = M.LcNIC.greedy_predict(orc, x, np.zeros((B, U)), np.zeros((B, U)), start, T)
    assert np.abs(plain[1] - wp).max() > 1e-3                      # the zero state decodes something else
    want, wscore, margin = orc.beam_search(x, None, None, start, T, k=3)
    got, gscore = model.beam_search(x, junk, junk, start, T, beam_width=3)
    ok = margin > 2e-4
    assert ok.any(), margin
    assert np.array_equal(got[ok], want[ok]) and np.abs(gscore[ok] - wscore[ok]).max() <= 1e-4 * max(1.0, np.abs(wscore).max())
    caps = rng.integers(1, V, (B, 2, T))
    lp, length = model.score_captions(x, junk, junk, caps)
    assert (np.asarray(length) == T - 1).all()
    for c in range(2):
        (p_tf, _), _ = orc.forward((x, caps[:, c, :-1], None, None), training=False)
        ref = np.log(np.take_along_axis(p_tf, caps[:, c, 1:, None], axis=2)[:, :, 0]).sum(axis=1)
        assert np.abs(np.asarray(lp)[:, c] - ref).max() <= 1e-4 * np.abs(ref).max()
    model.check_device_errors()


def test_test_step_changes_no_weight():
    dims = DIMS["chain"]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(64)
    model, orc = build(rng, dims, scale=SCALE["chain"])
    model.compile(adam())
    theta = model.arena.theta.clone()
    for _ in range(3):                         # eager, capture, replay
        data, tgt = synth_batch(B, N, T, V, U, rng)
        res, _ = orc.test_step(data, tgt)
        got = model.test_step((data, tgt)).as_floats()
        assert set(got) == {"loss", "L2", "accuracy", "attention"}
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (k, got[k], res[k])
    assert torch.equal(model.arena.theta, theta)


@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_frozen_layers_keep_their_bits_while_the_rest_trains(route):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(66)
    model, _ = build(rng, dims, DROP, scale=SCALE[route])
    model.compile(adam())
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(4)]
    model.train_step(batches[0])               # moments exist and are not zero
    model.freeze("hidden_init", "carry_init")
    held = {k: (model.get_weight(k).copy(), model.get_optimizer_slot(k, "m").copy(), model.get_optimizer_slot(k, "v").copy())
            for k in IO.NAMES}
    assert all(np.abs(m).max() > 0 for _, m, _ in held.values())
    other = model.get_weight("input_bn/gamma").copy()
    for b in batches[1:]:                      # eager, record / capture, replay
        model.train_step(b)
    for k, (w, m, v) in held.items():
        assert np.array_equal(model.get_weight(k), w), k
        assert np.array_equal(model.get_optimizer_slot(k, "m"), m) and np.array_equal(model.get_optimizer_slot(k, "v"), v), k
    assert not np.array_equal(model.get_weight("input_bn/gamma"), other)
    model.check_device_errors()


@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_none_is_the_model_without_the_argument(route):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(5)
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(3)]
    res = []
    for kw in (dict(with_arg=False), dict(with_arg=True)):
        m, _ = build(np.random.default_rng(65), dims, DROP, on=False, **kw)
        m.compile(adam())
        res.append((m, _run(m, batches)))
        assert ("train", B, T) in m._graphs and not hasattr(m, "fmean")
    (a, ra), (b, rb) = res
    assert ra == rb
    assert [(n, e.off) for n, e in a.arena.entries.items()] == [(n, e.off) for n, e in b.arena.entries.items()]
    assert torch.equal(a.arena.theta, b.arena.theta)
    assert torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
