"""lc_nic.NIC(attention_coverage=...) on the GPU against the float64 oracle model that differentiates
CE + L2 + weight * coverage (tests/coverage_oracle.py: CoverageLcNIC), both axes on both routes of the backward chain:
  per-step   a tiny model with U = 16 (tnt_attention_step_bwd_ext_f32 per step on the step's slab of the rider)
  chain      U = 512, B = 5, R = 129, T = 3 (tnt_lc_seq_bwd_ext_f32, lc_seq_bwd_kernel<8, 3, 8>; asserted: _lc_seq_bwd_ok())
with the tolerances tests/test_gpu_lcnic.py applies to the plain step: loss, L2, attention (and coverage) 1e-4 relative + 1e-7,
gradients 2e-4 of the variable's largest gradient + 1e-9 (dropout-free, as there), post-Adam weights 2e-2 * lr + 1e-4 of the
variable's largest weight.  ``WEIGHT`` is chosen per route and axis so that the oracle's gradient of attention/V/kernel
with and without the term differ by at least 100 times that gradient tolerance (asserted on the CPU in every case): near
initialisation the attention over 129 regions is almost uniform, where a gradient that is nearly the same for every region
cancels in the softmax, so the chain route's weight is the larger one.
Then: plan, hipGraph and eager steps bit-identical; two weights, two captures; test_step reports ``coverage`` and changes no
weight; attention_coverage=None is the model built without the argument, bit for bit."""
import numpy as np
import pytest
import torch

import coverage_oracle as CO
from oracle import models as M
from helpers import synth_batch, tiny_groups

pytestmark = pytest.mark.gpu

# route -> (B, N, R, D, A, U, Et, V, T)
DIMS = {"per-step": (3, 37, 4, 16, 3, 16, 8, 11, 4), "chain": (5, 700, 129, 32, 32, 512, 64, 101, 3)}
WEIGHT = {("per-step", "time"): 0.05, ("per-step", "batch"): 0.05, ("chain", "time"): 5.0, ("chain", "batch"): 5.0}
DROP = (0.0, 0.2, 0.2, 0.2, 0.2, 0.2)
GTOL = 2e-4


def build(rng, dims, rates=(0,) * 6, coverage=None, with_arg=True, **kw):
    from masters_thesis_amd.lc_nic import NIC
    from masters_thesis_amd.model_base import AttentionCoverage
    B, N, R, D, A, U, Et, V, T = dims
    g = (tiny_groups(N, R, rng), [D] * R)
    args = (g, U, 512, Et, A, V, T, *rates, 0.01, 0.001, 3e-5, 1e-5)
    if with_arg:
        kw["attention_coverage"] = AttentionCoverage(*coverage) if coverage is not None else None
    model = NIC(*args, seed=11, **kw)
    orc = CO.CoverageLcNIC(*args).init_params(rng)
    orc.coverage = coverage
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


@pytest.mark.parametrize("axis", CO.AXES)
@pytest.mark.parametrize("route,rates", [("per-step", (0,) * 6), ("chain", (0,) * 6), ("chain", DROP)],
                         ids=["per-step", "chain", "chain-dropout"])
def test_train_step_against_the_oracle(route, rates, axis):
    rng = np.random.default_rng(61)
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    weight = WEIGHT[route, axis]
    model, orc = build(rng, dims, rates, (weight, axis))
    model.compile(adam())
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    lam = lambda k: model.arena.entries[k].l2
    for step in range(3):                      # eager, record / capture, replay
        data, tgt = synth_batch(B, N, T, V, U, rng)
        w0 = {k: v.copy() for k, v in orc.p.items()}
        if step == 0:                          # the term is far above the tolerance of the gradient it is checked in
            (probs, attn), cache = orc.forward(data, training=True, drop=M.DropCtx(seed=11, step=0, training=True))
            on, _ = orc.backward(probs, cache, tgt)
            orc.coverage = None
            off, _ = orc.backward(probs, cache, tgt)
            orc.coverage = (weight, axis)
            k = "attention/V/kernel"
            moved = np.abs(on[k] - off[k]).max()
            print(f"\n[{route} {axis}] the term moves d {k} by {moved / (GTOL * np.abs(on[k]).max()):.0f} tolerances")
            assert moved >= 100 * GTOL * np.abs(on[k]).max(), (moved, np.abs(on[k]).max())
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        if step == 0:
            assert model._lc_seq_bwd_ok() == (route == "chain")
        assert set(got) == {"loss", "L2", "accuracy", "attention", "coverage", "lr"}
        for k in ("loss", "L2", "attention", "coverage"):
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


@pytest.mark.parametrize("axis", CO.AXES)
@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_plan_graph_and_eager_steps_are_bit_identical(route, axis):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(5)
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(4)]
    models = []
    for kind in ("plan", "graph", "eager"):
        m, _ = build(np.random.default_rng(62), dims, DROP, (WEIGHT[route, axis], axis), use_graph=kind != "eager")
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
    key = ("train", B, T, "coverage", WEIGHT[route, axis], axis)
    assert key in a._graphs and key in b._graphs


def test_two_weights_do_not_share_a_capture():
    """the coefficient is a launch argument fixed at record / capture time: a model with another weight records its own
    sequence under its own key, and each replay equals its eager twin"""
    dims = DIMS["chain"]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(5)
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(3)]
    thetas = {}
    for w in (5.0, 1.25):
        pair = []
        for graph in (True, False):
            m, _ = build(np.random.default_rng(63), dims, (0,) * 6, (w, "time"), use_graph=graph)
            m.compile(adam())
            _run(m, batches)
            pair.append(m)
        assert ("train", B, T, "coverage", w, "time") in pair[0]._graphs
        assert all(k[3:] == ("coverage", w, "time") for k in pair[0]._graphs if k[0] == "train")
        assert torch.equal(pair[0].arena.theta, pair[1].arena.theta)
        thetas[w] = pair[0].arena.theta.clone()
    assert not torch.equal(thetas[5.0], thetas[1.25])


@pytest.mark.parametrize("axis", CO.AXES)
def test_test_step_reports_coverage_and_changes_no_weight(axis):
    dims = DIMS["chain"]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(64)
    model, orc = build(rng, dims, (0,) * 6, (WEIGHT["chain", axis], axis))
    model.compile(adam())
    theta = model.arena.theta.clone()
    for _ in range(3):                         # eager, capture, replay
        data, tgt = synth_batch(B, N, T, V, U, rng)
        res, _ = orc.test_step(data, tgt)
        got = model.test_step((data, tgt)).as_floats()
        assert set(got) == {"loss", "L2", "accuracy", "attention", "coverage"}
        for k in ("loss", "L2", "attention", "coverage"):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (k, got[k], res[k])
        if axis == "batch":                    # the same sums as the attention metric, to float32 rounding
            assert abs(got["coverage"] - got["attention"]) <= 1e-5 * got["attention"]
    assert torch.equal(model.arena.theta, theta)


@pytest.mark.parametrize("route", ["per-step", "chain"])
def test_none_is_the_model_without_the_argument(route):
    dims = DIMS[route]
    B, N, R, D, A, U, Et, V, T = dims
    rng = np.random.default_rng(5)
    batches = [synth_batch(B, N, T, V, U, rng) for _ in range(3)]
    res = []
    for kw in (dict(with_arg=False), dict(coverage=None), dict(coverage=(0.0, "batch"))):
        m, _ = build(np.random.default_rng(65), dims, DROP, **kw)
        m.compile(adam())
        res.append((m, _run(m, batches)))
        assert all("coverage" not in r for r in res[-1][1])
        assert ("train", B, T) in m._graphs and not any("coverage" in k for k in m._graphs)
    for m, r in res[1:]:
        assert r == res[0][1]
        assert torch.equal(m.arena.theta, res[0][0].arena.theta)
        assert torch.equal(m.opt_m, res[0][0].opt_m) and torch.equal(m.opt_v, res[0][0].opt_v)
