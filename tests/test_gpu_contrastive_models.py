"""nic.NIC(semantic=SemanticTarget(..., loss="contrastive")) on a real MI355X against tests/contrastive_oracle.ContrastiveNIC
(float64; checked against central differences in tests/test_host_contrastive.py), at the tolerances
tests/test_gpu_semantic_models.py takes from tests/test_gpu_nic.py for the same quantities.

  small   N = 96, E = U = 32, V = 37, T = 6, B = 5, G = 24: every extent ragged, numpy batches (the general staging), all
          three Dropouts on; temperature 0.5, soft targets (soft_temperature 0.8), symmetric
  fused   N = 256, E = U = 512, V = 101, T = 4, B = 8, G = 512: device batches (the one-launch staging), the fused encoder
          update, the compact head and the launch plan; temperature 0.07, hard targets, symmetric
Three consecutive train_steps (eager, recorded, replayed), the middle one with a zero target row; the metrics of each,
semantic_top1 among them, the weights behind each; then test_step three times with the arena unchanged, then
predict_embedding.  And loss="cosine" against a model built with today's three-argument SemanticTarget: two steps, the same bits."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch
import contrastive_oracle as CO

pytestmark = pytest.mark.gpu

CASES = {"small": ((5, 96, 6, 37, 32, 32, 24), (0.1, 0.2, 0.2), False, dict(temperature=0.5, soft_temperature=0.8)),
         "fused": ((8, 256, 4, 101, 512, 512, 512), (0, 0.2, 0.2), True, dict(temperature=0.07, soft_temperature=None))}


def build(rng, dims, rates, sem):
    from masters_thesis_amd.nic import NIC
    B, N, T, V, U, E, G = dims
    args = (N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5)
    model = NIC(*args, seed=11, semantic=sem)
    orc = CO.ContrastiveNIC(*args).configure(G, sem.weight, sem.reg)
    orc.configure_loss(sem.temperature, sem.symmetric, sem.soft_temperature).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def batch(rng, dims, on_device, zero_row=None):
    B, N, T, V, U, E, G = dims
    data, tgt = synth_batch(B, N, T, V, U, rng)
    g = rng.standard_normal((B, G)).astype(np.float32)
    if zero_row is not None:
        g[zero_row] = 0
    data = data + (g,)
    if on_device:
        up = lambda a: torch.as_tensor(a).cuda()
        return (tuple(up(a) for a in data), up(tgt)), (data, tgt)
    return (data, tgt), (data, tgt)


def compare(got, res, where):
    for k in ("loss", "L2", "semantic"):
        assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]), (where, k, got, res)
    assert abs(got["accuracy"] - res["accuracy"]) < 1e-6 and abs(got["semantic_top1"] - res["semantic_top1"]) < 1e-6, (where, got, res)


@pytest.mark.parametrize("case", sorted(CASES))
def test_three_steps_test_step_and_embedding(case):
    from masters_thesis_amd.model_base import SemanticTarget
    from masters_thesis_amd.optimizers import Adam
    dims, rates, on_device, loss_kw = CASES[case]
    B, N, T, V, U, E, G = dims
    rng = np.random.default_rng(31)
    model, orc = build(rng, dims, rates, SemanticTarget(G, 0.7, 0.02, loss="contrastive", symmetric=True, **loss_kw))
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noisy_el = {}
    for step in range(3):                       # eager, recorded, replayed; the middle batch has a missing embedding
        given, (data, tgt) = batch(rng, dims, on_device, zero_row=2 if step == 1 else None)
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step(given).as_floats()
        print(f"  {case} step {step}: " + ", ".join(f"{k} {got[k]:.6f} / {res[k]:.6f}" for k in res))
        assert set(got) == set(res)
        compare(got, res, step)
        for k, v in orc.p.items():
            w = model.get_weight(k)
            tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()          # tests/test_gpu_nic.py: against the update size
            if k in grads and grads[k] is not None:
                noisy = noisy_el.setdefault(k, np.zeros(v.shape, bool))
                noisy |= np.abs(grads[k]) < 1e-8
                tol = tol + 1e-3 * (step + 1) * noisy
            assert (np.abs(w - v) <= tol).all(), (step, k, np.abs(w - v).max())
    if on_device:
        plans = [k for k, v in model._graphs.items() if isinstance(v, tuple)]
        print(f"  fused: plans {plans}")
        assert plans and all("semantic" in k and "contrastive" in k for k in plans)
    theta = model.arena.theta.clone()
    given, (data, tgt) = batch(rng, dims, on_device)
    res, _ = orc.test_step(data, tgt)
    for i in range(3):                          # eager, captured, replayed
        compare(model.test_step(given).as_floats(), res, f"test_step {i}")
    assert torch.equal(model.arena.theta, theta)
    want = orc.embed(data[0].astype(np.float64))
    for _ in range(3):
        z = model.predict_embedding(given[0][0])
        assert tuple(z.shape) == (B, G) and z.dtype == torch.float32 and z.is_cuda
        assert np.abs(z.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()
    model.check_device_errors()


@pytest.mark.parametrize("case", sorted(CASES))
def test_cosine_is_todays_three_argument_model(case):
    from masters_thesis_amd.model_base import SemanticTarget
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    dims, rates, on_device, _ = CASES[case]
    B, N, T, V, U, E, G = dims
    models = []
    for sem in (SemanticTarget(G, 0.7, 0.02), SemanticTarget(G, 0.7, 0.02, loss="cosine", temperature=0.5, symmetric=False,
                                                             soft_temperature=0.8)):
        rng = np.random.default_rng(41)
        model = NIC(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, seed=11, semantic=sem)
        model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        mets = []
        for step in range(2):
            given, _ = batch(rng, dims, on_device)
            mets.append(model.train_step(given).as_floats())
        torch.cuda.synchronize()
        assert not hasattr(model, "sem_work") and all(set(m) == {"loss", "L2", "accuracy", "semantic"} for m in mets)
        models.append((model, mets))
    (a, ma), (b, mb) = models
    assert ma == mb
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    assert sorted(map(str, a._graphs)) == sorted(map(str, b._graphs))
