"""nic.NIC(semantic=SemanticTarget(...)) on a real MI355X against tests/semantic_oracle.SemanticNIC (float64; checked against
central differences in tests/test_host_semantic.py), at the tolerances tests/test_gpu_nic.py applies to the same quantities of
the plain step.

  small   N = 96, E = U = 32, V = 37, T = 6, B = 5, G = 24: every extent ragged, numpy batches (the general staging), all
          three Dropouts on
  fused   N = 256, E = U = 512, V = 101, T = 4, B = 8, G = 512: device batches (the one-launch staging with the encoder
          forward riding in it), the streaming encoder with its Gram by-products, the fused encoder update, the compact head
          and the launch plan; feature and LSTM-input Dropout on, so that the term reads the dropped feature row and its
          gradient passes enc_tail_bwd_drop
Three consecutive train_steps (eager, recorded, replayed) with another target each, the metrics of each, the weights behind
the last, then test_step and predict_embedding.  Feature off: semantic=None and the model built without the keyword end two
steps with the same bits.  Retrieval end to end: 5 scans against a bank of 203, k = 4."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch
import semantic_oracle as SO

pytestmark = pytest.mark.gpu

CASES = {"small": ((5, 96, 6, 37, 32, 32, 24), (0.1, 0.2, 0.2), False),
         "fused": ((8, 256, 4, 101, 512, 512, 512), (0, 0.2, 0.2), True)}
RETRIEVAL_SEED = 6          # test_retrieval_end_to_end asserts the condition it was chosen for (smallest gap 6.4e-3)


def build(rng, dims, rates, sem, with_arg=True):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.model_base import SemanticTarget
    B, N, T, V, U, E, G = dims
    args = (N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5)
    kw = dict(semantic=SemanticTarget(G, *sem) if sem is not None else None) if with_arg else {}
    model = NIC(*args, seed=11, **kw)
    orc = (SO.SemanticNIC(*args).configure(G, *sem) if sem is not None else M.NICDense(*args)).init_params(rng)
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


@pytest.mark.parametrize("case", sorted(CASES))
def test_three_steps_test_step_and_embedding(case):
    from masters_thesis_amd.optimizers import Adam
    dims, rates, on_device = CASES[case]
    B, N, T, V, U, E, G = dims
    rng = np.random.default_rng(31)
    model, orc = build(rng, dims, rates, (0.7, 0.02))
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noisy_el = {}
    for step in range(3):                       # eager, recorded, replayed; the middle batch has a missing embedding
        given, (data, tgt) = batch(rng, dims, on_device, zero_row=2 if step == 1 else None)
        res, grads, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step(given).as_floats()
        print(f"  {case} step {step}: " + ", ".join(f"{k} {got[k]:.6f} / {res[k]:.6f}" for k in res))
        assert abs(got["loss"] - res["loss"]) <= 1e-4 * abs(res["loss"]), (step, got, res)
        assert abs(got["semantic"] - res["semantic"]) <= 1e-4 * abs(res["semantic"]), (step, got, res)
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        assert abs(got["L2"] - res["L2"]) <= 1e-4 * abs(res["L2"])
        for k, v in orc.p.items():
            w = model.get_weight(k)
            tol = 2e-2 * 1e-3 + 1e-4 * np.abs(v).max()          # tests/test_gpu_nic.py: against the update size
            if k in grads and grads[k] is not None:
                noisy = noisy_el.setdefault(k, np.zeros(v.shape, bool))
                noisy |= np.abs(grads[k]) < 1e-8
                tol = tol + 1e-3 * (step + 1) * noisy
            assert (np.abs(w - v) <= tol).all(), (step, k, np.abs(w - v).max())
    if on_device:                               # the routes the case is there for
        route = model._route
        plans = [k for k, v in model._graphs.items() if isinstance(v, tuple)]
        print(f"  fused: compact head {route.head_map_fresh}, staged forward {route.stage_fwd_done}, "
              f"Gram {model._enc_gram is not None}, fused encoder update {model._enc_last_fused is not None}, plans {plans}")
        assert model.enc_part is not None and model._enc_gram is not None and model._enc_last_fused is not None
        assert plans and all("semantic" in k for k in plans)
        if model._seq_lstm:                     # the persistent chains (a device census): with them the compact head
            assert route.head_map_fresh and route.stage_fwd_done
    theta = model.arena.theta.clone()
    given, (data, tgt) = batch(rng, dims, on_device)
    res, _ = orc.test_step(data, tgt)
    for _ in range(3):                          # eager, captured, replayed
        got = model.test_step(given).as_floats()
        for k in ("loss", "L2", "semantic"):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]), (k, got, res)
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
    assert torch.equal(model.arena.theta, theta)
    want = orc.embed(data[0].astype(np.float64))
    for _ in range(3):
        z = model.predict_embedding(given[0][0])
        assert tuple(z.shape) == (B, G) and z.dtype == torch.float32 and z.is_cuda
        assert np.abs(z.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()
    model.check_device_errors()


@pytest.mark.parametrize("case", sorted(CASES))
def test_none_is_the_model_without_the_keyword(case):
    from masters_thesis_amd.optimizers import Adam
    dims, rates, on_device = CASES[case]
    models = []
    for with_arg in (False, True):
        rng = np.random.default_rng(41)
        model, _ = build(rng, dims, rates, None, with_arg)
        model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        mets = []
        for step in range(2):
            given, _ = batch(rng, dims, on_device)          # the fifth input rides along and is ignored
            mets.append(model.train_step(given).as_floats())
        torch.cuda.synchronize()
        assert not hasattr(model, "sem_z") and all("semantic" not in m for m in mets)
        models.append((model, mets))
    (a, ma), (b, mb) = models
    assert ma == mb
    assert torch.equal(a.arena.theta, b.arena.theta) and torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    assert sorted(map(str, a._graphs)) == sorted(map(str, b._graphs))


def retrieval_inputs(seed):
    dims = CASES["small"][0]
    B, N, T, V, U, E, G = dims
    rng = np.random.default_rng(seed)
    args = (N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5)
    orc = SO.SemanticNIC(*args).configure(G).init_params(rng)
    x = rng.standard_normal((B, N)).astype(np.float32)
    bank = rng.standard_normal((203, G)).astype(np.float32)
    z = orc.embed(x.astype(np.float64))
    b64 = bank.astype(np.float64)
    sims = (z / np.linalg.norm(z, axis=1)[:, None]) @ (b64 / np.linalg.norm(b64, axis=1)[:, None]).T
    return args, orc, x, bank, sims


def test_retrieval_end_to_end():
    """5 queries, M = 203, G = 24, k = 4 through predict_embedding, SemanticBank and semantic_retrieve.  The product's rounding
    may reorder near ties, so first the condition on the input, in float64 on the CPU: every gap among each query's k + 1
    largest similarities is at least 1e-3.  Then the indices are the float64 ranking's."""
    from masters_thesis_amd import evaluate
    from masters_thesis_amd.model_base import SemanticTarget
    from masters_thesis_amd.nic import NIC
    k = 4
    args, orc, x, bank_rows, sims = retrieval_inputs(RETRIEVAL_SEED)
    top = -np.sort(-sims, axis=1)[:, :k + 1]
    assert (top[:, :-1] - top[:, 1:]).min() >= 1e-3, "RETRIEVAL_SEED: the input has a near tie among the top k + 1"
    model = NIC(*args, seed=11, semantic=SemanticTarget(24))
    for name, v in orc.p.items():
        model.set_weight(name, v)
    bank = evaluate.SemanticBank(bank_rows, device="cuda")
    idx, sim, full = evaluate.semantic_retrieve(model, x, bank, k=k, return_sims=True)
    want = np.argsort(-sims, axis=1)[:, :k]
    assert np.array_equal(idx, want.astype(np.int32)), (idx, want)
    assert np.abs(sim - np.take_along_axis(sims, want, 1)).max() <= 1e-4 and np.abs(full - sims).max() <= 1e-4
    assert np.array_equal(sim, np.take_along_axis(full, want, 1))
    res = evaluate.semantic_identification(model, x, bank, [{int(i), int(j)} for i, j in idx[:, 1:3]])
    assert res["rank"].tolist() == [1] * len(x) and res["top1"] == 0.0 and res["top5"] == 1.0 and res["mrr"] == 0.5
