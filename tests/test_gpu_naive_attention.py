"""Free-running decoder on the GPU: tnt_greedy_feedback_f32 against float64 numpy, lc_nic.NIC(teacher_forcing=False) against
the float64 restatement (tests/naive_oracle.py) at a small shape and at config 3's size, free-running inference against
greedy_predict, and launch-plan replay == hipGraph replay."""
import numpy as np
import pytest
import torch

from oracle import models as M
from mock_backend import _keep
from naive_oracle import NaiveLcNIC

pytestmark = pytest.mark.gpu


def _margins(logits):
    """top-2 gap of every row of float64 logits (..., V)"""
    s = np.sort(logits, axis=-1)
    return s[..., -1] - s[..., -2]


@pytest.mark.parametrize("B", [1, 7, 64, 128])
@pytest.mark.parametrize("Et,U", [(12, 16), (512, 512)])
@pytest.mark.parametrize("V", [13, 5001])
@pytest.mark.parametrize("rate", [0.0, 0.2])
def test_greedy_feedback_kernel(B, Et, U, V, rate):
    from masters_thesis_amd import ops
    be = ops.backend()
    rng = np.random.default_rng(B * 7 + Et + V)
    dev = "cuda:0"
    D, T, col, seed, site, step = 16, 5, 3, 1234567, 51, 9
    ld = (V + 3) // 4 * 4 + 4
    N = 4 * U
    lg = rng.standard_normal((B, ld)).astype(np.float32)
    lg[:, V:] = 1e9                                          # beyond V: never read
    if B > 1:
        lg[1, :V] = np.nan                                   # no winner: id 0
    if B > 2:
        m = lg[2, :V].max() + 1.0
        lg[2, [V // 3, V // 2, V - 1]] = m                   # exact tie: lowest index
    if B > 3:
        lg[3, : V // 2] = np.nan                             # NaN never wins
    table = rng.uniform(-0.08, 0.08, (V, Et)).astype(np.float32)
    w = rng.uniform(-0.1, 0.1, (Et, N)).astype(np.float32)
    ids_want = np.zeros(B, np.int64)
    for b in range(B):
        r = lg[b, :V]
        ok = ~np.isnan(r)
        if ok.any():
            ids_want[b] = np.flatnonzero(r == r[ok].max())[0]
    if B > 2:
        assert ids_want[2] == V // 3
    rows = table[ids_want]
    if rate > 0:
        keep = _keep(np.arange(B)[:, None] * (D + Et) + D + np.arange(Et)[None, :], rate, seed, site, step + 2)
        rows = np.where(keep, rows * (np.float32(1) / (np.float32(1) - np.float32(rate))), np.float32(0))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fed = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    text = torch.zeros(B, Et, device=dev)
    xz = torch.full((B, N), np.nan, device=dev)
    step_dev = torch.tensor([2], dtype=torch.int32, device=dev)
    be.greedy_feedback(t(lg), ld, V, t(table), Et, t(w), N, N, fed, T, col, text, Et, xz, N, B, rate, seed, site, step,
                       step_dev, lwidth=D + Et, lcol0=D)
    torch.cuda.synchronize()
    f = fed.cpu().numpy()
    assert np.array_equal(f[:, col], ids_want) and (f[:, col] >= 0).all() and (f[:, col] < V).all()
    assert (np.delete(f, col, axis=1) == -7).all()
    assert np.array_equal(text.cpu().numpy(), rows)          # gather + mask: exact
    want = rows.astype(np.float64) @ w.astype(np.float64)
    bound = 1e-6 * (np.abs(rows).astype(np.float64) @ np.abs(w).astype(np.float64)) + 1e-30
    assert (np.abs(xz.cpu().numpy() - want) <= bound).all(), np.abs(xz.cpu().numpy() - want).max()


def _small(rates, seed=11, **kw):
    from masters_thesis_amd.lc_nic import NIC
    from helpers import tiny_groups
    rng = np.random.default_rng(3)
    N, R, D, A, U, Et, V, T = 200, 6, 16, 8, 32, 16, 37, 6
    g = (tiny_groups(N, R, rng), [D] * R)
    model = NIC(g, U, 512, Et, A, V, T, *rates, 0.01, 0.001, 3e-5, 1e-5, device="cuda:0", seed=seed, teacher_forcing=False, **kw)
    orc = NaiveLcNIC(g, U, 512, Et, A, V, T, *rates, 0.01, 0.001, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc, dict(B=8, N=N, T=T, V=V, U=U)


@pytest.mark.parametrize("rates", [(0,) * 6, (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)])
def test_small_model_train_steps_match_restatement(rates):
    from masters_thesis_amd.optimizers import Adam
    from helpers import synth_batch
    rng = np.random.default_rng(41)
    model, orc, d = _small(rates)
    model.compile(Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    opt = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    for step in range(3):
        data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng)
        got = model.train_step((data, tgt)).as_floats()
        fed = model.fed_ids()
        res, _, _ = orc.train_step(data, tgt, opt, M.DropCtx(seed=11, step=step, training=True), fed_ids=fed)
        for k in ("loss", "L2", "attention"):
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        for k, v in orc.p.items():       # the bounds of tests/test_gpu_lcnic.py::test_train_parity
            if k == "attention/V/bias":
                continue
            w = model.get_weight(k)
            assert np.abs(w - v).max() <= 2e-2 * 1e-3 + 1e-4 * np.abs(v).max(), (step, k, np.abs(w - v).max())


# config 3 (BASELINE / bench.py make_model("attention"))
B3, T3, V3, U3, E3, N3 = 64, 15, 5001, 512, 512, 20000
RATES3 = (0.0, 0.2, 0.2, 0.2, 0.2, 0.2)


def _config3(seed=42):
    from masters_thesis_amd.lc_nic import NIC, synthetic_groups
    from masters_thesis_amd.optimizers import Adam
    g = synthetic_groups(N3, 360, 32, seed=42)
    m = NIC(g, U3, 512, E3, 32, V3, T3, *RATES3, 0.01, 0.001, 0.00003, 0.00001, seed=seed, teacher_forcing=False)
    m.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    orc = NaiveLcNIC(g, U3, 512, E3, 32, V3, T3, *RATES3, 0.01, 0.001, 0.00003, 0.00001)
    orc.p = {k: v.astype(np.float64) for k, v in m.get_weights_dict().items()}
    return m, orc


def _synth3(rng):
    x = rng.standard_normal((B3, N3)).astype(np.float32)
    cap = np.zeros((B3, T3), np.int32)
    cap[:, 0] = 1
    tgt = rng.integers(3, V3, size=(B3, T3)).astype(np.int32)
    z = np.zeros((B3, U3), np.float32)
    return (x, cap, z, z.copy()), tgt


def test_config3_training_step_matches_restatement():
    """One free-running training step at config 3's size: loss and every gradient within 1e-4 of the float64
    restatement run on the device's fed ids; the fed ids equal the restatement's own argmax wherever the top-2 logit
    margin exceeds 1e-4 (near ties are where float32 and float64 may legitimately disagree)."""
    rng = np.random.default_rng(21)
    model, orc = _config3()
    names = [k for k in orc.p if "moving_" not in k]
    lam = {k: model.arena.entries[k].l2 for k in names}
    w0 = {k: v.copy() for k, v in orc.p.items()}
    data, tgt = _synth3(rng)
    got = model.train_step((data, tgt)).as_floats()
    model.check_device_errors()
    fed = model.fed_ids()
    opt = M.AdamState({k: orc.p[k] for k in names}, lr=1e-4, clipnorm=0.1)
    res, grads, (_, _, cache) = orc.train_step(data, tgt, opt, M.DropCtx(seed=model.seed, step=0, training=True), fed_ids=fed)
    for k in ("loss", "L2", "attention", "accuracy"):
        tol = 1e-6 if k == "accuracy" else 1e-4 * abs(res[k]) + 1e-7
        assert abs(got[k] - res[k]) <= tol, (k, got[k], res[k])
    for k in names:
        if k == "attention/V/bias":                      # softmax shift invariance: the true gradient is 0
            continue
        gm = model.get_gradient(k).astype(np.float64) + 2 * lam[k] * w0[k]
        scale = np.abs(grads[k]).max()
        assert np.abs(gm - grads[k]).max() <= 1e-4 * scale + 1e-10, (k, np.abs(gm - grads[k]).max(), scale)
    mg = _margins(cache["logits"][:, :-1])               # (B, T-1): step i's prediction is fed to step i + 1
    ok = mg > 1e-4
    print(f"config-3 fed ids: {int((~ok).sum())} of {ok.size} predictions excluded as near ties (margin <= 1e-4)")
    assert ok.mean() > 0.9
    assert np.array_equal(fed[:, 1:][ok], cache["preds"][:, :-1][ok])


def test_config3_inference_matches_greedy_predict():
    """call_naive_attention(training=False) at config 3's size: the ids of greedy_predict for every sample whose decode
    has no near tie (top-2 logit margin > 1e-4 at every step of the float64 restatement), probabilities within 1e-5."""
    rng = np.random.default_rng(22)
    model, orc = _config3()
    data, _ = _synth3(rng)
    probs, _, ids = model.call_naive_attention(data, training=False, return_ids=True)
    z = np.zeros((B3, U3), np.float32)
    gw, gp, _, _ = model.greedy_predict(data[0], z, z, data[1][:, 0], T3, return_s=False)
    (_, _), cache = orc.forward(data, training=False)
    ok = (_margins(cache["logits"]) > 1e-4).all(axis=1)
    print(f"config-3 inference: {int((~ok).sum())} of {B3} samples excluded (a near tie on their decode)")
    assert ok.mean() > 0.75
    assert np.array_equal(ids.cpu().numpy()[ok], gw[ok, :, 0])
    assert np.array_equal(ids.cpu().numpy()[ok], cache["preds"][ok])
    assert np.abs(probs.cpu().numpy()[ok] - gp[ok]).max() < 1e-5


def test_launch_plan_replay_equals_graph_replay_free_running():
    """Three free-running training steps replayed as a launch plan (the default) and as a hipGraph (plan_step=False):
    bit-identical weights, Adam moments and metrics."""
    from masters_thesis_amd.optimizers import Adam
    from helpers import synth_batch
    rates = (0.1, 0.2, 0.2, 0.2, 0.2, 0.2)
    models = []
    for plan in (True, False):
        m, _, d = _small(rates, seed=5)
        m.plan_step = plan
        m.compile(Adam(learning_rate=1e-3, clipnorm=0.1))
        models.append(m)
    rng = np.random.default_rng(8)
    batches = [synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], rng) for _ in range(3)]
    mets = [[m.train_step(b).as_floats() for b in batches] for m in models]
    assert mets[0] == mets[1]
    a, b = models
    for k in a.trainable_names():
        assert np.array_equal(a.get_weight(k), b.get_weight(k)), k
        for slot in ("m", "v"):
            assert np.array_equal(a.get_optimizer_slot(k, slot), b.get_optimizer_slot(k, slot)), (k, slot)
    assert np.array_equal(a.fed_ids(), b.fed_ids())
