"""Scheduled sampling on the GPU: tnt_scheduled_feedback_f32 against numpy over a grid of shapes, rates and schedules
with planted ties and NaN rows; its ids and projection against tnt_greedy_feedback_f32 at p = 1; nic.NIC's scheduled-
sampling step against the float64 restatement (tests/ss_oracle.py) at a small shape and at config 2; p = 0 against the
teacher-forced step; launch-plan replay against hipGraph replay with the schedule advancing."""
import numpy as np
import pytest
import torch

from helpers import synth_batch
from ss_oracle import SSNICDense, coin, model_tokens, schedule_p, S_LSTM_IN

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
LAM = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, p, mode, seed=7, step=3, counter=5):
    dev = "cuda"
    text = torch.full((B, E), -7.0, device=dev)
    xz = torch.full((B, N), -7.0, device=dev)
    sched = torch.tensor([p, 0.0, 1.0], dtype=torch.float64, device=dev)
    cnt = torch.tensor([counter], dtype=torch.int64, device=dev)
    sd = torch.tensor([step], dtype=torch.int32, device=dev)
    be.scheduled_feedback(logits, logits.shape[1], V, table, E, w, w.shape[1], N, fed, T, col, text, E, xz, N, B, rate, seed,
                          S_LSTM_IN + 1, 0, sd, T * E, col * E, 0, mode, sched, cnt, 176 + col - 1, 208 + col - 1)
    torch.cuda.synchronize()
    return text, xz


@pytest.mark.parametrize("B", [1, 7, 64, 128])
@pytest.mark.parametrize("V", [1, 2, 13, 257, 5001, 16384])
def test_kernel_matches_numpy(be, B, V):
    g = torch.Generator(device="cuda").manual_seed(B * 100003 + V)
    rng = np.random.default_rng(B + V)
    T, col, seed, step = 5, 2, 7, 3
    excluded = total = 0
    for E, N in ((12, 48), (136, 80), (512, 2048)):
        ld = V + 3
        logits = torch.randn(B, ld, generator=g, device="cuda") * 3
        logits[:, V:] = float("nan")
        if V > 2 and B > 1:
            logits[0, :V] = torch.round(logits[0, :V])           # planted ties: the lowest index wins
            logits[1, :] = float("nan")                          # a NaN row: id 0
            logits[B - 1, V // 2] = float("nan")                 # a NaN that never wins
        table = torch.randn(V, E, generator=g, device="cuda")
        w = torch.randn(E, N + 4, generator=g, device="cuda")
        cap = rng.integers(0, V, (B, T)).astype(np.int32)
        lg, tab, wn = logits.cpu().numpy()[:, :V].astype(np.float64), table.cpu().numpy(), w.cpu().numpy()[:, :N]
        for p in (0.0, 0.3, 1.0):
            for mode in (0, 1):
                for rate in (0.0, 0.2):
                    fed = torch.from_numpy(cap.copy()).cuda()
                    text, xz = _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, p, mode)
                    c = coin(B, np.float32(p), seed, 176 + col - 1, step)
                    mids, mg = model_tokens(lg, mode, seed, 208 + col - 1, step)
                    got = fed.cpu().numpy()
                    want = cap.copy()
                    want[c, col] = mids[c]
                    assert np.array_equal(np.delete(got, col, 1), np.delete(cap, col, 1))
                    assert np.array_equal(got[~c, col], cap[~c, col])           # ground-truth rows exactly
                    # greedy ids exactly; sampled ids outside the draw margin, and not on the planted NaN rows, where the
                    # draw is undefined (the id only has to be in range)
                    nanrow = np.isnan(lg).any(1)
                    ok = (~c | ((mg > MARGIN) & ~nanrow)) if mode == 1 else np.ones(B, bool)
                    assert np.array_equal(got[ok, col], want[ok, col]), (E, p, mode, rate)
                    assert np.all((got[:, col] >= 0) & (got[:, col] < V))
                    if mode == 1:
                        excluded += int((~ok & ~nanrow).sum())
                        total += int((c & ~nanrow).sum())
                    ids = got[:, col]
                    rows = tab[ids]
                    if rate > 0:
                        e = np.arange(B)[:, None] * (T * E) + col * E + np.arange(E)[None, :]
                        from mock_backend import _keep
                        k = _keep(e, rate, seed, S_LSTM_IN + 1, step)
                        rows = np.where(k, rows * np.float32(1 / (1 - np.float32(rate))), 0)
                    assert np.allclose(text.cpu().numpy(), rows, rtol=1e-6, atol=1e-6)
                    ref = rows.astype(np.float64) @ wn
                    assert np.abs(xz.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    print(f"B={B} V={V}: {excluded} of {total} sampled rows inside the draw margin")
    assert excluded <= max(2, total // 8)            # the share of draws that fall within 1e-5 of a CDF edge grows with V


@pytest.mark.parametrize("rate", [0.0, 0.2])
def test_greedy_at_p1_equals_greedy_feedback(be, rate):
    g = torch.Generator(device="cuda").manual_seed(3)
    B, V, E, N, T, col = 64, 5001, 512, 2048, 15, 4
    logits = torch.randn(B, V + 3, generator=g, device="cuda")
    logits[:8, :V] = torch.round(logits[:8, :V])
    table = torch.randn(V, E, generator=g, device="cuda")
    w = torch.randn(E, N, generator=g, device="cuda")
    cap = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    fed = cap.clone()
    text, xz = _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, 1.0, 0)
    fed2, text2, xz2 = cap.clone(), torch.zeros(B, E, device="cuda"), torch.zeros(B, N, device="cuda")
    sd = torch.tensor([3], dtype=torch.int32, device="cuda")
    be.greedy_feedback(logits, V + 3, V, table, E, w, N, N, fed2, T, col, text2, E, xz2, N, B, rate, 7, S_LSTM_IN + 1, 0, sd,
                       T * E, col * E)
    torch.cuda.synchronize()
    assert torch.equal(fed, fed2)
    assert torch.equal(text, text2)
    assert torch.equal(xz, xz2)


# ---------------------------------------------------------------------------------------------------- the model
def _case(shape, spec, rates=(0.0, 0.2, 0.2), seed=42):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    if shape == "small":
        B, N, T, V, U, E = 16, 23, 6, 13, 16, 12
    else:
        B, N, T, V, U, E = 64, 20000, 15, 5001, 512, 512
    model = NIC(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, seed=seed, scheduled_sampling=spec)
    model.compile(Adam(1e-3, clipnorm=None))
    orc = SSNICDense(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5)
    orc.p = {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()}
    rng = np.random.default_rng(17)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    return model, orc, data, tgt


@pytest.mark.parametrize("shape", ["small", "config2"])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_model_matches_float64(shape, mode):
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    from oracle import models as M
    spec = SS.linear(0.5, 0.0, mode=mode)
    model, orc, data, tgt = _case(shape, spec)
    w0 = {k: v.copy() for k, v in orc.p.items()}
    drop = M.DropCtx(seed=42, step=0, training=True)
    fed, margin, coins = orc.decide(data, drop, spec, 0)
    got = model.train_step((data, tgt)).as_floats()
    dev_fed = model.cap.cpu().numpy()
    ok = margin > 1e-4
    bad = (dev_fed != fed) & ok
    print(f"{shape} {mode}: {int((~ok).sum())} of {int(coins.sum())} model decisions inside the margin")
    assert not bad.any(), np.argwhere(bad)[:5]
    assert coins.any() and not coins.all()
    ce, acc, grads = orc.loss_and_grads(data, dev_fed.astype(np.int64), tgt, drop)
    assert abs(got["loss"] - ce) < 1e-4 * max(1, abs(ce)) and abs(got["accuracy"] - acc) < 1e-6
    for k in M.NICDense.TRAINABLE:
        gk = model.get_gradient(k) + 2 * LAM.get(k, 0.0) * w0[k]
        ref = grads[k]
        assert np.abs(gk - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-9, k


def test_p_zero_matches_teacher_forced_step():
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    ms, _, data, tgt = _case("config2", SS.linear(0.0, 0.0))
    mt = NIC(20000, 512, 512, 5001, 15, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5, seed=42)
    mt.compile(Adam(1e-3, clipnorm=None))
    rs, rt = ms.train_step((data, tgt)).as_floats(), mt.train_step((data, tgt)).as_floats()
    assert np.array_equal(ms.cap.cpu().numpy(), data[1])
    assert abs(rs["loss"] - rt["loss"]) < 1e-5 * max(1, abs(rt["loss"]))
    for k in mt.trainable_names():
        a, b = ms.get_gradient(k), mt.get_gradient(k)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-12, k


def test_launch_plan_replay_equals_graph_replay():
    """Four scheduled-sampling steps (eager, record / capture, two replays) as a launch plan and as a hipGraph:
    bit-identical metrics, weights and fed ids; p = 0, 0.5, 1, 1 by the live update counter."""
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    spec = SS.linear(0.0, 0.5, mode="sample")
    models = []
    for plan in (True, False):
        m, _, data, tgt = _case("small", spec, rates=(0.1, 0.2, 0.2), seed=5)
        m.plan_step = plan
        models.append(m)
    mets, feds = [[], []], [[], []]
    for step in range(4):
        for i, m in enumerate(models):
            mets[i].append(m.train_step((data, tgt)).as_floats())
            feds[i].append(m.cap.cpu().numpy().copy())
    assert mets[0] == mets[1]
    for a, b in zip(*feds):
        assert np.array_equal(a, b)
    assert np.array_equal(feds[0][0], data[1])                                  # p = 0 at the eager step
    B, T = data[1].shape
    for s in (2, 3):                                                            # replayed, p = 1: every position fed
        c = coin(B, np.float32(1.0), 5, 176, s)
        assert c.all()
    assert not np.array_equal(feds[0][3][:, 1:], data[1][:, 1:])
    assert not np.array_equal(feds[0][3], feds[0][2])                           # a new stream step, new draws
    a, b = models
    for k in a.trainable_names():
        assert np.array_equal(a.get_weight(k), b.get_weight(k)), k
    assert schedule_p(0, spec.params(), 3) == np.float32(1.0)
