"""Scheduled sampling for the attention model on the GPU: tnt_scheduled_feedback2_f32 against numpy over a grid of shapes,
schedules and both masks' rates, with planted ties and NaN rows; against tnt_scheduled_feedback_f32 (rate_t = 0) and
tnt_embedding_fwd_drop2_f32 (p = 0); lc_nic.NIC's scheduled-sampling step against the float64 restatement
(tests/ss_att_oracle.py) at a small shape and at config 3; p = 0 against the teacher-forced step; launch-plan replay against
hipGraph replay with the schedule advancing."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import synth_batch, tiny_groups
from ss_att_oracle import SSAttLcNIC, coin, masked_rows, model_tokens, schedule_p

pytestmark = pytest.mark.gpu

S_TEXT, S_LSTM_IN = 3, 48
S_SS_COIN, S_SS_DRAW = 176, 208
MARGIN = 1e-5


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, rate_t, p, mode, D=16, seed=7, step=3, counter=5, two=True):
    """one launch on fresh outputs (pre-filled with -7); the teacher-forced masks of (b, col): the LSTM input mask over
    (B, D + E) on S_LSTM_IN + col, the text Dropout over (B, T, E) on S_TEXT"""
    dev = "cuda"
    text = torch.full((B, E), -7.0, device=dev)
    xz = torch.full((B, N), -7.0, device=dev)
    sched = torch.tensor([p, 0.0, 1.0], dtype=torch.float64, device=dev)
    cnt = torch.tensor([counter], dtype=torch.int64, device=dev)
    sd = torch.tensor([step], dtype=torch.int32, device=dev)
    args = (logits, logits.shape[1], V, table, E, w, w.shape[1], N, fed, T, col, text, E, xz, N, B, rate, seed,
            S_LSTM_IN + col, 0, sd, D + E, D, 0, mode, sched, cnt, S_SS_COIN + col - 1, S_SS_DRAW + col - 1)
    if two:
        be.scheduled_feedback2(*args, rate_t, S_TEXT, T * E, col * E)
    else:
        be.scheduled_feedback(*args)
    torch.cuda.synchronize()
    return text, xz


@pytest.mark.parametrize("B", [1, 7, 64, 128])
@pytest.mark.parametrize("V", [2, 13, 5001, 16384])
def test_kernel_matches_numpy(be, B, V):
    g = torch.Generator(device="cuda").manual_seed(B * 100003 + V)
    rng = np.random.default_rng(B + V)
    T, col, seed, step, D = 5, 2, 7, 3, 16
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
            c = coin(B, np.float32(p), seed, S_SS_COIN + col - 1, step)
            for mode in (0, 1):
                mids, mg = model_tokens(lg, mode, seed, S_SS_DRAW + col - 1, step)
                for rate_t, rate in ((0.0, 0.0), (0.2, 0.0), (0.0, 0.25), (0.2, 0.25)):
                    fed = torch.from_numpy(cap.copy()).cuda()
                    text, xz = _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, rate_t, p, mode)
                    got = fed.cpu().numpy()
                    want = cap.copy()
                    want[c, col] = mids[c]
                    assert np.array_equal(np.delete(got, col, 1), np.delete(cap, col, 1))      # untouched columns
                    assert np.array_equal(got[~c, col], cap[~c, col])                           # ground-truth rows
                    nanrow = np.isnan(lg).any(1)
                    ok = (~c | ((mg > MARGIN) & ~nanrow)) if mode == 1 else np.ones(B, bool)
                    assert np.array_equal(got[ok, col], want[ok, col]), (E, p, mode, rate_t, rate)
                    assert np.all((got[:, col] >= 0) & (got[:, col] < V))
                    if mode == 1:
                        excluded += int((~ok & ~nanrow).sum())
                        total += int((c & ~nanrow).sum())
                    rows = masked_rows(tab[got[:, col]], B, E, [(rate_t, S_TEXT, T * E, col * E),
                                                                 (rate, S_LSTM_IN + col, D + E, D)], seed, step)
                    assert np.array_equal(text.cpu().numpy(), rows), (E, p, mode, rate_t, rate)    # both masks: exact
                    ref = rows.astype(np.float64) @ wn
                    bound = 1e-6 * (np.abs(rows).astype(np.float64) @ np.abs(wn)) + 1e-30
                    assert (np.abs(xz.cpu().numpy() - ref) <= bound).all(), np.abs(xz.cpu().numpy() - ref).max()
    print(f"B={B} V={V}: {excluded} of {total} sampled rows inside the draw margin")
    assert excluded <= max(2, total // 8)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("p", [0.3, 1.0])
def test_rate_t_zero_equals_scheduled_feedback(be, mode, p):
    g = torch.Generator(device="cuda").manual_seed(3)
    B, V, E, N, T, col = 64, 5001, 512, 2048, 15, 4
    logits = torch.randn(B, V + 3, generator=g, device="cuda")
    logits[:8, :V] = torch.round(logits[:8, :V])
    table = torch.randn(V, E, generator=g, device="cuda")
    w = torch.randn(E, N, generator=g, device="cuda")
    cap = torch.randint(0, V, (B, T), generator=g, device="cuda", dtype=torch.int32)
    fed1, fed2 = cap.clone(), cap.clone()
    t1, x1 = _launch(be, logits, V, table, E, w, N, fed1, T, col, B, 0.2, 0.0, p, mode)
    t2, x2 = _launch(be, logits, V, table, E, w, N, fed2, T, col, B, 0.2, 0.0, p, mode, two=False)
    assert torch.equal(fed1, fed2) and torch.equal(t1, t2) and torch.equal(x1, x2)


@pytest.mark.parametrize("rate_t,rate", [(0.2, 0.2), (0.2, 0.0), (0.0, 0.2)])
def test_p_zero_rows_equal_embedding_drop2(be, rate_t, rate):
    """p = 0: every row keeps the caption, and its text row is the bits of tnt_embedding_fwd_drop2_f32's row (b, col)"""
    g = torch.Generator(device="cuda").manual_seed(4)
    B, V, E, N, T, D = 64, 5001, 512, 2048, 15, 32
    table = torch.randn(V, E, generator=g, device="cuda")
    w = torch.randn(E, N, generator=g, device="cuda")
    logits = torch.randn(B, V, generator=g, device="cuda")
    cap = torch.randint(0, V, (B, T), generator=g, device="cuda", dtype=torch.int32)
    full = torch.empty(T * B, E, device="cuda")
    sd = torch.tensor([3], dtype=torch.int32, device="cuda")
    be.embedding_fwd_drop(table, cap, None, full, B, T, E, E, V, rate_t, 7, S_TEXT, 0, sd,
                          mask2=(rate, S_LSTM_IN, D + E, D) if rate > 0 else None)
    for col in (1, 7, T - 1):
        fed = cap.clone()
        text, xz = _launch(be, logits, V, table, E, w, N, fed, T, col, B, rate, rate_t, 0.0, 1, D=D)
        assert torch.equal(fed, cap)
        assert torch.equal(text, full[col * B:(col + 1) * B]), col


# ---------------------------------------------------------------------------------------------------- the model
B3, T3, V3, U3, E3, N3 = 64, 15, 5001, 512, 512, 20000
RATES3 = (0.0, 0.2, 0.2, 0.2, 0.2, 0.2)


def _case(shape, spec, rates=None, seed=42):
    """the model with scheduled_sampling=spec, its restatement on the model's weights, one batch"""
    from masters_thesis_amd.lc_nic import NIC, synthetic_groups
    from masters_thesis_amd.optimizers import Adam
    rng = np.random.default_rng(17)
    if shape == "small":
        B, N, R, D, A, U, Et, V, T = 16, 200, 6, 16, 8, 32, 16, 37, 6
        g = (tiny_groups(N, R, rng), [D] * R)
        rates = (0.1, 0.2, 0.2, 0.2, 0.2, 0.2) if rates is None else rates
    else:
        B, N, A, U, Et, V, T = B3, N3, 32, U3, E3, V3, T3
        g = synthetic_groups(N, 360, 32, seed=42)
        rates = RATES3 if rates is None else rates
    args = (U, 512, Et, A, V, T, *rates, 0.01, 0.001, 0.00003, 0.00001)
    model = NIC(g, *args, seed=seed, scheduled_sampling=spec)
    model.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    orc = SSAttLcNIC(g, *args)
    orc.p = {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()}
    data, tgt = synth_batch(B, N, T, V, U, rng)
    return model, orc, data, tgt, (g, args)


@pytest.mark.parametrize("shape", ["small", "config3"])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_model_matches_float64(shape, mode):
    """One scheduled-sampling step at p = 0.5: the fed ids are the restatement's own decisions (on the device's history)
    wherever the decision margin is clear -- greedy: a top-2 logit gap above 1e-4; sample: the draw's distance from the
    nearest CDF edge above 1e-5 of the total (one CDF step at V = 5001 is ~2e-4 of it, so 1e-4 would exclude almost every
    draw); some rows took the model's token and some did not; loss and every gradient within 1e-4 of the max-abs value of
    the float64 step on the fed ids."""
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    spec = SS.linear(0.5, 0.0, mode=mode)
    model, orc, data, tgt, _ = _case(shape, spec)
    names = [k for k in orc.p if "moving_" not in k]
    w0 = {k: v.copy() for k, v in orc.p.items()}
    got = model.train_step((data, tgt)).as_floats()
    model.check_device_errors()
    dev = model.fed_ids().astype(np.int64)
    drop = M.DropCtx(seed=model.seed, step=0, training=True)
    own, margin, coins = orc.decide(data, drop, spec, 0, fed_ids=dev)
    th = 1e-4 if mode == "greedy" else 1e-5
    ok = margin > th
    print(f"{shape} {mode}: {int((~ok).sum())} of {int(coins.sum())} model decisions inside the {th:g} margin")
    assert np.array_equal(dev[ok], own[ok]), np.argwhere((dev != own) & ok)[:5]
    assert coins.any() and not coins.all()
    assert (~ok).sum() <= 0.25 * coins.sum()
    model_rows = np.pad(coins, ((0, 0), (1, 0)))
    assert np.array_equal(dev[~model_rows], data[1][~model_rows])
    assert not np.array_equal(dev, data[1])
    ce, acc, al, grads = orc.loss_and_grads(data, dev, tgt, drop)
    assert abs(got["loss"] - ce) <= 1e-4 * abs(ce) + 1e-7, (got["loss"], ce)
    assert abs(got["attention"] - al) <= 1e-4 * abs(al) + 1e-7, (got["attention"], al)
    assert abs(got["accuracy"] - acc) < 1e-6
    for k in names:
        if k == "attention/V/bias":                      # softmax shift invariance: the true gradient is 0
            continue
        gm = model.get_gradient(k).astype(np.float64) + 2 * model.arena.entries[k].l2 * w0[k]
        scale = np.abs(grads[k]).max()
        assert np.abs(gm - grads[k]).max() <= 1e-4 * scale + 1e-10, (k, np.abs(gm - grads[k]).max(), scale)


def test_p_zero_matches_teacher_forced_step():
    """p = 0 at config 3: the fed ids are the caption; loss and gradients within 1e-4 of the teacher-forced model's"""
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    from masters_thesis_amd.lc_nic import NIC
    from masters_thesis_amd.optimizers import Adam
    ms, _, data, tgt, (g, args) = _case("config3", SS.linear(0.0, 0.0))
    mt = NIC(g, *args, seed=42)
    mt.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    rs, rt = ms.train_step((data, tgt)).as_floats(), mt.train_step((data, tgt)).as_floats()
    ms.check_device_errors()
    mt.check_device_errors()
    assert np.array_equal(ms.fed_ids(), data[1])
    for k in ("loss", "attention"):
        assert abs(rs[k] - rt[k]) <= 1e-4 * abs(rt[k]) + 1e-7, (k, rs[k], rt[k])
    assert abs(rs["accuracy"] - rt["accuracy"]) < 1e-6
    for k in mt.trainable_names():
        if k == "attention/V/bias":
            continue
        a, b = ms.get_gradient(k), mt.get_gradient(k)
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max() + 1e-10, (k, np.abs(a - b).max())


def test_launch_plan_replay_equals_graph_replay():
    """Four scheduled-sampling steps (eager, record / capture, two replays) as a launch plan and as a hipGraph:
    bit-identical metrics, fed ids and weights; p = 0, 0.5, 1, 1 by the live update counter."""
    from masters_thesis_amd.model_base import ScheduledSampling as SS
    spec = SS.linear(0.0, 0.5, mode="sample")
    models = []
    for plan in (True, False):
        m, _, data, tgt, _ = _case("small", spec, seed=5)
        m.plan_step = plan
        models.append(m)
    mets, feds = [[], []], [[], []]
    for _ in range(4):
        for i, m in enumerate(models):
            mets[i].append(m.train_step((data, tgt)).as_floats())
            feds[i].append(m.fed_ids())
    for m in models:
        m.check_device_errors()
    assert mets[0] == mets[1]
    for a, b in zip(*feds):
        assert np.array_equal(a, b)
    assert np.array_equal(feds[0][0], data[1])                                  # p = 0 at the eager step
    assert not np.array_equal(feds[0][3][:, 1:], data[1][:, 1:])                # p = 1: every position fed
    assert not np.array_equal(feds[0][3], feds[0][2])                           # a new stream step, new draws
    a, b = models
    for k in a.trainable_names():
        assert np.array_equal(a.get_weight(k), b.get_weight(k)), k
    assert schedule_p(0, spec.params(), 3) == np.float32(1.0)
