"""Scan dropout and word dropout through the models on the GPU: the tiny nic.NIC and lc_nic.NIC of
test_gpu_weight_decay_models with ScanDropout(0.5, null=<fixed vector>) and WordDropout(0.5, unk_id=1).

Oracle parity: three train_steps against the unchanged float64 oracle step fed the restated corrupted batch
(tests/corrupt_oracle.py), with the loss and weight tolerances test_gpu_global_clip_models takes from test_gpu_nic.py /
test_gpu_lcnic.py; every step asserts from the restatement that a row and a token fired and that a row and a token did
not.  Replay: the same steps as a recorded launch plan and as a hipGraph give the bits of the eager run, and the staged
ids of consecutive steps on one batch differ.  Untouched: a model without the options is bit-identical to a twin that had
them set and taken back before its first step; test_step and greedy_predict of a model with the options are those of a
model without.  The flagship route (512 units, where the staging rides in the encoder forward): scan dropout takes the
separate staging launch, word dropout keeps the ride, and both train bit for bit like a plain model fed the restated
batch."""
import numpy as np
import pytest
import torch

import test_gpu_stage_forward as SF
from corrupt_oracle import corrupt, corrupt_batch
from oracle import models as M
from test_gpu_weight_decay_models import ADAM, N, RUNNERS, T, U, batches, build, check_weights, same, state_of

pytestmark = pytest.mark.gpu

SEED = 11                                                   # of the tiny models (test_gpu_nic.build / test_gpu_lcnic.build)
NULL = np.random.default_rng(79).standard_normal(N).astype(np.float32)
# The fixed inputs and the weight tolerance.  check_weights (test_gpu_nic's rule) widens the tolerance where the oracle's
# gradient is below 1e-8: there float32 leaves noise in the place of a zero, and Adam (epsilon 1e-8) turns noise into a
# full step.  dense_img/bias is the variable this happens to: its gradient is a sum over the batch that cancels exactly
# wherever a unit's five pre-activations share a sign, and nearly where they almost do.  Between the two regimes lies a gap
# the rule does not cover: a first update moves by lr * s g / (s |g| + 1e-8) (s <= 1 the clip factor), so a gradient error
# d moves the weight by lr * 1e-8 * s d / (s |g| + 1e-8)^2.  With d up to the rule's own noise threshold, 1e-8, and s >= 0.5
# this stays below half the tolerance (1e-5) only for |g| >= 1.2e-7.  The null vector is therefore one for which the
# ORACLE's gradients of that variable have no element in [1e-8, 2e-7) at any of the three steps -- decided on the float64
# oracle alone, and asserted below; rng seed 77 has one at 5.3e-8.
GRAD_GAP = (1e-8, 2e-7)
SR, WR, UNK = 0.5, 0.5, 1
CORRUPT = "tnt_input_corrupt_f32"


def adam():
    from masters_thesis_amd.optimizers import Adam
    return Adam(1e-3, **ADAM)


def options(model):
    from masters_thesis_amd.model_base import ScanDropout, WordDropout
    model.scan_dropout, model.word_dropout = ScanDropout(SR, NULL), WordDropout(WR, UNK)
    return model


def arrays(out):
    """a decode's return value (an array, or a tuple of arrays / tensors) as a list of host arrays"""
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in out]


def mixed(data, rows, words):
    elig = data[1] != 0
    elig[:, 0] = False
    return rows.any() and not rows.all() and words.any() and (elig & ~words).any()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_three_steps_match_the_oracle_on_the_restated_batch(kind):
    model, orc = build(kind)
    options(model).compile(adam())
    assert model._input_width() == N
    state = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    noisy = {}
    for step, (data, tgt) in enumerate(batches(3)):
        fed, rows, words = corrupt_batch(data, SR, WR, NULL, UNK, SEED, step)
        assert mixed(data, rows, words), (step, rows, words)
        res, grads, _ = orc.train_step(fed, tgt, state, M.DropCtx(seed=SEED, step=step, training=True))
        if kind == "dense":
            g = np.abs(grads["dense_img/bias"])
            assert not ((g >= GRAD_GAP[0]) & (g < GRAD_GAP[1])).any(), (step, g[(g >= GRAD_GAP[0]) & (g < GRAD_GAP[1])])
        got = model.train_step((data, tgt)).as_floats()
        for k in ("loss", "L2") + (("attention",) if kind == "attention" else ()):
            print(f"step {step} {k}: kernel {got[k]:.8g} oracle {res[k]:.8g}")
            assert abs(got[k] - res[k]) <= 1e-4 * abs(res[k]) + 1e-7, (step, k, got[k], res[k])
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        check_weights(kind, model, orc, step, noisy, grads)
        torch.cuda.synchronize()
        assert np.array_equal(model.x.cpu().numpy()[:, :N], fed[0]) and np.array_equal(model.cap.cpu().numpy(), fed[1])
    model.check_device_errors()


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_plan_and_graph_replays_are_the_eager_bits(kind):
    models = {r: options(build(kind, **kw)[0]) for r, kw in RUNNERS.items()}
    for m in models.values():
        m.compile(adam())
    d = batches(1)[0]
    caps = []
    for step in range(4):                                               # eager, record / capture, replay, replay: one batch
        mets = {r: m.train_step(d).as_floats() for r, m in models.items()}
        states = {r: state_of(m) + [m.cap.clone(), m.x.clone()] for r, m in models.items()}
        for r in ("plan", "graph"):
            assert mets[r] == mets["eager"], (step, r, mets[r], mets["eager"])
            assert same(states[r], states["eager"]), (step, r)
        caps.append(models["plan"].cap.cpu().numpy().copy())
        want = corrupt(d[0][0], d[0][1], SR, WR, NULL, UNK, SEED, step)
        assert np.array_equal(caps[-1], want[1]) and np.array_equal(models["graph"].x.cpu().numpy()[:, :N], want[0])
    for a, b in zip(caps, caps[1:]):
        assert not np.array_equal(a, b)                                 # the coins change per step on the same batch
    assert models["plan"]._graphs and models["graph"]._graphs, "the step was never recorded / captured"


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_a_model_without_the_options_is_untouched(kind, runner):
    a, b = build(kind, **RUNNERS[runner])[0], options(build(kind, **RUNNERS[runner])[0])
    b.scan_dropout = b.word_dropout = None                              # taken back before the first step
    a.compile(adam())
    b.compile(adam())
    for step, d in enumerate(batches(3)):
        assert a.train_step(d).as_floats() == b.train_step(d).as_floats(), step
        assert same(state_of(a), state_of(b)), step
    # ... and a twin that kept them is not: the comparison above can tell
    c = options(build(kind, **RUNNERS[runner])[0])
    c.compile(adam())
    for d in batches(3):
        c.train_step(d)
    assert not torch.equal(c.arena.theta, a.arena.theta)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_evaluation_and_decoding_are_those_of_a_model_without(kind):
    a, b = build(kind)[0], options(build(kind)[0])
    a.compile(adam())
    b.compile(adam())
    (data, tgt), = batches(1)
    z, start = np.zeros((data[0].shape[0], U), np.float32), np.ones(data[0].shape[0], np.int64)
    for _ in range(2):
        assert a.test_step((data, tgt)).as_floats() == b.test_step((data, tgt)).as_floats()
        wa, wb = (arrays(m.greedy_predict(data[0], z, z, start, T)) for m in (a, b))
        assert len(wa) == len(wb) >= 1 and all(np.array_equal(p, q) for p, q in zip(wa, wb))


# ------------------------------------------------------------------------------ the flagship route (512 units)
def flagship(stage_fwd=True, scan=None, word=None):
    from masters_thesis_amd.model_base import ScanDropout, WordDropout
    m = SF.make_model(stage_fwd)
    m.scan_dropout = None if scan is None else ScanDropout(scan, FNULL)
    m.word_dropout = None if word is None else WordDropout(word, UNK)
    return m


FNULL = np.random.default_rng(78).standard_normal(SF.NV).astype(np.float32)


def steps_of(m, feed, n=3):
    """n training steps, the first (eager) one with the backend recording -> (names launched in step 1, metrics, state)"""
    names, hist = None, []
    for step in range(n):
        if step == 0:
            rec = m.be._rec = []
        try:
            hist.append(m.train_step(feed(step)).as_floats())
        finally:
            m.be._rec = None
        if step == 0:
            names = [name for _, name, _ in rec]
    m.check_device_errors()
    torch.cuda.synchronize()
    return names, hist, [m.arena.theta.clone(), m.opt_m.clone(), m.opt_v.clone(), m.mov_mean.clone(), m.mov_var.clone()]


@pytest.mark.parametrize("scan,word", [(0.5, None), (None, 0.5), (0.5, 0.5)], ids=["scan", "word", "both"])
def test_the_ride_is_declined_only_under_scan_dropout_and_the_step_is_the_plain_one_on_the_restated_batch(scan, word):
    h = SF.host_batch()
    (x, cap, a0, c0), tgt = h
    batch = SF.dev_batch(h)
    model = flagship(True, scan, word)
    names, hist, state = steps_of(model, lambda step: batch)
    if not model._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    i = names.index(CORRUPT)
    assert names.count(CORRUPT) == 1
    if scan is not None:                # the separate staging launch, the corruption, then the encoder forward on the staged rows
        assert SF.MERGED not in names and names[:3] == [SF.STAGE, CORRUPT, SF.GRAM], names[:4]
    else:                               # word dropout alone keeps the ride
        assert names[:2] == [SF.MERGED, CORRUPT] and SF.STAGE not in names and SF.GRAM not in names, names[:4]
    feeds = []
    for step in range(3):
        x2, cap2, rows, words = corrupt(x, cap, scan or 0.0, word or 0.0, FNULL, UNK, 42, step)
        assert scan is None or (rows.any() and not rows.all()), step
        assert word is None or words.any(), step
        feeds.append(SF.dev_batch(((x2, cap2, a0, c0), tgt)))
    plain = flagship(scan is None)
    pn, phist, pstate = steps_of(plain, lambda step: feeds[step])
    assert CORRUPT not in pn and [n for n in names if n != CORRUPT] == pn
    assert hist == phist, (hist, phist)
    assert same(state, pstate)
    clean = steps_of(flagship(True), lambda step: batch)
    assert not torch.equal(clean[2][0], state[0])                        # (a clean run differs: the comparison can tell)
