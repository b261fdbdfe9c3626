"""Self-critical sequence training for the dense model (nic.NIC(self_critical=...)) on the CPU: the CIDEr-D reward
against hand-computed cases, SelfCritical's validation, truncation and advantages, and the model's SCST step through a
mock backend that follows tnt_scst_cce_f32's header definition, against the float64 restatement of tests/scst_oracle.py
(loss and every gradient against torch autograd, the post-Adam weights)."""
import math

import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import dp
from masters_thesis_amd.evaluate import CiderD, sentence_bleu
from masters_thesis_amd.model_base import SelfCritical as SC, ScheduledSampling as SS, S_SCST_LAST, S_SS_DRAW
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch
from scst_oracle import SCSTMockBackend, SCSTNICDense, counted_mask, scst_cce

B, N, T, V, U, E = 5, 23, 6, 13, 16, 12
END = 2


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = SCSTMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- CIDEr-D
def test_cider_candidate_equal_to_its_reference_scores_ten():
    docs = [[[1, 2, 3, 4, 5]], [[1, 6, 7, 8, 9]]]           # unigram 1 is in both documents (idf 0), the rest are not
    assert CiderD().batch_scores([[[1, 2, 3, 4, 5]], [[1, 6, 7, 8, 9]]], docs) == [10.0, 10.0]
    assert CiderD(corpus=docs)([1, 2, 3, 4, 5], docs[0]) == 10.0


def test_cider_disjoint_candidate_scores_zero():
    docs = [[[1, 2, 3, 4, 5]], [[6, 7, 8, 9]]]
    assert CiderD().batch_scores([[[10, 11, 12]], [[5, 4, 3, 2]]], docs)[0][0] == 0.0
    assert CiderD(corpus=docs)([10, 11, 12, 10], docs[1]) == 0.0


def test_cider_hand_worked_two_documents():
    # documents A = {[1 2 3]}, B = {[1 4]}: log(#docs) = ln 2; unigram 1 has df 2 (idf 0), every other n-gram df 1 (idf ln 2).
    # A's candidate [1 2]: n = 1: c = {1: 0, 2: ln2}, r = {1: 0, 2: ln2, 3: ln2} -> (ln2)^2 / (ln2 * sqrt(2) ln2) = 1/sqrt2;
    # n = 2: c = {12: ln2}, r = {12: ln2, 23: ln2} -> 1/sqrt2; n = 3, 4: the candidate has none -> 0.  Length penalty
    # exp(-(2 - 3)^2 / 72).  Score 10 * (2 / sqrt2) / 4 * exp(-1/72).  B's candidate [1 4] equals its reference: n = 1, 2
    # give 1, n = 3, 4 give 0 (no such n-grams): 10 * 2 / 4 = 5.
    got = CiderD().batch_scores([[[1, 2]], [[1, 4]]], [[[1, 2, 3]], [[1, 4]]])
    assert abs(got[0][0] - 10.0 * (2.0 / math.sqrt(2.0)) / 4.0 * math.exp(-1.0 / 72.0)) < 1e-12
    assert abs(got[1][0] - 5.0) < 1e-12
    # the same frequencies from a fixed corpus, with its reference vectors cached across calls
    cd = CiderD(corpus=[[[1, 2, 3]], [[1, 4]]])
    for _ in range(2):
        assert abs(cd([1, 2], [[1, 2, 3]]) - got[0][0]) < 1e-12
    assert len(cd._cache) == 1


def test_cider_reference_order_does_not_matter():
    docs = [[[1, 2, 3, 4], [3, 2, 5, 6, 7]], [[8, 9, 2]]]
    swapped = [docs[0][::-1], docs[1]]
    cands = [[[1, 2, 5, 6], [3, 2, 1]], [[8, 9]]]
    a, b = CiderD().batch_scores(cands, docs), CiderD().batch_scores(cands, swapped)
    assert np.allclose(a[0], b[0], rtol=1e-15, atol=0) and a[0].min() > 0


def test_cider_length_penalty():
    # one reference: the penalty is a common factor of every n, so against sigma = inf the score moves by exactly
    # exp(-(l_c - l_r)^2 / (2 * 6^2))
    docs = [[[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], [[11, 12]]]
    for cand in ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 2, 3]):
        s6 = CiderD().batch_scores([[cand], [[11]]], docs)[0][0]
        s_inf = CiderD(sigma=float("inf")).batch_scores([[cand], [[11]]], docs)[0][0]
        assert s_inf > 0 and abs(s6 - s_inf * math.exp(-(len(cand) - 10) ** 2 / 72.0)) < 1e-12 * s_inf


# ---------------------------------------------------------------------------------------------------- SelfCritical
@pytest.mark.parametrize("make_bad", [
    lambda: SC(0), lambda: SC(-1), lambda: SC(2.0), lambda: SC(True), lambda: SC(2, n_samples=0),
    lambda: SC(2, n_samples=17), lambda: SC(2, n_samples=2.0), lambda: SC(2, baseline="max"),
    lambda: SC(2, baseline="mean"), lambda: SC(2, n_samples=1, baseline="mean"), lambda: SC(2, reward="cider"),
    lambda: SC(2, reward=3), lambda: SC(2, corpus=5), lambda: SC(2, corpus=[3, 4])])
def test_bad_arguments_raise(make_bad):
    with pytest.raises(ValueError):
        make_bad()


def test_truncation_at_end_id_and_zero():
    sc = SC(END)
    assert sc.truncate([5, 6, END, 7]) == [5, 6] and sc.counted([5, 6, END, 7]) == 3
    assert sc.truncate([5, 0, 6, END]) == [5] and sc.counted([5, 0, 6, END]) == 2
    assert sc.truncate([END, 5]) == [] and sc.counted([END, 5]) == 1
    assert sc.truncate([5, 6, 7]) == [5, 6, 7] and sc.counted(np.array([5, 6, 7])) == 3
    m, _ = counted_mask(np.array([[1, 5, END, 7], [1, 0, 4, 4], [1, 3, 4, 5]]), np.array([9, 9, END]), END)
    assert m.tolist() == [[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]]


def _overlap(c, refs):
    return float(len(set(c) & set(refs[0])))


def test_advantages_greedy_and_mean_baselines():
    refs = [[[3, 4, 5]], [[6, 7]]]
    samples = np.array([[3, 4, END, 0], [3, 9, 9, 9], [6, 0, 7, 7], [8, 8, 8, END]])
    greedy = np.array([[3, 4, 5, END], [9, END, 6, 7]])
    sc = SC(END, n_samples=2, reward=_overlap)
    adv, rew, base, cnt = sc.advantages(samples, refs, greedy)
    assert rew.tolist() == [2, 1, 1, 0] and base.tolist() == [3, 3, 0, 0] and adv.tolist() == [-1, -2, 1, 0]
    assert cnt.tolist() == [3, 4, 2, 4]
    sc = SC(END, n_samples=2, baseline="mean", reward=_overlap)
    adv, rew, base, _ = sc.advantages(samples, refs)
    assert base.tolist() == [1, 2, 0, 1] and adv.tolist() == [1, -1, 1, -1]
    sc = SC(END, n_samples=3, baseline="mean", reward=_overlap)
    adv, rew, base, _ = sc.advantages(np.array([[3, 4, 5], [3, 1, 1], [1, 1, 1]]), [[[3, 4, 5]]])
    assert rew.tolist() == [3, 1, 0] and np.allclose(base, [0.5, 1.5, 2.0]) and np.allclose(adv, [2.5, -0.5, -2.0])
    # the named rewards
    sc = SC(END, reward="bleu4")
    _, rew, _, _ = sc.advantages(np.array([[3, 4, 5, END]]), [[[3, 4, 5, 6]]], np.array([[3, 4, END, 0]]))
    assert rew[0] == sentence_bleu([[3, 4, 5, 6]], [3, 4, 5], weights=(0.25,) * 4)
    docs = [[[3, 4, 5, 6]], [[7, 8]]]
    sc = SC(END, reward="cider-d", corpus=docs)
    _, rew, base, _ = sc.advantages(np.array([[3, 4, 5, 6], [7, 9, 9, 9]]), docs, np.array([[7, 8, 0, 0], [7, 8, 0, 0]]))
    assert rew[0] == 10.0 and base[0] == 0.0 and base[1] == 5.0         # [7 8] has no 3- or 4-grams


def test_scst_cce_restatement():
    rng = np.random.default_rng(0)
    R, T_, V_ = 4, 3, 7
    x = rng.standard_normal((T_ * R, V_))
    fed = np.array([[1, 3, 4], [1, END, 3], [1, 0, 5], [1, 6, 6]])
    last = np.array([2, 3, 3, 6])
    adv = np.array([0.5, -1.0, 2.0, 0.0])
    loss, lp, d, m = scst_cce(x, fed, last, adv, END, 1.0 / R)
    assert m.tolist() == [[1, 1, 1], [1, 0, 0], [1, 0, 0], [1, 1, 1]]
    lse = np.log(np.exp(x).sum(1))
    assert abs(loss[2 * R + 0] - (-0.5 * (x[2 * R, 2] - lse[2 * R]))) < 1e-12     # t = 3, the last token 2 of row 0
    assert loss[R + 1] == 0 and not d[R + 1].any() and not d[3].any() and not d[2 * R + 3].any()
    assert lp[2 * R + 3] != 0 and loss[2 * R + 3] == 0
    assert abs(d[0].sum()) < 1e-12 and abs(d[0, 3] - 0.5 / R * (np.exp(x[0, 3] - lse[0]) - 1)) < 1e-12


# ---------------------------------------------------------------------------------------------------- model
LAM = {"dense_img/kernel": 0.01, "lstm/kernel": 3e-5, "time_distributed_softmax/kernel": 3e-5}


def make(rng, sc, rates=(0, 0, 0), seed=11, norm="batch"):
    model = NIC(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, norm=norm, device="cpu", seed=seed, self_critical=sc)
    orc = SCSTNICDense(N, U, E, V, T, *rates, 0.01, 3e-5, 1e-5, norm=norm).init_params(rng)
    for k, v in orc.p.items():
        orc.p[k] = v.astype(np.float32).astype(np.float64)
        model.set_weight(k, orc.p[k])
    model.compile(Adam(1e-3, clipnorm=None))
    return model, orc


def test_model_refusals(mock_backend):
    sc = SC(END)
    with pytest.raises(ValueError):
        NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical="scst")
    with pytest.raises(ValueError):
        NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=sc, scheduled_sampling=SS.linear(0.5, 0))
    for e in (10, 1020):
        with pytest.raises(ValueError):
            NIC(N, U, e, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=sc)
    with pytest.raises(ValueError):
        NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=SC(V))
    rng = np.random.default_rng(1)
    model, _ = make(rng, sc)
    with pytest.raises(NotImplementedError):
        dp.attach(model, world=1, rank=0)
    data, tgt = synth_batch(B, N, 34, V, U, rng)
    with pytest.raises(ValueError):
        model.train_step((data, tgt))                           # 33 sampled positions: more than the sites
    data, tgt = synth_batch(B, N, T, V, U, rng)
    with pytest.raises(ValueError):
        model.train_step_scst((data, tgt), references=[[[3, 4]]] * (B - 1))
    model.grad_sync = lambda m: None
    with pytest.raises(NotImplementedError):
        model.train_step((data, tgt))
    plain, _ = make(rng, None)
    with pytest.raises(ValueError):
        plain.train_step_scst((data, tgt))
    plain.train_step((data, tgt))
    assert mock_backend.scst_calls == 0 and mock_backend.ss_calls == 0
    assert S_SCST_LAST == S_SS_DRAW + 32


@pytest.mark.parametrize("K,baseline,rates,norm", [(1, "greedy", (0, 0, 0), "batch"), (3, "mean", (0, 0, 0), "batch"),
                                                   (2, "greedy", (0.1, 0.2, 0.25), "batch"),
                                                   (2, "mean", (0.1, 0.2, 0.25), "layer")])
def test_scst_step_matches_float64(mock_backend, K, baseline, rates, norm):
    rng = np.random.default_rng(4)
    sc = SC(END, n_samples=K, baseline=baseline, reward=lambda c, refs: float(len(c)) + 0.5 * len(set(c) & set(refs[0])))
    model, orc = make(rng, sc, rates=rates, norm=norm)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    drop = M.DropCtx(seed=11, step=0, training=True)
    want = orc.scst_step(sc, data, drop)
    got = model.train_step((data, tgt)).as_floats()
    assert mock_backend.scst_calls == 1
    assert want["margin"].min() > 1e-6
    assert np.array_equal(model.cap.numpy(), want["fed"]) and np.array_equal(model._scst["last"].numpy(), want["last"])
    if baseline == "greedy":
        assert np.array_equal(model._scst["greedy"].numpy().T, want["greedy"])
    assert np.any(want["adv"] != 0)
    assert abs(got["reward"] - want["reward"].mean()) < 1e-12 and abs(got["baseline"] - want["base"].mean()) < 1e-12
    assert got["sample_len"] == want["counted"].mean()
    assert abs(got["loss"] - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    assert abs(got["L2"] - orc.l2_loss()) < 1e-5 * orc.l2_loss()
    for k in M.NICDense.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM.get(k, 0.0) * orc.p[k]
        w = want["grads"][k]
        assert np.allclose(g, w, rtol=1e-4, atol=1e-4 * np.abs(w).max() + 1e-9), k
    # the update: Adam on those gradients; BatchNorm's moving statistics once, over the R rows of the rollout
    _, cache = orc.forward((want["data_r"][0], want["fed"], want["data_r"][2], want["data_r"][3]), training=True, drop=drop)
    M.AdamState(orc.p, lr=1e-3, b2=0.999, eps=1e-7, clipnorm=None).apply(orc.p, want["grads"])
    for k in M.NICDense.TRAINABLE:
        assert np.allclose(model.get_weight(k), orc.p[k], rtol=1e-5, atol=1e-6), k
    if norm == "batch":
        assert np.allclose(model.get_weight("batch_norm/moving_mean"), cache["new_mm"], rtol=1e-5, atol=1e-6)
        assert np.allclose(model.get_weight("batch_norm/moving_variance"), cache["new_mv"], rtol=1e-5, atol=1e-6)


def test_scst_step_with_references_and_cider(mock_backend):
    rng = np.random.default_rng(5)
    refs = [[[int(v) for v in rng.integers(3, V, 4)] for _ in range(3)] for _ in range(B)]
    sc = SC(END, n_samples=2, baseline="greedy", reward="cider-d")
    model, orc = make(rng, sc)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    want = orc.scst_step(sc, data, M.DropCtx(seed=11, step=0, training=True), references=refs)
    got = model.train_step_scst((data, tgt), references=refs).as_floats()
    assert abs(got["reward"] - want["reward"].mean()) < 1e-12 and abs(got["loss"] - want["loss"]) < 1e-5 * max(1, abs(want["loss"]))
    for k in M.NICDense.TRAINABLE:
        g = model.get_gradient(k) + 2 * LAM.get(k, 0.0) * orc.p[k]
        w = want["grads"][k]
        assert np.allclose(g, w, rtol=1e-4, atol=1e-4 * np.abs(w).max() + 1e-9), k


def test_second_step_draws_new_samples_and_test_step_is_unchanged(mock_backend):
    rng = np.random.default_rng(6)
    sc = SC(END, n_samples=2, baseline="mean")
    ms, orc = make(rng, sc, rates=(0.1, 0.2, 0.2))
    mt = NIC(N, U, E, V, T, 0.1, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    for k, v in orc.p.items():
        mt.set_weight(k, v)
    mt.compile(Adam(1e-3, clipnorm=None))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    assert ms.test_step((data, tgt)).as_floats() == mt.test_step((data, tgt)).as_floats()
    ms.train_step((data, tgt))
    first = ms.cap.numpy().copy()
    ms.train_step((data, tgt))
    assert not np.array_equal(first, ms.cap.numpy())             # the stream step advanced: new draws
    assert np.array_equal(first[:, 0], np.repeat(data[1][:, 0], 2))
    z = np.zeros((B, U), np.float32)
    st = np.ones(B, np.int64)
    for k, v in orc.p.items():
        mt.set_weight(k, ms.get_weight(k))
    assert np.array_equal(ms.greedy_predict(data[0], z, z, st, T), mt.greedy_predict(data[0], z, z, st, T))
