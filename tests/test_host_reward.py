"""Device-scored self-critical training on the CPU: the float64 restatement of tnt_caption_reward_f32
(tests/reward_oracle.py) against evaluate.CiderD / evaluate.sentence_bleu and against hand-computed cases,
evaluate.RewardTable, SelfCritical(score_on=...)'s refusals, and the host logic of the device-scored step through a mock
backend whose caption_reward is the restatement: where the launch sits, and that nothing is scored in Python."""
import math

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.evaluate import CiderD, RewardTable, sentence_bleu
from masters_thesis_amd.model_base import SelfCritical as SC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch
from mock_backend import flat
from scst_oracle import SCSTMockBackend, SCSTNICDense
import reward_oracle as RO

B, N, T, V, U, E = 5, 23, 6, 13, 16, 12
END = 2
QUERIES = ("bn_nchunk", "gemm_fused_cfg", "gemm3_plan", "gemm3_work_floats", "gemm3_sync_words", "gemm3_pair_supported",
           "lstm_seq_supported", "gemm3_desc", "finalize_desc", "lstm_seq_bwd_work_floats", "lc_seq_fwd_work_floats",
           "lc_seq_bwd_work_floats", "attention_front_bwd_parts", "attention_metric_parts", "embedding_bwd_parts")


class RewardMockBackend(SCSTMockBackend):
    """SCSTMockBackend plus ``caption_reward`` from tests/reward_oracle.py (the header's refusals as assertions); ``log``
    names every launch in order"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []
        for name in dir(self):
            fn = getattr(self, name)
            if not name.startswith("_") and callable(fn) and name not in QUERIES:
                setattr(self, name, self._logged(name, fn))

    def _logged(self, name, fn):
        def call(*a, **k):
            self.log.append(name)
            return fn(*a, **k)
        return call

    def caption_reward(self, fed, T, last, greedy, ldg, refs, n_refs, M_, Lr, keys, idf, n_keys, params, B_, K, end_id, kind,
                       baseline, adv, score=None, counted=None):
        assert B_ > 0 and 1 <= T <= 64 and 1 <= Lr <= 64 and 1 <= K <= 16 and 1 <= M_ <= 8 and kind in (0, 1)
        assert baseline in (0, 1) and (baseline == 0 or K >= 2) and (baseline == 1 or (greedy is not None and ldg >= B_))
        assert kind == 1 or params is not None
        R = B_ * K
        kk = flat(keys)[:n_keys].view(np.uint64) if n_keys else np.zeros(0, np.uint64)
        a, s, c = RO.reward(flat(fed)[:R * T].reshape(R, T), flat(last)[:R],
                            None if baseline else flat(greedy)[:T * ldg].reshape(T, ldg), flat(refs)[:B_ * M_ * Lr].reshape(B_, M_, Lr),
                            flat(n_refs)[:B_], kk, flat(idf)[:n_keys] if n_keys else None,
                            flat(params)[:2] if params is not None else None, end_id, kind, baseline, K)
        flat(adv)[:R] = a.astype(np.float32)
        if score is not None:
            flat(score)[:B_ * (K + 1)] = s.reshape(-1)
        flat(counted)[:R] = c


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RewardMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def random_corpus(rng, ndoc, vocab, nref=(1, 4), length=(0, 9)):
    return [[[int(w) for w in rng.integers(3, vocab, rng.integers(*length))] for _ in range(rng.integers(*nref))]
            for _ in range(ndoc)]


# ---------------------------------------------------------------------------------------------------- oracle against the scorers
def test_oracle_agrees_with_the_host_scorers():
    rng = np.random.default_rng(0)
    corpus = random_corpus(rng, 40, 12)
    cd = CiderD(corpus)
    keys, idf, params = RO.table_of(corpus)
    worst_c = worst_b = 0.0
    nonzero = 0
    for _ in range(300):
        cand = [int(w) for w in rng.integers(3, 12, rng.integers(0, 10))]
        refs = [[int(w) for w in rng.integers(3, 12, rng.integers(0, 10))] for _ in range(rng.integers(0, 4))]
        want = cd._score(cd._vec(cand, cd._df, cd._log_docs), [cd._vec(r, cd._df, cd._log_docs) for r in refs])
        got = RO.cider_d(cand, refs, keys, idf, params)
        worst_c = max(worst_c, abs(got - want))
        wb = sentence_bleu(refs, cand, weights=(0.25,) * 4) if refs else 0.0
        worst_b = max(worst_b, abs(RO.bleu4(cand, refs) - wb))
        nonzero += (want > 0) + (wb > 0)
    assert worst_c <= 1e-12 and worst_b <= 1e-12 and nonzero > 200, (worst_c, worst_b, nonzero)


def test_oracle_step_agrees_with_selfcritical_advantages():
    rng = np.random.default_rng(1)
    corpus = random_corpus(rng, 30, 12, length=(1, 7))
    keys, idf, params = RO.table_of(corpus)
    for K, baseline, reward in ((1, "greedy", "cider-d"), (3, "mean", "cider-d"), (2, "greedy", "bleu4"), (4, "mean", "bleu4")):
        sc = SC(END, n_samples=K, baseline=baseline, reward=reward, corpus=corpus)
        Bn, Tn = 6, 7
        w = rng.integers(0, 12, (Bn * K, Tn))
        g = rng.integers(0, 12, (Bn, Tn))
        docs = [corpus[b] for b in range(Bn)]
        adv, rew, base, cnt = sc.advantages(w, docs, g if baseline == "greedy" else None)
        Mx, Lx = max(len(d) for d in docs), max(1, max(len(r) for d in docs for r in d))
        refs, n_refs = np.zeros((Bn, Mx, Lx), np.int32), np.zeros(Bn, np.int32)
        evaluate.pack_references(docs, refs, n_refs)
        fed = np.concatenate([np.ones((Bn * K, 1), np.int64), w[:, :-1]], 1)
        a, s, c = RO.reward(fed, w[:, -1], g.T, refs, n_refs, keys, idf, params, END, evaluate.REWARD_KINDS[reward],
                            0 if baseline == "greedy" else 1, K)
        assert np.abs(a - adv).max() <= 1e-12 and np.abs(s[:, :K].reshape(-1) - rew).max() <= 1e-12
        assert np.array_equal(c, cnt.astype(np.int64))
        if baseline == "greedy":
            assert np.abs(np.repeat(s[:, K], K) - base).max() <= 1e-12
        else:
            assert not s[:, K].any()


def test_hand_computed_cases():
    # corpus: A = {[3 4 5]}, B = {[3 6]}, ndoc 2: unigram 3 has df 2 (idf 0); every other gram df 1 (idf ln 2)
    corpus = [[[3, 4, 5]], [[3, 6]]]
    keys, idf, params = RO.table_of(corpus)
    ln2 = math.log(2.0)
    assert RO.idf_of((3,), keys, idf, ln2) == 0.0 and RO.idf_of((4,), keys, idf, ln2) == ln2
    # an empty candidate; no references
    assert RO.cider_d([], [[3, 4, 5]], keys, idf, params) == 0.0 and RO.bleu4([], [[3, 4, 5]]) == 0.0
    assert RO.cider_d([3, 4], [], keys, idf, params) == 0.0 and RO.bleu4([3, 4], []) == 0.0
    # a candidate shorter than the order: [3 4] against [3 4 5].  k = 1: c = {3: 0, 4: ln2}, r = {3: 0, 4: ln2, 5: ln2} ->
    # ln2^2 / sqrt(ln2^2 * 2 ln2^2) = 1/sqrt2; k = 2: {34} against {34, 45} -> 1/sqrt2; k = 3, 4: nothing.
    want = 10.0 * (2.0 / math.sqrt(2.0)) / 4.0 * math.exp(-1.0 / 72.0)
    assert abs(RO.cider_d([3, 4], [[3, 4, 5]], keys, idf, params) - want) < 1e-12
    # a gram with df == ndoc has idf 0: the unigram 3 alone gives nothing
    assert RO.cider_d([3], [[3]], keys, idf, params) == 0.0
    # a reference whose grams all have idf 0: the norm is 0 and the score is 0, not NaN
    assert RO.cider_d([3, 4], [[3]], keys, idf, params) == 0.0
    # a gram absent from the table has df 0, idf = log(ndoc): [7 8] against itself is a full match at k = 1, 2
    assert RO.idf_of((7,), keys, idf, ln2) == ln2 and RO.idf_of((7, 8), keys, idf, ln2) == ln2
    assert abs(RO.cider_d([7, 8], [[7, 8]], keys, idf, params) - 5.0) < 1e-12
    # an id outside [1, 65535] is in no table, and still matches itself
    assert RO.gram_key((70000,)) is None and RO.gram_key((3, 70000)) is None and RO.gram_key((1, 2)) == 1 | 2 << 16
    assert abs(RO.cider_d([70000, 8], [[70000, 8]], keys, idf, params) - 5.0) < 1e-12
    # clipping: the candidate's three 3s against at most two in one reference; 3 3 once in either
    assert abs(RO.bleu4([3, 3, 3, 4], [[3, 3, 5, 5], [3, 4, 4, 4]])
               - math.exp(0.25 * (math.log(3 / 4) + math.log(2 / 3) + math.log(0.1 / 2) + math.log(0.1 / 1)))) < 1e-15
    # two references equally far from the candidate length 3: the shorter (2) wins, so no brevity penalty
    p = math.exp(0.25 * (math.log(3 / 3) + math.log(2 / 2) + math.log(1 / 1) + math.log(0.1 / 1)))
    assert abs(RO.bleu4([3, 4, 5], [[3, 4, 5, 6], [9, 9]]) - p) < 1e-15
    assert abs(RO.bleu4([3, 4, 5], [[3, 4, 5, 6]]) - p * math.exp(1.0 - 4.0 / 3.0)) < 1e-15
    # no unigram match
    assert RO.bleu4([7, 8], [[3, 4]]) == 0.0
    # captions and counted positions
    assert RO.caption([5, 6, END, 7], END) == [5, 6] and RO.counted([5, 6, END, 7], END) == 3
    assert RO.caption([5, 0, 6], END) == [5] and RO.counted([5, 6, 7], END) == 3 and RO.counted([END, 5], END) == 1
    assert RO.caption([5, END, 6, 0, 7], -1) == [5, END, 6]


# ---------------------------------------------------------------------------------------------------- the table
def test_reward_table():
    rng = np.random.default_rng(2)
    corpus = random_corpus(rng, 25, 12, length=(1, 8))
    tab = RewardTable(corpus)
    assert tab.keys.dtype == np.uint64 and tab.idf.dtype == np.float64 and len(tab) == tab.idf.size > 100
    assert np.all(tab.keys[1:] > tab.keys[:-1])
    cd = CiderD(corpus)
    assert tab.params.tolist() == [cd._log_docs, 6.0]
    for gram, df in cd._df.items():
        i = int(np.searchsorted(tab.keys, np.uint64(evaluate.gram_key(gram))))
        assert int(tab.keys[i]) == evaluate.gram_key(gram)
        assert tab.idf[i] == cd._log_docs - math.log(max(1.0, float(df)))          # bit-equal to CiderD._vec's factor
    keys, idf, params = RO.table_of(corpus)
    assert np.array_equal(keys, tab.keys) and np.array_equal(idf, tab.idf) and np.array_equal(params, tab.params)
    # a 1-gram and the 2-gram starting with it differ; so do (a, b) and (b, a)
    assert evaluate.gram_key((5,)) == 5 and evaluate.gram_key((5, 7)) == 5 | 7 << 16 != evaluate.gram_key((7, 5))
    assert evaluate.gram_key((1, 2, 3, 65535)) == 1 | 2 << 16 | 3 << 32 | 65535 << 48 < 2 ** 64
    t2 = RewardTable([[[5, 7]], [[5]]])
    assert t2.keys.tolist() == [5, 7, 5 | 7 << 16] and t2.idf.tolist() == [0.0, math.log(2.0), math.log(2.0)]
    assert len(RewardTable([])) == 0 and len(RewardTable([[[]]])) == 0
    # uploaded once
    a = tab.device("cpu")
    assert a[0].dtype == torch.int64 and np.array_equal(a[0].numpy().view(np.uint64), tab.keys)
    assert tab.device("cpu") is a


def test_reward_table_refuses_a_vocabulary_above_65536():
    RewardTable([[[65535, 1]]], vocab_size=65536)
    for bad in (lambda: RewardTable([[[65536, 1]]]), lambda: RewardTable([[[3, 4]]], vocab_size=65537),
                lambda: RewardTable([[[3, 0, 4]]]), lambda: RewardTable([[[3, -1]]]), lambda: RewardTable([[[3]]], n=3),
                lambda: RewardTable(None)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------- SelfCritical
def test_score_on_refusals_and_default():
    corpus = [[[3, 4, 5]], [[3, 6]]]
    assert SC(END).score_on == "host" and SC(END).table is None and "score_on" not in repr(SC(END))
    sc = SC(END, reward="cider-d", corpus=corpus, score_on="device")
    assert sc.score_on == "device" and len(sc.table) == 8 and "score_on='device'" in repr(sc)
    assert SC(END, reward="bleu4", score_on="device").table is None
    with pytest.raises(ValueError, match="callable"):
        SC(END, reward=lambda c, r: 1.0, score_on="device")
    with pytest.raises(ValueError, match="every step"):
        SC(END, reward="cider-d", score_on="device")
    for bad in ("gpu", None, 1):
        with pytest.raises(ValueError, match="score_on"):
            SC(END, reward="bleu4", score_on=bad)
    with pytest.raises(ValueError, match="65536"):             # a key holds 16 bits per token id
        NIC(N, U, E, 65537, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=SC(END, reward="bleu4", score_on="device"))


# ---------------------------------------------------------------------------------------------------- the step's host logic
def make(rng, sc, seed=11):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=seed, self_critical=sc)
    orc = SCSTNICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        orc.p[k] = v.astype(np.float32).astype(np.float64)
        model.set_weight(k, orc.p[k])
    model.compile(Adam(1e-3, clipnorm=None))
    return model, orc


def no_host_scoring(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device-scored step scored a caption on the host")
    monkeypatch.setattr(SC, "advantages", boom)
    monkeypatch.setattr(SC, "scores", boom)


@pytest.mark.parametrize("K,baseline,reward,with_refs", [(1, "greedy", "cider-d", False), (3, "mean", "cider-d", True),
                                                         (2, "greedy", "bleu4", True), (2, "mean", "bleu4", False)])
def test_device_step_one_reward_launch_and_the_host_steps_numbers(mock_backend, monkeypatch, K, baseline, reward, with_refs):
    rng = np.random.default_rng(7)
    corpus = random_corpus(rng, 20, V, length=(1, 6))
    refs = [corpus[b] for b in range(B)] if with_refs else None
    kw = dict(n_samples=K, baseline=baseline, reward=reward, corpus=corpus)
    model, orc = make(rng, SC(END, score_on="device", **kw))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    want = orc.scst_step(SC(END, **kw), data, M.DropCtx(seed=11, step=0, training=True), references=refs)
    no_host_scoring(monkeypatch)
    del mock_backend.log[:]
    got = model.train_step_scst((data, tgt), references=refs).as_floats()
    log = mock_backend.log
    assert log.count("caption_reward") == 1 and log.count("scst_cce") == 1 and log.count("sample_rows") == 1
    assert log.index("sample_rows") + 1 == log.index("caption_reward") == log.index("scst_cce") - 1
    assert np.array_equal(model.cap.numpy(), want["fed"]) and np.array_equal(model._scst["last"].numpy(), want["last"])
    assert np.any(want["adv"] != 0)
    assert np.array_equal(model._scst["adv"].numpy(), want["adv"].astype(np.float32))
    assert abs(got["reward"] - want["reward"].mean()) < 1e-12 and abs(got["baseline"] - want["base"].mean()) < 1e-12
    assert got["sample_len"] == want["counted"].mean()
    assert abs(got["loss"] - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    # the second step stages other references into the same buffers
    refs2 = None if with_refs else [corpus[b + 5] for b in range(B)]
    model.train_step_scst((data, tgt), references=refs2)
    st = model._scst
    n = st["n_refs"].numpy()
    assert n.tolist() == ([1] * B if refs2 is None else [len(d) for d in refs2])
    if refs2 is None:
        own = st["refs"].numpy()
        assert np.array_equal(own[:, 0, :T - 1], np.asarray(data[1])[:, 1:]) and not own[:, 1:].any() and not own[:, 0, T - 1:].any()


def test_host_step_launches_no_reward_kernel(mock_backend):
    rng = np.random.default_rng(8)
    model, _ = make(rng, SC(END, n_samples=2, reward="bleu4"))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    model.train_step((data, tgt))
    assert "caption_reward" not in mock_backend.log and mock_backend.log.count("scst_cce") == 1
    assert "refs" not in model._scst


def test_too_many_or_too_long_references_raise_before_any_launch(mock_backend):
    rng = np.random.default_rng(9)
    model, _ = make(rng, SC(END, n_samples=2, reward="bleu4", score_on="device"))
    data, tgt = synth_batch(B, N, T, V, U, rng)
    ok = [[[3, 4, 5]]] * (B - 1)
    del mock_backend.log[:]
    with pytest.raises(ValueError, match="at most 8 references"):
        model.train_step_scst((data, tgt), references=ok + [[[3, 4]] * 9])
    with pytest.raises(ValueError, match="at most 64 tokens"):
        model.train_step_scst((data, tgt), references=ok + [[[3] * 65]])
    assert mock_backend.log == []
    model.train_step_scst((data, tgt), references=ok + [[[3, 4]] * 8 + []])
    model.train_step_scst((data, tgt), references=ok + [[[3] * 64]])
    assert mock_backend.log.count("caption_reward") == 2
