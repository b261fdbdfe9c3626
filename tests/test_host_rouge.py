"""ROUGE-L on the CPU: the float64 restatement of tnt_caption_rouge_f32 (tests/rouge_oracle.py) against hand-computed
cases and evaluate.rouge_l; that the inputs of tests/test_gpu_rouge.py (tests/rouge_cases.py) tell the definition from its
near misses; SelfCritical(reward="rouge-l") on the host; and, through a mock backend whose caption_rouge is the
restatement, where the launch sits in the device-scored step and what fit(validation_captions=...) logs."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.callbacks import EarlyStopping, ModelCheckpoint, ReduceLROnPlateau
from masters_thesis_amd.evaluate import CaptionValidation
from masters_thesis_amd.model_base import SelfCritical as SC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
from helpers import synth_batch
from dense_beam_oracle import BeamMockBackend
from scst_oracle import SCSTNICDense
from test_host_reward import RewardMockBackend, no_host_scoring
import rouge_cases as RC
import rouge_oracle as RG

B, N, T, V, U, E = 5, 23, 6, 13, 16, 12
END = 2
GPU_TOL = 1e-12                                           # tests/test_gpu_rouge.py's bound on the score


class RougeMockBackend(RG.RougeMockMixin, RewardMockBackend, BeamMockBackend):
    """RewardMockBackend (every launch named in ``log``) plus ``caption_rouge`` from tests/rouge_oracle.py and the dense
    beam step"""


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RougeMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- the definition
def test_hand_computed_cases():
    # [1 2 3 4] against [1 3 4 5 6]: the subsequence 1 3 4, P = 3/4, R = 3/5, (2.44 * 0.75 * 0.6) / (0.6 + 1.44 * 0.75)
    assert RG.lcs([1, 2, 3, 4], [1, 3, 4, 5, 6]) == 3 == evaluate.lcs_length([1, 2, 3, 4], [1, 3, 4, 5, 6])
    assert abs(RG.rouge_l([1, 2, 3, 4], [[1, 3, 4, 5, 6]]) - 1.098 / 1.68) < 1e-15
    assert abs(evaluate.rouge_l([[1, 3, 4, 5, 6]], [1, 2, 3, 4]) - 1.098 / 1.68) < 1e-15
    # separate maxima: the short reference gives the best recall, 2/2, at precision 2/4; the long one the best precision,
    # 4/4, at recall 4/8
    cand, short, long_ = [1, 2, 3, 4], [1, 2], [1, 2, 3, 4, 9, 9, 9, 9]
    assert (RG.lcs(cand, short), RG.lcs(cand, long_)) == (2, 4)
    want = RG.f_score(1.0, 1.0, 1.2)                      # P from the long reference, R from the short one
    assert want == 1.0 and RG.rouge_l(cand, [short, long_]) == want == evaluate.rouge_l([short, long_], cand)
    joint = max(RG.f_score(0.5, 1.0, 1.2), RG.f_score(1.0, 0.5, 1.2))
    assert RG.rouge_l(cand, [short, long_], joint=True) == joint < 0.75
    # an empty candidate, an empty reference (skipped: no division by its length), no references, no common word
    assert RG.rouge_l([], [[1, 2]]) == 0.0 == evaluate.rouge_l([[1, 2]], [])
    assert RG.rouge_l([1, 2], [[]]) == 0.0 == evaluate.rouge_l([[]], [1, 2])
    assert RG.rouge_l([1, 2], [[], [2]]) == RG.rouge_l([1, 2], [[2]]) == evaluate.rouge_l([[], [2]], [1, 2]) > 0
    assert RG.rouge_l([1, 2], []) == 0.0 == evaluate.rouge_l([], [1, 2])
    assert RG.rouge_l([1, 2], [[3, 4]]) == 0.0 == evaluate.rouge_l([[3, 4]], [1, 2])
    # a subsequence with gaps that no substring has; order matters
    assert RG.lcs([5, 1, 6, 2, 7, 3], [1, 2, 3]) == 3 and RG.substring([5, 1, 6, 2, 7, 3], [1, 2, 3]) == 1
    assert RG.lcs([1, 2, 3], [3, 2, 1]) == 1 and RG.lcs([4] * 64, [4] * 64) == 64
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e200):
        with pytest.raises(ValueError, match="beta"):
            evaluate.rouge_l([[1]], [1], beta=bad)


def test_evaluate_rouge_l_is_the_restatement():
    rng = np.random.default_rng(0)
    nonzero, worst = 0, 0.0
    for i in range(400):
        vocab = (2, 3, 9)[i % 3]
        cand = [int(w) for w in rng.integers(3, 3 + vocab, rng.integers(0, 12))]
        refs = [[int(w) for w in rng.integers(3, 3 + vocab, rng.integers(0, 12))] for _ in range(rng.integers(0, 4))]
        beta = (1.2, 1.0, 0.5, 8.0)[i % 4]
        want, got = RG.rouge_l(cand, refs, beta), evaluate.rouge_l(refs, cand, beta=beta)
        worst = max(worst, abs(want - got))
        nonzero += want > 0
        assert 0.0 <= got <= 1.0
        for r in refs:
            assert evaluate.lcs_length(cand, r) == RG.lcs(cand, r) == evaluate.lcs_length(r, cand)
    assert worst == 0.0 and nonzero > 200, (worst, nonzero)


def test_the_gpu_cases_tell_the_definition_from_its_near_misses():
    """for the longest common substring, the maximum of the per-reference F-scores and beta = 1: the restatement run with
    the variant differs from the true one by more than the GPU tolerance on at least one case"""
    gaps = dict(substring=0.0, joint=0.0, beta1=0.0)
    lcs_differs = False
    for name in RC.NAMES:
        true = RC.want(name, 0)
        for variant in ("substring", "joint"):
            other = RC.want(name, 0, variant=variant)
            gaps[variant] = max(gaps[variant], float(np.abs(other[1] - true[1]).max()))
            lcs_differs |= variant == "substring" and not np.array_equal(other[3], true[3])
        gaps["beta1"] = max(gaps["beta1"], float(np.abs(RC.want(name, 0, beta=1.0)[1] - true[1]).max()))
    assert all(g > 1e-3 > GPU_TOL for g in gaps.values()) and lcs_differs, gaps


def test_the_gpu_cases_hold_the_forced_lengths_and_values():
    c = RC.case("forced")
    adv, score, cnt, lcs = RC.want("forced", 0)
    cap = lambda row: RG.caption(row, END)
    assert len(cap(c["w"][0])) == 64 and lcs[0, 0, 0] == 64 and score[0, 0] == 1.0                # the all-ones mask
    assert cap(c["w"][1]) == cap(c["w"][0])[::-1] and 1 <= lcs[0, 1, 0] < 64 and lcs[0, 1, 1] == 64
    assert cap(c["greedy"][:, 0]) == [] and score[0, 2] == 0.0                                    # a terminator at position 0
    assert [len(cap(r)) for r in c["w"][2:4]] == [1, 0] and [len(cap(r)) for r in c["refs"][1]] == [0, 1]
    assert lcs[1].tolist() == [[0, 1], [0, 0], [0, 1]] and score[1, 0] == 1.0 and 0 < score[1, 2] < 0.1
    assert lcs[2, 0, 0] == 8 and lcs[2, 2, 0] == 1 and lcs[2, 2, 1] == 2                          # full int32 words compared
    assert {RC.I32_MIN, RC.I32_MAX, 70000} <= set(int(v) for v in c["w"][4])
    assert c["n_refs"].tolist() == [2, 2, 2, 0, 11] and not score[3].any() and not lcs[3].any() and score[4].any()
    assert c["greedy"].shape[1] > c["B"]                                                          # ldg > B
    # over all cases: every size the issue names
    shapes = [tuple(RC.case(n)[k] for k in ("B", "K", "T", "M", "Lr")) for n in RC.NAMES]
    for axis, values in ((0, {1, 3, 5}), (1, {1, 2, 16}), (2, {1, 2, 15, 63, 64}), (3, {1, 8}), (4, {1, 2, 15, 63, 64})):
        assert values <= {s[axis] for s in shapes}, (axis, values)
    assert {s[5] for s in RC.SHAPES} == {2, 3, 50}


# ---------------------------------------------------------------------------------------------------- SelfCritical
def test_selfcritical_rouge_l_host_advantages():
    rng = np.random.default_rng(1)
    assert "rouge-l" in SC.REWARDS and SC.REWARDS[:2] == ("cider-d", "bleu4")
    assert evaluate.REWARD_KINDS == {"cider-d": 0, "bleu4": 1}
    for K, baseline in ((1, "greedy"), (3, "mean"), (2, "greedy")):
        sc = SC(END, n_samples=K, baseline=baseline, reward="rouge-l")
        assert sc.table is None and sc.corpus is None and SC(END, reward="rouge-l", score_on="device").table is None
        Bn, Tn = 6, 7
        w = rng.integers(0, 8, (Bn * K, Tn))
        g = rng.integers(0, 8, (Bn, Tn))
        docs = [[[int(v) for v in rng.integers(3, 8, rng.integers(0, 7))] for _ in range(rng.integers(0, 4))] for _ in range(Bn)]
        adv, rew, base, cnt = sc.advantages(w, docs, g if baseline == "greedy" else None)
        Mx, Lx = max(1, max(len(d) for d in docs)), max(1, max((len(r) for d in docs for r in d), default=1))
        refs, n_refs = np.zeros((Bn, Mx, Lx), np.int32), np.zeros(Bn, np.int32)
        evaluate.pack_references(docs, refs, n_refs)
        fed = np.concatenate([np.ones((Bn * K, 1), np.int64), w[:, :-1]], 1)
        a, s, c, _ = RG.rouge(fed, w[:, -1], g.T, refs, n_refs, END, 1.2, 0 if baseline == "greedy" else 1, K)
        assert np.abs(a - adv).max() <= 1e-15 and np.abs(s[:, :K].reshape(-1) - rew).max() == 0.0 and rew.max() > 0
        assert np.array_equal(c, cnt.astype(np.int64))


def make(rng, sc, seed=11):
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=seed, self_critical=sc)
    orc = SCSTNICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        orc.p[k] = v.astype(np.float32).astype(np.float64)
        model.set_weight(k, orc.p[k])
    model.compile(Adam(1e-3, clipnorm=None))
    return model, orc


@pytest.mark.parametrize("K,baseline,with_refs", [(1, "greedy", False), (3, "mean", True), (2, "greedy", True)])
def test_device_step_has_caption_rouge_where_caption_reward_was(mock_backend, monkeypatch, K, baseline, with_refs):
    rng = np.random.default_rng(7)
    pool = [[[int(w) for w in rng.integers(3, V, rng.integers(1, 6))] for _ in range(rng.integers(1, 4))] for _ in range(B)]
    refs = pool if with_refs else None
    data, tgt = synth_batch(B, N, T, V, U, rng)
    logs = {}
    for reward in ("bleu4", "rouge-l"):
        model, orc = make(np.random.default_rng(3), SC(END, n_samples=K, baseline=baseline, reward=reward, score_on="device"))
        want = orc.scst_step(SC(END, n_samples=K, baseline=baseline, reward=reward), data, M.DropCtx(seed=11, step=0, training=True),
                             references=refs)
        with monkeypatch.context() as mp:
            no_host_scoring(mp)
            del mock_backend.log[:]
            got = model.train_step_scst((data, tgt), references=refs).as_floats()
        logs[reward] = list(mock_backend.log)
        assert np.any(want["adv"] != 0)
        assert np.array_equal(model._scst["adv"].numpy(), want["adv"].astype(np.float32))
        assert abs(got["reward"] - want["reward"].mean()) < 1e-12 and abs(got["baseline"] - want["base"].mean()) < 1e-12
        assert got["sample_len"] == want["counted"].mean()
    log = logs["rouge-l"]
    assert log.count("caption_rouge") == 1 and "caption_reward" not in log
    assert log.index("sample_rows") + 1 == log.index("caption_rouge") == log.index("scst_cce") - 1
    assert [("caption_reward" if n == "caption_rouge" else n) for n in log] == logs["bleu4"]        # nothing else moves


def test_rouge_l_on_the_device_takes_a_vocabulary_above_65536():
    # tokens are only compared: no 16-bit key; the other device rewards keep their refusal
    NIC(N, U, E, 65537, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=SC(END, reward="rouge-l", score_on="device"))
    with pytest.raises(ValueError, match="65536"):
        NIC(N, U, E, 65537, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", self_critical=SC(END, reward="bleu4", score_on="device"))


# ---------------------------------------------------------------------------------------------------- fit(validation_captions=)
def plain(seed=1):
    rng = np.random.default_rng(seed)
    model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    for name in model.trainable_names():
        model.set_weight(name, 0.3 * rng.standard_normal(model.keras_shapes[name]))
    model.compile(Adam(1e-2, clipnorm=0.1))
    return model


def batches(n, seed):
    return [synth_batch(B, N, T, V, U, np.random.default_rng(seed + s)) for s in range(n)]


def decoded(model, val):
    """(captions, references) of the validation set: the model's public greedy decode from each caption's column 0, cut at
    the first END or 0, and each row's own caption"""
    cut = SC(END).truncate
    caps, refs = [], []
    for (x, cap, a0, c0), _ in val:
        probs = model.greedy_predict(x, a0, c0, cap[:, 0], cap.shape[1] - 1)
        ids = probs[:, :, 0, :].argmax(-1).T
        caps += [cut(row) for row in ids]
        refs += [[cut(row[1:])] for row in cap]
    return caps, refs


class Expect:
    """a callback that scores the public decode on the host at the end of every epoch, while the weights are the ones the
    epoch validated"""

    def __init__(self, val):
        self.val, self.rouge, self.bleu = val, [], []

    def on_epoch_end(self, epoch, logs=None):
        caps, refs = decoded(self.model, self.val)
        self.rouge.append(float(np.mean([evaluate.rouge_l(r, c) for c, r in zip(caps, refs)])))
        self.bleu.append(float(np.mean([evaluate.sentence_bleu(r, c, weights=(0.25,) * 4) for c, r in zip(caps, refs)])))


def test_fit_without_the_keyword_launches_and_logs_as_before(mock_backend):
    train, val = batches(3, 30), batches(2, 40)
    runs = []
    for kw in ({}, dict(validation_captions=None), dict(validation_captions=CaptionValidation(END))):
        model = plain()
        del mock_backend.log[:]
        hist = model.fit(train, epochs=2, validation_data=val, verbose=0, **kw)
        runs.append((list(mock_backend.log), hist, model.arena.theta.numpy().copy()))
    (log0, hist0, th0), (log1, hist1, th1), (log2, hist2, th2) = runs
    assert log0 == log1 and hist0 == hist1 and np.array_equal(th0, th1)
    assert "caption_rouge" not in log0 and "caption_reward" not in log0 and "argmax_rows" not in log0
    # with the keyword: the same weights and the same pre-existing logs, bit for bit, and only decode / score launches added
    assert np.array_equal(th0, th2) and {k: hist2[k] for k in hist0} == hist0
    assert sorted(set(hist2) - set(hist0)) == ["val_bleu4", "val_rouge_l"]
    assert log2.count("caption_rouge") == log2.count("caption_reward") == 2 * len(val)
    first = log2.index("argmax_rows")
    assert log2[:first].count("softmax_cce") >= len(train) + len(val)                      # behind the epoch's test_step pass
    it = iter(log2)
    assert all(name in it for name in log0)                                                # log0 is a subsequence of log2


def test_fit_logs_the_decoded_captions_scores_and_the_callbacks_act_on_them(mock_backend, tmp_path):
    train, val = batches(3, 50), batches(2, 60)
    model = plain()
    seen, exp = [], Expect(val)

    class Seen:
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))
    path = str(tmp_path / "best_{epoch}.npz")
    ck = ModelCheckpoint(path, monitor="val_rouge_l", save_best_only=True, mode="max")
    hist = model.fit(train, epochs=3, validation_data=val, verbose=0, validation_captions=CaptionValidation(END),
                     callbacks=[exp, Seen(), ck])
    assert len(hist["val_rouge_l"]) == len(hist["val_bleu4"]) == 3
    assert np.abs(np.array(hist["val_rouge_l"]) - exp.rouge).max() <= 1e-12 and max(exp.rouge) > 0
    assert np.abs(np.array(hist["val_bleu4"]) - exp.bleu).max() <= 1e-9
    assert [s["val_rouge_l"] for s in seen] == hist["val_rouge_l"] and all("val_loss" in s for s in seen)
    # the checkpoint keeps the epochs whose val_rouge_l beat every earlier one
    best, kept = -np.inf, []
    for e, v in enumerate(hist["val_rouge_l"]):
        if v > best:
            best, kept = v, kept + [e + 1]
    assert sorted(int(p.stem.split("_")[1]) for p in tmp_path.iterdir()) == kept and ck.best == -best


def test_early_stopping_and_plateau_modes():
    class Model:
        stop_training = False

    def run(cb, values, monitor="val_rouge_l"):
        cb.model = Model()
        for e, v in enumerate(values):
            cb.on_epoch_end(e, {monitor: v})
            if cb.model.stop_training:
                return e
        return None
    rising, falling = [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, 0.4, 0.3, 0.2, 0.1]
    assert run(EarlyStopping("val_rouge_l", patience=1, mode="max"), rising) is None
    assert run(EarlyStopping("val_rouge_l", patience=1, mode="max"), falling) == 2
    assert run(EarlyStopping("val_rouge_l", patience=1, mode="max"), [0.1, 0.3, 0.2, 0.31, 0.3, 0.3]) == 5
    assert run(EarlyStopping("val_rouge_l", patience=0, min_delta=0.05, mode="max"), [0.1, 0.2, 0.24]) == 2
    # the default is "min", as it was
    assert run(EarlyStopping("val_loss", patience=1), rising, "val_loss") == 2
    assert run(EarlyStopping("val_loss", patience=1), falling, "val_loss") is None
    assert run(EarlyStopping("val_loss", patience=1, mode="min"), rising, "val_loss") == 2
    with pytest.raises(ValueError, match="mode"):
        EarlyStopping(mode="auto")
    assert ReduceLROnPlateau("val_rouge_l", mode="max").sign == -1 and ReduceLROnPlateau("val_loss", mode="min").sign == 1


def test_early_stopping_acts_on_val_rouge_l_in_fit(mock_backend):
    train, val = batches(2, 70), batches(1, 80)
    model = plain()
    model.optimizer.lr = 0.0                                  # nothing changes: the metric cannot improve after epoch 1
    hist = model.fit(train, epochs=5, validation_data=val, verbose=0, validation_captions=CaptionValidation(END, metrics="rouge-l"),
                     callbacks=[EarlyStopping("val_rouge_l", patience=1, mode="max")])
    assert len(hist["val_rouge_l"]) == 3 and "val_bleu4" not in hist and model.stop_training


def test_validation_references_tables_and_beam(mock_backend):
    rng = np.random.default_rng(5)
    train, val = batches(1, 90), batches(2, 95)
    refs = [[[[int(w) for w in rng.integers(3, V, rng.integers(1, 6))] for _ in range(rng.integers(1, 4))] for _ in range(B)]
            for _ in val]
    corpus = [doc for batch in refs for doc in batch]
    table = evaluate.RewardTable(corpus)
    cv = CaptionValidation(END, table=table, references=refs)
    assert cv.metrics == ("bleu4", "rouge-l", "cider-d")
    model = plain()
    hist = model.fit(train, epochs=1, validation_data=val, verbose=0, validation_captions=cv)
    caps, _ = decoded(model, val)
    cd = evaluate.CiderD(corpus)
    assert abs(hist["val_rouge_l"][0] - np.mean([evaluate.rouge_l(r, c) for c, r in zip(caps, corpus)])) <= 1e-12
    assert abs(hist["val_cider_d"][0] - np.mean([cd(c, r) for c, r in zip(caps, corpus)])) <= 1e-9
    assert abs(hist["val_bleu4"][0] - np.mean([evaluate.sentence_bleu(r, c, weights=(0.25,) * 4) for c, r in zip(caps, corpus)])) <= 1e-9
    # the best beam of a width-1 search is the greedy caption
    beam = model.fit(train[:0], epochs=1, steps_per_epoch=0, validation_data=val, verbose=0,
                     validation_captions=CaptionValidation(END, metrics=("rouge-l",), references=refs, decode="beam", beam_width=1))
    greedy = model.fit(train[:0], epochs=1, steps_per_epoch=0, validation_data=val, verbose=0,
                       validation_captions=CaptionValidation(END, metrics=("rouge-l",), references=refs))
    assert abs(beam["val_rouge_l"][0] - greedy["val_rouge_l"][0]) <= 1e-12 and greedy["val_rouge_l"][0] > 0


def test_refusals(mock_backend):
    train, val = batches(1, 30), batches(1, 40)
    model = plain()
    model.dp_world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.fit(train, epochs=1, validation_data=val, verbose=0, validation_captions=CaptionValidation(END))
    model.dp_world = 1
    with pytest.raises(ValueError, match="validation_data"):
        model.fit(train, epochs=1, verbose=0, validation_captions=CaptionValidation(END))
    with pytest.raises(ValueError, match="CaptionValidation"):
        model.fit(train, epochs=1, validation_data=val, verbose=0, validation_captions="rouge-l")
    with pytest.raises(ValueError, match="reference lists"):
        model.fit(train, epochs=1, validation_data=val, verbose=0, validation_captions=CaptionValidation(END, references=[[[[3]]]]))
    assert mock_backend.log.count("caption_rouge") == 0
    for bad in (dict(end_id=0), dict(metrics=("meteor",)), dict(metrics=("cider-d",)), dict(metrics=()), dict(decode="sample"),
                dict(decode="beam"), dict(beam_width=3), dict(table="corpus")):
        with pytest.raises(ValueError):
            CaptionValidation(**dict(dict(end_id=END), **bad))
    for kind in ("rouge-l",):
        assert kind in evaluate.DEVICE_KINDS
    with pytest.raises(ValueError, match="kind"):
        evaluate.device_scores([[[3]]], [[[3]]], "meteor")


def test_a_model_without_a_device_decode_is_refused_before_training(mock_backend):
    from masters_thesis_amd.fc_nic import NICfc
    from masters_thesis_amd.lc_nic import NIC as LcNIC
    from masters_thesis_amd.ms_nic import NIC as MsNIC
    from masters_thesis_amd.think_and_tell import CaptionGenerator
    for cls in (NICfc, CaptionGenerator):
        model = cls.__new__(cls)                              # fit refuses before it touches the model
        model.dp_world, model.average = 1, None
        del mock_backend.log[:]
        with pytest.raises(NotImplementedError, match="validation_captions"):
            model.fit(batches(1, 30), epochs=1, validation_data=batches(1, 40), verbose=0, validation_captions=CaptionValidation(END))
        assert mock_backend.log == []
    for cls in (NIC, LcNIC, MsNIC):
        CaptionValidation.check_model(cls.__new__(cls))


def test_host_float64_scalars_are_kept_once_per_value():
    import ctypes
    from masters_thesis_amd.ops import HipBackend
    be = HipBackend.__new__(HipBackend)
    be._f64 = {}
    a, b = be._host_f64(1.2), be._host_f64(1.2)
    assert a is b and isinstance(a, ctypes.c_double) and a.value == 1.2
    n1, n2 = be._host_f64(float("nan")), be._host_f64(float("nan"))
    assert n1 is n2 and n1.value != n1.value and len(be._f64) == 2
