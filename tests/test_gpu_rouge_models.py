"""ROUGE-L on the GPU, the models.  nic.NIC(self_critical=SelfCritical(reward="rouge-l")) scored on the device against the
same step scored on the host, with the comparison and the tolerances tests/test_gpu_scst_device.py applies to its two arms
(both baselines, launch plans and hipGraphs), and launch-plan replay against hipGraph replay.  fit(validation_captions=...)
of nic.NIC at the small shape of tests/test_gpu_scst.py and of lc_nic.NIC at the tiny golden shape: two epochs over two
validation batches with and without the keyword -- the trained weights and every pre-existing log are bit-identical, and
val_rouge_l / val_bleu4 are the means of evaluate.rouge_l (1e-12) / evaluate.sentence_bleu (1e-9, the reward kernel's
bound) over the captions of the model's public greedy decode, taken at the end of each epoch."""
import numpy as np
import pytest
import torch

from helpers import synth_batch
from test_gpu_scst import END, _case
from test_gpu_scst_device import adv_close

pytestmark = pytest.mark.gpu


def spec(K, baseline, score_on):
    from masters_thesis_amd.model_base import SelfCritical
    return SelfCritical(END, n_samples=K, baseline=baseline, reward="rouge-l", score_on=score_on)


@pytest.mark.parametrize("plan", [True, False])
@pytest.mark.parametrize("K,baseline", [(1, "greedy"), (3, "mean"), (2, "greedy")])
def test_device_scored_rouge_step_matches_the_host_scored_step(K, baseline, plan):
    host, _, data, tgt = _case("small", spec(K, baseline, "host"), plan=plan)
    dev, _, _, _ = _case("small", spec(K, baseline, "device"), plan=plan)
    mh = host.train_step((data, tgt)).as_floats()
    md = dev.train_step((data, tgt)).as_floats()
    dfed, dlast = dev.cap.cpu().numpy(), dev._scst["last"].cpu().numpy()
    assert np.array_equal(dfed, host.cap.cpu().numpy()) and np.array_equal(dlast, host._scst["last"].cpu().numpy())
    for k in ("reward", "baseline", "sample_len"):
        assert abs(mh[k] - md[k]) <= 1e-9, (k, mh[k], md[k])
    # the advantages the update read, against SelfCritical.advantages on the ids the device sampled
    sc = host.self_critical
    refs = [[sc.truncate(row[1:])] for row in data[1]]
    g = dev._scst["greedy"].cpu().numpy().T if baseline == "greedy" else None
    samples = np.concatenate([dfed[:, 1:], dlast[:, None]], 1)
    adv, rew, base, counted = sc.advantages(samples, refs, g)
    assert np.any(adv != 0) and rew.max() > 0
    assert adv_close(dev._scst["adv"].cpu().numpy(), adv)
    assert np.array_equal(host._scst["adv"].cpu().numpy(), adv.astype(np.float32))
    assert np.abs(dev._scst["score"].cpu().numpy()[:, :K].reshape(-1) - rew).max() <= 1e-9
    assert np.array_equal(dev._scst["counted"].cpu().numpy(), counted.astype(np.int32))
    assert abs(md["loss"] - mh["loss"]) <= 1e-5 * max(1.0, abs(mh["loss"]))
    # the update: the two models read advantages a float32 ulp apart at most
    for k in dev.trainable_names():
        a, b = dev.get_weight(k), host.get_weight(k)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-7, k


@pytest.mark.parametrize("K,baseline", [(2, "greedy"), (2, "mean")])
def test_launch_plan_replay_equals_graph_replay(K, baseline):
    """Four device-scored steps (eager, record / capture, two replays) as launch plans and as hipGraphs: bit-identical
    metrics, sampled ids and weights; the ROUGE launch opens the recorded update segment, and the replayed step's
    advantages are the host scorer's on the ids that step sampled"""
    models = [_case("small", spec(K, baseline, "device"), rates=(0.1, 0.2, 0.2), seed=5, plan=p) for p in (True, False)]
    mets, feds = [[], []], [[], []]
    for _ in range(4):
        for i, (m, _, data, tgt) in enumerate(models):
            mets[i].append(m.train_step((data, tgt)).as_floats())
            feds[i].append(m.cap.cpu().numpy().copy())
    assert mets[0] == mets[1]
    for a, b in zip(*feds):
        assert np.array_equal(a, b)
    assert not np.array_equal(feds[0][3], feds[0][2]) and mets[0][3]["reward"] != mets[0][2]["reward"]
    a, b = models[0][0], models[1][0]
    plan = a._graphs[("scst_update", 8 * K, 6)]
    assert isinstance(plan, tuple) and [name for _, name, _ in plan[1]][:2] == ["tnt_caption_rouge_f32", "tnt_scst_cce_f32"]
    assert isinstance(b._graphs[("scst_update", 8 * K, 6)], torch.cuda.CUDAGraph)
    for k in a.trainable_names():
        assert np.array_equal(a.get_weight(k), b.get_weight(k)), k
    data = models[0][2]
    for m in (a, b):
        sc = m.self_critical
        samples = np.concatenate([m.cap.cpu().numpy()[:, 1:], m._scst["last"].cpu().numpy()[:, None]], 1)
        g = m._scst["greedy"].cpu().numpy().T if baseline == "greedy" else None
        adv, rew, _, _ = sc.advantages(samples, [[sc.truncate(row[1:])] for row in data[1]], g)
        assert adv_close(m._scst["adv"].cpu().numpy(), adv) and abs(mets[0][3]["reward"] - rew.mean()) <= 1e-9


# ---------------------------------------------------------------------------------------------------- fit(validation_captions=)
def dense_model():
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    B, N, T, V, U, E = 8, 23, 6, 13, 16, 12
    model = NIC(N, U, E, V, T, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5, seed=42)
    model.compile(Adam(1e-2, clipnorm=None))
    return model, (B, N, T, V, U)


def lc_model():
    from masters_thesis_amd.optimizers import Adam
    from test_gpu_consensus_models import device_model
    _, model = device_model("lc")
    import make_golden as G                                  # device_model has put tests/golden on the path
    model.compile(Adam(1e-2, clipnorm=None))
    return model, (8, G.N, G.T, G.V, G.U)


def public_greedy(kind, model, x, a0, c0, start, L):
    if kind == "dense":
        return model.greedy_predict(x, a0, c0, start, L)[:, :, 0, :].argmax(-1).T
    return model.greedy_predict(x, a0, c0, start, L, return_s=False)[0][:, :, 0]


class Expect:
    """scores the public greedy decode on the host at the end of every epoch, under the weights the epoch validated"""

    def __init__(self, kind, val):
        self.kind, self.val, self.rouge, self.bleu, self.lengths = kind, val, [], [], []

    def on_epoch_end(self, epoch, logs=None):
        from masters_thesis_amd import evaluate
        from masters_thesis_amd.model_base import SelfCritical
        cut = SelfCritical(END).truncate
        r, b = [], []
        for (x, cap, a0, c0), _ in self.val:
            ids = public_greedy(self.kind, self.model, x, a0, c0, cap[:, 0], cap.shape[1] - 1)
            for row, own in zip(ids, cap):
                c, ref = cut(row), [cut(own[1:])]
                r.append(evaluate.rouge_l(ref, c))
                b.append(evaluate.sentence_bleu(ref, c, weights=(0.25,) * 4))
                self.lengths.append(len(c))
        self.rouge.append(float(np.mean(r)))
        self.bleu.append(float(np.mean(b)))


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_fit_validation_captions(kind):
    from masters_thesis_amd.evaluate import CaptionValidation
    make = dense_model if kind == "dense" else lc_model
    runs = []
    for with_captions in (False, True):
        model, (B, N, T, V, U) = make()
        # captions over the three words 3, 4, 5 of the V the model holds: a decode shares a word with its reference often
        train = [synth_batch(B, N, T, 6, U, np.random.default_rng(100 + s)) for s in range(3)]
        val = [synth_batch(B, N, T, 6, U, np.random.default_rng(200 + s)) for s in range(2)]
        exp = Expect(kind, val)
        kw = dict(validation_captions=CaptionValidation(END), callbacks=[exp]) if with_captions else {}
        hist = model.fit(train, epochs=2, validation_data=val, verbose=0, **kw)
        model.check_device_errors()
        runs.append((hist, {k: model.get_weight(k) for k in model.trainable_names()}, exp))
    (h0, w0, _), (h1, w1, exp) = runs
    assert sorted(set(h1) - set(h0)) == ["val_bleu4", "val_rouge_l"] and "val_loss" in h0
    assert {k: h1[k] for k in h0} == h0                                          # every pre-existing log, bit for bit
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    print(kind, "val_rouge_l", h1["val_rouge_l"], exp.rouge, "val_bleu4", h1["val_bleu4"], exp.bleu)
    assert len(h1["val_rouge_l"]) == 2 and np.abs(np.array(h1["val_rouge_l"]) - exp.rouge).max() <= 1e-12
    assert np.abs(np.array(h1["val_bleu4"]) - exp.bleu).max() <= 1e-9
    assert max(exp.rouge) > 0 and max(exp.lengths) > 0
