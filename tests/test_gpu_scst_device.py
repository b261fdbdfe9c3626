"""Device-scored self-critical training on the GPU, the model: nic.NIC(self_critical=SelfCritical(score_on="device"))
against the host-scored step from the same seed and batch (metrics, advantages) and against the float64 step of
tests/scst_oracle.py (loss, gradients) at the small sizes of tests/test_gpu_scst.py; launch-plan replay against hipGraph
replay; several references per scan; and that nothing waits for the stream between the rollout and the update."""
import numpy as np
import pytest
import torch

from helpers import synth_batch
from test_gpu_scst import END, LAM, _case
from scst_oracle import expand, greedy, policy_grads, rollout

pytestmark = pytest.mark.gpu


def batch():
    """the batch _case("small", ...) hands out"""
    return synth_batch(8, 23, 6, 13, 16, np.random.default_rng(17))


def corpus_of(data, V, n_extra=30, seed=3):
    """documents: each scan's own caption (what references=None scores against) and random others"""
    from masters_thesis_amd.model_base import SelfCritical
    cut = SelfCritical(END).truncate
    rng = np.random.default_rng(seed)
    docs = [[cut(row[1:])] for row in np.asarray(data[1])]
    docs += [[[int(w) for w in rng.integers(3, V, rng.integers(1, 6))] for _ in range(rng.integers(1, 4))] for _ in range(n_extra)]
    return docs


def spec(K, baseline, reward, score_on, corpus):
    from masters_thesis_amd.model_base import SelfCritical
    return SelfCritical(END, n_samples=K, baseline=baseline, reward=reward, corpus=corpus if reward == "cider-d" else None,
                        score_on=score_on)


def adv_close(got, want64):
    """within one float32 ulp of float32(want); where the advantage is below the float64 noise of its two scores
    (1e-9 each, the bound of tests/test_gpu_reward.py), within 2e-9 of it"""
    w32 = want64.astype(np.float32)
    return bool(((np.abs(got - w32) <= np.spacing(np.abs(w32))) | (np.abs(got.astype(np.float64) - want64) <= 2e-9)).all())


@pytest.mark.parametrize("reward", ["cider-d", "bleu4"])
@pytest.mark.parametrize("K,baseline", [(1, "greedy"), (3, "mean")])
def test_device_scored_step_matches_the_host_scored_step_and_float64(K, baseline, reward):
    from oracle import models as M
    data, _ = batch()
    corpus = corpus_of(data, 13)
    host, _, data, tgt = _case("small", spec(K, baseline, reward, "host", corpus))
    dev, orc, _, _ = _case("small", spec(K, baseline, reward, "device", corpus))
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
    # loss and every gradient of the device-scored model against float64, with test_model_matches_float64's margin rule
    drop = M.DropCtx(seed=42, step=0, training=True)
    data_r = expand(data, K)
    fed, last, margin = rollout(orc, data_r, drop)
    ok = margin > 1e-4
    assert np.array_equal(dfed[ok], fed[ok]) and np.array_equal(dlast[ok], last[ok])
    if baseline == "greedy":
        assert np.array_equal(g, greedy(orc, data, data[1].shape[1]))
    loss, grads = policy_grads(orc, data_r, dfed.astype(np.int64), dlast, adv, END, drop)
    assert abs(md["loss"] - loss) < 1e-4 * max(1, abs(loss))
    for k in M.NICDense.TRAINABLE:
        gk = dev.get_gradient(k) + 2 * LAM.get(k, 0.0) * orc.p[k]
        assert np.abs(gk - grads[k]).max() <= 1e-4 * np.abs(grads[k]).max() + 1e-9, k
    # the update: the two models read advantages a float32 ulp apart at most
    for k in dev.trainable_names():
        a, b = dev.get_weight(k), host.get_weight(k)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-7, k


@pytest.mark.parametrize("K,baseline,reward", [(2, "greedy", "cider-d"), (2, "mean", "bleu4")])
def test_launch_plan_replay_equals_graph_replay(K, baseline, reward):
    """Four device-scored steps (eager, record / capture, two replays) as launch plans and as hipGraphs: bit-identical
    metrics, sampled ids and weights; the reward launch is part of the recorded update segment"""
    data, _ = batch()
    corpus = corpus_of(data, 13)
    models = [_case("small", spec(K, baseline, reward, "device", corpus), rates=(0.1, 0.2, 0.2), seed=5, plan=p) for p in (True, False)]
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
    assert isinstance(plan, tuple) and [name for _, name, _ in plan[1]][:2] == ["tnt_caption_reward_f32", "tnt_scst_cce_f32"]
    assert isinstance(b._graphs[("scst_update", 8 * K, 6)], torch.cuda.CUDAGraph)
    for k in a.trainable_names():
        assert np.array_equal(a.get_weight(k), b.get_weight(k)), k


@pytest.mark.parametrize("reward", ["cider-d", "bleu4"])
def test_several_references_per_scan(reward):
    data, _ = batch()
    corpus = corpus_of(data, 13)
    rng = np.random.default_rng(9)
    host, _, data, tgt = _case("small", spec(2, "greedy", reward, "host", corpus))
    dev, _, _, _ = _case("small", spec(2, "greedy", reward, "device", corpus))
    refs = [[[int(w) for w in rng.integers(3, 13, rng.integers(1, 6))] for _ in range(1 + b)] for b in range(8)]      # 1 .. 8 of them
    mh = host.train_step_scst((data, tgt), references=refs).as_floats()
    md = dev.train_step_scst((data, tgt), references=refs).as_floats()
    assert np.array_equal(dev.cap.cpu().numpy(), host.cap.cpu().numpy())
    for k in ("reward", "baseline", "sample_len"):
        assert abs(mh[k] - md[k]) <= 1e-9, (k, mh[k], md[k])
    assert mh["reward"] > 0 and mh["baseline"] > 0
    assert adv_close(dev._scst["adv"].cpu().numpy(), host._scst["adv"].cpu().numpy().astype(np.float64))
    assert dev._scst["n_refs"].cpu().numpy().tolist() == list(range(1, 9))
    # the next step scores against the scans' own captions again, in the same buffers
    sc = host.self_critical
    md = dev.train_step_scst((data, tgt)).as_floats()
    samples = np.concatenate([dev.cap.cpu().numpy()[:, 1:], dev._scst["last"].cpu().numpy()[:, None]], 1)
    adv, rew, base, _ = sc.advantages(samples, [[sc.truncate(row[1:])] for row in data[1]], dev._scst["greedy"].cpu().numpy().T)
    assert abs(md["reward"] - rew.mean()) <= 1e-9 and abs(md["baseline"] - base.mean()) <= 1e-9
    assert adv_close(dev._scst["adv"].cpu().numpy(), adv)


def test_nothing_waits_between_the_rollout_and_the_update(monkeypatch):
    """counted on the first (eager) step, where every launch goes through the backend's methods: between the rollout's
    last launch (sample_rows) and the enqueue of scst_cce the device-scored step synchronises no stream and copies
    nothing to the host; the host-scored step, under the same probes, does both"""
    from masters_thesis_amd.model_base import SelfCritical
    events = []
    sync, copy_ = torch.cuda.Stream.synchronize, torch.Tensor.copy_

    def probe_sync(self, *a, **k):
        events.append("sync")
        return sync(self, *a, **k)

    def probe_copy(self, src, *a, **k):
        if self.device.type == "cpu" and isinstance(src, torch.Tensor) and src.device.type == "cuda":
            events.append("d2h")
        return copy_(self, src, *a, **k)

    def between(score_on):
        sc = SelfCritical(END, n_samples=2, baseline="greedy", reward="bleu4", score_on=score_on)
        model, _, data, tgt = _case("small", sc)
        be = model.be
        del events[:]
        with monkeypatch.context() as mp:
            for name in ("sample_rows", "scst_cce", "caption_reward"):
                def logged(*a, _fn=getattr(be, name), _name=name, **k):
                    events.append(_name)
                    return _fn(*a, **k)
                mp.setattr(be, name, logged)
            mp.setattr(torch.cuda.Stream, "synchronize", probe_sync)
            mp.setattr(torch.Tensor, "copy_", probe_copy)
            out = model.train_step((data, tgt))
        seen = list(events)
        assert seen.count("sample_rows") == 1 and seen.count("scst_cce") == 1, seen
        out.as_floats()
        return seen[seen.index("sample_rows") + 1:seen.index("scst_cce")]

    assert between("device") == ["caption_reward"]
    mid = between("host")
    assert "sync" in mid and "d2h" in mid and "caption_reward" not in mid
