"""Minimum Bayes risk decoding on the GPU, the models: mbr_decode of nic.NIC and lc_nic.NIC with the weights of the tiny
golden fixtures -- every candidate is sample_predict's draw at its stream step, the last one greedy_predict's caption; best,
expected and the returned ids are the restatement (tests/mbr_oracle.py) applied to those candidates; a second call
repeats the output; constraints and guidance reach every candidate decode."""
import numpy as np
import pytest

import consensus_oracle as CO
import mbr_oracle as MO
from test_gpu_consensus_models import device_model
from test_gpu_mbr import REL0, rel1

pytestmark = pytest.mark.gpu

N_SAMPLES, MAX_LEN, END, STEP = 4, 6, 2, 7
FILTERS = dict(temperature=0.9, top_k=5, top_p=0.95)


def sample_ids(kind, model, x, z, start, **kw):
    return model.sample_predict(x, z, z, start, MAX_LEN, **kw)[0][:, :, 0]


def greedy_ids(kind, model, x, z, start, **kw):
    if kind == "dense":
        return model.greedy_predict(x, z, z, start, MAX_LEN, **kw)[:, :, 0, :].argmax(-1).T
    return model.greedy_predict(x, z, z, start, MAX_LEN, return_s=False, **kw)[0][:, :, 0]


def decode_kw(case):
    from masters_thesis_amd.model_base import DecodeConstraints, Guidance
    if case == "constraints":
        return dict(constraints=DecodeConstraints(no_repeat_ngram_size=2, min_length=3, end_id=END))
    if case == "guidance":
        return dict(guidance=Guidance(1.5, plausibility=0.05))
    return {}


@pytest.mark.parametrize("case,utility,filters", [("plain", "ngram-f", FILTERS), ("plain", "bleu", dict(temperature=1.1)),
                                                  ("constraints", "bleu", FILTERS), ("guidance", "ngram-f", FILTERS)])
@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_candidates_choice_and_replay(kind, case, utility, filters):
    from masters_thesis_amd.model_base import MBR
    _, model = device_model(kind)
    x, z, start = CO.scans(1, 3, 21)
    M, Nc = 3, N_SAMPLES + 1
    mbr = MBR(END, n_samples=N_SAMPLES, utility=utility, order=3, **filters)
    kw = decode_kw(case)
    words, info = model.mbr_decode(x, z, z, start, MAX_LEN, mbr, sample_step=STEP, return_candidates=True, **kw)
    cand = info["candidates"]
    assert words.shape == (M, MAX_LEN, 1) and cand.shape == (M, Nc, MAX_LEN)
    assert info["expected"].shape == (M, Nc) and info["best"].shape == (M,)
    # the candidates: sample_predict's draws at the stream steps STEP + c, then greedy_predict's caption
    for c in range(N_SAMPLES):
        assert np.array_equal(cand[:, c], sample_ids(kind, model, x, z, start, sample_step=STEP + c, **filters, **kw)), c
    assert np.array_equal(cand[:, N_SAMPLES], greedy_ids(kind, model, x, z, start, **kw))
    assert len({row.tobytes() for row in cand.reshape(-1, MAX_LEN)}) > M           # the draws differ
    if case == "constraints":
        assert not np.any(cand[:, :, :3] == END)                                   # min_length = 3 on every candidate
    # the choice: the restatement on those candidates (float tolerances of tests/test_gpu_mbr.py)
    want = MO.select(cand.transpose(1, 2, 0), M, N_SAMPLES, END, mbr.order, mbr.kind)
    rel = REL0 if mbr.kind == 0 else rel1(MAX_LEN)
    assert np.all(np.abs(info["expected"] - want["expected"]) <= rel * want["expected"])
    assert np.array_equal(info["best"], MO.first_max(info["expected"]))
    e64 = want["expected"]
    assert np.all(e64[np.arange(M), info["best"]] >= e64.max(axis=1) * (1 - 2 * rel))
    assert np.array_equal(words[:, :, 0], cand[np.arange(M), info["best"]])
    # a second call (the captured decodes replayed): identical output
    again, info2 = model.mbr_decode(x, z, z, start, MAX_LEN, mbr, sample_step=STEP, return_candidates=True, **kw)
    assert np.array_equal(again, words) and np.array_equal(info2["candidates"], cand) and np.array_equal(info2["best"], info["best"])
    assert np.array_equal(info2["expected"].view(np.int32), info["expected"].view(np.int32))
