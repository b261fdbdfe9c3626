"""Minimum Bayes risk decoding on the CPU: the restatement (tests/mbr_oracle.py) on hand-computed cases, model_base.MBR's
validation, and the host orchestration of mbr_decode of nic.NIC and lc_nic.NIC through a mock backend that gets
``mbr_select`` from the restatement: the launch sequence and the stream step of every sampled decode, the arguments of
the one selection launch (plain and under consensus), the results, the refusals, evaluate.mbr_captions."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.model_base import MBR, Consensus, DecodeConstraints, SelfCritical
from mock_backend import flat
import mbr_oracle as MO
from test_host_consensus import members_of, names
from test_host_constrain import MAKERS, T, V, greedy_ids, sample_ids
from test_host_guidance import GuidanceMockBackend

END = 2


class MbrMockBackend(GuidanceMockBackend):
    """GuidanceMockBackend plus ``mbr_select`` from tests/mbr_oracle.py (the header's refusals as assertions), logged like
    the launches of a decode's tail; ``steps`` lists the Philox stream step of every sampler launch"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.steps = []
        self.mbr_select = self._logged("mbr_select", self.mbr_select)
        self.sample_topkp = self._stepped(self.sample_topkp)
        self.sample_rows = self._stepped(self.sample_rows)

    def _stepped(self, fn):
        def call(x, out, rows, V, ld, *a, **k):
            step, step_dev = a[-2:] if len(a) in (6, 8) else (a[-1], k.get("step_dev"))
            self.steps.append((int(step) + (int(flat(step_dev)[0]) if step_dev is not None else 0)) & 0xFFFFFFFF)
            return fn(x, out, rows, V, ld, *a, **k)
        return call

    def mbr_select(self, ids, ld, B, Nc, Nr, L, end_id, order, kind, expected, best, out_ids=None, ldo=0, match=None,
                   util=None):
        assert B > 0 and ld >= B and 1 <= Nc <= 64 and 1 <= Nr <= Nc and 1 <= L <= 64 and 1 <= order <= 4 and kind in (0, 1)
        assert ids is not None and expected is not None and best is not None and (out_ids is None or ldo >= B)
        res = MO.select(flat(ids)[:Nc * L * ld].reshape(Nc, L, ld), B, Nr, end_id, order, kind)
        flat(expected)[:B * Nc] = res["expected"].astype(np.float32).reshape(-1)
        flat(best)[:B] = res["best"]
        if out_ids is not None:
            flat(out_ids)[:L * ldo].reshape(L, ldo)[:, :B] = res["out_ids"]
        if match is not None:
            flat(match)[:B * Nc * Nr * order] = res["match"].reshape(-1)
        if util is not None:
            flat(util)[:B * Nc * Nr] = res["util"].astype(np.float32).reshape(-1)


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = MbrMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_hand_computed_cases():
    assert MO.caption([3, 4, 2, 9, 9], 2) == [3, 4] and MO.caption([3, 0, 4], 2) == [3] and MO.caption([2, 3], 2) == []
    assert MO.caption([3, 2, 4, 0, 5], -1) == [3, 2, 4] and MO.caption([0], -1) == [] and MO.caption([5, 6], 7) == [5, 6]
    # clipping: h holds 3 three times and (3, 3) twice, r holds 3 twice and (3, 3) once
    h, r = [3, 3, 3, 4], [3, 3, 4, 4]
    assert MO.match_counts(h, r, 4) == [3, 2, 1, 0] and MO.match_counts(r, h, 4) == [3, 2, 1, 0]
    assert MO.match_counts([3], r, 4) == [1, 0, 0, 0] and MO.match_counts([], r, 2) == [0, 0]
    # ngram-f: (2*3/8 + 2*2/6 + 2*1/4 + 0) / 4
    assert MO.utility(h, r, 4, "ngram-f") == pytest.approx((0.75 + 4 / 6 + 0.5) / 4)
    assert MO.utility(h, h, 4, 0) == 1.0 and MO.utility([], [], 4, 0) == 0.0 and MO.utility([3], [3], 4, 0) == 0.25
    # bleu is the library's own sentence_bleu with uniform weights; it is not symmetric (brevity penalty)
    assert MO.utility([3, 4], [3, 4, 5, 6], 2, "bleu") == evaluate.sentence_bleu([[3, 4, 5, 6]], [3, 4], weights=(0.5, 0.5))
    assert MO.utility([3, 4], [3, 4, 5, 6], 2, 1) == pytest.approx(np.exp(1 - 2))
    assert MO.utility([3, 4, 5, 6], [3, 4], 2, 1) == pytest.approx(np.sqrt(0.5 * 1 / 3))
    assert MO.utility([], [3], 2, 1) == 0.0 and MO.utility([4], [3], 2, 1) == 0.0
    # expected utility over the first Nr, the self term included; first maximum
    cands = [[3, 4, 5], [3, 4, 5], [6, 7], [3, 4]]
    m, u, e, best = MO.select_captions(cands, 3, 2, "ngram-f")
    assert m.shape == (4, 3, 2) and u.shape == (4, 3) and e[0] == e[1] and best == 0
    assert e[0] == pytest.approx((1 + 1 + 0) / 3) and e[2] == pytest.approx(1 / 3)
    assert e[3] == pytest.approx(2 * ((2 * 2 / 5 + 2 * 1 / 3) / 2) / 3)
    # the kernel's layout: candidate c of scan b at position t is ids[c, t, b]; columns behind B are not read
    ids = np.array([[[3, 6, 9], [4, 7, 9], [2, 2, 9]], [[6, 6, 9], [7, 7, 9], [2, 2, 9]]])
    res = MO.select(ids, 2, 1, END, 2, 0)
    assert res["best"].tolist() == [0, 0] and res["expected"].tolist() == [[1.0, 0.0], [1.0, 1.0]]
    assert res["out_ids"].tolist() == [[3, 6], [4, 7], [2, 2]]
    assert MO.select(ids, 2, 2, END, 2, 0)["best"].tolist() == [0, 0]          # a tie goes to the smaller index


def test_truncation_is_self_criticals():
    sc = SelfCritical(END)
    rng = np.random.default_rng(0)
    for row in rng.integers(0, 5, (50, 7)):
        assert MO.caption(row, END) == sc.truncate(row)


# ---------------------------------------------------------------------------------------------------- MBR
@pytest.mark.parametrize("kw", [dict(end_id=0), dict(end_id=-1), dict(end_id=2.0), dict(end_id=True), dict(end_id=None),
                                dict(n_samples=0), dict(n_samples=-3), dict(n_samples=4.0), dict(n_samples=True),
                                dict(n_samples=64), dict(n_samples=65, include_greedy=False), dict(n_samples=1000),
                                dict(utility="cider"), dict(utility=0), dict(utility=None),
                                dict(order=0), dict(order=5), dict(order=2.0), dict(order=True),
                                dict(include_greedy=1), dict(include_greedy=None), dict(include_greedy="yes"),
                                dict(temperature=0.0), dict(temperature=-1.0), dict(temperature="hot"),
                                dict(top_k=-1), dict(top_k=2.5), dict(top_k=True),
                                dict(top_p=0.0), dict(top_p=1.5), dict(top_p=None)])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        MBR(**{"end_id": END, **kw})


def test_defaults_limits_and_repr():
    m = MBR(END)
    assert (m.n_samples, m.utility, m.order, m.include_greedy, m.temperature, m.top_k, m.top_p) == (16, "ngram-f", 4, True, 1.0, 0, 1.0)
    assert m.kind == 0 and m.n_candidates == 17 and MBR(END, utility="bleu").kind == 1
    assert MBR(END, n_samples=63).n_candidates == 64 and MBR(END, n_samples=64, include_greedy=False).n_candidates == 64
    assert "n_samples=16" in repr(m) and "ngram-f" in repr(m)


# ---------------------------------------------------------------------------------------------------- the decodes
def check_against_candidates(words, info, mbr, M, Nc):
    """the returned shapes, and best / expected / ids against the restatement applied to the returned candidates"""
    cand = info["candidates"]
    assert words.shape == (M, T, 1) and words.dtype == np.int64 and cand.shape == (M, Nc, T) and cand.dtype == np.int64
    assert info["expected"].shape == (M, Nc) and info["expected"].dtype == np.float32
    assert info["best"].shape == (M,) and info["best"].dtype == np.int32
    want = MO.select(cand.transpose(1, 2, 0), M, mbr.n_samples, mbr.end_id, mbr.order, mbr.kind)
    assert np.array_equal(info["best"], want["best"])
    assert np.array_equal(info["expected"], want["expected"].astype(np.float32))
    assert np.array_equal(words[:, :, 0], cand[np.arange(M), info["best"]])


@pytest.mark.parametrize("kind,seed", [("dense", 3), ("lc", 4)])
@pytest.mark.parametrize("filtered", [True, False])
def test_launch_sequence_steps_and_results(mock_backend, kind, seed, filtered):
    model, orc, x, z, start = MAKERS[kind](seed)
    M, N, s = x.shape[0], 3, 5
    skw = dict(temperature=0.8, top_k=6, top_p=0.9) if filtered else dict(temperature=0.8)
    mbr = MBR(END, n_samples=N, utility="bleu", order=3, **skw)
    mock_backend.log.clear()
    words, info = model.mbr_decode(x, z, z, start, T, mbr, sample_step=s, return_candidates=True)
    # N sampled decodes, one greedy decode, one selection launch; the attention model's unfiltered draw is its sample_rows
    sampler = "sample_topkp" if filtered or kind == "dense" else "sample_rows"
    assert names(mock_backend) == ["softmax_cce", sampler] * (T * N) + ["softmax_cce", "argmax_rows"] * T + ["mbr_select"]
    assert mock_backend.steps == [s + c for c in range(N) for _ in range(T)]
    a = mock_backend.log[-1][1]
    assert a[1:9] == (M, M, N + 1, N, T, END, 3, 1) and a[12] == M                   # ld, B, Nc, Nr, L, end_id, order, kind; ldo
    assert a[0].dtype == a[10].dtype == a[11].dtype == torch.int32 and tuple(a[0].shape) == (N + 1, T, M)
    check_against_candidates(words, info, mbr, M, N + 1)
    # candidate c is sample_predict's draw at sample_step + c, the last one greedy_predict's caption
    for c in range(N):
        assert np.array_equal(info["candidates"][:, c], sample_ids(kind, model, x, z, start, sample_step=s + c, **skw)[0])
    assert np.array_equal(info["candidates"][:, N], greedy_ids(kind, model, x, z, start)[0])
    # a second call: the same output; without the candidates
    again, info2 = model.mbr_decode(x, z, z, start, T, mbr, sample_step=s)
    assert np.array_equal(again, words) and set(info2) == {"expected", "best"}
    assert np.array_equal(info2["expected"], info["expected"]) and np.array_equal(info2["best"], info["best"])


@pytest.mark.parametrize("kind,seed", [("dense", 5), ("lc", 6)])
def test_without_greedy_every_candidate_is_a_reference(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    M, N = x.shape[0], 4
    mbr = MBR(END, n_samples=N, include_greedy=False, top_k=5)
    mock_backend.log.clear()
    words, info = model.mbr_decode(x, z, z, start, T, mbr, return_candidates=True)
    assert names(mock_backend) == ["softmax_cce", "sample_topkp"] * (T * N) + ["mbr_select"]
    assert mock_backend.log[-1][1][3:5] == (N, N) and mock_backend.log[-1][1][7:9] == (4, 0)
    check_against_candidates(words, info, mbr, M, N)


@pytest.mark.parametrize("kind,seed", [("dense", 7), ("lc", 8)])
def test_consensus_reads_the_mixed_rows_of_the_member_buffer(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    G, N, s = 2, 3, 1
    xs, zs, st = members_of(model, x, z, start, G, seed)
    M = st.shape[0]
    mbr = MBR(END, n_samples=N, top_k=6, top_p=0.95, temperature=0.9)
    cons = Consensus(G)
    mock_backend.log.clear()
    words, info = model.mbr_decode(xs, zs, zs, st, T, mbr, sample_step=s, consensus=cons, return_candidates=True)
    assert names(mock_backend) == (["consensus_mix", "sample_topkp", "consensus_spread"] * (T * N) + ["consensus_mix"] * T
                                   + ["mbr_select"])
    assert mock_backend.steps == [s + c for c in range(N) for _ in range(T)]
    a = mock_backend.log[-1][1]
    assert a[1:6] == (G * M, M, N + 1, N, T) and a[12] == M and tuple(a[0].shape) == (N + 1, T, G * M)
    check_against_candidates(words, info, mbr, M, N + 1)
    kw = dict(temperature=0.9, top_k=6, top_p=0.95, consensus=cons)
    for c in range(N):
        assert np.array_equal(info["candidates"][:, c], sample_ids(kind, model, xs, zs, st, sample_step=s + c, **kw)[0])
    assert np.array_equal(info["candidates"][:, N], greedy_ids(kind, model, xs, zs, st, consensus=cons)[0])


def test_constraints_reach_every_candidate_decode(mock_backend):
    model, orc, x, z, start = MAKERS["dense"](9)
    N = 2
    con = DecodeConstraints(no_repeat_ngram_size=1)
    mbr = MBR(END, n_samples=N, top_k=8)
    mock_backend.log.clear()
    words, info = model.mbr_decode(x, z, z, start, T, mbr, constraints=con, return_candidates=True)
    assert names(mock_backend).count("decode_constrain") == T * (N + 1) and names(mock_backend)[-1] == "mbr_select"
    for row in info["candidates"].reshape(-1, T):
        assert len(set(row.tolist())) == T                                       # no token twice in any candidate
    check_against_candidates(words, info, mbr, x.shape[0], N + 1)


@pytest.mark.parametrize("kind,seed", [("dense", 11), ("lc", 12)])
def test_decode_refuses_before_any_launch(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    mbr = MBR(END, n_samples=2)
    mock_backend.log.clear()
    for bad in (65, 0, -1, 6.0, True):
        with pytest.raises(ValueError, match="max_len"):
            model.mbr_decode(x, z, z, start, bad, mbr)
    with pytest.raises(ValueError, match="MBR"):
        model.mbr_decode(x, z, z, start, T, dict(n_samples=2))
    with pytest.raises(ValueError, match="sample_step"):
        model.mbr_decode(x, z, z, start, T, mbr, sample_step=0.5)
    with pytest.raises(ValueError, match="Consensus"):
        model.mbr_decode(x, z, z, start, T, mbr, consensus=dict(members=2))
    model.grad_sync = SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        model.mbr_decode(x, z, z, start, T, mbr)
    model.grad_sync = None
    assert not mock_backend.log and "_mbr_bufs" not in model.__dict__


def test_models_without_a_candidate_decode_refuse():
    from masters_thesis_amd.model_base import ModelBase
    stub = SimpleNamespace(grad_sync=None)
    stub._mbr_candidate = lambda *a, **k: ModelBase._mbr_candidate(stub, *a, **k)
    with pytest.raises(NotImplementedError, match="minimum Bayes risk"):
        ModelBase.mbr_decode(stub, None, None, None, [1], T, MBR(END))


def test_evaluate_mbr_captions(mock_backend):
    model, orc, x, z, start = MAKERS["dense"](13)
    tok = SimpleNamespace(word_index={"<start>": 1, "<end>": END}, index_word={i: f"w{i}" for i in range(3, V)})
    tok.index_word.update({1: "<start>", END: "<end>"})
    mbr = MBR(END, n_samples=3, top_k=5)
    ids, caps, info = evaluate.mbr_captions(model, x, z, z, tok, T, mbr, sample_step=2)
    words, want = model.mbr_decode(x, z, z, start, T, mbr, sample_step=2)
    assert ids.shape == (x.shape[0], T) and np.array_equal(ids, words[:, :, 0]) and np.array_equal(info["best"], want["best"])
    assert len(caps) == x.shape[0]
    for row, cap in zip(ids, caps):
        cut = row.tolist().index(END) if END in row else T
        assert cap == [f"w{i}" for i in row[:cut] if i not in (0, 1)]             # ids_to_captions' rule
    with pytest.raises(ValueError, match="end_id"):
        evaluate.mbr_captions(model, x, z, z, tok, T, MBR(3, n_samples=3))
