"""Beam search of the dense model (nic.NIC.beam_search), length normalisation of both models' results and
evaluate.beam_captions, on the CPU: the float64 restatement (tests/dense_beam_oracle.py) checked for its properties, and
the model's host orchestration through a mock backend that follows tnt_beam_step_f32's header definition."""
from types import SimpleNamespace

import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import beam_backtrack, beam_init_scores, length_normalise
from masters_thesis_amd.nic import NIC as DenseNIC
from oracle import models as M
from helpers import synth_batch, tiny_groups
from dense_beam_oracle import BeamMockBackend, BeamNICDense, length_normalise as length_normalise_ref

MARGIN = 1e-4


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = BeamMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def make_dense(rng, N=23, T=6, V=13, U=16, E=10, norm="batch", seed=11):
    model = DenseNIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, norm=norm, device="cpu", seed=seed)
    orc = BeamNICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, norm=norm).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def dense_case(seed, B=6, norm="batch"):
    rng = np.random.default_rng(seed)
    model, orc = make_dense(rng, norm=norm)
    data, _ = synth_batch(B, 23, 6, 13, 16, rng)
    z = np.zeros((B, 16), np.float32)
    return model, orc, data[0], z, np.ones(B, np.int64)


def emitted_id(orc, x, z, start, T):
    """a token other than 0 that the greedy decode really emits after its first position (the most frequent one)"""
    g = orc.greedy_predict(x, z, z, start, T)[1:, :, 0, :].argmax(-1).reshape(-1)
    ids, n = np.unique(g[g != 0], return_counts=True)
    return int(ids[n.argmax()])


# ---------------------------------------------------------------------------------------------------- restatement
def test_width1_is_greedy():
    _, orc, x, z, start = dense_case(71)
    T = 6
    seqs, _, margin = orc.beam_search(x, z, z, start, T, k=1)
    greedy = orc.greedy_predict(x, z, z, start, T)[:, :, 0, :].argmax(-1).T
    ok = margin > 0
    assert ok.sum() >= len(ok) - 1
    assert np.array_equal(seqs[ok, 0], greedy[ok])


@pytest.mark.parametrize("k", [2, 3, 5])
def test_scores_non_increasing_and_equal_to_path_scores(k):
    _, orc, x, z, start = dense_case(72)
    T = 6
    eid = emitted_id(orc, x, z, start, T)
    for end_id in (-1, eid):
        seqs, score, _ = orc.beam_search(x, z, z, start, T, k=k, end_id=end_id)
        assert np.all(np.diff(score, axis=1) <= 0)
        assert np.allclose(orc.path_score(x, z, z, start, seqs, end_id), score, rtol=1e-12, atol=1e-9)


def test_end_id_finishes_and_pads_with_zero():
    _, orc, x, z, start = dense_case(73)
    T = 6
    eid = emitted_id(orc, x, z, start, T)
    seqs, score, _ = orc.beam_search(x, z, z, start, T, k=4, end_id=eid)
    hit = seqs == eid
    assert hit.any()                                 # the finished-beam rule is exercised
    first = np.where(hit.any(2), hit.argmax(2), T)
    after = np.arange(T)[None, None, :] > first[:, :, None]
    assert after.any() and np.all(seqs[after] == 0)
    # end_id = -1 never finishes: every beam keeps extending with the decoder's own tokens
    seqs1, score1, _ = orc.beam_search(x, z, z, start, T, k=4, end_id=-1)
    assert np.allclose(orc.path_score(x, z, z, start, seqs1, -1), score1)
    assert not np.array_equal(seqs1, seqs)


# ---------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("norm", ["batch", "layer"])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_dense_beam_search_matches_restatement(mock_backend, k, norm):
    model, orc, x, z, start = dense_case(74 + k, norm=norm)
    T = 6
    eid = emitted_id(orc, x, z, start, T)
    for end_id in (-1, eid):
        want, wscore, margin = orc.beam_search(x, z, z, start, T, k=k, end_id=end_id)
        got, gscore = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id)
        assert got.shape == (6, k, T) and got.dtype == np.int64
        assert gscore.shape == (6, k) and gscore.dtype == np.float32
        ok = margin > MARGIN
        assert ok.sum() >= 3, margin
        assert np.array_equal(got[ok], want[ok]), (k, norm, end_id)
        assert np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)
    assert mock_backend.beam_step_calls == 2 * T


def test_dense_width1_is_greedy_predict():
    model, orc, x, z, start = dense_case(80)
    T = 6
    probs = model.greedy_predict(x, z, z, start, T)
    seqs, score = model.beam_search(x, z, z, start, T, beam_width=1)
    assert np.array_equal(seqs[:, 0], probs[:, :, 0].argmax(-1).T)
    p = np.take_along_axis(probs[:, :, 0], seqs[:, 0].T[:, :, None], axis=2)[:, :, 0]
    assert np.allclose(score[:, 0], np.log(p.astype(np.float64)).sum(0), rtol=1e-4)


def test_dense_beam_search_encodes_once(mock_backend, monkeypatch):
    """the encoder GEMM runs on the B rows, not B*k: the k beams are gathered from the feature step's state"""
    model, orc, x, z, start = dense_case(81)
    rows = []
    real = model.gemm_sk
    monkeypatch.setattr(model, "gemm_sk", lambda A, Bm, C, Mr, Nc, K, *a, **kw: (rows.append((Mr, Nc, K)),
                                                                               real(A, Bm, C, Mr, Nc, K, *a, **kw))[1])
    model.beam_search(x, z, z, start, 4, beam_width=5)
    assert (6, 10, 23) in rows and (30, 10, 23) not in rows


@pytest.mark.parametrize("kw", [dict(beam_width=0), dict(beam_width=17), dict(beam_width=2.0), dict(beam_width=True),
                                dict(beam_width="3"), dict(max_len=0), dict(max_len=2.5), dict(end_id=13),
                                dict(end_id=-2), dict(end_id=1.0), dict(length_penalty=-0.1),
                                dict(length_penalty=float("nan")), dict(length_penalty=float("inf")),
                                dict(length_penalty="0.6"), dict(length_penalty=None)])
def test_bad_arguments_raise_before_any_launch(mock_backend, kw):
    model, _, x, z, start = dense_case(82)
    args = dict(max_len=4)
    args.update(kw)
    max_len = args.pop("max_len")
    with pytest.raises(ValueError):
        model.beam_search(x, z, z, start, max_len, **args)
    assert mock_backend.beam_step_calls == 0
    assert model._shape is None                     # nothing was staged either


def test_refuses_what_greedy_predict_refuses():
    model, _, x, z, start = dense_case(83)
    bad = np.zeros((6, 22), np.float32)              # wrong input width
    with pytest.raises(AssertionError):
        model.greedy_predict(bad, z, z, start, 3)
    with pytest.raises(AssertionError):
        model.beam_search(bad, z, z, start, 3, beam_width=2)


# ---------------------------------------------------------------------------------------------------- length normalisation
def test_length_penalty_zero_is_identity():
    rng = np.random.default_rng(84)
    seqs = rng.integers(0, 9, (5, 4, 7))
    score = np.sort(rng.standard_normal((5, 4)).astype(np.float32), axis=1)[:, ::-1].copy()
    s2, k2 = length_normalise(seqs, score, 3, 0.0)
    assert np.array_equal(s2, seqs)
    assert k2.dtype == np.float32 and np.array_equal(k2.view(np.int32), score.view(np.int32))


def test_longer_beams_overtake_a_short_finished_one():
    """log-probability sums are <= 0, so the divisor ((5 + L) / 6) ** length_penalty, which grows with L, can only move a
    longer result ahead of a shorter one: here the search's best result, finished after 2 tokens, falls behind"""
    end = 2
    seqs = np.array([[[5, 2, 0, 0, 0, 0],          # finished after 2 tokens: L = 2
                      [5, 6, 7, 8, 9, 4],          # runs to max_len: L = 6
                      [5, 6, 7, 2, 0, 0]]])        # L = 4
    score = np.array([[-6.0, -6.5, -7.2]], np.float32)
    for lp in (0.0, 0.3, 0.6, 1.0, 2.0):
        got_s, got_k = length_normalise(seqs, score, end, lp)
        want_s, want_k = length_normalise_ref(seqs, score, end, lp)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_k, want_k), lp
        assert np.all(np.diff(got_k, axis=1) <= 0)
    # lp = 0.3: keys -6 / 1.0473 = -5.73, -6.5 / 1.1994 = -5.42, -7.2 / 1.1294 = -6.38: the 6-token result overtakes
    s, key = length_normalise(seqs, score, end, 0.3)
    assert [int((row != 0).sum()) for row in s[0]] == [6, 2, 4]
    # lp = 1: keys -5.14, -3.55, -4.8: both longer results overtake it
    s, key = length_normalise(seqs, score, end, 1.0)
    assert [int((row != 0).sum()) for row in s[0]] == [6, 4, 2]
    assert np.allclose(key[0], [-6.5 / (11 / 6), -7.2 / (9 / 6), -6.0 / (7 / 6)], rtol=1e-6)
    # equal keys keep the search's order
    s, key = length_normalise(np.array([[[1, 1], [3, 3]]]), np.array([[-1.0, -1.0]], np.float32), -1, 0.8)
    assert np.array_equal(s[0], [[1, 1], [3, 3]])


@pytest.mark.parametrize("lp", [0.6, 1.2])
def test_dense_length_penalty_matches_restatement(lp):
    model, orc, x, z, start = dense_case(85)
    T = 6
    eid = emitted_id(orc, x, z, start, T)
    want, wscore, margin = orc.beam_search(x, z, z, start, T, k=3, end_id=eid)
    want, wkey = length_normalise_ref(want, wscore, eid, lp)
    got0, gscore0 = model.beam_search(x, z, z, start, T, beam_width=3, end_id=eid)
    got, gkey = model.beam_search(x, z, z, start, T, beam_width=3, end_id=eid, length_penalty=lp)
    s2, k2 = length_normalise(got0, gscore0, eid, lp)
    assert np.array_equal(got, s2) and np.array_equal(gkey, k2)
    ok = margin > MARGIN
    assert ok.sum() >= 3
    assert np.array_equal(got[ok], want[ok])
    assert np.allclose(gkey[ok], wkey[ok], rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------- the host helpers
@pytest.mark.parametrize("max_len", [1, 4])
@pytest.mark.parametrize("k", [1, 5])
def test_beam_backtrack_is_the_walk_of_every_beam(k, max_len):
    """against the beam-by-beam walk of the parent links, on parents drawn within the row's own sample"""
    import torch
    M = 3
    rng = np.random.default_rng(90 + 10 * k + max_len)
    parents = (np.arange(M * k) // k * k + rng.integers(0, k, (max_len, M * k))).astype(np.int32)
    tokens = rng.integers(0, 50, (max_len, M * k)).astype(np.int32)
    want = np.zeros((M, k, max_len), np.int64)
    for b in range(M):
        for r in range(k):
            row = b * k + r
            for i in range(max_len - 1, -1, -1):
                want[b, r, i] = tokens[i, row]
                row = parents[i, row]
    got = beam_backtrack(parents, tokens, M, k)
    assert got.dtype == np.int64 and got.shape == (M, k, max_len) and np.array_equal(got, want)
    # the models pass what .cpu().numpy() gives them (rows of one buffer, or two buffers)
    pt = torch.tensor(np.stack([parents, tokens])).numpy()
    assert np.array_equal(beam_backtrack(pt[0], pt[1], M, k), want)


@pytest.mark.parametrize("M,k,groups", [(2, 1, 1), (2, 6, 1), (2, 6, 3), (1, 16, 4)])
def test_beam_init_scores_are_the_models_expressions(M, k, groups):
    import torch
    plain = torch.zeros(M, k)
    plain[:, 1:] = -1e30                      # only beam 0 of the sample counts
    grouped = torch.zeros(M, groups, k // groups)
    grouped[:, :, 1:] = -1e30                 # only the first beam of every group counts
    got = beam_init_scores(M, k, groups)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (M * k,)
    assert np.array_equal(got, grouped.view(M * k).numpy())
    if groups == 1:
        assert np.array_equal(got, plain.view(M * k).numpy())
        assert np.array_equal(beam_init_scores(M, k), got)


ARGS = dict(B=4, N=41, R=5, D=16, A=6, U=16, Et=12, V=13, T=5)


def make_lc(rng, seed=11):
    d = ARGS
    g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
    model = LcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5, device="cpu",
                  seed=seed)
    orc = M.LcNIC(g, d["U"], 512, d["Et"], d["A"], d["V"], d["T"], *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


def test_lcnic_length_penalty():
    rng = np.random.default_rng(86)
    model, orc = make_lc(rng)
    B, T = ARGS["B"], ARGS["T"]
    x = rng.standard_normal((B, ARGS["N"])).astype(np.float32)
    z = np.zeros((B, ARGS["U"]), np.float32)
    start = np.ones(B, np.int64)
    gw = model.greedy_predict(x, z, z, start, T, ARGS["U"], None)[0]
    eid = int(gw[0, 1, 0])
    s, sc = model.beam_search(x, z, z, start, T, beam_width=3, end_id=eid)
    s0, sc0 = model.beam_search(x, z, z, start, T, beam_width=3, end_id=eid, length_penalty=0.0)
    assert np.array_equal(s, s0) and np.array_equal(sc.view(np.int32), sc0.view(np.int32))
    want, wscore, margin = orc.beam_search(x, z, z, start, T, k=3, end_id=eid)
    ok = margin > 1e-5
    assert np.array_equal(s[ok], want[ok])
    s6, k6 = model.beam_search(x, z, z, start, T, beam_width=3, end_id=eid, length_penalty=0.6)
    r6, rk6 = length_normalise_ref(s, sc, eid, 0.6)
    assert np.array_equal(s6, r6) and np.array_equal(k6, rk6)
    with pytest.raises(ValueError):
        model.beam_search(x, z, z, start, T, beam_width=3, length_penalty=-1.0)


# ---------------------------------------------------------------------------------------------------- beam_captions
def tokenizer(V):
    words = ["<start>", "<end>"] + [f"w{i}" for i in range(3, V)]
    wi = {w: i + 1 for i, w in enumerate(words)}
    return SimpleNamespace(word_index=wi, index_word={i: w for w, i in wi.items()})


def test_beam_captions_both_models():
    from masters_thesis_amd.evaluate import beam_captions, ids_to_captions
    tok = tokenizer(13)
    end_id = tok.word_index["<end>"]
    model, orc, x, z, _ = dense_case(87)
    T = 6
    start = np.full(6, tok.word_index["<start>"], np.int64)
    ids, caps = beam_captions(model, x, z, z, tok, T, beam_width=3, length_penalty=0.6)
    seqs, _ = model.beam_search(x, z, z, start, T, beam_width=3, end_id=end_id, length_penalty=0.6)
    assert ids.dtype == np.int64 and ids.shape == (6, T)
    assert np.array_equal(ids, seqs[:, 0]) and caps == ids_to_captions(ids, tok)
    want, wscore, margin = orc.beam_search(x, z, z, start, T, k=3, end_id=end_id)
    want, _ = length_normalise_ref(want, wscore, end_id, 0.6)
    ok = margin > MARGIN
    assert ok.sum() >= 3 and np.array_equal(ids[ok], want[ok, 0])
    assert all("<end>" not in c for c in caps)

    rng = np.random.default_rng(88)
    lc, _ = make_lc(rng)
    B = ARGS["B"]
    xl = rng.standard_normal((B, ARGS["N"])).astype(np.float32)
    zl = np.zeros((B, ARGS["U"]), np.float32)
    ids, caps = beam_captions(lc, xl, zl, zl, tok, ARGS["T"], beam_width=2)
    seqs, _ = lc.beam_search(xl, zl, zl, np.full(B, 1, np.int64), ARGS["T"], beam_width=2, end_id=end_id)
    assert np.array_equal(ids, seqs[:, 0]) and caps == ids_to_captions(ids, tok)
