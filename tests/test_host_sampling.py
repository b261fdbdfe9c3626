"""Top-k / nucleus sampling (tnt_sample_topkp_f32) on CPU: properties of the float64 restatement (tests/topkp_oracle.py),
and lc_nic.NIC.sample_predict, nic.NIC.sample_predict and evaluate.simple_eval with the filters through the mock backend
against the float64 models."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import think_and_tell as TT
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.nic import NIC as DenseNIC
from oracle import models as M
from oracle import ops as O
from oracle.models_tt import CaptionGeneratorTT
from oracle.philox import uniform24
from helpers import synth_batch, tiny_groups
from topkp_oracle import SampledNICDense, TopkpMockBackend, filter_weights, sample_topkp


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = TopkpMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("from_logits", [True, False])
def test_unfiltered_is_sample_rows(from_logits):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((200, 37)) * 2
    if not from_logits:
        x = np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    got, gm = sample_topkp(x, 0.8, 0, 1.0, from_logits, 7, 112, 3)
    want, wm = O.sample_rows(x, 0.8, from_logits, 7, 112, 3)
    assert np.array_equal(got, want)
    assert np.allclose(gm, wm)


def test_top1_is_the_argmax_lowest_tied_index():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((100, 29))
    for r in range(0, 100, 3):                       # plant ties of the max
        j = rng.choice(29, 3, replace=False)
        x[r, j] = x[r].max() + 1.0
    for p in (1.0, 0.5, 0.01):
        ids, _ = sample_topkp(x, 1.3, 1, p, True, 3, 5, 0)
        want = np.array([np.flatnonzero(row == row.max())[0] for row in x])
        assert np.array_equal(ids, want)


def test_kept_set_is_the_minimal_rank_prefix():
    rng = np.random.default_rng(3)
    for _ in range(200):
        V = int(rng.integers(1, 40))
        w = np.exp(rng.standard_normal(V) * 2)
        w /= w.max()
        k, p = int(rng.integers(0, V + 3)), float(rng.choice([0.05, 0.3, 0.6, 0.9, 1.0]))
        keep, _ = filter_weights(w, k, p)
        order = np.lexsort((np.arange(V), -w))
        K = min(k, V) if k >= 1 else V
        n = int(keep.sum())
        assert n >= 1 and keep[order[0]]
        assert keep[order[:n]].all() and not keep[order[n:]].any()       # a prefix of rank order
        assert n <= K
        S = w[order[:K]].sum()
        if p < 1:
            assert w[order[:n]].sum() >= p * S * (1 - 1e-12) or n == K  # reaches top_p * S_K ...
            assert n == 1 or w[order[:n - 1]].sum() < p * S              # ... and no shorter prefix does
        else:
            assert n == K


def test_zero_weight_never_drawn():
    rng = np.random.default_rng(4)
    p = rng.random((3000, 11))
    p[:, [0, 4, 10]] = 0.0
    p /= p.sum(-1, keepdims=True)
    for k, tp in ((0, 1.0), (9, 1.0), (0, 0.99), (11, 0.999999)):
        ids, _ = sample_topkp(p, 1.0, k, tp, False, 9, 1, 2)
        assert not np.isin(ids, [0, 4, 10]).any()


def test_boundary_ties_resolve_by_index():
    # K boundary: weights (1, .5, .5, .5, .1): top_k = 2 keeps index 0 and the lowest of the tied .5s
    x = np.log(np.array([[1.0, 0.5, 0.5, 0.5, 0.1]]))
    keep, _ = filter_weights(np.exp(x[0]), 2, 1.0)
    assert np.flatnonzero(keep).tolist() == [0, 1]
    # tied weights listed in reverse: the lower indices rank first
    w = np.array([0.1, 0.5, 0.5, 0.5, 1.0])
    keep, _ = filter_weights(w, 3, 1.0)
    assert np.flatnonzero(keep).tolist() == [1, 2, 4]
    # nucleus boundary: S = 2.6, p * S = 1.56: masses before the ranks 1, .5, .5, .5 are 0, 1, 1.5, 2 -> 3 kept
    keep, _ = filter_weights(np.array([0.5, 1.0, 0.5, 0.1, 0.5]), 0, 0.6)
    assert np.flatnonzero(keep).tolist() == [0, 1, 2]
    # ... and the tied weights' ties are no near-decision: the margin stays large
    _, m = filter_weights(np.array([0.5, 1.0, 0.5, 0.1, 0.5]), 0, 0.6)
    assert m > 0.01


@pytest.mark.parametrize("k,p", [(3, 1.0), (0, 0.6), (4, 0.7)])
def test_frequencies_match_the_filtered_distribution(k, p):
    probs = np.array([0.3, 0.05, 0.25, 0.1, 0.2, 0.1])
    n = 60000
    x = np.tile(probs, (n, 1))
    ids, _ = sample_topkp(x, 1.0, k, p, False, 21, 7, 0)
    keep, _ = filter_weights(probs / probs.max(), k, p)
    want = np.where(keep, probs, 0) / probs[keep].sum()
    got = np.bincount(ids, minlength=6) / n
    assert np.abs(got - want).max() < 0.01
    assert got[~keep].sum() == 0


def test_nan_rows_stay_in_range():
    x = np.full((3, 7), np.nan)
    x[1, 2] = 0.5
    ids, _ = sample_topkp(x, 1.0, 2, 0.5, False, 1, 1, 1)
    assert ids.tolist() == [0, 2, 0]


# ---------------------------------------------------------------------------------------------------- attention model
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


@pytest.mark.parametrize("k,p,temp,step", [(3, 1.0, 1.0, 0), (0, 0.5, 0.8, 3), (5, 0.9, 1.5, 7), (1, 1.0, 1.0, 2)])
def test_lcnic_sample_predict_matches_oracle(mock_backend, k, p, temp, step):
    rng = np.random.default_rng(31)
    model, orc = make_lc(rng)
    B, N, T, V, U = ARGS["B"], ARGS["N"], ARGS["T"], ARGS["V"], ARGS["U"]
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    sampler = lambda probs, i: sample_topkp(probs, temp, k, p, False, model.seed, M.S_SAMPLE + i, step)[0]
    want = orc.greedy_predict(data[0], z, z, np.ones(B, np.int64), T, sampler=sampler)
    got = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, temperature=temp, sample_step=step, top_k=k,
                               top_p=p)
    assert mock_backend.topkp_calls == T
    assert np.array_equal(got[0], want[0])
    assert np.allclose(got[1], want[1], rtol=1e-4, atol=1e-6)
    assert got[2].shape == want[2].shape and got[3].shape == want[3].shape
    if k == 1:
        assert np.array_equal(got[0], model.greedy_predict(data[0], z, z, np.ones(B, np.int64), T)[0])


def test_lcnic_defaults_route_to_sample_rows(mock_backend):
    rng = np.random.default_rng(32)
    model, orc = make_lc(rng)
    B, N, T, V, U = ARGS["B"], ARGS["N"], ARGS["T"], ARGS["V"], ARGS["U"]
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    calls = []
    orig = mock_backend.sample_rows
    mock_backend.sample_rows = lambda *a, **kw: (calls.append(1), orig(*a, **kw))
    a = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, temperature=0.8, sample_step=3)
    b = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, temperature=0.8, sample_step=3, top_k=0, top_p=1.0)
    assert len(calls) == 2 * T and mock_backend.topkp_calls == 0
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("kw", [dict(top_k=-1), dict(top_k=2.5), dict(top_k=True), dict(top_k="3"), dict(top_p=0.0),
                                dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan")), dict(temperature=0.0),
                                dict(temperature=-1.0), dict(top_k=3, temperature=0.0)])
def test_bad_filters_raise(kw):
    rng = np.random.default_rng(33)
    model, _ = make_lc(rng)
    dense, _ = make_dense(rng)
    B, U = ARGS["B"], ARGS["U"]
    z = np.zeros((B, U), np.float32)
    x = np.zeros((B, ARGS["N"]), np.float32)
    with pytest.raises(ValueError):
        model.sample_predict(x, z, z, np.ones(B, np.int64), 3, **kw)
    with pytest.raises(ValueError):
        dense.sample_predict(np.zeros((B, 23), np.float32), z, z, np.ones(B, np.int64), 3, **kw)


# ---------------------------------------------------------------------------------------------------- dense model
def make_dense(rng, N=23, T=6, V=13, U=16, E=10, seed=11):
    model = DenseNIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=seed)
    orc = SampledNICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model, orc


@pytest.mark.parametrize("k,p,temp,step", [(0, 1.0, 1.0, 0), (4, 1.0, 0.7, 1), (0, 0.6, 1.0, 5), (6, 0.8, 1.5, 9)])
def test_dense_sample_predict_matches_oracle(k, p, temp, step):
    rng = np.random.default_rng(41)
    B, N, T, V, U = 6, 23, 6, 13, 16
    model, orc = make_dense(rng)
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    sampler = lambda probs, i: sample_topkp(probs, temp, k, p, False, model.seed, M.S_SAMPLE + i, step)[0]
    want_ids, want_p = orc.sample_predict(data[0], z, z, start, T, sampler)
    ids, probs = model.sample_predict(data[0], z, z, start, T, temperature=temp, top_k=k, top_p=p, sample_step=step)
    assert ids.shape == (B, T, 1) and probs.shape == (T, B, 1, V)
    assert np.array_equal(ids, want_ids)
    assert np.allclose(probs, want_p, rtol=1e-4, atol=1e-6)


def test_dense_sampled_zero_masks_the_next_step():
    """a sampled id 0 masks the following LSTM step: the step's output is zeros, so its probabilities are
    softmax(bias) exactly"""
    rng = np.random.default_rng(42)
    B, N, T, V, U = 8, 23, 6, 13, 16
    model, orc = make_dense(rng)
    # make token 0 the likely draw: a large output bias on it
    b = orc.p['time_distributed_softmax/bias'].copy()
    b[0] = 4.0
    orc.p['time_distributed_softmax/bias'] = b
    model.set_weight('time_distributed_softmax/bias', b)
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    sampler = lambda probs, i: sample_topkp(probs, 1.0, 0, 0.9, False, model.seed, M.S_SAMPLE + i, 0)[0]
    want_ids, want_p = orc.sample_predict(data[0], z, z, np.ones(B, np.int64), T, sampler)
    ids, probs = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, top_p=0.9)
    assert np.array_equal(ids, want_ids) and np.allclose(probs, want_p, rtol=1e-4, atol=1e-6)
    zeros = np.argwhere(ids[:, :-1, 0] == 0)
    assert len(zeros) > 0
    sb = O.softmax(b[None, :].astype(np.float64))[0]
    for bi, t in zeros:
        assert np.allclose(probs[t + 1, bi, 0], sb, rtol=1e-5)


def test_dense_greedy_unchanged_and_top1_is_greedy():
    rng = np.random.default_rng(43)
    B, N, T, V, U = 5, 23, 6, 13, 16
    model, orc = make_dense(rng)
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    want = orc.greedy_predict(data[0], z, z, np.ones(B, np.int64), T)
    got = model.greedy_predict(data[0], z, z, np.ones(B, np.int64), T, U)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-6)
    ids, probs = model.sample_predict(data[0], z, z, np.ones(B, np.int64), T, top_k=1)
    assert np.allclose(probs, want, rtol=1e-4, atol=1e-6)
    assert np.array_equal(ids[:, :, 0], want[:, :, 0, :].argmax(-1).T)


# ---------------------------------------------------------------------------------------------------- simple_eval
def test_simple_eval_filters(mock_backend):
    from masters_thesis_amd.evaluate import simple_eval
    rng = np.random.default_rng(85)
    B, N, E, U, V, T = 4, 19, 10, 16, 13, 5
    orc = CaptionGeneratorTT(N, E, U, V, T, l2_reg=0.01, dropout=0.0, show_and_tell=False).init_params(rng)
    model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                None, T, device="cpu", seed=11)
    x = rng.standard_normal((B, N)).astype(np.float32)
    tgt = rng.integers(1, V, (B, T)).astype(np.int32)
    model._stage(x, tgt)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    logits, _ = orc.forward(x, tgt, False)
    ids, _ = simple_eval(model, x, tgt, None, temperature=0.9, sample_step=2, top_k=4, top_p=0.8)
    assert mock_backend.topkp_calls == 1
    want, margin = sample_topkp(logits.reshape(B * (T + 1), V), 0.9, 4, 0.8, True, model.seed, M.S_SAMPLE, 2)
    bad = ids.reshape(-1) != want
    assert np.all(margin[bad] < 1e-5)
    simple_eval(model, x, tgt, None, temperature=0.9, sample_step=2)
    assert mock_backend.topkp_calls == 1                    # the defaults keep sample_rows
    with pytest.raises(ValueError):
        simple_eval(model, x, tgt, None, top_p=0.0)
