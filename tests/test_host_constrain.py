"""Constrained caption decoding on the CPU: the restatement (tests/constrain_oracle.py) on hand-computed cases, and the
host orchestration of the six decode paths (greedy_predict, sample_predict, beam_search of nic.NIC and lc_nic.NIC) with
``constraints=`` through a mock backend that follows tnt_decode_constrain_f32's header definition."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import DecodeConstraints
from masters_thesis_amd.nic import NIC as DenseNIC
from masters_thesis_amd.optimizers import Adam
from helpers import synth_batch, tiny_groups
from constrain_oracle import (ConstrainMockBackend, ConstrainedLcNIC, ConstrainedNICDense, as_dict, constrain_logits,
                              constrain_logits_f32, constrained_beam, constrained_decode, violations)

MARGIN = 1e-4           # decision margin below which a sample's ids are not compared (tests/test_host_beam.py)
T = 8                   # decoded tokens
V = 29


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = ConstrainMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_hand_computed_cases():
    x = np.arange(8, dtype=np.float64) - 2.5                   # -2.5 .. 4.5
    inf = -np.inf
    # history [3, 5, 3], n = 2: the bigram (3, 5) exists and the last token is 3, so 5 is banned
    y = constrain_logits(x, [3, 5, 3], 1.0, 2, 0, -1, (), 3)
    assert np.flatnonzero(y == inf).tolist() == [5] and np.array_equal(np.delete(y, 5), np.delete(x, 5))
    # n = 1: every history token
    y = constrain_logits(x, [3, 5, 3], 1.0, 1, 0, -1, (), 3)
    assert np.flatnonzero(y == inf).tolist() == [3, 5]
    # i < n: no complete n-gram yet
    assert np.array_equal(constrain_logits(x, [3, 5], 1.0, 3, 0, -1, (), 2), x)
    assert np.array_equal(constrain_logits(x, [], 1.0, 1, 0, -1, (), 0), x)
    # n = 3 with a repeated context (3, 5): 3 5 7 3 5 -> 7
    y = constrain_logits(x, [3, 5, 7, 3, 5], 1.0, 3, 0, -1, (), 5)
    assert np.flatnonzero(y == inf).tolist() == [7]
    # theta = 2 on {+1, -1}: {0.5, -2}, once although token 0 occurs twice
    y = constrain_logits(np.array([1.0, -1.0, 3.0]), [0, 1, 0], 2.0, 0, 0, -1, (), 3)
    assert y.tolist() == [0.5, -2.0, 3.0]
    # a ban beats the penalty
    y = constrain_logits(np.array([1.0, -1.0, 3.0]), [0, 1, 0], 2.0, 0, 0, -1, (0,), 3)
    assert y.tolist() == [inf, -2.0, 3.0]
    # min_length bans exactly end_id, and only while i < m
    for i in range(5):
        y = constrain_logits(x, [1] * i, 1.0, 0, 3, 6, (), i)
        assert np.flatnonzero(y == inf).tolist() == ([6] if i < 3 else [])
    # an id outside [0, V) is ignored
    assert np.array_equal(constrain_logits(x, [8, -1, 99], 2.0, 1, 0, -1, (12,), 3), x)
    # the float32 twin: the same decisions, float32 arithmetic
    x32 = (np.arange(8) - 2.5).astype(np.float32) * np.float32(1.1)
    y = constrain_logits_f32(x32, [0, 7, 7, 2], 1.2, 2, 0, -1, (4,), 4)
    assert y.dtype == np.float32 and y[4] == inf
    assert y[0] == x32[0] * np.float32(1.2) and y[7] == x32[7] / np.float32(1.2) and y[2] == x32[2] * np.float32(1.2)


def test_mock_fin_rows_and_pad_columns_are_untouched(mock_backend):
    rng = np.random.default_rng(5)
    rows, Vv, ld, i, ldh = 6, 11, 16, 3, 5
    x = torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32))
    x0 = x.numpy().copy()
    hin = torch.from_numpy(rng.integers(0, Vv, (rows, ldh)).astype(np.int32))
    hout = torch.full((rows, ldh), -7, dtype=torch.int32)
    last = torch.from_numpy(rng.integers(0, Vv, rows).astype(np.int32))
    fin = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.int32)
    bad = torch.tensor([2, 9], dtype=torch.int32)
    mock_backend.decode_constrain(x, ld, Vv, rows, i, hin, hout, ldh, last, None, fin, 1.5, 1, 9, 4, bad, 2)
    got = x.numpy()
    assert np.array_equal(got[:, Vv:].view(np.int32), x0[:, Vv:].view(np.int32))
    assert np.array_equal(got[[1, 4]].view(np.int32), x0[[1, 4]].view(np.int32))
    want_h = np.concatenate([hin.numpy()[:, :2], last.numpy()[:, None]], axis=1)
    assert np.array_equal(hout.numpy()[:, :3], want_h) and np.all(hout.numpy()[:, 3:] == -7)
    for r in (0, 2, 3, 5):
        assert np.array_equal(got[r, :Vv], constrain_logits_f32(x0[r, :Vv], want_h[r], 1.5, 1, 9, 4, (2, 9), 3))
        assert np.all(got[r, [2, 4, 9]] == -np.inf)


# ---------------------------------------------------------------------------------------------------- the models
LC = dict(B=5, N=41, R=5, D=16, A=6, U=16, Et=12)


def sharpen(orc, scale=8.0):
    """a larger head kernel: the freshly initialised models' distributions are close to uniform, which leaves beam search's
    decisions (gaps of 1e-5 between candidates) below the comparison margin"""
    orc.p['time_distributed_softmax/kernel'] = orc.p['time_distributed_softmax/kernel'] * scale


def make_dense(seed, norm="batch"):
    rng = np.random.default_rng(seed)
    N, U, E, B = 23, 16, 10, 6
    model = DenseNIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, norm=norm, device="cpu", seed=11)
    orc = ConstrainedNICDense(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, norm=norm).init_params(rng)
    sharpen(orc)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    data, _ = synth_batch(B, N, T, V, U, rng)
    z = np.zeros((B, U), np.float32)
    return model, orc, data[0], z, np.ones(B, np.int64)


def make_lc(seed):
    rng = np.random.default_rng(seed)
    d = LC
    g = (tiny_groups(d["N"], d["R"], rng), [d["D"]] * d["R"])
    model = LcNIC(g, d["U"], 512, d["Et"], d["A"], V, T, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11)
    orc = ConstrainedLcNIC(g, d["U"], 512, d["Et"], d["A"], V, T, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5).init_params(rng)
    sharpen(orc)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    x = rng.standard_normal((d["B"], d["N"])).astype(np.float32)
    z = np.zeros((d["B"], d["U"]), np.float32)
    return model, orc, x, z, np.ones(d["B"], np.int64)


MAKERS = {"dense": make_dense, "lc": make_lc}


def greedy_ids(kind, model, x, z, start, **kw):
    """(ids (B, T), probs (T, B, V)) of the model's greedy_predict"""
    if kind == "dense":
        p = model.greedy_predict(x, z, z, start, T, **kw)[:, :, 0, :]
        return p.argmax(-1).T, p
    w, p = model.greedy_predict(x, z, z, start, T, **kw)[:2]
    return w[:, :, 0], p.transpose(1, 0, 2)


def sample_ids(kind, model, x, z, start, **kw):
    if kind == "dense":
        ids, p = model.sample_predict(x, z, z, start, T, **kw)
        return ids[:, :, 0], p[:, :, 0, :]
    out = model.sample_predict(x, z, z, start, T, **kw)
    return out[0][:, :, 0], out[1].transpose(1, 0, 2)


def pick_constraints(ids):
    """constraints that the unconstrained sequences ``ids`` (rows, T) violate: end_id = the most frequent token of the
    first two positions, min_length 3, bad ids = the two most frequent other tokens, no repeated bigram, penalty 1.3"""
    first = np.bincount(ids[:, :2].reshape(-1), minlength=V)
    first[0] = 0
    end_id = int(first.argmax())
    cnt = np.bincount(ids.reshape(-1), minlength=V)
    cnt[[0, end_id]] = 0
    bad = tuple(int(v) for v in np.argsort(-cnt, kind="stable")[:2])
    return DecodeConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=3, bad_ids=bad, end_id=end_id)


def assert_violates_each_rule(seqs, c, end_id):
    seen = set()
    for row in seqs:
        seen |= violations(row, c.no_repeat_ngram_size, c.min_length, end_id, c.bad_ids)
    assert seen == {"ngram", "min_length", "bad"}, f"the unconstrained decode only violates {seen}: the properties show nothing"


def assert_obeys(seqs, c, end_id):
    for row in seqs:
        assert not violations(row, c.no_repeat_ngram_size, c.min_length, end_id, c.bad_ids), (row, c)


@pytest.mark.parametrize("kind,seed", [("dense", 101), ("lc", 102)])
def test_greedy_matches_restatement_and_obeys_the_rules(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    free, _, _ = constrained_decode(orc, x, z, z, start, T)
    c = pick_constraints(free)
    assert_violates_each_rule(free, c, c.end_id)
    want, wp, margin = constrained_decode(orc, x, z, z, start, T, as_dict(c))
    got, gp = greedy_ids(kind, model, x, z, start, constraints=c)
    assert [d["i"] for d in mock_backend.constrain_calls] == list(range(T))
    ok = margin > MARGIN
    assert ok.sum() >= (len(ok) + 1) // 2
    assert np.array_equal(got[ok], want[ok])
    assert np.allclose(gp[:, ok], wp[:, ok], rtol=1e-4, atol=1e-6)
    assert_obeys(got, c, c.end_id)
    assert_obeys(want, c, c.end_id)
    assert np.all(gp[:, :, list(c.bad_ids)] == 0.0)             # a banned token's probability is exactly 0


@pytest.mark.parametrize("kind,seed", [("dense", 103), ("lc", 104)])
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (6, 0.9)])
def test_sampled_matches_restatement_and_obeys_the_rules(mock_backend, kind, seed, top_k, top_p):
    model, orc, x, z, start = MAKERS[kind](seed)
    draws = 26                                                  # x T = 208 draws per row
    free = np.concatenate([constrained_decode(orc, x, z, z, start, T, None, (1.0, top_k, top_p, model.seed, s))[0]
                           for s in range(4)])
    c = pick_constraints(free)
    assert_violates_each_rule(free, c, c.end_id)
    for s in range(draws):
        got, gp = sample_ids(kind, model, x, z, start, temperature=1.0, top_k=top_k, top_p=top_p, sample_step=s, constraints=c)
        assert_obeys(got, c, c.end_id)
        if s < 3:
            want, wp, margin = constrained_decode(orc, x, z, z, start, T, as_dict(c), (1.0, top_k, top_p, model.seed, s))
            ok = margin > 1e-5                                  # the sampler's relative margin (tests/test_host_sampling.py)
            assert ok.sum() >= (len(ok) + 1) // 2
            assert np.array_equal(got[ok], want[ok])
            assert np.allclose(gp[:, ok], wp[:, ok], rtol=1e-4, atol=1e-6)
    assert len(mock_backend.constrain_calls) == draws * T


@pytest.mark.parametrize("kind,seed", [("dense", 105), ("lc", 106)])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_beam_matches_restatement_and_obeys_the_rules(mock_backend, kind, seed, k):
    model, orc, x, z, start = MAKERS[kind](seed)
    free0, _, _ = constrained_beam(orc, x, z, z, start, T, k=k)
    c0 = pick_constraints(free0.reshape(-1, T))
    end_id = c0.end_id
    free, _, _ = constrained_beam(orc, x, z, z, start, T, k=k, end_id=end_id)
    c = DecodeConstraints(1.3, 2, 3, c0.bad_ids)                # end_id: the beam's
    assert_violates_each_rule(np.concatenate([free.reshape(-1, T), free0.reshape(-1, T)]), c, end_id)
    want, wscore, margin = constrained_beam(orc, x, z, z, start, T, k=k, end_id=end_id, con=as_dict(c, end_id))
    got, gscore = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, constraints=c)
    assert [d["i"] for d in mock_backend.constrain_calls] == list(range(T))
    assert all(d["rows"] == x.shape[0] * k for d in mock_backend.constrain_calls)
    ok = margin > MARGIN
    assert ok.sum() >= (len(ok) + 1) // 2, margin
    assert np.array_equal(got[ok], want[ok])
    assert np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)
    assert_obeys(got.reshape(-1, T), c, end_id)
    # the object may name the same end id; a different one is refused
    got2, _ = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id,
                                constraints=DecodeConstraints(1.3, 2, 3, c0.bad_ids, end_id=end_id))
    assert np.array_equal(got2, got)
    with pytest.raises(ValueError):
        model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id,
                          constraints=DecodeConstraints(1.3, 2, 3, c0.bad_ids, end_id=end_id + 1))


@pytest.mark.parametrize("kind,seed", [("dense", 107), ("lc", 108)])
def test_beam_history_follows_permuting_parents(mock_backend, kind, seed):
    """the device-side history buffer against the host back-track of the parents / tokens, at every step"""
    model, orc, x, z, start = MAKERS[kind](seed)
    k = 4
    trace = []
    c = DecodeConstraints(no_repeat_ngram_size=2)
    want, _, margin = constrained_beam(orc, x, z, z, start, T, k=k, con=as_dict(c), trace=trace)
    got, _ = model.beam_search(x, z, z, start, T, beam_width=k, constraints=c)
    calls = mock_backend.constrain_calls
    ident = np.arange(x.shape[0] * k)
    assert any(d["parent"] is not None and not np.array_equal(d["parent"], ident) for d in calls), "no step permutes"
    ok = np.repeat(margin > MARGIN, k)
    assert ok.sum() >= len(ok) // 2
    for i, d in enumerate(calls):
        assert d["hist"].shape == (x.shape[0] * k, i)
        assert np.array_equal(d["hist"][ok], trace[i][ok]), i
    assert np.array_equal(got[margin > MARGIN], want[margin > MARGIN])


@pytest.mark.parametrize("kind,seed", [("dense", 109), ("lc", 110)])
def test_none_and_neutral_change_nothing(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    neutral = DecodeConstraints()
    assert neutral.neutral and not DecodeConstraints(min_length=1, end_id=3).neutral
    bits = lambda t: [np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype) for a in t if a is not None]
    same = lambda p, q: all(np.array_equal(a, b) for a, b in zip(bits(p), bits(q)))
    for c in (None, neutral):
        a = greedy_ids(kind, model, x, z, start)
        b = greedy_ids(kind, model, x, z, start, constraints=c)
        assert same(a, b)
        a = sample_ids(kind, model, x, z, start, top_k=5, sample_step=2)
        b = sample_ids(kind, model, x, z, start, top_k=5, sample_step=2, constraints=c)
        assert same(a, b)
        a = model.beam_search(x, z, z, start, T, beam_width=3, end_id=4)
        b = model.beam_search(x, z, z, start, T, beam_width=3, end_id=4, constraints=c)
        assert same(a, b)
    assert mock_backend.constrain_calls == []
    assert "_con_bufs" not in model.__dict__


@pytest.mark.parametrize("kind,seed", [("dense", 111), ("lc", 112)])
def test_train_step_after_a_constrained_decode(kind, seed):
    rng = np.random.default_rng(7)
    outs = []
    for constrained in (False, True):
        model, orc, x, z, start = MAKERS[kind](seed)
        model.compile(Adam(1e-3, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        B = x.shape[0]
        data, tgt = synth_batch(B, x.shape[1], T, V, z.shape[1], np.random.default_rng(8))
        if constrained:
            c = DecodeConstraints(1.2, 2, 2, (3, 4), end_id=5)
            greedy_ids(kind, model, x, z, start, constraints=c)
            sample_ids(kind, model, x, z, start, top_k=4, constraints=c)
            model.beam_search(x, z, z, start, T, beam_width=2, constraints=c)
        met = model.train_step((data, tgt)).as_floats()
        outs.append((met, {k: model.get_weight(k) for k in orc.p}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k].view(np.int32), outs[1][1][k].view(np.int32)), k


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.9), dict(repetition_penalty=float("nan")),
                                dict(repetition_penalty=float("inf")), dict(repetition_penalty="1.2"),
                                dict(repetition_penalty=True), dict(repetition_penalty=1e39),
                                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5),
                                dict(min_length=-1), dict(min_length=2.0), dict(bad_ids=(-1,)), dict(bad_ids=(1.0,)), dict(bad_ids=3),
                                dict(bad_ids=tuple(range(65))), dict(end_id=-2), dict(end_id=1.0)])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        DecodeConstraints(**kw)


def test_repr_and_neutral():
    c = DecodeConstraints(1.2, 2, 3, [4, 5], end_id=2)
    assert repr(c) == ("DecodeConstraints(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3, bad_ids=(4, 5), "
                       "end_id=2)")
    assert not c.neutral
    for kw in (dict(repetition_penalty=1.5), dict(no_repeat_ngram_size=1), dict(min_length=1), dict(bad_ids=(0,))):
        assert not DecodeConstraints(**kw).neutral
    assert DecodeConstraints(end_id=7).neutral


@pytest.mark.parametrize("kind,seed", [("dense", 113), ("lc", 114)])
def test_decode_refuses_before_any_launch(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    calls = [lambda c, n=T: model.greedy_predict(x, z, z, start, n, constraints=c),
             lambda c, n=T: model.sample_predict(x, z, z, start, n, top_k=3, constraints=c),
             lambda c, n=T: model.sample_predict(x, z, z, start, n, constraints=c),
             lambda c, n=T: model.beam_search(x, z, z, start, n, beam_width=3, constraints=c)]
    for call in calls:
        with pytest.raises(ValueError):                            # max_len > 64
            call(DecodeConstraints(no_repeat_ngram_size=2), 65)
        with pytest.raises(ValueError):                            # a bad id outside [0, V)
            call(DecodeConstraints(bad_ids=(V,)))
        with pytest.raises(ValueError):                            # min_length without an end id
            call(DecodeConstraints(min_length=2))
        with pytest.raises(ValueError):                            # ... or with end id 0
            call(DecodeConstraints(min_length=2, end_id=0))
        with pytest.raises(ValueError):                            # min_length > max_len
            call(DecodeConstraints(min_length=T + 1, end_id=3))
        with pytest.raises(ValueError):                            # not a DecodeConstraints
            call(dict(min_length=1))
        with pytest.raises(ValueError):                            # too few tokens left: 20 + 8 + 1 + 1 > 29
            call(DecodeConstraints(bad_ids=tuple(range(1, 21))))
    # the beam width counts: 18 + 8 + 1 + 1 = 28 fits greedy, 18 + 8 + 1 + 3 = 30 does not fit a beam of 3
    c = DecodeConstraints(bad_ids=tuple(range(1, 19)))
    with pytest.raises(ValueError):
        calls[3](c)
    assert mock_backend.constrain_calls == []
    assert model._shape is None                                   # nothing was staged either
    calls[0](c)
    assert len(mock_backend.constrain_calls) == T


def test_ms_nic_inherits_the_keyword():
    import inspect
    from masters_thesis_amd import ms_nic
    for name in ("greedy_predict", "sample_predict", "beam_search"):
        assert "constraints" in inspect.signature(getattr(ms_nic.NIC, name)).parameters


# ---------------------------------------------------------------------------------------------------- evaluate
def tokenizer():
    words = ["<start>", "<end>"] + [f"w{i}" for i in range(3, V)]
    wi = {w: i + 1 for i, w in enumerate(words)}
    return SimpleNamespace(word_index=wi, index_word={i: w for w, i in wi.items()})


def test_beam_captions_passes_the_constraints(mock_backend):
    from masters_thesis_amd.evaluate import beam_captions
    model, orc, x, z, _ = make_dense(115)
    tok = tokenizer()
    end_id = tok.word_index["<end>"]
    start = np.full(x.shape[0], tok.word_index["<start>"], np.int64)
    c = DecodeConstraints(1.2, 2, 4, (tok.word_index["<start>"],))
    ids, caps = beam_captions(model, x, z, z, tok, T, beam_width=3, constraints=c)
    seqs, _ = model.beam_search(x, z, z, start, T, beam_width=3, end_id=end_id, constraints=c)
    assert np.array_equal(ids, seqs[:, 0]) and len(mock_backend.constrain_calls) == 2 * T
    assert_obeys(ids, c, end_id)
    assert all(len(cap) >= 4 for cap in caps)                      # <end> never before position 4
    ids0, _ = beam_captions(model, x, z, z, tok, T, beam_width=3)
    assert len(mock_backend.constrain_calls) == 2 * T


def test_simple_eval_constrained(mock_backend):
    from masters_thesis_amd import think_and_tell as TT
    from masters_thesis_amd.evaluate import simple_eval
    from oracle.models_tt import CaptionGeneratorTT
    rng = np.random.default_rng(116)
    B, N, E, U, Tt = 4, 19, 10, 16, 7
    orc = CaptionGeneratorTT(N, E, U, V, Tt, l2_reg=0.01, dropout=0.0, show_and_tell=False).init_params(rng)
    model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                None, Tt, device="cpu", seed=11)
    x = rng.standard_normal((B, N)).astype(np.float32)
    tgt = rng.integers(1, V, (B, Tt)).astype(np.int32)
    model._stage(x, tgt)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    c = DecodeConstraints(1.2, 1, 3, (5, 6), end_id=2)
    for s in range(30):
        ids, _ = simple_eval(model, x, tgt, None, sample_step=s, constraints=c)
        assert ids.shape == (B, Tt + 1)
        assert_obeys(ids, c, 2)                                     # n = 1: no token twice
    assert len(mock_backend.constrain_calls) == 30 * (Tt + 1)
    a, _ = simple_eval(model, x, tgt, None, sample_step=3)
    b, _ = simple_eval(model, x, tgt, None, sample_step=3, constraints=DecodeConstraints())
    assert np.array_equal(a, b) and len(mock_backend.constrain_calls) == 30 * (Tt + 1)


def test_simple_eval_constrained_refuses_more_than_32_positions(mock_backend):
    """one Philox site per position, S_SAMPLE + t: position 32 would draw on lc_nic's S_NOUT"""
    from masters_thesis_amd import think_and_tell as TT
    from masters_thesis_amd.evaluate import simple_eval
    from oracle.models_tt import CaptionGeneratorTT
    rng = np.random.default_rng(117)
    B, N, E, U, Vv = 2, 9, 6, 16, 80
    for Tt, refused in ((31, False), (32, True)):
        orc = CaptionGeneratorTT(N, E, U, Vv, Tt, l2_reg=0.01, dropout=0.0, show_and_tell=False).init_params(rng)
        model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, Vv, 0.01, "glorot_uniform", 0.0),
                                    None, Tt, device="cpu", seed=11)
        x = rng.standard_normal((B, N)).astype(np.float32)
        tgt = rng.integers(1, Vv, (B, Tt)).astype(np.int32)
        model._stage(x, tgt)
        for k, v in orc.p.items():
            model.set_weight(k, v)
        n0 = len(mock_backend.constrain_calls)
        if refused:
            with pytest.raises(ValueError):
                simple_eval(model, x, tgt, None, constraints=DecodeConstraints(bad_ids=(5,)))
            assert len(mock_backend.constrain_calls) == n0
            assert simple_eval(model, x, tgt, None)[0].shape == (B, Tt + 1)        # unconstrained: one launch, any length
        else:
            assert simple_eval(model, x, tgt, None, constraints=DecodeConstraints(bad_ids=(5,)))[0].shape == (B, Tt + 1)


# ---------------------------------------------------------------------------------------------------- the GPU tests' cases
@pytest.mark.parametrize("shape", ["tiny", "mid"])
@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_gpu_cases_survive_float32(kind, shape):
    """the cases tests/test_gpu_constrain.py compares a device model on (weight scale, seed): the restatement run in
    float32 decides like itself in float64 wherever the float64 margin exceeds the cap, on at least half of the samples"""
    from constrain_oracle import case_constraints, restatement_case, run_path
    orc, x, z, start, Tc, _ = restatement_case(kind, shape, 7)
    ckw, k, end_id = case_constraints(shape)
    p64 = orc.p
    for path in ("greedy", "sample", "beam"):
        con = as_dict(DecodeConstraints(end_id=-1 if path == "beam" else end_id, **ckw), end_id)
        orc.p = p64
        a = run_path(orc, path, x, z, start, Tc, con, k, end_id, 11)
        orc.p = {name: v.astype(np.float32) for name, v in p64.items()}
        b = run_path(orc, path, x, z, start, Tc, con, k, end_id, 11)
        ok = a[2] > (1e-5 if path == "sample" else MARGIN)
        assert ok.mean() >= 0.5, (path, a[2])
        assert np.array_equal(a[0][ok], b[0][ok]), path
