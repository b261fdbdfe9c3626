"""Consensus decoding on the CPU: the restatement (tests/consensus_oracle.py) on hand-computed cases, and the host
orchestration of greedy_predict, sample_predict and beam_search of nic.NIC and lc_nic.NIC (ms_nic.NIC included) with
``consensus=`` through a mock backend that follows the header definitions of tnt_consensus_mix_f32 and
tnt_consensus_spread_i32: launch sequences, capture keys, row layout, results, refusals."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.model_base import Consensus, DecodeConstraints
from mock_backend import flat, mat
from constrain_oracle import ConstrainMockBackend
import consensus_oracle as CO
from test_host_constrain import MAKERS, T, V, greedy_ids, sample_ids

GAP = 1e-4              # decision gap of the restatement below which a caption's ids are not compared
LOGGED = ("softmax_cce", "argmax_rows", "sample_topkp", "sample_rows", "beam_step", "beam_topk", "decode_constrain",
          "consensus_mix", "consensus_spread")


class ConsensusMockBackend(ConstrainMockBackend):
    """ConstrainMockBackend plus the two consensus ops from the header text; ``log`` lists (name, arguments) of the
    launches of the decode's tail (LOGGED)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []
        for name in LOGGED:
            setattr(self, name, self._logged(name, getattr(self, name)))

    def _logged(self, name, fn):
        def call(*a, **k):
            self.log.append((name, a))
            return fn(*a, **k)
        return call

    def consensus_mix(self, logits, ld, V, Rm, G, w, mode, mix, ldm, token):
        assert Rm > 0 and V > 0 and ld >= V and ldm >= V and 1 <= G <= 16 and mode in (0, 1)
        assert logits is not None and mix is not None and logits.data_ptr() != mix.data_ptr()
        wv = None if w is None else flat(w)[:G].astype(np.float64)
        p, _ = CO.mix(mat(logits, G * Rm, V, ld), G, wv, CO.MODES[mode])
        out = mat(mix, Rm, V, ldm)
        out[...] = p.astype(np.float32)
        if token is not None:
            flat(token)[:G * Rm] = np.tile(CO.first_max(out), G)

    def consensus_spread(self, token, parent, fin, Rm, G, token_out, parent_out, fin_out):
        assert Rm > 0 and 1 <= G <= 16
        res = CO.spread(*(None if a is None else flat(a) for a in (token, parent, fin)), Rm, G)
        for src, dst in zip(res, (token_out, parent_out, fin_out)):
            if src is not None:
                flat(dst)[:G * Rm] = src


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = ConsensusMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def names(be):
    return [n for n, _ in be.log]


def members_of(model, x, z, start, G, seed):
    """G different scans per image at the maker's shapes: (x (G*M, N), z, start (M,))"""
    rng = np.random.default_rng(seed)
    Mn = 3
    xs = rng.standard_normal((G * Mn, x.shape[1])).astype(np.float32)
    return xs, np.zeros((G * Mn, z.shape[1]), np.float32), start[:Mn]


# ---------------------------------------------------------------------------------------------------- the restatement
def test_hand_computed_cases():
    ln = np.log
    x = np.array([[ln(1.0), ln(3.0)], [ln(3.0), ln(1.0)]])        # two members, softmaxes (1/4, 3/4) and (3/4, 1/4)
    p, t = CO.mix(x, 2, None, "mean")
    assert np.allclose(p, [[0.5, 0.5]]) and t.tolist() == [0]      # the exact tie goes to the lower index
    p, t = CO.mix(x, 2, [0.25, 0.75], "mean")
    assert np.allclose(p, [[0.25 * 0.25 + 0.75 * 0.75, 0.25 * 0.75 + 0.75 * 0.25]]) and t.tolist() == [0]
    p, _ = CO.mix(x, 2, [0.25, 0.75], "logmean")
    g = np.array([0.25 ** 0.25 * 0.75 ** 0.75, 0.75 ** 0.25 * 0.25 ** 0.75])
    assert np.allclose(p, [g / g.sum()])
    # -inf: mean keeps what any member allows, logmean bans what any member bans
    x = np.array([[0.0, -np.inf, 0.0], [0.0, 0.0, -np.inf]])
    p, _ = CO.mix(x, 2, None, "mean")
    assert np.allclose(p, [[0.5, 0.25, 0.25]])
    p, t = CO.mix(x, 2, None, "logmean")
    assert p.tolist() == [[1.0, 0.0, 0.0]] and t.tolist() == [0]
    x = np.array([[0.0, -np.inf], [-np.inf, 0.0]])                # every l_v is -inf
    p, t = CO.mix(x, 2, None, "logmean")
    assert p.tolist() == [[0.0, 0.0]] and t.tolist() == [0]
    # member-major rows: member g of mixed row r is row g*Rm + r
    x = np.log(np.array([[0.9, 0.1], [0.2, 0.8], [0.5, 0.5], [0.4, 0.6]]))
    p, t = CO.mix(x, 2, None, "mean")
    assert np.allclose(p, [[0.7, 0.3], [0.3, 0.7]]) and t.tolist() == [0, 1]
    tok, par, fin = CO.spread(np.array([7, 8, 9]), np.array([2, 0, 1]), np.array([0, 1, 0]), 3, 2)
    assert tok.tolist() == [7, 8, 9, 7, 8, 9] and par.tolist() == [2, 0, 1, 5, 3, 4] and fin.tolist() == [0, 1, 0, 0, 1, 0]
    assert CO.spread(None, None, None, 3, 2) == (None, None, None)


def test_mock_ops_follow_the_restatement(mock_backend):
    rng = np.random.default_rng(1)
    G, Rm, Vv, ld = 3, 2, 7, 9
    x = torch.from_numpy(rng.standard_normal((G * Rm, ld)).astype(np.float32) * 3)
    mixd, tok = torch.full((Rm, ld), -7.0), torch.full((G * Rm,), -9, dtype=torch.int32)
    w = torch.tensor([0.5, 0.25, 0.25])
    mock_backend.consensus_mix(x, ld, Vv, Rm, G, w, 1, mixd, ld, tok)
    want, wt = CO.mix(x.numpy()[:, :Vv], G, w.numpy(), "logmean")
    assert np.allclose(mixd.numpy()[:, :Vv], want, rtol=1e-6) and np.all(mixd.numpy()[:, Vv:] == -7.0)
    assert tok.numpy().tolist() == np.tile(wt, G).tolist()


# ---------------------------------------------------------------------------------------------------- the decodes
@pytest.mark.parametrize("kind,seed", [("dense", 3), ("lc", 4)])
@pytest.mark.parametrize("mode", CO.MODES)
def test_greedy_launches_and_matches_the_restatement(mock_backend, kind, seed, mode):
    model, orc, x, z, start = MAKERS[kind](seed)
    G = 3
    xs, zs, st = members_of(model, x, z, start, G, seed)
    keys = []
    run_captured = model._run_captured
    model._run_captured = lambda key, fn: (keys.append(key), run_captured(key, fn))
    mock_backend.log.clear()
    cons = Consensus(G, mode, (2, 1, 1))
    ids, probs = greedy_ids(kind, model, xs, zs, st, consensus=cons)
    # per token: one mix launch with the token output, in the place of softmax + argmax
    assert names(mock_backend) == ["consensus_mix"] * T
    for _, a in mock_backend.log:
        assert a[3:5] == (3, G) and a[6] == CO.MODES.index(mode) and a[9] is not None and a[5] is not None
    assert keys[0][0] == "greedy" and keys[0][-4:] == ("consensus", G, mode, (0.5, 0.25, 0.25))
    want_ids, want_p, gap = CO.consensus_decode(orc, xs, zs, zs, st, T, G, mode, np.array([0.5, 0.25, 0.25]))
    ok = gap >= GAP
    assert ok.sum() >= 2 and ids.shape == (3, T) and probs.shape == (T, 3, V)
    assert np.array_equal(ids[ok], want_ids[ok]) and np.abs(probs[:, ok] - want_p[:, ok]).max() <= 1e-4
    # the staged start tokens: M entries tiled over the members
    cb = [v for k, v in model._cons_bufs.items() if isinstance(v, dict)][0]
    assert cb["start"].numpy().reshape(-1).tolist() == np.tile(st, G).tolist()
    assert np.array_equal(cb["ids"].numpy().reshape(T, G, 3), np.repeat(ids.T[:, None, :], G, axis=1))
    if kind == "lc":                               # alpha and s stay per member row
        out = model.greedy_predict(xs, zs, zs, st, T, consensus=cons)
        assert out[0].shape == (3, T, 1) and out[1].shape == (3, T, V) and out[2].shape[:2] == (T, G * 3)
        assert out[3].shape[:2] == (T, G * 3)


@pytest.mark.parametrize("kind,seed", [("dense", 5), ("lc", 6)])
def test_sampled_launches_mix_sampler_on_the_mixed_rows_and_spread(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    G = 2
    xs, zs, st = members_of(model, x, z, start, G, seed)
    mock_backend.log.clear()
    kw = dict(temperature=0.9, top_k=6, top_p=0.95, sample_step=3)
    ids, probs = sample_ids(kind, model, xs, zs, st, consensus=Consensus(G), **kw)
    assert names(mock_backend) == ["consensus_mix", "sample_topkp", "consensus_spread"] * T
    for name, a in mock_backend.log:
        if name == "consensus_mix":
            assert a[9] is None                                       # no argmax: the sampler chooses
        elif name == "sample_topkp":
            assert a[2] == 3                                          # the M mixed rows
        else:
            assert a[1] is None and a[2] is None and a[3:5] == (3, G)
    want_ids, want_p, margin = CO.consensus_decode(orc, xs, zs, zs, st, T, G, "mean", None,
                                                   sampler=(0.9, 6, 0.95, model.seed, 3))
    ok = margin > 1e-5
    assert ok.sum() >= 2 and np.array_equal(ids[ok], want_ids[ok])
    # a plain decode of M rows draws row r from the same stream: identical copies give the plain draw
    xc, zc = np.tile(xs[:3], (G, 1)), np.tile(zs[:3], (G, 1))
    a = sample_ids(kind, model, xc, zc, st, consensus=Consensus(G), **kw)[0]
    b = sample_ids(kind, model, xs[:3], zs[:3], st, **kw)[0]
    assert np.array_equal(a, b)
    if kind == "lc":                               # the unfiltered draw
        mock_backend.log.clear()
        model.sample_predict(xs, zs, zs, st, T, sample_step=3, consensus=Consensus(G))
        assert names(mock_backend) == ["consensus_mix", "sample_rows", "consensus_spread"] * T


@pytest.mark.parametrize("kind,seed", [("dense", 7), ("lc", 8)])
@pytest.mark.parametrize("constrained", [False, True])
def test_beam_launches_and_matches_the_restatement(mock_backend, kind, seed, constrained):
    model, orc, x, z, start = MAKERS[kind](seed)
    G, k, end_id = 3, 3, 2
    xs, zs, st = members_of(model, x, z, start, G, seed)
    ckw, con = {}, None
    if constrained:
        ckw = dict(constraints=DecodeConstraints(no_repeat_ngram_size=2, min_length=3))
        con = dict(theta=1.0, n=2, m=3, end_id=end_id, bad_ids=())
    mock_backend.log.clear()
    seqs, scores = model.beam_search(xs, zs, zs, st, T, beam_width=k, end_id=end_id, consensus=Consensus(G, "logmean"), **ckw)
    expand = "beam_step" if kind == "dense" else "beam_topk"
    step = (["decode_constrain"] if constrained else []) + ["consensus_mix", expand, "consensus_spread"]
    # (the mock's beam_step calls its own beam_topk for the expansion: not a launch of the decode)
    assert [n for n in names(mock_backend) if not (kind == "dense" and n == "beam_topk")] == step * T
    for name, a in mock_backend.log:
        if name == "consensus_mix":
            assert a[3:5] == (3 * k, G) and a[9] is None
        elif name == "beam_step":
            assert a[4] == 3 and a[15] == 0 and a[12] is None         # B = M samples, U = 0: no fused reorder
        elif name == "beam_topk":
            assert a[3] == 3                                          # B = M samples
        elif name == "consensus_spread":
            assert all(v is not None for v in a[:3]) and a[3:5] == (3 * k, G)
        else:
            assert a[3] == G * 3 * k                                  # the constraints run on every member row
    want, wsc, margin = CO.consensus_beam(orc, xs, zs, zs, st, T, G, k, end_id, "logmean", None, con=con)
    ok = margin >= GAP
    assert ok.sum() >= 2 and seqs.shape == (3, k, T) and scores.shape == (3, k)
    assert np.array_equal(seqs[ok], want[ok]) and np.abs(scores[ok] - wsc[ok]).max() <= 1e-4 * np.abs(wsc[ok]).max()


@pytest.mark.parametrize("kind,seed", [("dense", 9), ("lc", 10)])
def test_none_changes_no_launch_and_no_key(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    keys = []
    run_captured = model._run_captured
    model._run_captured = lambda key, fn: (keys.append(key), run_captured(key, fn))
    shape = lambda a: tuple(v if isinstance(v, (int, float)) or v is None else "t" for v in a)
    runs = []
    for kw in ({}, dict(consensus=None)):
        mock_backend.log.clear(); keys.clear()
        out = [greedy_ids(kind, model, x, z, start, **kw), sample_ids(kind, model, x, z, start, top_k=5, **kw),
               model.beam_search(x, z, z, start, T, beam_width=3, end_id=2, **kw)]
        runs.append(([(n, shape(a)) for n, a in mock_backend.log], list(keys), out))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert not any(n.startswith("consensus") for n, _ in runs[0][0]) and "_cons_bufs" not in model.__dict__
    for a, b in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_ms_model_mixes_its_subject_slices(mock_backend):
    from masters_thesis_amd.ms_nic import NIC as MsNIC
    from helpers import tiny_groups
    rng = np.random.default_rng(12)
    N, R, D, A, U, Et, S = 41, 5, 16, 6, 16, 12, 2
    g = (tiny_groups(N, R, rng), [D] * R)
    args = (g, U, 512, Et, A, V, T, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5)
    model = MsNIC(*args, n_subjects=S, device="cpu", seed=11)
    orc = CO.ConsensusMsLcNIC(*args, n_subjects=S).init_params(rng)
    orc.p['time_distributed_softmax/kernel'] = orc.p['time_distributed_softmax/kernel'] * 8.0
    for k, v in orc.p.items():
        model.set_weight(k, v)
    x = rng.standard_normal((S * 3, N)).astype(np.float32)
    z, st = np.zeros((S * 3, U), np.float32), np.ones(3, np.int64)
    words, probs = model.greedy_predict(x, z, z, st, T, consensus=Consensus(S))[:2]
    want, wp, gap = CO.consensus_decode(orc, x, z, z, st, T, S)
    ok = gap >= GAP
    assert ok.sum() >= 2 and np.array_equal(words[ok, :, 0], want[ok])
    assert np.abs(probs.transpose(1, 0, 2)[:, ok] - wp[:, ok]).max() <= 1e-4
    for G in (1, 3):
        with pytest.raises(ValueError, match="n_subjects"):
            model.greedy_predict(x, z, z, np.ones(S * 3 // G, np.int64), T, consensus=Consensus(G))


# ---------------------------------------------------------------------------------------------------- the refusals
@pytest.mark.parametrize("kw", [dict(members=0), dict(members=17), dict(members=-1), dict(members=2.0), dict(members=True),
                                dict(members=2, mode="max"), dict(members=2, weights=(1, 0)), dict(members=2, weights=(1, -1)),
                                dict(members=2, weights=(1, float("nan"))), dict(members=2, weights=(1, float("inf"))),
                                dict(members=2, weights=(1, 2, 3)), dict(members=2, weights=("a", "b")),
                                dict(members=2, weights=(1, 1e-60))])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        Consensus(**kw)


def test_weights_are_normalised_and_repr():
    c = Consensus(4, "logmean", (1, 1, 2, 4))
    assert c.weights == (0.125, 0.125, 0.25, 0.5) and c.members == 4 and c.mode == "logmean"
    assert Consensus(3).weights is None and Consensus(1).mode == "mean"
    assert "members=4" in repr(c) and "logmean" in repr(c)


@pytest.mark.parametrize("kind,seed", [("dense", 13), ("lc", 14)])
def test_decode_refuses_before_any_launch(mock_backend, kind, seed):
    from types import SimpleNamespace
    model, orc, x, z, start = MAKERS[kind](seed)
    B = x.shape[0]                                 # 6 (dense) or 5 (lc) scans
    G = 4
    calls = [lambda **kw: model.greedy_predict(x, z, z, start[:1], T, **kw),
             lambda **kw: model.sample_predict(x, z, z, start[:1], T, top_k=3, **kw),
             lambda **kw: model.beam_search(x, z, z, start[:1], T, beam_width=3, **kw)]
    mock_backend.log.clear()
    for call in calls:
        with pytest.raises(ValueError, match="input rows"):            # the row count does not divide by G
            call(consensus=Consensus(G))
        with pytest.raises(ValueError, match="start_seq"):             # it divides, but start_seq is per scan
            model.greedy_predict(x[:4], z[:4], z[:4], start[:4], T, consensus=Consensus(2))
        with pytest.raises(ValueError, match="Consensus"):
            call(consensus=dict(members=2))
    model.grad_sync = SimpleNamespace(world=2)     # a data-parallel model
    for call in calls:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            call(consensus=Consensus(1))
    model.grad_sync = None
    if kind == "lc":
        with pytest.raises(ValueError, match="training"):
            model.greedy_predict(x[:4], z[:4], z[:4], start[:2], T, training=True, consensus=Consensus(2))
    assert not mock_backend.log and "_cons_bufs" not in model.__dict__


def test_evaluate_passes_the_keyword(mock_backend):
    from types import SimpleNamespace
    model, orc, x, z, start = MAKERS["dense"](15)
    G = 2
    xs, zs, st = members_of(model, x, z, start, G, 15)
    tok = SimpleNamespace(word_index={"<start>": 1, "<end>": 2}, index_word={i: f"w{i}" for i in range(3, V)})
    tok.index_word.update({1: "<start>", 2: "<end>"})
    ids, caps = evaluate.beam_captions(model, xs, zs, zs, tok, T, beam_width=3, consensus=Consensus(G))
    want = model.beam_search(xs, zs, zs, st, T, beam_width=3, end_id=2, consensus=Consensus(G))[0][:, 0]
    assert ids.shape == (3, T) and len(caps) == 3 and np.array_equal(ids, want)
    assert evaluate._con_kw(None) == {} and set(evaluate._con_kw(None, Consensus(2))) == {"consensus"}
