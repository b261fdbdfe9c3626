"""Diverse (group) beam search on the CPU: model_base.BeamDiversity and the ``diversity=`` keyword of nic.NIC.beam_search,
lc_nic.NIC.beam_search and evaluate.beam_captions through a mock backend that follows tnt_beam_step_diverse_f32's header
definition, against the float64 restatement (tests/diverse_beam_oracle.py) on the tiny golden fixtures; and
evaluate.distinct_n."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.model_base import BeamDiversity, Consensus, DecodeConstraints
from mock_backend import flat
from constrain_oracle import constrained_beam
from dense_beam_oracle import length_normalise as length_normalise_ref
import consensus_oracle as CO
import diverse_beam_oracle as DO
from test_host_consensus import ConsensusMockBackend

MARGIN = 1e-4            # decision gap of the restatement below which a sample's results are not compared
T, END = 4, 2            # the tiny fixtures decode 4 tokens
K, GD, LAM = 6, 3, 0.8
# scans (one per image, or two with consensus) whose float64 restatement decides every sample of every case below by more
# than MARGIN; the tests assert at least two of three on the restatement
SEED = {"dense": 3, "lc": 3}


class Backend(DO.DiverseBeamMock, ConsensusMockBackend):
    """the logging mock of the consensus tests plus tnt_beam_step_diverse_f32; ``score_ins`` keeps a copy of every diverse
    launch's score_in"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.score_ins = []
        inner = self.beam_step_diverse

        def call(*a):
            self.log.append(("beam_step_diverse", a))
            self.score_ins.append(flat(a[2])[:a[4] * a[6]].copy())
            return inner(*a)
        self.beam_step_diverse = call


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = Backend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def names(be):
    return [n for n, _ in be.log]


def make(kind, G=1, Mn=3, seed=None):
    """(model on the mock backend, restatement, x, z, start): the tiny golden fixture of ``kind``, G scans per image"""
    orc, ctor, kw = CO.golden_case(kind)
    if kind == "dense":
        from masters_thesis_amd.nic import NIC
    else:
        from masters_thesis_amd.lc_nic import NIC
    model = NIC(*ctor, seed=11, device="cpu", **kw)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return (model, orc) + CO.scans(G, Mn, SEED[kind] if seed is None else seed)


def search(model, x, z, start, k=K, **kw):
    return model.beam_search(x, z, z, start, T, beam_width=k, end_id=END, **kw)


# ---------------------------------------------------------------------------------------------------- the keyword object
@pytest.mark.parametrize("kw", [dict(groups=0), dict(groups=-2), dict(groups=1.5), dict(groups=True), dict(groups="2"),
                                dict(groups=None), dict(groups=2, penalty=-0.1), dict(groups=2, penalty=float("nan")),
                                dict(groups=2, penalty=float("inf")), dict(groups=2, penalty="0.5"),
                                dict(groups=2, penalty=None), dict(groups=2, penalty=True), dict(groups=2, penalty=1e39)])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        BeamDiversity(**kw)


def test_constructor_accepts_and_repr():
    d = BeamDiversity(3, 0.5)
    assert (d.groups, d.penalty) == (3, 0.5) and repr(d) == "BeamDiversity(groups=3, penalty=0.5)"
    assert BeamDiversity(np.int64(2), np.float32(0.25)).penalty == 0.25
    assert BeamDiversity(1, 0).penalty == 0.0
    assert BeamDiversity(2, 0.1).penalty == float(np.float32(0.1))          # the float32 the kernel receives


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_search_refuses_before_any_launch(mock_backend, kind):
    model, _, x, z, start = make(kind)
    for k, d in ((5, BeamDiversity(2)), (6, BeamDiversity(4)), (2, BeamDiversity(4)), (6, 3), (6, "groups"),
                 (6, dict(groups=3))):
        mock_backend.log.clear()
        with pytest.raises(ValueError):
            search(model, x, z, start, k=k, diversity=d)
        assert mock_backend.log == [] and model._shape is None
    model.grad_sync = object()                       # a data-parallel model
    with pytest.raises(NotImplementedError):
        search(model, x, z, start, diversity=BeamDiversity(3))
    assert mock_backend.log == []


# ---------------------------------------------------------------------------------------------------- the mock op
def test_mock_op_consequences(mock_backend):
    """the header's consequences on the mock: lambda = 0 is beam_step on (B*Gd, k'), Gd = 1 is beam_step on (B, k)"""
    import torch
    rng = np.random.default_rng(1)
    B, k, V, ld = 3, 6, 17, 19
    probs = torch.tensor(rng.random((B * k, ld)).astype(np.float32))
    score = torch.tensor((-5 * rng.random(B * k)).astype(np.float32))
    fin = torch.tensor((rng.random(B * k) < 0.3).astype(np.int32))

    def run(diverse, Bn, kn, *tail):
        so, pa, to, fo = torch.zeros(B * k), *(torch.zeros(B * k, dtype=torch.int32) for _ in range(3))
        fn = mock_backend.beam_step_diverse if diverse else mock_backend.beam_step
        fn(probs, ld, score, fin, Bn, V, kn, 4, so, pa, to, fo, None, None, 0, 0, None, None, *tail)
        return [t.numpy().copy() for t in (so, pa, to, fo)]
    for gd in (2, 3):
        for a, b in zip(run(True, B, k, gd, 0.0), run(False, B * gd, k // gd)):
            assert np.array_equal(a, b)
    for a, b in zip(run(True, B, k, 1, 0.7), run(False, B, k)):
        assert np.array_equal(a, b)
    assert not np.array_equal(run(True, B, k, 3, 5.0)[2], run(True, B, k, 3, 0.0)[2])


def test_step_restatement_by_hand():
    """two groups of one beam over three tokens: group 1 would repeat group 0's token and is steered to the next one"""
    p = np.array([[0.6, 0.3, 0.1], [0.5, 0.4, 0.1]])
    s, par, tok, fin, gap, nv = DO.diverse_step(p, np.zeros(2), np.zeros(2, bool), 2, 0.5, -1)
    assert tok.tolist() == [0, 1] and par.tolist() == [0, 1] and nv == 1
    assert np.allclose(s, np.log([0.6, 0.4]))                      # the scores carry no penalty
    # keys of group 1: log .5 - .5 = -1.193, log .4 = -0.916, log .1 = -2.303; group 0: log .6, log .3
    assert np.isclose(gap, min(np.log(0.4) - (np.log(0.5) - 0.5), np.log(0.6) - np.log(0.3)))
    # a finished beam keeps token 0 at its own score, is not penalised and counts for no n_v
    s, par, tok, fin, _, nv = DO.diverse_step(p, np.array([-1.0, -2.0]), np.array([True, True]), 2, 9.0, -1)
    assert tok.tolist() == [0, 0] and s.tolist() == [-1.0, -2.0] and fin.all() and nv == 0
    # lambda = 0: every group chooses alike
    _, _, tok, _, _, _ = DO.diverse_step(np.tile(p[:1], (4, 1)), np.zeros(4), np.zeros(4, bool), 2, 0.0, -1)
    assert tok.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------- the neutral cases
@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_neutral_objects_change_no_launch_no_key_no_bit(mock_backend, kind):
    model, _, x, z, start = make(kind)
    keys = []
    run_captured = model._run_captured
    model._run_captured = lambda key, fn: (keys.append(key), run_captured(key, fn))
    shape = lambda a: tuple(v if isinstance(v, (int, float)) or v is None else "t" for v in a)
    runs = []
    for kw in ({}, dict(diversity=None), dict(diversity=BeamDiversity(1, 0.7))):
        mock_backend.log.clear(); keys.clear()
        out = [search(model, x, z, start, **kw), search(model, x, z, start, length_penalty=0.6, **kw)]
        runs.append(([(n, shape(a)) for n, a in mock_backend.log], list(keys), out,
                     sorted(map(str, model.__dict__.get("_beam_bufs", {})))))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and r[3] == runs[0][3]
        for a, b in zip(runs[0][2], r[2]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert "beam_step_diverse" not in names(mock_backend)
    if kind == "dense":
        assert not any(isinstance(key, tuple) for b in model._beam_bufs.values() for key in b)


# ---------------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize("kind", ["dense", "lc"])
@pytest.mark.parametrize("k,gd", [(K, GD), (4, 2), (4, 4)])
def test_models_match_the_restatement(mock_backend, kind, k, gd):
    model, orc, x, z, start = make(kind)
    keys = []
    run_captured = model._run_captured
    model._run_captured = lambda key, fn: (keys.append(key), run_captured(key, fn))
    kp = k // gd
    for end_id in (-1, END):
        mock_backend.log.clear(); mock_backend.score_ins.clear()
        want, wscore, margin = DO.diverse_beam(orc, x, z, z, start, T, k, gd, LAM, end_id)
        got, gscore = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, diversity=BeamDiversity(gd, LAM))
        assert got.shape == (3, k, T) and got.dtype == np.int64 and gscore.shape == (3, k) and gscore.dtype == np.float32
        ok = margin > MARGIN
        assert ok.sum() >= 2, margin
        assert np.array_equal(got[ok], want[ok]), (kind, end_id)
        assert np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)
        # one diverse launch per token in the place of the plain expansion; the attention path without the fused reorder
        launched = [n for n in names(mock_backend) if n.startswith("beam")]
        assert launched == ["beam_step_diverse"] * T
        for _, a in mock_backend.log:
            if _ == "beam_step_diverse":
                assert a[4] == 3 and a[6] == k and a[18:] == (gd, float(np.float32(LAM)))
                assert (a[15] == model.U and a[12] is not None) if kind == "dense" else (a[15] == 0 and a[12] is None)
        # the initial scores: 0 at the first slot of every group, -1e30 elsewhere
        init = np.full((3, gd, kp), np.float32(-1e30)); init[:, :, 0] = 0
        assert np.array_equal(mock_backend.score_ins[0], init.reshape(-1))
        if kind == "dense":
            assert keys[-1] == ("beam", 3, k, T, end_id, "diverse", gd, float(np.float32(LAM)))
    # the scores are sums of log-probabilities: non-increasing within every group
    assert np.all(np.diff(gscore.reshape(3, gd, kp), axis=2) <= 0)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_group0_is_the_plain_search_of_its_width(kind):
    model, orc, x, z, start = make(kind)
    kp = K // GD
    _, _, margin = constrained_beam(orc, x, z, z, start, T, k=kp, end_id=END)
    got, gscore = search(model, x, z, start, diversity=BeamDiversity(GD, LAM))
    plain, pscore = search(model, x, z, start, k=kp)
    ok = margin > MARGIN
    assert ok.sum() >= 2
    assert np.array_equal(got[ok, :kp], plain[ok]) and np.allclose(gscore[ok, :kp], pscore[ok], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(got[:, kp:2 * kp], got[:, :kp])                 # the penalty moved group 1


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_penalty_zero_gives_identical_groups(kind):
    model, orc, x, z, start = make(kind)
    kp = K // GD
    _, _, margin = DO.diverse_beam(orc, x, z, z, start, T, K, GD, 0.0, END)
    got, gscore = search(model, x, z, start, diversity=BeamDiversity(GD, 0.0))
    ok = margin > MARGIN
    assert ok.sum() >= 2
    for g in range(1, GD):
        assert np.array_equal(got[ok, g * kp:(g + 1) * kp], got[ok, :kp])
        assert np.allclose(gscore[ok, g * kp:(g + 1) * kp], gscore[ok, :kp], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_length_penalty_reorders_within_a_group_only(kind):
    model, _, x, z, start = make(kind)
    kp = K // GD
    raw, rscore = search(model, x, z, start, diversity=BeamDiversity(GD, LAM))
    got, gkey = search(model, x, z, start, diversity=BeamDiversity(GD, LAM), length_penalty=0.9)
    for g in range(GD):
        sl = slice(g * kp, (g + 1) * kp)
        ws, wk = length_normalise_ref(raw[:, sl], rscore[:, sl], END, 0.9)
        assert np.array_equal(got[:, sl], ws) and np.array_equal(gkey[:, sl], wk)
    assert np.array_equal(np.repeat(np.arange(GD), kp), [0, 0, 1, 1, 2, 2])     # the group index of the k slots


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_composes_with_constraints(mock_backend, kind):
    model, orc, x, z, start = make(kind)
    con = dict(theta=1.3, n=2, m=3, end_id=END, bad_ids=())
    mock_backend.log.clear()
    got, gscore = search(model, x, z, start, diversity=BeamDiversity(GD, LAM),
                         constraints=DecodeConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=3))
    want, wscore, margin = DO.diverse_beam(orc, x, z, z, start, T, K, GD, LAM, END, con=con)
    tail = [n for n in names(mock_backend) if n in ("decode_constrain", "softmax_cce", "beam_step_diverse", "beam_step",
                                                    "beam_topk")]
    assert tail == ["decode_constrain", "softmax_cce", "beam_step_diverse"] * T
    ok = margin > MARGIN
    assert ok.sum() >= 2, margin
    assert np.array_equal(got[ok], want[ok]) and np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)
    assert not np.any(got[:, :, :3] == END)                                     # min_length held in every group


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_composes_with_consensus(mock_backend, kind):
    G = 2
    model, orc, x, z, start = make(kind, G=G)
    mock_backend.log.clear()
    got, gscore = search(model, x, z, start, diversity=BeamDiversity(GD, LAM), consensus=Consensus(G, "logmean"))
    want, wscore, margin = DO.diverse_beam(orc, x, z, z, start, T, K, GD, LAM, END, members=G, mode="logmean")
    assert names(mock_backend) == ["consensus_mix", "beam_step_diverse", "consensus_spread"] * T
    for name, a in mock_backend.log:
        if name == "beam_step_diverse":                 # on the M*k mixed rows, without the fused reorder
            assert a[4] == 3 and a[15] == 0 and a[12] is None
    ok = margin > MARGIN
    assert ok.sum() >= 2, margin
    assert got.shape == (3, K, T)
    assert np.array_equal(got[ok], want[ok]) and np.allclose(gscore[ok], wscore[ok], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_beam_captions_passes_the_keyword(mock_backend, kind):
    from test_host_beam import tokenizer
    model, _, x, z, start = make(kind)
    tok = tokenizer(11)                                  # <start> = 1, <end> = 2
    d = BeamDiversity(GD, LAM)
    ids, caps = evaluate.beam_captions(model, x, z, z, tok, T, beam_width=K, diversity=d)
    assert "beam_step_diverse" in names(mock_backend)
    want = search(model, x, z, start, diversity=d)[0][:, 0]
    assert np.array_equal(ids, want) and caps == evaluate.ids_to_captions(ids, tok)
    mock_backend.log.clear()
    evaluate.beam_captions(model, x, z, z, tok, T, beam_width=K)
    assert "beam_step_diverse" not in names(mock_backend)


# ---------------------------------------------------------------------------------------------------- distinct_n
def test_distinct_n_by_hand():
    d = evaluate.distinct_n
    caps = [["a", "dog", "runs"], ["a", "dog", "sits"], ["a", "cat", "sits"]]
    assert d(caps, 1) == 5 / 9                           # a dog runs sits cat
    assert d(caps, 2) == 5 / 6                           # (a dog) twice
    assert d(caps, 3) == 1.0
    assert d(caps, 4) == 0.0                             # no 4-gram at all
    assert d([[1, 2, 3]] * 6, 2) == 2 / 12               # six copies
    assert d([np.array([1, 2]), (1, 2), []], 1) == 0.5   # any sequence type; an empty caption adds nothing
    assert d([], 1) == 0.0
    for n in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            d(caps, n)
