"""Classifier-free guidance on the CPU: the restatement (tests/guidance_oracle.py) on hand-computed cases, model_base.Guidance's
validation, and the host orchestration of greedy_predict, sample_predict and beam_search of nic.NIC and lc_nic.NIC with
``guidance=`` through a mock backend that follows the header definition of tnt_guidance_mix_f32: launch sequences, capture
keys, the row layout (the null slab holds the null scan), results, the neutral object, refusals, evaluate's pass-through."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.model_base import BeamDiversity, Consensus, DecodeConstraints, Guidance
from mock_backend import flat, mat
import guidance_oracle as GO
from test_host_consensus import ConsensusMockBackend, GAP, names
from test_host_constrain import MAKERS, T, V, greedy_ids, sample_ids

SCALE, PLAUS = 1.5, 0.05
# The model computes its logits in float32, the restatement in float64 from the same weights: the consensus host tests bound
# what that does to a softmax by 1e-4; a logit's error enters the guided logit (1 + scale) times through lc and scale times
# through ln.
PTOL = 1e-4 * (1 + 2 * SCALE)
LEFT_OUT = 0.1          # the share of captions a test may leave out for a decision gap under GAP, at most
# (kind, path) -> the maker's seed; found on the CPU with the restatement alone: no caption's decision gap is under 3 x the bound, in any of the three null forms
SEEDS = {("dense", "greedy"): 1, ("lc", "greedy"): 2, ("dense", "sample"): 2, ("lc", "sample"): 1,
         ("dense", "beam"): 9, ("lc", "beam"): 2}


class GuidanceMockBackend(ConsensusMockBackend):
    """ConsensusMockBackend plus tnt_guidance_mix_f32 from the header text, logged like the launches of the decode's tail"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.guidance_mix = self._logged("guidance_mix", self.guidance_mix)

    def guidance_mix(self, logits, ld, V, Rm, scale, plaus, mix, ldm, token):
        assert Rm > 0 and V > 0 and ld >= V and ldm >= V
        assert np.isfinite(np.float32(scale)) and scale >= 0 and 0 <= np.float32(plaus) < 1
        assert logits is not None and mix is not None and logits.data_ptr() != mix.data_ptr()
        p, _ = GO.mix(mat(logits, 2 * Rm, V, ld), np.float32(scale), np.float32(plaus))
        out = mat(mix, Rm, V, ldm)
        out[...] = p.astype(np.float32)
        if token is not None:
            flat(token)[:2 * Rm] = np.tile(GO.first_max(out), 2)


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = GuidanceMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def capture_keys(model):
    keys = []
    run_captured = model._run_captured
    model._run_captured = lambda key, fn: (keys.append(key), run_captured(key, fn))
    return keys


def null_forms(x, seed):
    """the three forms of ``null`` with the rows they put into the null slab"""
    rng = np.random.default_rng(seed + 100)
    one = rng.standard_normal(x.shape[1]).astype(np.float32)
    each = rng.standard_normal(x.shape).astype(np.float32)
    return [(None, np.zeros_like(x)), (one, np.tile(one, (x.shape[0], 1))), (each, each)]


def staged_scans(model, rows, n):
    return model.x.numpy()[:rows, :n]


def kept(gap, bound=GAP):
    """the captions whose restated decode decides nothing by less than ``bound``; at most LEFT_OUT of them may be left out"""
    ok = gap >= bound
    assert (~ok).mean() <= LEFT_OUT, gap
    return ok


# ---------------------------------------------------------------------------------------------------- the restatement
def test_hand_computed_cases():
    ln = np.log
    pc = np.array([0.5, 0.3, 0.2])
    # scale 1 against a uniform null: p proportional to pc^2 (the null's log 1/3 is a constant); the logits' offsets drop out
    x = np.stack([ln(pc) + 2.0, np.zeros(3) - 5.0])
    p, t = GO.mix(x, 1.0)
    assert np.allclose(p, [pc ** 2 / (pc ** 2).sum()]) and t.tolist() == [0]
    # scale 0: the conditional softmax, whatever the null says
    p, _ = GO.mix(np.stack([ln(pc), ln(pc[::-1])]), 0.0)
    assert np.allclose(p, [pc])
    # a general scale: p proportional to pc^(1+s) / pn^s; here the contrast moves the maximum from 0 to 2
    pn = np.array([0.7, 0.2, 0.1])
    p, t = GO.mix(np.stack([ln(pc), ln(pn)]), 2.0)
    want = pc ** 3 / pn ** 2
    assert np.allclose(p, [want / want.sum()]) and t.tolist() == [2]
    # the mask keeps exactly {v: pc_v >= plaus * max pc}: 0.2 < 0.5 * 0.5 <= 0.3
    p, t = GO.mix(np.stack([ln(pc), ln(pn)]), 2.0, 0.5)
    keep = want * np.array([1, 1, 0])
    assert np.allclose(p, [keep / keep.sum()]) and p[0, 2] == 0.0 and t.tolist() == [1]
    p, _ = GO.mix(np.stack([ln(pc), ln(pn)]), 2.0, 0.39)            # 0.2 >= 0.39 * 0.5: all three stay
    assert np.all(p > 0)
    p, _ = GO.mix(np.stack([ln(pc), ln(pn)]), 0.0, 0.7)             # only the conditional maximum: always kept
    assert p.tolist() == [[1.0, 0.0, 0.0]]
    # a column banned in the conditional row stays 0 (also when the null bans it too: no inf - inf); one banned in the null
    # row only drops the contrast term, g = lc
    inf = np.inf
    p, _ = GO.mix(np.array([[0.0, -inf, 0.0, -inf], [0.0, 0.0, -inf, -inf]]), 1.0)
    assert p[0, 1] == 0.0 and p[0, 3] == 0.0 and not np.any(np.isnan(p))
    g = np.array([ln(0.5) + (ln(0.5) - ln(0.5)), ln(0.5)])          # columns 0 and 2
    assert np.allclose(p[0, [0, 2]], np.exp(g) / np.exp(g).sum())
    # the all-banned conditional row: p = 0 everywhere, token 0; an all-banned null row: the conditional softmax
    p, t = GO.mix(np.array([[-inf, -inf, -inf], [0.0, 1.0, 2.0]]), 1.0, 0.1)
    assert p.tolist() == [[0.0, 0.0, 0.0]] and t.tolist() == [0]
    p, t = GO.mix(np.stack([ln(pc), np.full(3, -inf)]), 3.0)
    assert np.allclose(p, [pc]) and t.tolist() == [0]
    # member-major rows: conditional row r, null row Rm + r; an exact tie goes to the lower index
    x = np.stack([ln(pc), np.zeros(3), ln(pn), np.zeros(3)])
    p, t = GO.mix(x, 2.0)
    assert np.allclose(p, [want / want.sum(), np.full(3, 1 / 3)]) and t.tolist() == [2, 0]
    # the float32 twin computes the same thing in float32
    p32, t32 = GO.mix(x, 2.0, 0.0, np.float32)
    assert p32.dtype == np.float32 and np.allclose(p32, p, rtol=1e-5) and t32.tolist() == [2, 0]


def test_mock_op_follows_the_restatement(mock_backend):
    rng = np.random.default_rng(1)
    Rm, Vv, ld = 2, 7, 9
    x = torch.from_numpy(rng.standard_normal((2 * Rm, ld)).astype(np.float32) * 3)
    mixd, tok = torch.full((Rm, ld), -7.0), torch.full((2 * Rm,), -9, dtype=torch.int32)
    mock_backend.guidance_mix(x, ld, Vv, Rm, 1.5, 0.1, mixd, ld, tok)
    want, wt = GO.mix(x.numpy()[:, :Vv], np.float32(1.5), np.float32(0.1))
    assert np.allclose(mixd.numpy()[:, :Vv], want, rtol=1e-6) and np.all(mixd.numpy()[:, Vv:] == -7.0)
    assert tok.numpy().tolist() == np.tile(wt, 2).tolist()


# ---------------------------------------------------------------------------------------------------- Guidance
@pytest.mark.parametrize("kw", [dict(scale=-1), dict(scale=-1e-9), dict(scale=float("nan")), dict(scale=float("inf")),
                                dict(scale="1"), dict(scale=None), dict(scale=True), dict(scale=1e39),
                                dict(scale=1, plausibility=-0.1), dict(scale=1, plausibility=1.0),
                                dict(scale=1, plausibility=1 - 1e-12), dict(scale=1, plausibility=2),
                                dict(scale=1, plausibility=float("nan")), dict(scale=1, plausibility="0.1"),
                                dict(scale=1, plausibility=True),
                                dict(scale=1, null="zeros"), dict(scale=1, null=np.zeros((2, 3, 4))), dict(scale=1, null=3.0),
                                dict(scale=1, null=np.zeros(0)), dict(scale=1, null=[1.0, float("nan")]),
                                dict(scale=1, null=[[1.0, 2.0], [3.0]])])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        Guidance(**kw)


def test_neutral_and_repr():
    g = Guidance(1.5, np.zeros((2, 3)), 0.1)
    assert g.scale == 1.5 and g.plausibility == 0.1 and g.null.shape == (2, 3) and g.null.dtype == np.float32
    assert not g.neutral and "scale=1.5" in repr(g) and "(2, 3)" in repr(g)
    assert Guidance(0).neutral and Guidance(0.0, np.ones(4), 0.0).neutral and Guidance(0, plausibility=1e-60).neutral
    assert not Guidance(0, plausibility=0.1).neutral and not Guidance(1e-3).neutral
    assert Guidance(2, torch.ones(5)).null.tolist() == [1.0] * 5 and Guidance(np.float32(2)).scale == 2.0


# ---------------------------------------------------------------------------------------------------- the decodes
@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_greedy_launches_layout_keys_and_results(mock_backend, kind):
    model, orc, x, z, start = MAKERS[kind](SEEDS[kind, "greedy"])
    Mn, N = x.shape
    keys = capture_keys(model)
    for form, (null, rows) in enumerate(null_forms(x, 0)):
        mock_backend.log.clear(); keys.clear()
        ids, probs = greedy_ids(kind, model, x, z, start, guidance=Guidance(SCALE, null, PLAUS))
        # per token: one mix launch with the token output, in the place of softmax + argmax
        assert names(mock_backend) == ["guidance_mix"] * T
        for _, a in mock_backend.log:
            assert a[3] == Mn and a[4:6] == (SCALE, float(np.float32(PLAUS))) and a[8] is not None
        assert keys[0][0] == "greedy" and keys[0][-3:] == ("guidance", SCALE, float(np.float32(PLAUS)))
        # the row layout: the scans, then their null scans; the start tokens and the common word on both slabs
        assert np.array_equal(staged_scans(model, 2 * Mn, N), np.concatenate([x, rows]))
        cb = [v for k, v in model._cons_bufs.items() if isinstance(v, dict)][0]
        assert cb["start"].numpy().reshape(-1).tolist() == np.tile(start, 2).tolist()
        assert np.array_equal(cb["ids"].numpy().reshape(T, 2, Mn), np.repeat(ids.T[:, None, :], 2, axis=1))
        want_ids, want_p, gap = GO.guided_decode(orc, x, z, z, start, T, SCALE, PLAUS, null)
        ok = kept(gap) if form == 0 else gap >= GAP
        assert ids.shape == (Mn, T) and probs.shape == (T, Mn, V)
        assert np.array_equal(ids[ok], want_ids[ok]) and np.abs(probs[:, ok] - want_p[:, ok]).max() <= PTOL
    # the capture key differs per (scale, plausibility), and not per null scan (it travels in the staged inputs)
    seen = set()
    for sc, pl in ((SCALE, PLAUS), (SCALE, 0.0), (0.5, PLAUS), (0.0, PLAUS)):
        keys.clear()
        greedy_ids(kind, model, x, z, start, guidance=Guidance(sc, None, pl))
        seen.add(keys[0])
    assert len(seen) == 4
    if kind == "lc":                               # alpha and s stay per member row
        out = model.greedy_predict(x, z, z, start, T, guidance=Guidance(SCALE))
        assert out[0].shape == (Mn, T, 1) and out[1].shape == (Mn, T, V) and out[2].shape[:2] == (T, 2 * Mn)
        assert out[3].shape[:2] == (T, 2 * Mn)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_sampled_launches_layout_keys_and_results(mock_backend, kind):
    model, orc, x, z, start = MAKERS[kind](SEEDS[kind, "sample"])
    Mn, N = x.shape
    keys = capture_keys(model)
    kw = dict(temperature=0.9, top_k=6, top_p=0.95, sample_step=3)
    for form, (null, rows) in enumerate(null_forms(x, 1)):
        mock_backend.log.clear(); keys.clear()
        ids, probs = sample_ids(kind, model, x, z, start, guidance=Guidance(SCALE, null, PLAUS), **kw)
        assert names(mock_backend) == ["guidance_mix", "sample_topkp", "consensus_spread"] * T
        for name, a in mock_backend.log:
            if name == "guidance_mix":
                assert a[3] == Mn and a[8] is None                    # no argmax: the sampler chooses
            elif name == "sample_topkp":
                assert a[2] == Mn                                     # the M guided rows
            else:
                assert a[1] is None and a[2] is None and a[3:5] == (Mn, 2)
        assert keys[0][0] == "sample" and keys[0][-3:] == ("guidance", SCALE, float(np.float32(PLAUS)))
        assert np.array_equal(staged_scans(model, 2 * Mn, N), np.concatenate([x, rows]))
        want_ids, want_p, margin = GO.guided_decode(orc, x, z, z, start, T, SCALE, PLAUS, null,
                                                    sampler=(0.9, 6, 0.95, model.seed, 3))
        ok = kept(margin, 1e-5) if form == 0 else margin > 1e-5
        assert np.array_equal(ids[ok], want_ids[ok]) and np.abs(probs[:, ok] - want_p[:, ok]).max() <= PTOL
    sample_ids(kind, model, x, z, start, guidance=Guidance(SCALE, None, 0.0), **kw)
    sample_ids(kind, model, x, z, start, guidance=Guidance(0.5, None, PLAUS), **kw)
    assert len(set(keys)) == 3                     # the loop's key, and one more per (scale, plausibility)
    # row r draws from the stream row r of a plain decode draws from: the batch's own scans as the null scans contrast
    # nothing, and the guided draw is the plain one
    a = sample_ids(kind, model, x, z, start, guidance=Guidance(SCALE, x), **kw)[0]
    b = sample_ids(kind, model, x, z, start, **kw)[0]
    assert np.array_equal(a, b)
    if kind == "lc":                               # the unfiltered draw
        mock_backend.log.clear()
        model.sample_predict(x, z, z, start, T, sample_step=3, guidance=Guidance(SCALE))
        assert names(mock_backend) == ["guidance_mix", "sample_rows", "consensus_spread"] * T


@pytest.mark.parametrize("kind", ["dense", "lc"])
@pytest.mark.parametrize("constrained", [False, True])
def test_beam_launches_layout_keys_and_results(mock_backend, kind, constrained):
    model, orc, x, z, start = MAKERS[kind](SEEDS[kind, "beam"])
    Mn, N = x.shape
    k, end_id = 3, 2
    keys = capture_keys(model)
    ckw, con = {}, None
    if constrained:
        ckw = dict(constraints=DecodeConstraints(no_repeat_ngram_size=2, min_length=3))
        con = dict(theta=1.0, n=2, m=3, end_id=end_id, bad_ids=())
    expand = "beam_step" if kind == "dense" else "beam_topk"
    step = (["decode_constrain"] if constrained else []) + ["guidance_mix", expand, "consensus_spread"]
    for form, (null, rows) in enumerate(null_forms(x, 2)):
        mock_backend.log.clear(); keys.clear()
        seqs, scores = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, guidance=Guidance(SCALE, null, PLAUS),
                                         **ckw)
        # (the mock's beam_step calls its own beam_topk for the expansion: not a launch of the decode)
        assert [n for n in names(mock_backend) if not (kind == "dense" and n == "beam_topk")] == step * T
        for name, a in mock_backend.log:
            if name == "guidance_mix":
                assert a[3] == Mn * k and a[4:6] == (SCALE, float(np.float32(PLAUS))) and a[8] is None
            elif name == "beam_step":
                assert a[4] == Mn and a[15] == 0 and a[12] is None        # B = M samples, U = 0: no fused reorder
            elif name == "beam_topk":
                assert a[3] == Mn                                         # B = M samples
            elif name == "consensus_spread":
                assert all(v is not None for v in a[:3]) and a[3:5] == (Mn * k, 2)
            else:
                assert a[3] == 2 * Mn * k                                 # the constraints run on both slabs
        if kind == "dense":                        # lc_nic's beam loop is eager, and stages every scan k times
            assert keys[0][0] == "beam" and ("guidance", SCALE, float(np.float32(PLAUS))) == keys[0][-3:]
            assert np.array_equal(staged_scans(model, 2 * Mn, N), np.concatenate([x, rows]))
        else:
            assert np.array_equal(staged_scans(model, 2 * Mn * k, N), np.repeat(np.concatenate([x, rows]), k, axis=0))
        want, wsc, margin = GO.guided_beam(orc, x, z, z, start, T, SCALE, PLAUS, null, k, end_id, con=con)
        ok = kept(margin) if form == 0 else margin >= GAP
        assert seqs.shape == (Mn, k, T) and scores.shape == (Mn, k)
        assert np.array_equal(seqs[ok], want[ok]) and np.abs(scores[ok] - wsc[ok]).max() <= PTOL * np.abs(wsc[ok]).max()
    if kind == "dense":
        keys.clear()
        model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, guidance=Guidance(SCALE, None, 0.0), **ckw)
        model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, guidance=Guidance(0.5, None, PLAUS), **ckw)
        assert keys[0] != keys[1] and keys[0][-3:] == ("guidance", SCALE, 0.0) and keys[1][-3:-1] == ("guidance", 0.5)


@pytest.mark.parametrize("kind,seed", [("dense", 9), ("lc", 10)])
def test_neutral_changes_no_launch_no_key_and_no_output(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    keys = capture_keys(model)
    shape = lambda a: tuple(v if isinstance(v, (int, float)) or v is None else "t" for v in a)
    runs = []
    for kw in ({}, dict(guidance=None), dict(guidance=Guidance(0.0)), dict(guidance=Guidance(0, np.ones(3), 0.0))):
        mock_backend.log.clear(); keys.clear()
        out = [greedy_ids(kind, model, x, z, start, **kw), sample_ids(kind, model, x, z, start, top_k=5, **kw),
               model.beam_search(x, z, z, start, T, beam_width=3, end_id=2, **kw)]
        runs.append(([(n, shape(a)) for n, a in mock_backend.log], list(keys), out))
    assert not any(n.startswith(("consensus", "guidance")) for n, _ in runs[0][0]) and "_cons_bufs" not in model.__dict__
    for other in runs[1:]:
        assert runs[0][0] == other[0] and runs[0][1] == other[1]
        for a, b in zip(runs[0][2], other[2]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_ms_nic_inherits_the_keyword_and_refuses_more_than_one_subject(mock_backend):
    import inspect
    from masters_thesis_amd.ms_nic import NIC as MsNIC
    from helpers import tiny_groups
    for name in ("greedy_predict", "sample_predict", "beam_search"):
        assert "guidance" in inspect.signature(getattr(MsNIC, name)).parameters
    rng = np.random.default_rng(12)
    N, R, D, A, U, Et = 41, 5, 16, 6, 16, 12
    g = (tiny_groups(N, R, rng), [D] * R)
    args = (g, U, 512, Et, A, V, T, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5)
    x, z, st = rng.standard_normal((4, N)).astype(np.float32), np.zeros((4, U), np.float32), np.ones(4, np.int64)
    model = MsNIC(*args, n_subjects=2, device="cpu", seed=11)
    mock_backend.log.clear()
    for call in (lambda **kw: model.greedy_predict(x, z, z, st, T, **kw),
                 lambda **kw: model.sample_predict(x, z, z, st, T, top_k=3, **kw),
                 lambda **kw: model.beam_search(x, z, z, st, T, beam_width=3, **kw)):
        with pytest.raises(ValueError, match="n_subjects"):
            call(guidance=Guidance(1.0))
    assert not mock_backend.log
    one = MsNIC(*args, n_subjects=1, device="cpu", seed=11)
    words = one.greedy_predict(x, z, z, st, T, guidance=Guidance(1.0))[0]
    assert words.shape == (4, T, 1) and names(mock_backend) == ["guidance_mix"] * T


# ---------------------------------------------------------------------------------------------------- the refusals
@pytest.mark.parametrize("kind,seed", [("dense", 13), ("lc", 14)])
def test_decode_refuses_before_any_launch(mock_backend, kind, seed):
    model, orc, x, z, start = MAKERS[kind](seed)
    Mn, N = x.shape
    calls = [lambda **kw: model.greedy_predict(x, z, z, start, T, **kw),
             lambda **kw: model.sample_predict(x, z, z, start, T, top_k=3, **kw),
             lambda **kw: model.beam_search(x, z, z, start, T, beam_width=4, **kw)]
    mock_backend.log.clear()
    g = Guidance(1.0)
    for call in calls:
        with pytest.raises(ValueError, match="consensus"):
            call(guidance=g, consensus=Consensus(1))
        with pytest.raises(ValueError, match="Guidance"):
            call(guidance=dict(scale=1.0))
        for null in (np.zeros(N + 1), np.zeros((Mn + 1, N)), np.zeros((Mn, N + 1)), np.zeros((1, N)), np.zeros((2 * Mn, N))):
            with pytest.raises(ValueError, match="null scan"):
                call(guidance=Guidance(1.0, null))
    with pytest.raises(ValueError, match="diversity"):
        calls[2](guidance=g, diversity=BeamDiversity(2, 0.5))
    with pytest.raises(ValueError, match="start_seq"):                  # one scan per caption
        model.greedy_predict(x, z, z, start[:2], T, guidance=g)
    model.grad_sync = SimpleNamespace(world=2)     # a data-parallel model
    for call in calls:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            call(guidance=g)
    model.grad_sync = None
    if kind == "lc":
        with pytest.raises(ValueError, match="training"):
            model.greedy_predict(x, z, z, start, T, training=True, guidance=g)
    assert not mock_backend.log and "_cons_bufs" not in model.__dict__
    # one group is no diversity: the guided search runs
    seqs, _ = calls[2](guidance=g, diversity=BeamDiversity(1, 0.5))
    assert seqs.shape == (Mn, 4, T)


def test_models_without_the_keyword_refuse_it():
    import inspect
    from masters_thesis_amd import fc_nic, model_base
    assert "guidance" not in inspect.signature(fc_nic.NICfc.greedy_predict).parameters
    assert "guidance" not in inspect.signature(model_base.ModelBase.score_captions).parameters


# ---------------------------------------------------------------------------------------------------- evaluate
def tokenizer():
    tok = SimpleNamespace(word_index={"<start>": 1, "<end>": 2}, index_word={i: f"w{i}" for i in range(3, V)})
    tok.index_word.update({1: "<start>", 2: "<end>"})
    tok.to_json = lambda: "{}"
    return tok


def test_evaluate_passes_the_keyword(mock_backend, tmp_path):
    tok = tokenizer()
    g = Guidance(SCALE, None, PLAUS)
    model, orc, x, z, start = MAKERS["dense"](15)
    ids, caps = evaluate.beam_captions(model, x, z, z, tok, T, beam_width=3, guidance=g)
    want = model.beam_search(x, z, z, start, T, beam_width=3, end_id=2, guidance=g)[0][:, 0]
    assert ids.shape == (x.shape[0], T) and len(caps) == x.shape[0] and np.array_equal(ids, want)
    assert evaluate._con_kw(None) == {} and set(evaluate._con_kw(None, None, g)) == {"guidance"}
    assert set(evaluate._con_kw(DecodeConstraints(), Consensus(2), g)) == {"constraints", "consensus", "guidance"}
    # eval_model: two batches of the attention model; the files hold the guided decode of every scan
    model, orc, x, z, start = MAKERS["lc"](16)
    gen = [((x[:3], None, z[:3], z[:3]), None), ((x[3:], None, z[3:], z[3:]), None)]
    config = dict(max_length=T, units=z.shape[1])
    mock_backend.log.clear()
    outputs, attn = evaluate.eval_model(model, gen, tok, config, str(tmp_path), 0, guidance=g)
    assert names(mock_backend) == ["guidance_mix"] * (2 * T)
    words = np.concatenate([model.greedy_predict(x[s], z[s], z[s], start[s], T, guidance=g)[0] for s in (slice(0, 3), slice(3, None))])
    plain = evaluate.eval_model(model, gen, tok, config, str(tmp_path), 1)[0]
    assert np.array_equal(outputs, words) and outputs.shape == plain.shape and attn.shape[0] == x.shape[0]
    raw = np.load(tmp_path / "output_captions_raw_0.npy")
    assert raw.shape == (x.shape[0], T, V) and np.abs(raw.sum(-1) - 1).max() <= 1e-5
    # a model without the keyword refuses the call instead of ignoring it
    refusing = SimpleNamespace(greedy_predict=lambda *a, **kw: (_ for _ in ()).throw(TypeError(sorted(kw))))
    with pytest.raises(TypeError, match="guidance"):
        evaluate.eval_fc_model(refusing, gen, tok, config, str(tmp_path), 0, guidance=g)
