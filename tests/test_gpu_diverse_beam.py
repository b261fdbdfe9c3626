"""Diverse (group) beam search on the GPU: tnt_beam_step_diverse_f32 bit for bit against tnt_beam_step_f32 where the
header says the two coincide (lambda = 0, one group), against the float64 restatement (tests/diverse_beam_oracle.py) with
lambda > 0 on inputs drawn so that no decision is a near tie, its state reorder and refusals; and both caption models'
``diversity=`` searches on the sharpened tiny golden fixtures against the float64 searches, captured replay against
eager decoding, and diversity=None against the call without the keyword."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import consensus_oracle as CO
import diverse_beam_oracle as DO
from dense_beam_oracle import length_normalise as length_normalise_ref
from test_gpu_beam import MARGIN

pytestmark = pytest.mark.gpu

VS = (5, 257, 5001)
BS = (1, 3)
KG = ((2, 2), (4, 2), (6, 2), (6, 3), (15, 5), (16, 4), (16, 16), (3, 1))        # every k' = k / Gd <= min(VS)
LAM = 1.0
# The restatement's smallest key gap of every drawn sample.  score_out may differ from float64 by 2 ulp of the largest of
# |score_in|, |log p|, |score_out| (1 ulp for logf, half an ulp for the addition, doubled); the magnitudes here stay below
# 100 (score_in in [-10, 0], log p >= log 1e-30 = -69.1), where a float32 ulp is 7.6e-6: the 1e-3 gap is about 100 times
# the error a key can carry, so the device has to order the keys as the restatement does.
GAP = 1e-3
bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


# ---------------------------------------------------------------------------------------------------- the inputs
def _draw_sample(rng, V, k, gd):
    """one sample: float32 probs (k, V) whose rows resemble each other (so that without a penalty the groups choose alike),
    zero-probability columns, scores in [-10, 0], some finished beams (at most one of a group of several, never group 0's
    only beam), and an
    end_id among the likely tokens"""
    kp = k // gd
    base = 2.5 * rng.standard_normal(V)
    logit = base[None, :] + 0.7 * rng.standard_normal((k, V))
    p = np.exp(logit - logit.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    p[:, rng.random(V) < 0.2] = 0.0
    p[rng.random((k, V)) < 0.05] = 0.0
    score = (-10 * rng.random(k)).astype(np.float32)
    fin = np.zeros(k, np.int32)
    if kp > 1:
        for g in range(gd):
            if rng.random() < 0.5:
                fin[g * kp + rng.integers(kp)] = 1
    else:
        fin[1:][rng.random(k - 1) < 0.2] = 1
    end_id = int(np.argsort(-base)[1])
    return p, score, fin, end_id


@functools.lru_cache(maxsize=None)
def _case(V, B, k, gd):
    """B samples drawn (rejection sampling, fixed seeds) until the float64 restatement orders no two adjacent keys by less
    than GAP and, with more than one group, some group >= 1 chooses differently from its lambda = 0 choice.  Returns
    dict(probs (B*k, V) f32, score, fin, end_id, want: the restatement's outputs, gap (B,), nv_max)."""
    rng = np.random.default_rng(1000 * V + 100 * B + 10 * k + gd)
    probs, score, fin, want, gaps, nv_max = [], [], [], [], [], 0
    end_id = None
    while len(probs) < B:
        p, s, f, e = _draw_sample(rng, V, k, gd)
        e = end_id if end_id is not None else e          # one end_id per launch: the first sample's
        w = DO.diverse_step(p, s, f, gd, LAM, e)
        if w[4] < GAP:
            continue
        if gd > 1:
            w0 = DO.diverse_step(p, s, f, gd, 0.0, e)
            kp = k // gd
            if np.array_equal(w[1][kp:], w0[1][kp:]) and np.array_equal(w[2][kp:], w0[2][kp:]):
                continue
        end_id = e
        probs.append(p); score.append(s); fin.append(f); want.append(w[:4]); gaps.append(w[4]); nv_max = max(nv_max, w[5])
    cat = lambda i: np.concatenate([w[i] for w in want])
    parent = np.concatenate([w[1] + b * k for b, w in enumerate(want)])
    return dict(probs=np.concatenate(probs), score=np.concatenate(score), fin=np.concatenate(fin), end_id=end_id,
                want=(cat(0), parent, cat(2), cat(3)), gap=np.array(gaps), nv_max=nv_max)


def _dev_probs(p, ld):
    """(rows, ld) on the device, NaN in the pad columns [V, ld)"""
    x = torch.full((p.shape[0], ld), float("nan"), device="cuda")
    x[:, :p.shape[1]] = torch.as_tensor(p).cuda()
    return x


def _launch(be, probs, ld, score, fin, B, V, k, end_id, state=None, U=0, ldh=0, diverse=None):
    """one launch of tnt_beam_step_f32 (diverse None) or tnt_beam_step_diverse_f32 (diverse = (Gd, lambda)) into fresh
    sentinel-filled outputs -> (score_out, parent, token, fin_out, h_out, c_out) as numpy (the state None without one)"""
    Bk = B * k
    i32 = dict(dtype=torch.int32, device="cuda")
    so = torch.full((Bk,), 7.0, device="cuda")
    pa, to, fo = (torch.full((Bk,), -5, **i32) for _ in range(3))
    hi, ci = state if state is not None else (None, None)
    ho = torch.full_like(hi, -3.0) if hi is not None else None
    co = torch.full_like(ci, -3.0) if ci is not None else None
    args = (probs, ld, score, fin, B, V, k, end_id, so, pa, to, fo, hi, ci, ldh, U, ho, co)
    be.beam_step(*args) if diverse is None else be.beam_step_diverse(*args, *diverse)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (so, pa, to, fo, ho, co))


def _state(g, rows, ldh):
    return (torch.randn(rows, ldh, generator=g, device="cuda"), torch.randn(rows, ldh, generator=g, device="cuda"))


def _check_reorder(out, state, U):
    h, c = (t.cpu().numpy() for t in state)
    par = out[1]
    assert np.array_equal(bits(out[4][:, :U]), bits(h[par, :U])) and np.array_equal(bits(out[5][:, :U]), bits(c[par, :U]))
    assert (out[4][:, U:] == -3.0).all() and (out[5][:, U:] == -3.0).all()           # the row padding stays unwritten


# ---------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("k,gd", KG)
@pytest.mark.parametrize("V", VS)
def test_lambda0_and_one_group_equal_beam_step(be, V, k, gd):
    """lambda = 0 is tnt_beam_step_f32(B*Gd, k') on the same buffers; Gd = 1 is tnt_beam_step_f32(B, k) for any lambda"""
    g = torch.Generator(device="cuda")
    g.manual_seed(V * 31 + k * 7 + gd)
    ld, U, ldh = V + 3, 12, 13
    for B in BS:
        case = _case(V, B, k, gd)
        Bk = B * k
        for kind in ("drawn", "grid"):
            p = case["probs"]
            score = torch.as_tensor(case["score"]).cuda()
            if kind == "grid":                           # exact ties within and across the rows of a group
                p = np.round(p * 64).astype(np.float32) / 64
                p[1::2] = p[0::2][:p[1::2].shape[0]]
                score = torch.round(score)
            probs = _dev_probs(p, ld)
            fin = torch.as_tensor(case["fin"]).cuda()
            state = _state(g, Bk, ldh)
            for end_id in (-1, 0, case["end_id"]):
                ref = _launch(be, probs, ld, score, fin, B * gd, V, k // gd, end_id, state, U, ldh)
                got = _launch(be, probs, ld, score, fin, B, V, k, end_id, state, U, ldh, diverse=(gd, 0.0))
                for a, b in zip(ref, got):
                    assert np.array_equal(bits(a), bits(b)), (V, B, k, gd, kind, end_id)
                _check_reorder(got, state, U)
                ref = _launch(be, probs, ld, score, fin, B, V, k, end_id, state, U, ldh)
                got = _launch(be, probs, ld, score, fin, B, V, k, end_id, state, U, ldh, diverse=(1, 0.7))
                for a, b in zip(ref, got):
                    assert np.array_equal(bits(a), bits(b)), (V, B, k, kind, end_id)


def test_u0_leaves_the_state_untouched(be):
    V, B, k, gd = 257, 3, 6, 3
    case = _case(V, B, k, gd)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    state = _state(g, B * k, 16)
    probs = _dev_probs(case["probs"], V)
    score, fin = torch.as_tensor(case["score"]).cuda(), torch.as_tensor(case["fin"]).cuda()
    ref = _launch(be, probs, V, score, fin, B, V, k, case["end_id"], state, 16, 16, diverse=(gd, LAM))
    got = _launch(be, probs, V, score, fin, B, V, k, case["end_id"], state, 0, 16, diverse=(gd, LAM))
    for a, b in zip(ref[:4], got[:4]):
        assert np.array_equal(bits(a), bits(b))
    assert (got[4] == -3.0).all() and (got[5] == -3.0).all()
    _check_reorder(ref, state, 16)


# ---------------------------------------------------------------------------------------------------- lambda > 0
def test_some_case_counts_a_token_twice():
    assert max(_case(V, B, k, gd)["nv_max"] for V in VS for B in BS for k, gd in KG) >= 2


@pytest.mark.parametrize("k,gd", KG)
@pytest.mark.parametrize("V", VS)
def test_penalised_step_matches_the_restatement(be, V, k, gd):
    g = torch.Generator(device="cuda")
    g.manual_seed(V + k + gd)
    ld, U, ldh = V + 1, 8, 9
    for B in BS:
        case = _case(V, B, k, gd)
        assert case["gap"].min() >= GAP                      # the restatement alone, before the device is looked at
        p, s_in = case["probs"], case["score"]
        assert np.abs(s_in).max() <= 100
        state = _state(g, B * k, ldh)
        got = _launch(be, _dev_probs(p, ld), ld, torch.as_tensor(s_in).cuda(), torch.as_tensor(case["fin"]).cuda(), B, V, k,
                      case["end_id"], state, U, ldh, diverse=(gd, LAM))
        ws, wp, wt, wf = case["want"]
        assert np.array_equal(got[1], wp) and np.array_equal(got[2], wt), (V, B, k, gd)
        assert np.array_equal(got[3], wf.astype(np.int32))
        logp = np.log(np.maximum(p[wp, wt].astype(np.float64), 1e-30))
        live = case["fin"][wp] == 0
        mag = np.maximum(np.abs(s_in[wp].astype(np.float64)), np.maximum(np.where(live, np.abs(logp), 0), np.abs(ws)))
        tol = 2 * np.spacing(mag.astype(np.float32)).astype(np.float64)
        err = np.abs(got[0].astype(np.float64) - ws)
        print(f"V={V} B={B} k={k} Gd={gd}: gap {case['gap'].min():.2e}, worst score error {np.max(err / tol) * 2:.2f} ulp")
        assert np.all(err <= tol), (V, B, k, gd, float(np.max(err / tol)))
        assert np.array_equal(bits(got[0][~live]), bits(s_in[wp][~live]))      # a finished beam keeps its score's bits
        _check_reorder(got, state, U)


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    f = torch.full((4096,), 0.25, device="cuda")
    hs = [torch.zeros(64, 32, device="cuda") for _ in range(4)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    si, fi = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    outs = [torch.full((64,), 7.0, device="cuda")] + [torch.full((64,), -5, dtype=torch.int32, device="cuda") for _ in range(3)]
    so, pa, to, fo = outs

    def call(ld=8, B=2, V=8, k=4, score_out=so, fin_out=fo, h_in=hs[0], c_in=hs[1], ldh=32, U=32, h_out=hs[2], c_out=hs[3],
             groups=2, lam=0.5):
        return lib.tnt_beam_step_diverse_f32(p(f), ld, p(si), p(fi), B, V, k, -1, p(score_out), p(pa), p(to), p(fin_out),
                                             p(h_in), p(c_in), ldh, U, p(h_out), p(c_out), groups, lam, None)
    bad = [dict(B=0), dict(B=-1), dict(V=0), dict(k=0), dict(k=17, groups=1), dict(ld=7), dict(U=-1), dict(ldh=31),
           dict(score_out=si), dict(fin_out=fi), dict(h_out=hs[0]), dict(h_out=hs[1]), dict(c_out=hs[0]),
           dict(c_out=hs[1]), dict(h_out=hs[0][1:]), dict(h_in=None),
           dict(groups=0), dict(groups=-1), dict(groups=3), dict(k=6, groups=4), dict(groups=8),
           dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf"))]
    for kw in bad:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                   # TNT_BADARG
    torch.cuda.synchronize()
    assert bool((so == 7.0).all()) and all(bool((t == -5).all()) for t in (pa, to, fo))      # nothing was launched
    assert call() == 0
    # U = 0: the state pointers are not read, aliasing included
    assert call(U=0, h_out=hs[0], c_out=hs[1]) == 0
    torch.cuda.synchronize()
    assert bool((so[:8] != 7.0).all())


# ---------------------------------------------------------------------------------------------------- the models
T, K, GD, END, MLAM = 4, 6, 3, 2, 0.8
MN = 8                   # scans per model case
# scans of which the float64 searches on the sharpened fixture decide at least six of eight samples by more than MARGIN,
# for end_id in (-1, END) (found on the CPU; asserted on the restatement in the test)
SEED = {"dense": 0, "lc": 0}


def sharpened_case(kind):
    """(orc, ctor, kw, x, z, start): the tiny golden fixture with its output layer scaled so that the logits spread like a
    trained model's (std 2.5 over the vocabulary, the rule of test_gpu_beam._sharpen), the factor taken from the float64
    restatement's first decode step so that the case is the same on every machine; weights rounded to float32"""
    orc, ctor, kw = CO.golden_case(kind)
    x, z, start = CO.scans(1, MN, SEED[kind])
    p0, _ = CO.mix(orc.dec_logits(orc.dec_init(x, z, z), start), 1)
    f = 2.5 / np.log(np.maximum(p0, 1e-30)).std(-1).mean()
    for key in ("time_distributed_softmax/kernel", "time_distributed_softmax/bias"):
        orc.p[key] = (orc.p[key] * f).astype(np.float32).astype(np.float64)
    return orc, ctor, kw, x, z, start


def device_model(kind, **mkw):
    orc, ctor, kw, x, z, start = sharpened_case(kind)
    if kind == "dense":
        from masters_thesis_amd.nic import NIC
    else:
        from masters_thesis_amd.lc_nic import NIC
    model = NIC(*ctor, seed=11, **kw, **mkw)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return orc, model, x, z, start


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_models_match_the_float64_search(kind):
    from masters_thesis_amd.model_base import BeamDiversity
    orc, model, x, z, start = device_model(kind)
    kp = K // GD
    for end_id in (-1, END):
        want, wscore, margin = DO.diverse_beam(orc, x, z, z, start, T, K, GD, MLAM, end_id)
        ok = margin > MARGIN
        print(f"{kind} end_id={end_id}: {int((~ok).sum())} of {MN} samples within the {MARGIN} margin")
        assert ok.mean() >= 0.75                            # the restatement alone
        for lp in (0.0, 0.7):
            got, gscore = model.beam_search(x, z, z, start, T, beam_width=K, end_id=end_id, length_penalty=lp,
                                            diversity=BeamDiversity(GD, MLAM))
            ws, wk = want, wscore
            if lp > 0:                                      # within every group only
                parts = [length_normalise_ref(want[:, g * kp:(g + 1) * kp], wscore[:, g * kp:(g + 1) * kp].astype(np.float32),
                                              end_id, lp) for g in range(GD)]
                ws, wk = np.concatenate([a for a, _ in parts], axis=1), np.concatenate([b for _, b in parts], axis=1)
            assert got.shape == (MN, K, T) and gscore.shape == (MN, K) and gscore.dtype == np.float32
            if lp == 0:
                assert np.array_equal(got[ok], ws[ok]), (kind, end_id)
            else:       # a reorder decided by float32 scores: compare each group's set of results and the keys
                for b in np.flatnonzero(ok):
                    for g in range(GD):
                        sl = slice(g * kp, (g + 1) * kp)
                        assert sorted(map(tuple, got[b, sl])) == sorted(map(tuple, ws[b, sl])), (kind, end_id, b, g)
            assert np.abs(gscore[ok] - wk[ok]).max() <= 1e-4 * max(1.0, np.abs(wk[ok]).max())
        assert len({tuple(s) for s in got[ok][:, ::kp].reshape(-1, T)}) > ok.sum()     # the groups' best results differ
    model.check_device_errors()


def test_captured_replay_equals_eager():
    from masters_thesis_amd.model_base import BeamDiversity
    graph = device_model("dense", use_graph=True)[1]
    _, eager, x, z, start = device_model("dense", use_graph=False)
    d = BeamDiversity(GD, MLAM)
    outs = []
    for call in range(3):              # eager warm-up, capture + replay, replay
        a = graph.beam_search(x, z, z, start, T, beam_width=K, end_id=END, diversity=d)
        b = eager.beam_search(x, z, z, start, T, beam_width=K, end_id=END, diversity=d)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), call
        outs.append(a)
    assert np.array_equal(outs[1][0], outs[2][0]) and np.array_equal(bits(outs[1][1]), bits(outs[2][1]))
    assert isinstance(graph._graphs[("beam", MN, K, T, END, "diverse", GD, d.penalty)], torch.cuda.CUDAGraph)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_none_is_the_call_without_the_keyword(kind):
    from masters_thesis_amd.model_base import BeamDiversity
    _, model, x, z, start = device_model(kind)
    for _ in range(2):                  # eager, then the captured replay
        base = model.beam_search(x, z, z, start, T, beam_width=K, end_id=END)
    keys = set(model._graphs)
    for d in (None, BeamDiversity(1, 0.7)):
        got = model.beam_search(x, z, z, start, T, beam_width=K, end_id=END, diversity=d)
        assert np.array_equal(got[0], base[0]) and np.array_equal(bits(got[1]), bits(base[1]))
        assert set(model._graphs) == keys
