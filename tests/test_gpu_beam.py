"""Beam search on the GPU: tnt_beam_step_f32 against tnt_beam_topk_f32 bit for bit over a grid of shapes with planted
ties, zero probabilities and finished beams; its reorder of the state; nic.NIC.beam_search against the float64
restatement (tests/dense_beam_oracle.py) at a small shape and at the config-2 shape; captured replay against eager
decoding; and no effect of a beam search on a following greedy_predict or train_step."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import synth_batch
from dense_beam_oracle import BeamNICDense

pytestmark = pytest.mark.gpu

MARGIN = 1e-4


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def _probs(g, rows, V, ld, kind):
    """float32 rows (rows, ld) in [0, 1): plain, quantised to a coarse grid (exact ties everywhere, and values that
    logf and the score addition merge), or with zero-probability columns; the padding columns are NaN"""
    p = torch.rand(rows, V, generator=g, device="cuda")
    if kind == "grid":
        p = torch.round(p * 8) / 8
    elif kind == "zeros":
        p = torch.where(torch.rand(rows, V, generator=g, device="cuda") < 0.4, torch.zeros_like(p), p)
    x = torch.full((rows, ld), float("nan"), device="cuda")
    x[:, :V] = p
    return x


def _run_both(be, probs, ld, score, fin, B, V, k, end_id, h=None, U=0, ldh=0):
    Bk = B * k
    i32 = dict(dtype=torch.int32, device="cuda")
    outs = []
    for fused in (False, True):
        so = torch.full((Bk,), 7.0, device="cuda")
        pa, to, fo = torch.full((Bk,), -5, **i32), torch.full((Bk,), -5, **i32), torch.full((Bk,), -5, **i32)
        if fused:
            hi, ci = h if h is not None else (None, None)
            ho = torch.full_like(hi, -3.0) if hi is not None else None
            co = torch.full_like(ci, -3.0) if ci is not None else None
            be.beam_step(probs, ld, score, fin, B, V, k, end_id, so, pa, to, fo, hi, ci, ldh, U, ho, co)
            outs.append((so, pa, to, fo, ho, co))
        else:
            be.beam_topk(probs, score, fin, B, V, ld, k, end_id, so, pa, to, fo)
            outs.append((so, pa, to, fo))
    torch.cuda.synchronize()
    return outs


def _same(ref, got):
    so, pa, to, fo = (t.cpu().numpy() for t in ref)
    gs, gp, gt, gf = (t.cpu().numpy() for t in got[:4])
    assert np.array_equal(so.view(np.int32), gs.view(np.int32))
    assert np.array_equal(pa, gp) and np.array_equal(to, gt) and np.array_equal(fo, gf)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("V", [1, 2, 13, 257, 5001, 16384, 40000])
def test_expansion_equals_beam_topk(be, V, k):
    g = torch.Generator(device="cuda")
    g.manual_seed(V * 31 + k)
    ld = V + 3
    cases = 0
    for B in (1, 7, 64):
        Bk = B * k
        for kind in ("plain", "grid", "zeros"):
            probs = _probs(g, Bk, V, ld, kind)
            score = -10 * torch.rand(Bk, generator=g, device="cuda")
            fin = torch.zeros(Bk, dtype=torch.int32, device="cuda")
            if kind == "grid":
                score = torch.round(score)                      # equal scores across beams
                if V > 3:                                       # equal probabilities within a row ...
                    probs[:, 1:V:3] = probs[:, :1]
                if k > 1:                                       # ... and across rows of a sample
                    probs.view(B, k, ld)[:, 1] = probs.view(B, k, ld)[:, 0]
                    score.view(B, k)[:, 1] = score.view(B, k)[:, 0]
            ref, _ = _run_both(be, probs, ld, score, fin, B, V, k, -1)
            emitted = int(ref[2][0].item())
            for end_id in (-1, 0, emitted):
                for fin_kind in ("none", "some", "step0"):
                    f, s = fin, score
                    if fin_kind == "some":
                        f = (torch.rand(Bk, generator=g, device="cuda") < 0.4).to(torch.int32)
                    elif fin_kind == "step0":                   # the k copies of step 0: only beam 0 counts
                        s = score.clone()
                        s.view(B, k)[:, 1:] = -1e30
                    ref, got = _run_both(be, probs, ld, s, f, B, V, k, end_id)
                    _same(ref, got)
                    cases += 1
    print(f"V={V} k={k}: {cases} cases bit-identical")


@pytest.mark.parametrize("U,ldh", [(512, 512), (512, 520), (13, 15), (16, 17)])
def test_reorder_is_the_row_gather(be, U, ldh):
    g = torch.Generator(device="cuda")
    g.manual_seed(U + ldh)
    for B, k, V in ((7, 5, 257), (64, 16, 13), (3, 1, 40)):
        Bk = B * k
        probs = _probs(g, Bk, V, V, "plain")
        score = -10 * torch.rand(Bk, generator=g, device="cuda")
        fin = (torch.rand(Bk, generator=g, device="cuda") < 0.3).to(torch.int32)
        h = torch.randn(Bk, ldh, generator=g, device="cuda")
        c = torch.randn(Bk, ldh, generator=g, device="cuda")
        ref, got = _run_both(be, probs, V, score, fin, B, V, k, 2, (h, c), U, ldh)
        _same(ref, got)
        par = ref[1].long()
        if k > 1:                                                           # the gather really moves rows
            assert not torch.equal(par, torch.arange(Bk, device="cuda"))
        ho, co = got[4], got[5]
        assert torch.equal(ho[:, :U], h[par, :U]) and torch.equal(co[:, :U], c[par, :U])
        assert bool((ho[:, U:] == -3.0).all()) and bool((co[:, U:] == -3.0).all())   # the row padding is not written


def test_u0_leaves_the_state_untouched(be):
    B, k, V, U = 5, 3, 29, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    probs = _probs(g, B * k, V, V, "plain")
    score = -torch.rand(B * k, generator=g, device="cuda")
    fin = torch.zeros(B * k, dtype=torch.int32, device="cuda")
    h = torch.randn(B * k, U, generator=g, device="cuda")
    ref, got = _run_both(be, probs, V, score, fin, B, V, k, -1, (h, h.clone()), 0, U)
    _same(ref, got)
    assert bool((got[4] == -3.0).all()) and bool((got[5] == -3.0).all())


def test_bad_arguments_return_badarg():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    f = torch.zeros(4096, device="cuda")
    i = torch.zeros(4096, dtype=torch.int32, device="cuda")
    hs = [torch.zeros(64, 32, device="cuda") for _ in range(4)]
    p = lambda t: C.c_void_p(t.data_ptr())
    so, si = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    fo, fi = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")

    def call(ld=8, B=2, V=8, k=2, score_out=so, fin_out=fo, h_in=hs[0], c_in=hs[1], ldh=32, U=32, h_out=hs[2],
             c_out=hs[3]):
        return lib.tnt_beam_step_f32(p(f), ld, p(si), p(fi), B, V, k, -1, p(score_out), p(i), p(i), p(fin_out),
                                     p(h_in), p(c_in), ldh, U, p(h_out), p(c_out), None)
    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(B=0), dict(B=-1), dict(V=0), dict(k=0), dict(k=17), dict(ld=7), dict(U=-1), dict(ldh=31),
           dict(score_out=si), dict(fin_out=fi), dict(h_out=hs[0]), dict(h_out=hs[1]), dict(c_out=hs[0]),
           dict(c_out=hs[1]), dict(h_out=hs[0][1:])]
    for kw in bad:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                   # TNT_BADARG
    # U = 0: the state pointers are not read, aliasing included
    assert call(U=0, h_out=hs[0], c_out=hs[1]) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the model
B0, T0, V0, U0, E0, N0 = 64, 15, 5001, 512, 512, 20000


def _sharpen(model, p0):
    """scale the output layer so that the logits spread like a trained model's (std 2.5 over the vocabulary) instead of
    the near-uniform distribution of the initial weights, where nearly every beam decision is a near tie"""
    f = 2.5 / np.log(np.maximum(p0, 1e-30)).std(-1).mean()
    for key in ("time_distributed_softmax/kernel", "time_distributed_softmax/bias"):
        model.set_weight(key, model.get_weight(key) * f)


def _emitted(probs):
    g = probs[1:, :, 0, :].argmax(-1).reshape(-1)
    ids, n = np.unique(g[g != 0], return_counts=True)
    return int(ids[n.argmax()])


def _model_case(shape):
    from masters_thesis_amd.nic import NIC
    if shape == "small":
        B, N, T, V, U, E = 16, 23, 6, 13, 16, 10
    else:
        B, N, T, V, U, E = B0, N0, T0, V0, U0, E0
    model = NIC(N, U, E, V, T, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5, seed=42)
    rng = np.random.default_rng(61)
    x = rng.standard_normal((B, N)).astype(np.float32)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    _sharpen(model, model.greedy_predict(x, z, z, start, 1)[0, :, 0])
    orc = BeamNICDense(N, U, E, V, T, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5)
    orc.p = {key: v.astype(np.float64) for key, v in model.get_weights_dict().items()}
    return model, orc, x, z, start, T


@pytest.mark.parametrize("shape", ["small", "config2"])
def test_model_matches_restatement(shape):
    model, orc, x, z, start, T = _model_case(shape)
    eid = _emitted(model.greedy_predict(x, z, z, start, T))
    for k in (1, 3, 5):
        for end_id in (-1, eid):
            want, wscore, margin = orc.beam_search(x, z, z, start, T, k=k, end_id=end_id)
            got, gscore = model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id)
            ok = margin > MARGIN
            print(f"{shape} k={k} end_id={end_id}: {int((~ok).sum())} of {len(ok)} samples within the {MARGIN} margin")
            assert ok.mean() >= 0.5
            assert np.array_equal(got[ok], want[ok]), (shape, k, end_id)
            assert np.abs(gscore[ok] - wscore[ok]).max() <= 1e-4 * max(1.0, np.abs(wscore[ok]).max())
            if end_id >= 0 and k > 1:
                hit = got == end_id
                first = np.where(hit.any(2), hit.argmax(2), T)
                assert np.all(got[np.arange(T)[None, None, :] > first[:, :, None]] == 0)


def test_captured_replay_equals_eager():
    from masters_thesis_amd.nic import NIC
    rng = np.random.default_rng(62)
    B, N, T, V, U, E = 8, 23, 6, 13, 16, 10
    graph, eager = (NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, seed=9, use_graph=ug) for ug in (True, False))
    for key, v in eager.get_weights_dict().items():
        graph.set_weight(key, v)
    x = rng.standard_normal((B, N)).astype(np.float32)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    outs = []
    for call in range(3):              # eager warm-up, capture + replay, replay
        a = graph.beam_search(x, z, z, start, T, beam_width=4, end_id=5)
        b = eager.beam_search(x, z, z, start, T, beam_width=4, end_id=5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), call
        outs.append(a)
    assert np.array_equal(outs[1][0], outs[2][0]) and np.array_equal(outs[1][1].view(np.int32), outs[2][1].view(np.int32))
    assert isinstance(graph._graphs[("beam", B, 4, T, 5)], torch.cuda.CUDAGraph)


@pytest.mark.parametrize("shape", ["small", "config2"])
def test_no_side_effects(shape):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    if shape == "small":
        B, N, T, V, U, E = 8, 23, 6, 13, 16, 16
    else:
        B, N, T, V, U, E = B0, N0, T0, V0, U0, E0
    rng = np.random.default_rng(63)
    data, tgt = synth_batch(B, N, T, V, U, rng)
    x, z = data[0], data[2]
    start = np.ones(B, np.int64)
    runs = []
    for interleave in (False, True):
        model = NIC(N, U, E, V, T, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5, seed=42)
        model.compile(Adam(1e-3, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        beam = (lambda: model.beam_search(x, z, z, start, T, beam_width=5, end_id=2)) if interleave else (lambda: None)
        out = []
        beam()
        out.append(model.greedy_predict(x, z, z, start, T))
        beam()
        out.append(model.train_step((data, tgt)).as_floats()["loss"])
        beam()
        out.append(model.greedy_predict(x, z, z, start, T))
        out.extend(model.get_weight(key) for key in ("dense_img/kernel", "lstm/kernel", "time_distributed_softmax/kernel"))
        model.check_device_errors()
        runs.append(out)
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
