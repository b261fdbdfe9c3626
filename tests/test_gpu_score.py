"""Caption log-likelihood scoring on the GPU: tnt_caption_score_f32 against the float64 restatement over the grid of
vocabularies, leading dimensions, layouts and rows that test_gpu_scst.py uses (plus a vocabulary for the generic path), with
NaN / 1e30 in the pad columns,
every terminator kind by row and the optional outputs on and off; score_captions of both caption models against the
float64 oracle at a small shape and at the BASELINE shape; ranking; captured replay; and training after scoring."""
import numpy as np
import pytest
import torch

from helpers import synth_batch
from test_gpu_head import fill_pad, layouts
from score_oracle import (END, SMALL, build_pair, caption_score, ident_case, make_captions, rank_margin_check, ranks, scans,
                          score_model)

pytestmark = pytest.mark.gpu
KINDS = ("dense", "attention")


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bound(want):
    return 1e-4 * np.maximum(1.0, np.abs(want))


def launch(be, x, ld, V, cap, steps, end_id, tok_on=True, len_on=True, shift=0):
    R, T = cap.shape
    tok = torch.full((steps * R,), -9.0, device="cuda") if tok_on else None
    lp = torch.full((R,), -9.0, device="cuda")
    ln = torch.full((R,), -9, dtype=torch.int32, device="cuda") if len_on else None
    buf = torch.full((shift + x.size,), -7.0, device="cuda")                            # the view starts `shift` floats in
    logits = buf[shift:].view(x.shape)
    logits.copy_(dev(x))
    be.caption_score(logits, ld, V, dev(cap), T, steps, R, end_id, tok, lp, ln)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), x, equal_nan=True)                       # read-only
    return (tok.cpu().numpy() if tok_on else None), lp.cpu().numpy(), (ln.cpu().numpy() if len_on else None)


# both sides of every bound of the kernel ladder (tnt_row_ladder, csrc/tnt_rowhead.h): every caption_score_row_kernel<NV4> and
# caption_score_cap_kernel<NV4> and, in the "odd" and "shift" layouts, their re-reading forms at the same V
LADDER_V = (1024, 1025, 2048, 2049, 4096, 4097, 5120, 5121, 8192, 8193)
# (R, V, ld, float offset of the logits view); the ids of the first group are those of the former (V, ld) x R grid
KERNEL_CASES = [pytest.param(R, V, ld, 0, id=f"{R}-{V}-{ld}") for R in (6, 64, 320)
                for V, ld in ((13, 16), (13, 16 + 3), (5001, 5004), (5001, 5001 + 7), (5001, 5012), (9000, 9000))]
KERNEL_CASES += [pytest.param(6, V, ld, shift, id=f"6-{V}-{name}") for V in LADDER_V for name, ld, shift in layouts(V)]


@pytest.mark.parametrize("R,V,ld,shift", KERNEL_CASES)
def test_kernel_matches_float64(be, R, V, ld, shift):
    rng = np.random.default_rng(V + R + ld + shift)
    T = 6
    for end_id, steps in ((END, T - 1), (-1, T - 1), (END, 3)):
        cap = make_captions(rng, R, T, V, end_id)
        x = (rng.standard_normal((steps * R, ld)) * 3).astype(np.float32)
        want_tok, want_lp, want_len = caption_score(x[:, :V].astype(np.float64), cap, end_id, steps)
        fill_pad(x, V)                                       # pad columns: NaN / 1e30 would swamp any row that used them
        x[(want_tok == 0).reshape(-1)] = np.nan              # rows that do not count: never read
        outs = []
        for tok_on, len_on in ((True, True), (False, True), (True, False), (False, False)):
            tok, lp, ln = launch(be, x, ld, V, cap, steps, end_id, tok_on, len_on, shift)
            if tok_on:
                assert np.allclose(tok, want_tok.reshape(-1), rtol=1e-5, atol=1e-5)
                assert np.all(tok[(want_tok == 0).reshape(-1)] == 0.0)
            assert np.all(np.abs(lp - want_lp) <= 1e-5 * steps), np.abs(lp - want_lp).max()
            if len_on:
                assert np.array_equal(ln, want_len)
            outs.append(lp)
        for lp in outs[1:]:                                  # with or without tok_lp, run to run: the same bits
            assert np.array_equal(lp, outs[0])
        assert np.array_equal(launch(be, x, ld, V, cap, steps, end_id, shift=shift)[1], outs[0])
        assert 0 < (want_tok != 0).sum() < want_tok.size


def test_kernel_bad_id_gives_nan_for_that_caption_only(be):
    rng = np.random.default_rng(3)
    R, T, V, ld = 12, 6, 5001, 5004
    cap = make_captions(rng, R, T, V)
    x = (rng.standard_normal(((T - 1) * R, ld)) * 3).astype(np.float32)
    _, good, _ = launch(be, x, ld, V, cap, T - 1, END)
    for bad_id in (V, V + 100000, -7):
        c = cap.copy()
        c[2, 2] = bad_id
        c[7, 4] = bad_id                                     # row 7 ends at position 3: the bad id is not counted
        for tok_on in (True, False):
            tok, lp, ln = launch(be, x, ld, V, c, T - 1, END, tok_on)
            assert np.isnan(lp[2]) and np.array_equal(np.delete(lp, 2), np.delete(good, 2))
            if tok_on:
                assert np.isnan(tok.reshape(T - 1, R)[1, 2]) and np.isnan(tok).sum() == 1


def test_kernel_bad_arguments(be):
    from masters_thesis_amd._lib import KernelLibraryError
    R, T, V, ld = 4, 5, 13, 16
    x, cap = torch.zeros((T - 1) * R, ld, device="cuda"), torch.ones(R, T, dtype=torch.int32, device="cuda")
    lp = torch.zeros(R, device="cuda")
    ok = dict(logits=x, ld=ld, V=V, cap=cap, T=T, steps=T - 1, R=R, end_id=END, tok_lp=None, cap_lp=lp, cap_len=None)
    be.caption_score(**ok)
    for bad in (dict(ld=V - 1), dict(end_id=V), dict(logits=None), dict(cap=None), dict(cap_lp=None), dict(steps=0),
                dict(steps=T), dict(V=0), dict(R=0), dict(T=1, steps=1)):
        with pytest.raises(KernelLibraryError):
            be.caption_score(**{**ok, **bad})
    torch.cuda.synchronize()


def _model_case(kind, d, seed=3, C=None, **kw):
    rng = np.random.default_rng(seed)
    model, orc = build_pair(kind, d, rng, "cuda:0", **kw)
    x, a0, c0 = scans(rng, d)
    caps = make_captions(rng, d["B"] * (C or 1), d["T"], d["V"])
    return model, orc, (x, a0, c0), caps.reshape(d["B"], C, d["T"]) if C else caps


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [None, 3])
def test_models_match_oracle_at_the_small_shape(kind, C):
    model, orc, (x, a0, c0), caps = _model_case(kind, SMALL[kind], C=C)
    want_lp, want_len, want_tok = score_model(orc, x, a0, c0, caps, END)
    for call in range(3):                                    # eager, capture, replay
        lp, ln, tok = model.score_captions(x, a0, c0, caps, end_id=END, return_tokens=True)
        err = np.abs(lp - want_lp)
        print(kind, C, call, "max |logprob error| / bound", (err / bound(want_lp)).max())
        assert np.array_equal(ln, want_len) and np.all(err <= bound(want_lp))
        assert np.all(np.abs(tok - want_tok) <= bound(want_tok))
    model.check_device_errors()


def _baseline(kind):
    from test_gpu_fullsize import make, make_oracle
    return make(kind), make_oracle(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [None, 3])
def test_models_match_oracle_at_the_baseline_shape(kind, C):
    from test_gpu_fullsize import B, N, T, U, V
    model, orc = _baseline(kind)
    rng = np.random.default_rng(17)
    orc.init_params(rng)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    x = rng.standard_normal((B, N)).astype(np.float32)
    a0 = np.zeros((B, U), np.float32)
    caps = make_captions(rng, B * (C or 1), T, V)
    caps = caps.reshape(B, C, T) if C else caps
    nb = 8                                                   # the float64 oracle scores the first scans only
    want_lp, want_len, _ = score_model(orc, x[:nb], a0[:nb], a0[:nb], caps[:nb], END)
    for call in range(3):
        lp, ln = model.score_captions(x, a0, a0, caps, end_id=END)
        err = np.abs(lp[:nb] - want_lp)
        print(kind, C, call, "max |logprob error| / bound", (err / bound(want_lp)).max())
        assert np.array_equal(ln[:nb], want_len) and np.all(err <= bound(want_lp))
    model.check_device_errors()


@pytest.mark.parametrize("kind", KINDS)
def test_identification_ranks_against_float64(kind):
    from masters_thesis_amd import evaluate
    model, orc, (x, a0, c0), caps = ident_case(kind, "cuda:0")
    B = len(caps)
    want, _, _ = score_model(orc, x, a0, c0, np.broadcast_to(caps[None], (B,) + caps.shape), END)
    got = evaluate.identification(model, x, a0, c0, caps, END, max_rows=3 * B)
    checked, left, bad = rank_margin_check(got["scores"], want, caps)
    print(f"{kind}: {checked} pairs checked, {left} inside the margin and left out, {bad} out of order")
    assert bad == 0
    assert left <= 0.02 * (checked + left)
    if left == 0:
        assert np.array_equal(got["rank"], ranks(want, caps))


@pytest.mark.parametrize("kind", KINDS)
def test_captured_replay_equals_the_eager_sequence(kind):
    d = SMALL[kind]
    model, orc, (x, a0, c0), caps = _model_case(kind, d, C=5)
    eager, _, _, _ = _model_case(kind, d, C=5, use_graph=False)
    other = make_captions(np.random.default_rng(99), d["B"] * 5, d["T"], d["V"]).reshape(caps.shape)[:, ::-1].copy()
    want = [eager.score_captions(x, a0, c0, c, end_id=END, return_tokens=True, max_rows=2 * d["B"]) for c in (caps, other)]
    for call in range(4):                                    # eager, capture, replay, replay with other captions
        c, w = (other, want[1]) if call == 3 else (caps, want[0])
        got = model.score_captions(x, a0, c0, c, end_id=END, return_tokens=True, max_rows=2 * d["B"])
        for g, e in zip(got, w):
            assert np.array_equal(g, e), call
    assert any(isinstance(k, tuple) and k[0] == "score" and not isinstance(g, str) for k, g in model._graphs.items())
    assert not np.array_equal(want[0][0], want[1][0])
    want_lp, _, _ = score_model(orc, x, a0, c0, other, END)
    assert np.all(np.abs(want[1][0] - want_lp) <= bound(want_lp))


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_after_scoring_equals_a_twin_that_never_scored(kind):
    from masters_thesis_amd.optimizers import Adam
    d = SMALL[kind]
    out = []
    for score in (False, True):
        rng = np.random.default_rng(13)
        model, _ = build_pair(kind, d, rng, "cuda:0")
        model.compile(Adam(1e-3, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        x, a0, c0 = scans(rng, d)
        cand = make_captions(rng, d["B"] * 3, d["T"], d["V"]).reshape(d["B"], 3, d["T"])
        mets = []
        for step in range(4):
            data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], np.random.default_rng(100 + step))
            if score and step > 0:
                model.score_captions(x, a0, c0, cand, end_id=END, max_rows=2 * d["B"])
            mets.append(model.train_step((data, tgt)).as_floats())
        out.append((mets, {k: model.get_weight(k) for k in model.trainable_names()}))
    (m0, w0), (m1, w1) = out
    assert m0 == m1
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
