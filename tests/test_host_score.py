"""Caption log-likelihood scoring on the CPU through a mock backend that follows tnt_caption_score_f32's header
definition: the float64 restatement against torch.log_softmax, score_captions of both caption models against the
float64 oracle (plain and with candidates, chunked and not), the masks, the encoder's row count, the evaluation helpers,
consistency with greedy decoding, and that scoring leaves training untouched."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate
from masters_thesis_amd.optimizers import Adam
from helpers import synth_batch
from score_oracle import (END, TINY, ScoreMockBackend, build_pair, caption_score, counted, ident_case, make_captions,
                          rank_margin_check, ranks, scans, score_model)

KINDS = ("dense", "attention")


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = ScoreMockBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def bound(want):
    """the project's model-level bound: 1e-4 * max(1, |logprob|)"""
    return 1e-4 * np.maximum(1.0, np.abs(want))


def case(kind, seed=3, C=None, end_id=END):
    rng = np.random.default_rng(seed)
    d = TINY[kind]
    model, orc = build_pair(kind, d, rng)
    x, a0, c0 = scans(rng, d)
    n = d["B"] * (C or 1)
    caps = make_captions(rng, n, d["T"], d["V"], end_id)
    caps = caps.reshape(d["B"], C, d["T"]) if C else caps
    return model, orc, d, (x, a0, c0), caps


def test_restatement_against_log_softmax():
    rng = np.random.default_rng(0)
    R, T, V = 12, 7, 11
    cap = make_captions(rng, R, T, V)
    x = rng.standard_normal((T - 1, R, V)) * 3
    tok, lp, ln = caption_score(x.reshape(-1, V), cap, END)
    ls = torch.log_softmax(torch.tensor(x), -1).numpy()
    for r in range(R):
        total, n, ended = 0.0, 0, False
        for j in range(1, T):
            w = cap[r, j]
            if not ended and w != 0:
                total += ls[j - 1, r, w]
                n += 1
                assert abs(tok[j - 1, r] - ls[j - 1, r, w]) < 1e-12
            else:
                assert tok[j - 1, r] == 0.0
            ended = ended or w == 0 or w == END
        assert abs(lp[r] - total) < 1e-12 and ln[r] == n
    assert ln.tolist()[:6] == [1, T // 2, T - 1, 1, 0, T - 1]       # the six mask kinds of make_captions
    assert lp[4] == 0.0
    # end_id = -1: up to the first 0; the id END is an ordinary token
    assert counted(np.array([[1, 5, END, 7, 0, 3]]), -1).tolist() == [[True, True, True, False, False]]
    # a counted id outside [0, V): NaN for that caption only
    bad = cap.copy()
    bad[2, 2] = V + 3
    _, lp_b, _ = caption_score(x.reshape(-1, V), bad, END)
    assert np.isnan(lp_b[2]) and np.array_equal(np.delete(lp_b, 2), np.delete(lp, 2))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("end_id", [END, -1])
def test_score_captions_matches_oracle(kind, end_id, mock_backend):
    model, orc, d, (x, a0, c0), caps = case(kind, end_id=end_id)
    mock_backend.input_width = d["N"]
    lp, ln, tok = model.score_captions(x, a0, c0, caps, end_id=end_id, return_tokens=True)
    want_lp, want_ln, want_tok = score_model(orc, x, a0, c0, caps, end_id)
    assert lp.shape == (d["B"],) and lp.dtype == np.float32 and ln.dtype == np.int32 and tok.shape == (d["B"], d["T"] - 1)
    assert np.array_equal(ln, want_ln)
    assert np.all(np.abs(lp - want_lp) <= bound(want_lp)), np.abs(lp - want_lp).max()
    assert np.all(np.abs(tok - want_tok) <= bound(want_tok))
    assert np.all(tok[want_tok == 0] == 0)
    assert np.allclose(tok.sum(1), lp, rtol=1e-6, atol=1e-6)
    lp2, ln2 = model.score_captions(x, a0, c0, caps, end_id=end_id)          # plain return, same values
    assert np.array_equal(lp2, lp) and np.array_equal(ln2, ln)
    mean, _ = model.score_captions(x, a0, c0, caps, end_id=end_id, normalise="mean")
    assert np.allclose(mean, lp / np.maximum(ln, 1), rtol=1e-6) and mean[ln == 0].tolist() == [0.0] * int((ln == 0).sum())


@pytest.mark.parametrize("kind", KINDS)
def test_candidates_match_oracle_and_the_encoder_sees_the_scans_only(kind, mock_backend):
    C = 7
    model, orc, d, (x, a0, c0), caps = case(kind, C=C)
    B = d["B"]
    mock_backend.input_width = d["N"]
    lp, ln, tok = model.score_captions(torch.from_numpy(x), a0, c0, torch.from_numpy(caps), end_id=END, return_tokens=True)
    want_lp, want_ln, want_tok = score_model(orc, x, a0, c0, caps, END)
    assert lp.shape == (B, C) and tok.shape == (B, C, d["T"] - 1)
    assert np.array_equal(ln, want_ln)
    assert np.all(np.abs(lp - want_lp) <= bound(want_lp))
    assert np.all(np.abs(tok - want_tok) <= bound(want_tok))
    assert mock_backend.score_rows == [B * C]
    rows_ok = {B} if kind == "dense" else {B, B * d["R"]}
    assert mock_backend.enc_rows and {r for _, r in mock_backend.enc_rows} <= rows_ok, mock_backend.enc_rows
    # chunked: 3 passes of 3, 3 and 1 candidates, over buffers for 3
    mock_backend.score_rows.clear()
    mock_backend.enc_rows.clear()
    lp_c, ln_c, tok_c = model.score_captions(x, a0, c0, caps, end_id=END, return_tokens=True, max_rows=3 * B + 1)
    assert mock_backend.score_rows == [3 * B, 3 * B, B]
    assert {r for _, r in mock_backend.enc_rows} <= rows_ok
    assert len([1 for n, _ in mock_backend.enc_rows if n in ("gemm", "locally_dense_fwd")]) == 1      # one encoder pass
    assert np.array_equal(ln_c, ln)
    assert np.all(np.abs(lp_c - lp) <= bound(want_lp)) and np.all(np.abs(tok_c - tok) <= bound(want_tok))
    assert np.all(np.abs(lp_c - want_lp) <= bound(want_lp))
    with pytest.raises(ValueError):
        model.score_captions(x, a0, c0, caps, end_id=END, max_rows=B - 1)


def test_bad_arguments_and_refusals():
    model, _, d, (x, a0, c0), caps = case("dense")
    for kw in (dict(normalise="sum"), dict(end_id=d["V"]), dict(end_id=0), dict(end_id=-2)):
        with pytest.raises(ValueError):
            model.score_captions(x, a0, c0, caps, **kw)
    with pytest.raises(ValueError):
        model.score_captions(x, a0, c0, caps.astype(np.float32))
    with pytest.raises(ValueError):
        model.score_captions(x, a0, c0, caps[:, :1])
    rng = np.random.default_rng(1)
    from masters_thesis_amd.lc_nic import NIC
    from helpers import tiny_groups
    da = TINY["attention"]
    g = (tiny_groups(da["N"], da["R"], rng), [da["D"]] * da["R"])
    m = NIC(g, da["U"], 512, da["Et"], da["A"], da["V"], da["T"], 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu",
            use_layer_norm=True)
    xa, aa, ca = scans(rng, da)
    with pytest.raises(NotImplementedError):
        m.score_captions(xa, aa, ca, make_captions(rng, da["B"], da["T"], da["V"]))


@pytest.mark.parametrize("kind", KINDS)
def test_perplexity_and_identification(kind):
    model, orc, d, (x, a0, c0), caps = case(kind, seed=5)
    caps[1] = caps[0]                                   # a duplicated caption in the batch
    B = d["B"]
    want_lp, want_ln, _ = score_model(orc, x, a0, c0, caps, END)
    ppl, lp, ln = evaluate.caption_perplexity(model, x, a0, c0, caps, END)
    assert np.array_equal(ln, want_ln)
    assert abs(ppl - np.exp(-want_lp.sum() / want_ln.sum())) <= 1e-4 * ppl
    cand = np.broadcast_to(caps[None], (B,) + caps.shape)
    want, _, _ = score_model(orc, x, a0, c0, cand, END)
    got = evaluate.identification(model, x, a0, c0, caps, END, max_rows=2 * B)
    assert got["scores"].shape == (B, B) and np.all(np.abs(got["scores"] - want) <= bound(want))
    mine = ranks(got["scores"].astype(np.float64), caps)              # numpy argsort of the same matrix
    assert np.array_equal(got["rank"], mine)
    assert abs(got["top1"] - (mine == 0).mean()) < 1e-12 and abs(got["mrr"] - (1.0 / (mine + 1)).mean()) < 1e-12
    # duplicates count once: scan 2's rank does not grow when candidates 0 and 1 are the same caption
    s = got["scores"]
    higher = {tuple(caps[c]) for c in range(B) if s[2, c] > s[2, 2]}
    assert got["rank"][2] == len(higher)
    norm = evaluate.identification(model, x, a0, c0, caps, END, normalise="mean")
    want_n = want / np.maximum(score_model(orc, x, a0, c0, cand, END)[1], 1)
    assert np.all(np.abs(norm["scores"] - want_n) <= bound(want_n))


@pytest.mark.parametrize("kind", KINDS)
def test_identification_ranks_at_the_small_shape(kind):
    """the ranking case of the GPU suite, on the mock: its float64 scores leave at most 2 % of the pairs inside the
    margin (so the seed is usable there), and the mock's ranks equal the float64 ranks outside it"""
    model, orc, (x, a0, c0), caps = ident_case(kind)
    B = len(caps)
    cand = np.broadcast_to(caps[None], (B,) + caps.shape)
    want, _, _ = score_model(orc, x, a0, c0, cand, END)
    checked, left, bad = rank_margin_check(want, want, caps)
    print(f"{kind}: {checked} pairs checked, {left} inside the margin")
    assert left <= 0.02 * (checked + left) and bad == 0
    got = evaluate.identification(model, x, a0, c0, caps, END)
    checked, left, bad = rank_margin_check(got["scores"], want, caps)
    assert bad == 0 and left <= 0.02 * (checked + left)
    if left == 0:
        assert np.array_equal(got["rank"], ranks(want, caps))


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_caption_scores_to_the_probabilities_greedy_predict_returned(kind):
    model, orc, d, (x, a0, c0), _ = case(kind, seed=9)
    B, L = d["B"], d["T"] - 1
    start = np.ones(B, np.int32)
    if kind == "dense":
        probs = model.greedy_predict(x, a0, c0, start, L)[:, :, 0, :]                  # (L, B, V)
        ids = probs.argmax(-1).T
        p_chosen = np.take_along_axis(probs, ids.T[..., None], 2)[..., 0].T
    else:
        words, probs, _, _ = model.greedy_predict(x, a0, c0, start, L)                 # (B, L, 1), (B, L, V)
        ids = words[:, :, 0]
        p_chosen = np.take_along_axis(probs, ids[..., None], 2)[..., 0]
    caps = np.concatenate([start[:, None], ids.astype(np.int32)], 1)
    _, ln, tok = model.score_captions(x, a0, c0, caps, end_id=-1, return_tokens=True)
    m = counted(caps, -1)
    assert m.any() and np.array_equal(ln, m.sum(1))
    want = np.log(p_chosen.astype(np.float64))
    assert np.all(np.abs(tok[m] - want[m]) <= bound(want[m]))


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_after_scoring_equals_train_step_without(kind):
    d = TINY[kind]
    out = []
    for score in (False, True):
        rng = np.random.default_rng(13)
        model, _ = build_pair(kind, d, rng)
        model.compile(Adam(1e-3, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
        x, a0, c0 = scans(rng, d)
        cand = make_captions(rng, d["B"] * 3, d["T"], d["V"]).reshape(d["B"], 3, d["T"])
        mets = []
        for step in range(3):
            data, tgt = synth_batch(d["B"], d["N"], d["T"], d["V"], d["U"], np.random.default_rng(100 + step))
            if score and step > 0:
                model.score_captions(x, a0, c0, cand, end_id=END, max_rows=2 * d["B"])
                model.score_captions(x[:3], a0[:3], c0[:3], cand[:3, 0, :4], end_id=END)       # another shape as well
            mets.append(model.train_step((data, tgt)).as_floats())
        out.append((mets, {k: model.get_weight(k) for k in model.trainable_names()}))
    (m0, w0), (m1, w1) = out
    assert m0 == m1
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
