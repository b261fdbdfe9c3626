"""ridge.RidgeDecoder end to end on a real MI355X against the float64 restatement (tests/ridge_oracle.py), at (n, N, G) =
(130, 97, 24) -- fewer voxels than scans, which only the dual form handles -- and (200, 300, 24), on planted data
Y = X W* + noise.  Cases: the intercept on and off at a single alpha; five alphas chosen by cv = 4, by cv = 4 over groups of
three rows, and by a held-out set.

Predictions of 32 further rows match the oracle's to a relative Frobenius error of
    bound = (n + N) 2^-24 cond_2(Kc + alpha I)          cond_2 from eigvalsh of the oracle's centred Gram matrix, in the test
alpha_ equals the oracle's; the seeds are such that the oracle's best two cv_scores_ differ by more than 1e-3, asserted here.
semantic_identification ranks equal the oracle's on every row whose similarity margins exceed what the prediction bound can
move: a prediction row p_b moves by at most bound * ||P||_F, its cosine to any bank row by at most twice that over ||p_b||, and
a comparison of two cosines by twice that again, plus the float32 evaluation of the similarity itself (4 (G + 8) 2^-24 each,
tests/test_gpu_semantic.py): margin_b = 4 bound ||P||_F / ||p_b|| + 8 (G + 8) 2^-24.  At most 5 % of the rows may be left
out for a thinner margin.

Measured on an MI355X: prediction errors 1.4e-07 to 2.7e-07 at the single alpha (bounds 8.0e-05 and 7.7e-04), 2.5e-07 and
1.0e-06 at the selected alpha = 30 (bounds 6.8e-04 and 7.4e-03); no row left out in any case.
"""
import functools

import numpy as np
import pytest
import torch

import ridge_oracle as RO
from masters_thesis_amd import evaluate, ridge

gpu = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = [(130, 97, 24), (200, 300, 24)]
ALPHAS = [3e4, 30.0, 3e6, 1e3, 3e8]
ALPHA = 300.0
EXTRA, BANK = 32, 40
MODES = ["single", "no_intercept", "cv", "groups", "validation"]


@functools.lru_cache(maxsize=None)
def case(n, N, G, mode):
    """data, the constructor arguments and the oracle's model; computed once per case"""
    X, Y = RO.planted(n, N, G, 0.2, 7 * n + N, extra=2 * EXTRA)
    Xt, Yt, Xv, Yv, Xe, Ye = X[:n], Y[:n], X[n:n + EXTRA], Y[n:n + EXTRA], X[n + EXTRA:], Y[n + EXTRA:]
    intercept = mode != "no_intercept"
    if mode in ("single", "no_intercept"):
        kw = dict(alpha=ALPHA, fit_intercept=intercept)
        m = RO.fit(Xt, Yt, ALPHA, intercept)
    else:
        sel = dict(cv=4) if mode == "cv" else dict(cv=4, groups=(np.arange(n) // 3) * 5 % 97) if mode == "groups" else dict(
            validation=(Xv, Yv))
        kw = dict(alphas=ALPHAS, **sel)
        m = RO.fit_select(Xt, Yt, ALPHAS, **sel)
    ev = np.linalg.eigvalsh(m["Kc"] + m["alpha"] * np.eye(n))
    bound = (n + N) * U * ev[-1] / ev[0]
    return Xt, Yt, Xe, Ye, kw, m, bound


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,N,G", SHAPES, ids=lambda v: str(v))
def test_decoder_matches_the_oracle(n, N, G, mode):
    Xt, Yt, Xe, Ye, kw, m, bound = case(n, N, G, mode)
    r = ridge.RidgeDecoder(**kw).fit(Xt, Yt)
    if "alphas" in kw:
        top = np.sort(m["cv_scores"])
        assert top[-1] - top[-2] > 1e-3, "the oracle's best two scores are too close for alpha_ to be a test"
        assert r.alpha_ == m["alpha"]
        np.testing.assert_allclose(r.cv_scores_, m["cv_scores"], rtol=0, atol=1e-3)
    want = RO.predict(m, Xe)
    pe = r.predict_embedding(torch.as_tensor(Xe).cuda())
    assert pe.is_cuda and pe.dtype == torch.float32 and pe.shape == (EXTRA, G)
    got = r.predict(Xe)
    assert np.array_equal(got, pe.cpu().numpy())
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"n={n} N={N} {mode}: alpha {m['alpha']} prediction error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert tuple(r.coef_.shape) == (N, G) and tuple(r.intercept_.shape) == (G,) and tuple(r.dual_coef_.shape) == (n, G)

    # identification of the 32 further scans among their own embeddings and BANK distractors
    rows = np.concatenate([Ye, np.random.default_rng(5).standard_normal((BANK, G)).astype(np.float32)])
    own = [[b] for b in range(EXTRA)]
    res = evaluate.semantic_identification(r, Xe, evaluate.SemanticBank(rows), own)
    bn = rows.astype(np.float64)
    sims = (want / np.linalg.norm(want, axis=1, keepdims=True)) @ (bn / np.linalg.norm(bn, axis=1, keepdims=True)).T
    rank, best = evaluate.semantic_ranks(sims, own)
    margin = 4 * bound * np.linalg.norm(want) / np.linalg.norm(want, axis=1) + 8 * (G + 8) * U
    gap = np.abs(sims - best[:, None])
    gap[np.arange(EXTRA), np.arange(EXTRA)] = np.inf
    safe = gap.min(1) > margin
    print(f"rows left out for a thin margin: {(~safe).sum()} of {EXTRA}")
    assert (~safe).mean() <= 0.05
    assert np.array_equal(res["rank"][safe], rank[safe])
