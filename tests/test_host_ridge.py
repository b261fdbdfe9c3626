"""ridge.RidgeDecoder on the CPU through a mock backend that follows the header text of tnt_cholesky_f32 /
tnt_cholesky_solve_f32 / tnt_gram_center_f32 (tests/ridge_mock.py), against the float64 restatement (tests/ridge_oracle.py):
fit, predict and the selection of alpha by folds, by groups and by a held-out set under both scores; the Gram matrix computed
once per fit however many folds and alphas there are; groups kept whole; every refusal; RidgeError on a nonzero status;
evaluate.semantic_identification on a decoder; ridge.stack on the synthetic generator."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import evaluate, ridge
from masters_thesis_amd.data import SyntheticGenerator
import ridge_oracle as RO
from ridge_mock import RidgeMockBackend

ALPHAS = [0.01, 1.0, 30.0, 1000.0, 1e5]


class Counting(RidgeMockBackend):
    def __init__(self):
        super().__init__()
        self.products, self.factorisations = [], 0

    def gemm(self, A, B, C, M, N, K, *a, **k):
        self.products.append((M, N, K))
        return super().gemm(A, B, C, M, N, K, *a, **k)

    def cholesky(self, *a, **k):
        self.factorisations += 1
        return super().cholesky(*a, **k)


@pytest.fixture(autouse=True)
def be():
    old = ops._backend
    b = Counting()
    ops.set_backend(b)
    yield b
    ops.set_backend(old)


def close(got, want, tol=2e-4):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == np.shape(want)
    assert np.linalg.norm(got - want) <= tol * max(np.linalg.norm(want), 1e-30), np.linalg.norm(got - want) / np.linalg.norm(want)


@pytest.mark.parametrize("n,N,G", [(37, 21, 5), (30, 52, 8)])
@pytest.mark.parametrize("intercept", [True, False])
def test_fit_and_predict_match_the_oracle(n, N, G, intercept):
    X, Y = RO.planted(n, N, G, 0.1, 3, extra=9)
    m = RO.fit(X[:n], Y[:n], 3.0, intercept)
    r = ridge.RidgeDecoder(alpha=3.0, fit_intercept=intercept, device="cpu").fit(X[:n], Y[:n])
    assert r.alpha_ == 3.0 and r.cv_scores_ is None
    close(r.coef_, m["coef"])
    close(r.intercept_, m["intercept"])
    close(r.dual_coef_, m["dual"])
    p = r.predict(X[n:])
    assert isinstance(p, np.ndarray) and p.dtype == np.float32
    close(p, RO.predict(m, X[n:]))
    e = r.predict_embedding(torch.as_tensor(X[n:]))
    assert isinstance(e, torch.Tensor) and e.shape == (9, G) and np.array_equal(e.numpy(), p)


@pytest.mark.parametrize("score", ["cosine", "r2"])
@pytest.mark.parametrize("how", ["cv", "groups", "validation"])
def test_selection_matches_the_oracle_and_takes_one_gram(how, score, be):
    n, N, G = 46, 24, 6
    X, Y = RO.planted(n, N, G, 0.8, 11, extra=14)
    kw = dict(cv=4) if how == "cv" else dict(cv=3, groups=np.arange(n) // 3 * 7 % 31) if how == "groups" else dict(
        validation=(X[n:], Y[n:]))
    m = RO.fit_select(X[:n], Y[:n], ALPHAS, score=score, **kw)
    top = np.sort(m["cv_scores"])
    assert top[-1] - top[-2] > 1e-3, "the oracle's best two scores must be apart for the choice to be a test"
    r = ridge.RidgeDecoder(alphas=ALPHAS, score=score, device="cpu", **kw).fit(X[:n], Y[:n])
    over_voxels = [p for p in be.products if p[2] == N]
    assert r.alpha_ == m["alpha"]
    assert r.cv_scores_.shape == (len(ALPHAS),)
    np.testing.assert_allclose(r.cv_scores_, m["cv_scores"], rtol=0, atol=5e-4)
    close(r.coef_, m["coef"])
    close(r.predict(X[n:]), RO.predict(m, X[n:]))
    # products over the voxels (K = N): the training Gram once, the cross-Gram of a held-out set, the coefficients (K = n)
    assert over_voxels == [(n, n, N)] + ([(14, n, N)] if how == "validation" else [])
    nsplit = 1 if how == "validation" else kw["cv"]
    assert be.factorisations == nsplit * len(ALPHAS) + 1


def test_first_maximiser_wins_in_the_order_given():
    n, N, G = 30, 12, 4
    X, Y = RO.planted(n, N, G, 0.5, 5)
    r = ridge.RidgeDecoder(alphas=[7.0, 7.0, 7.0], cv=3, device="cpu").fit(X, Y)
    assert r.alpha_ == 7.0 and np.ptp(r.cv_scores_) == 0.0
    order = [1e5, 30.0, 0.01, 1.0]
    m = RO.fit_select(X, Y, order, cv=3)
    assert ridge.RidgeDecoder(alphas=order, cv=3, device="cpu").fit(X, Y).alpha_ == m["alpha"]


def test_folds_follow_kfold_sizes_and_keep_groups_whole():
    assert np.array_equal(ridge.kfold(10, 3), [0, 0, 0, 0, 1, 1, 1, 2, 2, 2])
    assert np.array_equal(ridge.kfold(10, 3), RO.kfold(10, 3))
    groups = np.array([50, 50, 50, 7, 7, 7, 21, 21, 21, 3, 3, 3, 90, 90])
    fold = ridge.kfold(len(groups), 3, groups)
    assert np.array_equal(fold, RO.kfold(len(groups), 3, groups))
    for g in np.unique(groups):
        assert np.unique(fold[groups == g]).size == 1
    assert np.array_equal(fold, [0, 0, 0, 1, 1, 1, 2, 2, 2, 0, 0, 0, 1, 1])      # ranks: 3 -> 0, 7 -> 1, 21 -> 2, 50 -> 3, 90 -> 4


def test_refusals():
    X, Y = RO.planted(12, 7, 3, 0.1, 0)
    R = ridge.RidgeDecoder
    for bad in (0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError):
            R(alpha=bad)
        with pytest.raises(ValueError):
            R(alphas=[1.0, bad], cv=2)
    with pytest.raises(ValueError):
        R(alphas=[], cv=2)
    with pytest.raises(ValueError):
        R(score="mse")
    for cv in (1, 0, 2.5, True):
        with pytest.raises(ValueError):
            R(alphas=[1.0], cv=cv)
    with pytest.raises(ValueError):
        R(alphas=[1.0], cv=13).fit(X, Y)                                   # cv > n
    with pytest.raises(ValueError):
        R(alphas=[1.0])                                                    # nothing to choose by
    with pytest.raises(ValueError):
        R(alphas=[1.0], cv=2, validation=(X, Y))                           # both
    with pytest.raises(ValueError):
        R(alphas=[1.0], groups=np.arange(12), validation=(X, Y))           # groups without cv
    with pytest.raises(ValueError):
        R(cv=2)                                                            # cv without alphas
    with pytest.raises(ValueError):
        R(validation=(X, Y))
    with pytest.raises(ValueError):
        R(groups=np.arange(12))
    with pytest.raises(ValueError):
        R(alphas=[1.0], validation=(X,))
    with pytest.raises(ValueError):
        R(device="cpu").fit(X, Y[:11])                                     # row counts
    with pytest.raises(ValueError):
        R(device="cpu").fit(X[:1], Y[:1])                                  # n < 2
    with pytest.raises(ValueError):
        R(device="cpu").fit(torch.zeros(32769, 1), torch.zeros(32769, 1))  # n > 32768
    with pytest.raises(ValueError):
        R(alphas=[1.0], cv=2, groups=np.arange(11), device="cpu").fit(X, Y)
    with pytest.raises(ValueError):
        R(alphas=[1.0], cv=3, groups=np.arange(12) % 2, device="cpu").fit(X, Y)     # an empty fold
    with pytest.raises(ValueError):
        R(alphas=[1.0], validation=(X[:, :6], Y), device="cpu").fit(X, Y)
    with pytest.raises(ValueError):
        R(alphas=[1.0], validation=(X[:5], Y[:4]), device="cpu").fit(X, Y)
    r = R(device="cpu")
    with pytest.raises(RuntimeError):
        r.predict(X)
    with pytest.raises(ValueError):
        r.fit(X, Y).predict(X[:, :6])


def test_ridge_error_carries_the_pivot(be):
    X, Y = RO.planted(12, 7, 3, 0.1, 0)
    be.force_status = 9
    with pytest.raises(ridge.RidgeError) as e:
        ridge.RidgeDecoder(device="cpu").fit(X, Y)
    assert e.value.pivot == 8 and isinstance(e.value, RuntimeError)
    with pytest.raises(ridge.RidgeError):
        ridge.RidgeDecoder(alphas=[1.0, 2.0], cv=2, device="cpu").fit(X, Y)
    be.force_status = 0
    Xn = X.copy()
    Xn[3, 2] = np.nan                              # the mock's own pivot test: a NaN row poisons the Gram matrix
    with pytest.raises(ridge.RidgeError):
        ridge.RidgeDecoder(device="cpu").fit(Xn, Y)


def test_semantic_identification_takes_a_decoder():
    n, N, G, B = 40, 18, 6, 10
    X, Y = RO.planted(n, N, G, 0.05, 21, extra=B)
    bank_rows = np.concatenate([Y[n:], np.random.default_rng(2).standard_normal((15, G)).astype(np.float32)])
    own = [[b] for b in range(B)]
    r = ridge.RidgeDecoder(alpha=2.0, device="cpu").fit(X[:n], Y[:n])
    bank = evaluate.SemanticBank(bank_rows, device="cpu")
    res = evaluate.semantic_identification(r, X[n:], bank, own)
    P = RO.predict(RO.fit(X[:n], Y[:n], 2.0), X[n:])
    bn = bank_rows.astype(np.float64)
    sims = (P / np.linalg.norm(P, axis=1, keepdims=True)) @ (bn / np.linalg.norm(bn, axis=1, keepdims=True)).T
    want, _ = evaluate.semantic_ranks(sims, own)
    assert np.array_equal(res["rank"], want)
    np.testing.assert_allclose(res["sims"], sims, atol=1e-5)
    idx, _ = evaluate.semantic_retrieve(r, X[n:], bank, k=3)
    assert np.array_equal(idx, np.argsort(-sims, axis=1, kind="stable")[:, :3])


def test_stack_collects_an_epoch():
    gen = SyntheticGenerator(4, 5, 9, 8, 6, 11, seed=1, guse_dim=7)
    X, Yg = ridge.stack(gen, device="cpu")
    assert X.shape == (20, 9) and Yg.shape == (20, 7) and X.dtype == Yg.dtype == torch.float32
    for i in range(4):
        x = gen[i][0]
        assert np.array_equal(X[5 * i:5 * i + 5].numpy(), x[0]) and np.array_equal(Yg[5 * i:5 * i + 5].numpy(), x[4])
    X2, _ = ridge.stack(gen, steps=2, device="cpu")
    assert X2.shape == (10, 9)
    with pytest.raises(ValueError):
        ridge.stack(SyntheticGenerator(4, 5, 9, 8, 6, 11), device="cpu")
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError):
            ridge.stack(gen, steps=bad, device="cpu")
