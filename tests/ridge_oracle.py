"""Float64 restatement of masters_thesis_amd/ridge.py -- TEST INFRASTRUCTURE ONLY.  Everything is formed the plain way: the
training rows are centred explicitly, (Kc + alpha I) A = Yc goes to numpy.linalg.solve, every fold is fitted from its own
rows (nothing is shared between folds or alphas), and the scores follow the texts of RidgeDecoder and tnt_cosine_loss_f32.
Beside it a float32 restatement of the blocked left-looking factorisation and sweeps of csrc/cholesky.hip, used only to show
what float32 arithmetic can reach on a test's input."""
import numpy as np

NB = 64
EPS = 1e-12


# ------------------------------------------------------------------------------------------------ the model
def fit(X, Y, alpha, fit_intercept=True):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n = X.shape[0]
    mu_x = X.mean(0) if fit_intercept else np.zeros(X.shape[1])
    mu_y = Y.mean(0) if fit_intercept else np.zeros(Y.shape[1])
    Xc, Yc = X - mu_x, Y - mu_y
    Kc = Xc @ Xc.T
    A = np.linalg.solve(Kc + alpha * np.eye(n), Yc)
    coef = Xc.T @ A
    return dict(coef=coef, intercept=mu_y - mu_x @ coef, dual=A, Kc=Kc, mu_x=mu_x, mu_y=mu_y, alpha=alpha)


def predict(m, X):
    return np.asarray(X, np.float64) @ m["coef"] + m["intercept"]


def kfold(n, k, groups=None):
    """fold of every row: scikit-learn's unshuffled KFold sizes, or rank(group id) % k"""
    if groups is None:
        out, start = np.zeros(n, np.int64), 0
        for f in range(k):
            size = n // k + (1 if f < n % k else 0)
            out[start:start + size] = f
            start += size
        return out
    ids = sorted(set(np.asarray(groups).tolist()))
    rank = {g: i for i, g in enumerate(ids)}
    return np.array([rank[g] % k for g in np.asarray(groups).tolist()], np.int64)


def score_cosine(P, Y):
    """mean over rows of cos as tnt_cosine_loss_f32 defines it: squared norms floored at 1e-12, an all-zero row gives 0"""
    P, Y = np.asarray(P, np.float64), np.asarray(Y, np.float64)
    ip = 1.0 / np.sqrt(np.maximum((P * P).sum(1), EPS))
    iy = 1.0 / np.sqrt(np.maximum((Y * Y).sum(1), EPS))
    return float((((P * Y).sum(1) * ip) * iy).mean())


def score_r2(P, Y):
    """mean over columns of R^2, the column mean taken over the validation rows (scikit-learn's r2_score)"""
    P, Y = np.asarray(P, np.float64), np.asarray(Y, np.float64)
    num, den = ((Y - P) ** 2).sum(0), ((Y - Y.mean(0)) ** 2).sum(0)
    r2 = np.where(den > 0, 1.0 - num / np.where(den > 0, den, 1.0), np.where(num > 0, 0.0, 1.0))
    return float(r2.mean())


def select(X, Y, alphas, cv=None, groups=None, validation=None, score="cosine", fit_intercept=True):
    """(alpha_, cv_scores_): the fold means of the score per alpha and their first maximiser"""
    fn = score_cosine if score == "cosine" else score_r2
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if validation is not None:
        splits = [(X, Y, np.asarray(validation[0], np.float64), np.asarray(validation[1], np.float64))]
    else:
        fold = kfold(len(X), cv, groups)
        splits = [(X[fold != f], Y[fold != f], X[fold == f], Y[fold == f]) for f in range(cv)]
    sc = np.array([[fn(predict(fit(xt, yt, a, fit_intercept), xv), yv) for a in alphas] for xt, yt, xv, yv in splits])
    means = sc.mean(0)
    best = 0
    for i in range(1, len(alphas)):
        if means[i] > means[best]:
            best = i
    return alphas[best], means


def fit_select(X, Y, alphas, **kw):
    alpha, scores = select(X, Y, alphas, **kw)
    m = fit(X, Y, alpha, kw.get("fit_intercept", True))
    m["cv_scores"] = scores
    return m


# ------------------------------------------------------------------------------------------------ float32, blocked
def _factor_block(D):
    """lower factor of a small block in float64, or the index of the first bad pivot"""
    D = D.copy()
    n = D.shape[0]
    for k in range(n):
        d = D[k, k]
        lf = np.float32(np.sqrt(d)) if d > 0 else np.float32(0)
        if not (d > 0) or not (lf > 0) or np.isinf(lf):
            return None, k
        for i in range(k + 1, n):
            f = D[i, k] / d
            D[i, k + 1:i + 1] -= f * D[k + 1:i + 1, k]
    d = np.sqrt(np.diag(D))
    L = np.tril(D) / d[None, :]
    return L, -1


def cholesky_blocked_f32(K, shift):
    """(L float32, status): left-looking at NB = 64 over the lower triangle of the float32 K; the products in float32, the
    64 x 64 work in float64 rounded once, L21 against the rounded L11"""
    K = np.asarray(K, np.float32)
    n = K.shape[0]
    L = np.zeros((n, n), np.float32)
    for j0 in range(0, n, NB):
        nb = min(NB, n - j0)
        P = (L[j0:, :j0] @ L[j0:j0 + nb, :j0].T).astype(np.float32) if j0 else np.zeros((n - j0, nb), np.float32)
        D = np.tril(K[j0:j0 + nb, j0:j0 + nb]).astype(np.float64) + np.float64(np.float32(shift)) * np.eye(nb) - np.tril(P[:nb])
        L11, bad = _factor_block(D)
        if bad >= 0:
            return L, 1 + j0 + bad
        L11 = L11.astype(np.float32)
        L[j0:j0 + nb, j0:j0 + nb] = L11
        if j0 + nb < n:
            Bm = K[j0 + nb:, j0:j0 + nb].astype(np.float64) - P[nb:].astype(np.float64)
            L[j0 + nb:, j0:j0 + nb] = _tri(L11.astype(np.float64), Bm.T, False).T.astype(np.float32)
    return L, 0


def _tri(T, B, trans):
    """T^-1 B (lower T) or T^-T B by substitution in float64"""
    B = B.copy()
    n = T.shape[0]
    order = range(n - 1, -1, -1) if trans else range(n)
    for k in order:
        B[k] /= T[k, k]
        if trans:
            B[:k] -= np.outer(T[k, :k], B[k])
        else:
            B[k + 1:] -= np.outer(T[k + 1:, k], B[k])
    return B


def solve_blocked_f32(L, Y):
    """(L L^T)^-1 Y by the two sweeps of tnt_cholesky_solve_f32: float32 products, float64 block solves rounded once"""
    L, X = np.asarray(L, np.float32), np.array(Y, np.float32)
    n = L.shape[0]
    starts = list(range(0, n, NB))
    for j0 in starts:
        nb = min(NB, n - j0)
        P = (L[j0:j0 + nb, :j0] @ X[:j0]).astype(np.float32) if j0 else 0.0
        X[j0:j0 + nb] = _tri(L[j0:j0 + nb, j0:j0 + nb].astype(np.float64), X[j0:j0 + nb].astype(np.float64) - P, False)
    for j0 in reversed(starts):
        nb = min(NB, n - j0)
        P = (L[j0 + nb:, j0:j0 + nb].T @ X[j0 + nb:]).astype(np.float32) if j0 + nb < n else 0.0
        X[j0:j0 + nb] = _tri(L[j0:j0 + nb, j0:j0 + nb].astype(np.float64), X[j0:j0 + nb].astype(np.float64) - P, True)
    return X


def backward_error(L, K, shift):
    """|| L L^T - (K + shift I) ||_F / || K + shift I ||_F in float64, K and shift as the float32 numbers the kernel gets"""
    L = np.tril(np.asarray(L, np.float64))
    M = np.asarray(K, np.float32).astype(np.float64) + np.float64(np.float32(shift)) * np.eye(len(L))
    return float(np.linalg.norm(L @ L.T - M) / np.linalg.norm(M))


def solve_residual(K, shift, A, Y):
    """|| (K + shift I) A - Y ||_F / (|| K + shift I ||_F || A ||_F + || Y ||_F) in float64"""
    M = np.asarray(K, np.float32).astype(np.float64) + np.float64(np.float32(shift)) * np.eye(len(K))
    A, Y = np.asarray(A, np.float64), np.asarray(Y, np.float64)
    return float(np.linalg.norm(M @ A - Y) / (np.linalg.norm(M) * np.linalg.norm(A) + np.linalg.norm(Y)))


def spd_case(n, N, shift, seed):
    """the float32 Gram matrix of n standard-normal rows of N features, formed in float64 and rounded (without the shift:
    the kernel adds it)"""
    X = np.random.default_rng(seed).standard_normal((n, N))
    return (X @ X.T).astype(np.float32)


def planted(n, N, G, noise, seed, extra=0, rank=16):
    """scans with `rank` strong directions (as responses driven by a few stimulus features are) on a floor of voxel noise,
    voxel means that are not zero, and embeddings Y = X W* + 0.3 + noise (with `extra` further rows of the same model)"""
    rng = np.random.default_rng(seed)
    rows = n + extra
    X = rng.standard_normal((rows, rank)) @ rng.standard_normal((rank, N)) / np.sqrt(rank)
    X += 0.1 * rng.standard_normal((rows, N)) + 0.2 * rng.standard_normal(N)
    W = rng.standard_normal((N, G)) / np.sqrt(N)
    Y = X @ W + 0.3 + noise * rng.standard_normal((rows, G))
    return X.astype(np.float32), Y.astype(np.float32)
