"""float64 restatement of masters_thesis_amd/pca.py -- TEST INFRASTRUCTURE ONLY: the SVD of the explicitly centred scans, with
the attributes under pca.PCA's formulas and the sign rule of tnt_syev_jacobi_f32 applied to the left singular vectors."""
import numpy as np


def planted(n, N, lead, tail, seed, mean_sd=0.02, extra=0):
    """X (n + extra, N) float32 = A diag(s) B^T + column means: s = ``lead`` followed by ``tail`` for every further direction,
    A, B random with orthonormal columns (over the first n rows), the means normal with standard deviation ``mean_sd``.
    tail = None: plain standard normal rows instead."""
    rng = np.random.default_rng(seed)
    if tail is None:
        X = rng.standard_normal((n + extra, N))
    else:
        r = min(n + extra, N)
        s = np.full(r, float(tail))
        s[:len(lead)] = lead
        a, _ = np.linalg.qr(rng.standard_normal((n + extra, r)))
        b, _ = np.linalg.qr(rng.standard_normal((N, r)))
        X = (a * s) @ b.T
    return (X + mean_sd * rng.standard_normal(N)).astype(np.float32)


def fit(X, k, center=True):
    X = np.asarray(X, np.float64)
    n, N = X.shape
    mean = X.mean(0) if center else np.zeros(N)
    Xc = X - mean
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    for i in range(len(s)):                                   # the kernel's sign rule on U's columns
        if U[np.argmax(np.abs(U[:, i])), i] < 0:
            U[:, i], Vt[i] = -U[:, i], -Vt[i]
    lam = np.zeros(n)
    lam[:len(s)] = s * s                                     # the eigenvalues of Kc, descending
    return dict(s=s[:k], components=Vt[:k], mean=mean, ev=s[:k] ** 2 / (n - 1), ratio=s[:k] ** 2 / (s ** 2).sum(), U=U[:, :k],
                lam=lam, Kc=Xc @ Xc.T, k=k)


def transform(m, X, whiten=False):
    Z = (np.asarray(X, np.float64) - m["mean"]) @ m["components"].T
    return Z / np.sqrt(m["ev"]) if whiten else Z


def inverse_transform(m, Z, whiten=False):
    Z = np.asarray(Z, np.float64)
    return (Z * np.sqrt(m["ev"]) if whiten else Z) @ m["components"] + m["mean"]


def gaps(m):
    """for each of the k leading eigenvalues of Kc the distance to the nearest other one"""
    lam = m["lam"]
    d = np.abs(lam[:, None] - lam[None, :])
    d[np.diag_indices(len(lam))] = np.inf
    return d.min(1)[:m["k"]]
