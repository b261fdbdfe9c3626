"""Matrix families and a float32 numpy restatement of csrc/eigen.hip (tnt_syev_jacobi_f32 / tnt_gram_whiten_f32; the
definitions are in include/tnt_hip.h) -- TEST INFRASTRUCTURE ONLY.  The restatement keeps what the header fixes: the
round-robin ordering, the two rotation thresholds, (c, s) and the new diagonal pair in float64 rounded once, float32
rotations, the sort and the sign rule.  It differs from the kernel where the header leaves room: numpy multiplies and adds
where the kernel contracts to FMA.  The GPU test holds both to the same float64 bounds on the same inputs."""
import functools

import numpy as np

U = 2.0 ** -24
FAMILIES = ("gram", "cond1e6", "cond1e12", "indefinite", "rank_third", "identity", "fours")


def _sym32(A):
    A = np.asarray(A, np.float64)
    return ((A + A.T) / 2).astype(np.float32)


def _ortho(m, rng):
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    return q * np.sign(np.diag(r) + (np.diag(r) == 0))


def _spectrum(ev, rng):
    q = _ortho(len(ev), rng)
    return _sym32((q * np.asarray(ev, np.float64)) @ q.T)


@functools.lru_cache(maxsize=None)
def family(name, m):
    """the float32 symmetric test matrix of a family at order m (the same bits on every call)"""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + m)
    if name == "gram":
        x = rng.standard_normal((m, 2 * m))
        return _sym32(x @ x.T)
    if name == "cond1e6":
        return _spectrum(np.logspace(0, -6, m), rng)
    if name == "cond1e12":
        return _spectrum(np.logspace(0, -12, m), rng)
    if name == "indefinite":
        return _spectrum(np.linspace(-1, 1, m), rng)
    if name == "rank_third":
        r = max(1, m // 3)
        return _spectrum(np.concatenate([np.linspace(1, 0.1, r), np.zeros(m - r)]), rng)
    if name == "identity":
        return np.eye(m, dtype=np.float32)
    if name == "fours":
        return _spectrum(1.0 / (1 + np.arange(m) // 4), rng)
    raise KeyError(name)


def rounds(m):
    """rounds per sweep: m - 1 for even m, m for odd m (a bye per round)"""
    return m - 1 + (m & 1) if m > 1 else 0


def pairs(m, r):
    """the disjoint pairs (p < q) of round r, in slot order: the circle method over m rounded up to even, the last player
    fixed; for odd m that player is the bye and its pair is left out"""
    n2 = m + (m & 1)
    n1 = n2 - 1
    out = []
    if n2 == m:
        out.append((r, n1))
    for k in range(1, n2 // 2):
        a, b = (r + k) % n1, (r - k + n1) % n1
        out.append((min(a, b), max(a, b)))
    return np.asarray(out, np.int64).reshape(-1, 2)


def _sort_and_sign(w, V):
    m = len(w)
    order = sorted(range(m), key=lambda i: (-w[i], i))         # descending, ties by the column they came from
    w, V = w[order], V[:, order].copy()
    for i in range(m):
        if V[np.argmax(np.abs(V[:, i])), i] < 0:                # argmax: the first entry on ties
            V[:, i] = -V[:, i]
    return w, V


def jacobi_f32(A, max_sweeps=64):
    """(w, V, info) of the lower triangle of the float32 matrix A as the kernel computes them"""
    A = np.asarray(A, np.float32)
    m = len(A)
    low = np.tril(A)
    if not np.all(np.isfinite(low)):
        return None, None, (2, 0, m)
    a = low + np.tril(A, -1).T
    V = np.eye(m, dtype=np.float32)
    fro = float(np.sqrt(np.sum(a.astype(np.float64) ** 2)))
    floor = U * fro / np.sqrt(m)
    f32 = np.float32
    sweeps, converged = 0, False
    while sweeps < max_sweeps and not converged:
        sweeps += 1
        rotated = False
        for r in range(rounds(m)):
            pq = pairs(m, r)
            p, q = pq[:, 0], pq[:, 1]
            app, aqq, apq = (a[p, p].astype(np.float64), a[q, q].astype(np.float64), a[q, p].astype(np.float64))
            go = (np.abs(apq) > U * np.sqrt(np.abs(app * aqq))) & (np.abs(apq) > floor)
            if not go.any():
                continue
            rotated = True
            p, q, app, aqq, apq = p[go], q[go], app[go], aqq[go], apq[go]
            tau = (aqq - app) / (2 * apq)
            t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1 + tau * tau))
            c64 = 1 / np.sqrt(1 + t * t)
            c, s = c64.astype(f32), (t * c64).astype(f32)
            x, y = a[:, p].copy(), a[:, q].copy()                 # columns
            a[:, p], a[:, q] = c * x - s * y, s * x + c * y
            x, y = a[p, :].copy(), a[q, :].copy()                 # rows
            a[p, :], a[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            a[p, p], a[q, q] = (app - t * apq).astype(f32), (aqq + t * apq).astype(f32)
            a[p, q] = a[q, p] = 0
            x, y = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * x - s * y, s * x + c * y
        converged = not rotated
    w, V = _sort_and_sign(np.diag(a).copy(), V)
    return w, V, (0 if converged else 1, sweeps, m)


def whiten_f32(S, tau, max_sweeps=64):
    """(M, w, info) of tnt_gram_whiten_f32 from the lower triangle of the float32 Gram matrix S"""
    S = np.asarray(S, np.float32)
    m = len(S)
    if not np.all(np.isfinite(np.tril(S))):
        return None, None, (2, 0, 0)
    d = np.diag(S).astype(np.float64)
    r = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), 0.0)
    s64 = np.tril(S).astype(np.float64)
    s64 = s64 + np.tril(s64, -1).T
    C = (s64 * r[:, None] * r[None, :]).astype(np.float32)
    w, W, info = jacobi_f32(C, max_sweeps)
    den = np.maximum(w.astype(np.float64), np.float64(np.float32(tau)) * np.float64(w[0]))
    scale = np.where(den > 0, 1 / np.sqrt(np.where(den > 0, den, 1)), 0.0)
    M = (r[:, None] * W.astype(np.float64) * scale[None, :]).astype(np.float32)
    rank = int(np.sum(w.astype(np.float64) > np.float64(np.float32(tau)) * np.float64(w[0])))
    return M, w, (info[0], info[1], rank)


def errors(A, w, V):
    """(residual, orthogonality, eigenvalue error) in float64 against the rounded input, each as the issue defines it"""
    a = np.tril(np.asarray(A, np.float64))
    a = a + np.tril(a, -1).T
    w, V = np.asarray(w, np.float64), np.asarray(V, np.float64)
    m = len(a)
    ref = np.linalg.eigvalsh(a)[::-1]
    res = np.linalg.norm(a @ V - V * w[None, :]) / np.linalg.norm(a)
    orth = np.linalg.norm(V.T @ V - np.eye(m))
    ev = np.abs(w - ref).max() / np.abs(ref).max()
    return res, orth, ev


def bounds(m):
    return 2 * (m + 4) * U, 8 * m * U, 2 * (m + 4) * U
