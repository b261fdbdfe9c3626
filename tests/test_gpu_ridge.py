"""tnt_cholesky_f32 / tnt_cholesky_solve_f32 / tnt_gram_center_f32 on a real MI355X against float64 (tests/ridge_oracle.py).

Factorisation: n in {1, 5, 63, 64, 65, 130, 200} -- below, at and just over a block edge, two and three block columns with a
ragged last one -- K = X X^T (X standard normal, n x N, formed in float64 and rounded), shift added by the kernel.  ldk, ldl
> n; NaN in K's strict upper triangle and pad columns (never read: a NaN that was read would reach L or the status), a
sentinel in L's strict upper triangle and pad columns (intact afterwards).  Acceptance, both evaluated in float64:
    || L L^T - (K + shift I) ||_F / || K + shift I ||_F                              <= n 2^-24
    || (K + shift I) A - Y ||_F / (|| K + shift I ||_F || A ||_F + || Y ||_F)        <= n 2^-24    G in {1, 3, 24, 130}, ragged ldx
The float32 restatement of the blocked algorithm (ridge_oracle.cholesky_blocked_f32 / solve_blocked_f32) is held to the same
two bounds on the same input, so an input on which float32 cannot reach the bound fails the test by itself.
Measured on an MI355X: see MEASURED at the end of this text.

Failure path: at n = 130, K[70, 70] replaced (from the float64 factor of the leading block) so that the exact Schur pivot is
-1: status 71, and a following solve leaves X with its bits; a NaN at K[3, 0]: a nonzero status.  Two runs: the same bits.
Every TNT_BADARG.  gram_center against float64 at n in {1, 63, 130}: with u = 2^-24 and k = max |K_ij|, a mean is a float64
sum rounded once (|error| <= u k, the float64 sum's own error is below u k / 2^20), and the result is a float64 expression
of K_ij and three such means rounded once, |value| <= 4 k: |error| <= 3 u k + 4 u k, held here to 8 u k.

MEASURED on an MI355X (kernel; the float32 restatement on the host in brackets; solve: the largest of the four G):
  n = 1     backward error 2.17e-08 (2.17e-08)   solve residual 3.10e-08 (3.10e-08)   bound 5.96e-08
  n = 5     backward error 4.20e-08 (4.20e-08)   solve residual 1.66e-08 (1.66e-08)   bound 2.98e-07
  n = 63    backward error 3.20e-08 (3.20e-08)   solve residual 4.01e-09 (4.01e-09)   bound 3.76e-06
  n = 64    backward error 3.61e-08 (3.61e-08)   solve residual 4.90e-09 (4.90e-09)   bound 3.81e-06
  n = 65    backward error 3.01e-08 (2.98e-08)   solve residual 4.01e-09 (4.00e-09)   bound 3.87e-06
  n = 130   backward error 5.65e-08 (5.40e-08)   solve residual 1.06e-08 (7.05e-09)   bound 7.75e-06
  n = 200   backward error 6.29e-08 (6.27e-08)   solve residual 7.46e-09 (7.71e-09)   bound 1.19e-05
Up to one block (n <= 64) the kernel and the restatement agree to every printed digit: the same float64 arithmetic rounded once.
"""
import functools

import numpy as np
import pytest
import torch

import ridge_oracle as RO
from masters_thesis_amd.ops import cholesky_solve_work_floats, cholesky_work_floats

gpu = pytest.mark.gpu
U = 2.0 ** -24
SENT = -777.25
CASES = {1: (40, 3.0), 5: (40, 3.0), 63: (40, 3.0), 64: (200, 10.0), 65: (40, 3.0), 130: (97, 10.0), 200: (300, 10.0)}   # n: (N, shift)
GS = [1, 3, 24, 130]


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


@functools.lru_cache(maxsize=None)
def case(n):
    N, shift = CASES[n]
    K = RO.spd_case(n, N, shift, 100 + n)
    Y = np.random.default_rng(200 + n).standard_normal((n, max(GS))).astype(np.float32)
    L, st = RO.cholesky_blocked_f32(K, shift)
    assert st == 0
    return K, shift, Y, L


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def k_buffer(K, ldk):
    """the lower triangle of K at stride ldk; NaN everywhere else"""
    n = len(K)
    buf = np.full((n, ldk), np.nan, np.float32)
    low = np.tril_indices(n)
    buf[low] = K[low]
    return dev(buf)


def factor(be, K, shift, pad=4):
    n = len(K)
    ld = (n + 3) // 4 * 4 + pad
    Kd = k_buffer(K, ld)
    Ld = torch.full((n, ld + 4), SENT, dtype=torch.float32, device="cuda")
    work = torch.zeros(cholesky_work_floats(n), dtype=torch.float32, device="cuda")
    status = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    be.cholesky(Kd, ld, Ld, ld + 4, n, shift, work, status)
    return Kd, Ld, status


def lower(Ld, n):
    """the factor as float64, after checking that nothing outside the lower triangle was written"""
    full = Ld.cpu().numpy()
    up = np.triu_indices(n, 1)
    assert np.all(full[:, :n][up] == SENT) and np.all(full[:, n:] == SENT), "L's strict upper triangle / pad columns were written"
    return np.tril(full[:, :n]).astype(np.float64)


@gpu
@pytest.mark.parametrize("n", sorted(CASES))
def test_factorisation_and_solve_reach_the_backward_error_bound(n, be):
    K, shift, Y, Lref = case(n)
    bound = n * U
    ref_err = RO.backward_error(Lref, K, shift)
    assert ref_err <= bound, ("the float32 restatement misses the bound: a bad input", ref_err, bound)
    Kd, Ld, status = factor(be, K, shift)
    assert int(status.item()) == 0
    low = np.tril_indices(n)
    assert np.array_equal(Kd.cpu().numpy()[:, :n][low], K[low]), "K was written"
    L = lower(Ld, n)
    assert np.all(np.isfinite(L)), "a NaN of K's upper triangle was read"
    err = RO.backward_error(L, K, shift)
    print(f"n={n} backward error {err:.3e} (float32 restatement {ref_err:.3e}) bound {bound:.3e}")
    assert err <= bound
    for G in GS:
        ldx = (G + 3) // 4 * 4 + 4
        ref_res = RO.solve_residual(K, shift, RO.solve_blocked_f32(Lref, Y[:, :G]), Y[:, :G])
        assert ref_res <= bound, ("the float32 restatement misses the bound: a bad input", ref_res, bound)
        X = torch.full((n, ldx), SENT, dtype=torch.float32, device="cuda")
        X[:, :G] = dev(Y[:, :G])
        work = torch.zeros(cholesky_solve_work_floats(ldx), dtype=torch.float32, device="cuda")
        be.cholesky_solve(Ld, Ld.shape[1], n, X, ldx, G, work, status)
        out = X.cpu().numpy()
        assert np.all(out[:, G:] == SENT), "X's pad columns were written"
        lower(Ld, n)
        res = RO.solve_residual(K, shift, out[:, :G], Y[:, :G])
        print(f"n={n} G={G} solve residual {res:.3e} (float32 restatement {ref_res:.3e}) bound {bound:.3e}")
        assert res <= bound


@gpu
def test_a_negative_pivot_sets_the_status_and_stops_the_solve(be):
    n = 130
    K, shift, Y, _ = case(n)
    K = K.copy()
    M = K.astype(np.float64) + np.float64(np.float32(shift)) * np.eye(n)
    L70 = np.linalg.cholesky(M[:70, :70])
    row = np.linalg.solve(L70, M[70, :70])
    K[70, 70] = np.float32(row @ row - 1.0 - np.float64(np.float32(shift)))       # the exact Schur pivot of row 70: -1
    _, Ld, status = factor(be, K, shift)
    assert int(status.item()) == 71
    X = dev(Y[:, :24].copy())
    before = X.clone()
    work = torch.zeros(64 * 24, dtype=torch.float32, device="cuda")
    be.cholesky_solve(Ld, Ld.shape[1], n, X, 24, 24, work, status)
    assert torch.equal(X.view(torch.int32), before.view(torch.int32))
    assert int(status.item()) == 71
    lower(Ld, n)                                     # whatever L holds, nothing outside its lower triangle was written


@gpu
def test_a_nan_sets_the_status(be):
    K, shift, _, _ = case(130)
    K = K.copy()
    K[3, 0] = np.nan
    _, Ld, status = factor(be, K, shift)
    assert int(status.item()) != 0
    lower(Ld, 130)


@gpu
@pytest.mark.parametrize("n", [65, 200])
def test_two_runs_give_the_same_bits(n, be):
    K, shift, Y, _ = case(n)
    outs = []
    for _ in range(2):
        _, Ld, status = factor(be, K, shift)
        X = dev(Y[:, :24].copy())
        be.cholesky_solve(Ld, Ld.shape[1], n, X, 24, 24, torch.zeros(64 * 24, dtype=torch.float32, device="cuda"), status)
        outs.append((Ld.cpu().numpy().view(np.int32), X.cpu().numpy().view(np.int32), int(status.item())))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2] == 0


@gpu
def test_refusals(be):
    n, ld = 8, 8
    t = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    K, L, X, work, mean = t(n, ld), t(n, ld), t(n, 4), t(64 * 8 + 4), t(n + 1)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    s = be._s()
    chol = lambda K_=p(K), ldk=ld, L_=p(L), ldl=ld, n_=n, w=p(work), st=p(status): be.lib.tnt_cholesky_f32(
        K_, ldk, L_, ldl, n_, 1.0, w, st, s)
    solve = lambda L_=p(L), ldl=ld, n_=n, X_=p(X), ldx=4, G=3, w=p(work), st=p(status): be.lib.tnt_cholesky_solve_f32(
        L_, ldl, n_, X_, ldx, G, w, st, s)
    center = lambda K_=p(K), ldk=ld, n_=n, m=p(mean): be.lib.tnt_gram_center_f32(K_, ldk, n_, m, s)
    code = lambda k: -1000 - k
    assert chol() == 0 and solve() == 0 and center() == 0
    assert chol(K_=None) == code(1) and chol(K_=p(K) + 4) == code(1)
    assert chol(ldk=7) == code(2) and chol(ldk=10) == code(2) and chol(n_=6, ldk=6) == code(2)
    assert chol(L_=None) == code(3) and chol(L_=p(L) + 4) == code(3) and chol(L_=p(K)) == code(3)
    assert chol(ldl=4) == code(4) and chol(ldl=10) == code(4)
    assert chol(n_=0) == code(5) and chol(n_=-1) == code(5) and chol(n_=32769, ldk=32772, ldl=32772) == code(5)
    assert chol(w=None) == code(7) and chol(w=p(work) + 4) == code(7)
    assert chol(st=None) == code(8)
    assert solve(L_=None) == code(1) and solve(L_=p(L) + 4) == code(1)
    assert solve(ldl=4) == code(2) and solve(ldl=10) == code(2)
    assert solve(n_=0) == code(3) and solve(n_=32769, ldl=32772) == code(3)
    assert solve(X_=None) == code(4) and solve(X_=p(X) + 4) == code(4)
    assert solve(ldx=2, G=3) == code(5) and solve(ldx=6, G=3) == code(5)
    assert solve(G=0) == code(6)
    assert solve(w=None) == code(7) and solve(w=p(work) + 4) == code(7)
    assert solve(st=None) == code(8)
    assert center(K_=None) == code(1) and center(K_=p(K) + 4) == code(1)
    assert center(ldk=4) == code(2) and center(ldk=10) == code(2)
    assert center(n_=0) == code(3) and center(n_=32769, ldk=32772) == code(3)
    assert center(m=None) == code(4)
    torch.cuda.synchronize()
    assert be.lib.tnt_version() >= 138


@gpu
@pytest.mark.parametrize("n", [1, 63, 130])
def test_gram_center_matches_float64(n, be):
    K = RO.spd_case(n, 40, 0.0, 300 + n)
    ld = (n + 3) // 4 * 4 + 4
    buf = np.full((n, ld), SENT, np.float32)
    buf[:, :n] = K
    Kd, mean = dev(buf), torch.full((n + 2,), SENT, dtype=torch.float32, device="cuda")
    be.gram_center(Kd, ld, n, mean)
    out, m = Kd.cpu().numpy(), mean.cpu().numpy()
    assert np.all(out[:, n:] == SENT) and m[n + 1] == SENT
    K64 = K.astype(np.float64)
    H = np.eye(n) - np.ones((n, n)) / n
    k = np.abs(K64).max()
    assert np.abs(m[:n] - K64.mean(1)).max() <= 2 * U * k
    assert abs(m[n] - K64.mean()) <= 2 * U * k
    assert np.abs(out[:, :n] - H @ K64 @ H).max() <= 8 * U * k
    Kd2, mean2 = dev(buf), torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    be.gram_center(Kd2, ld, n, mean2)
    assert np.array_equal(Kd2.cpu().numpy().view(np.int32), out.view(np.int32))
