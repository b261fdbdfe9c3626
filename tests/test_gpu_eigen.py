"""tnt_syev_jacobi_f32 / tnt_gram_whiten_f32 (csrc/eigen.hip) on a real MI355X against float64 (tests/eigen_oracle.py).

Eigensolver: m in {1, 2, 3, 5, 63, 64, 65, 127, 128} -- the smallest orders, odd orders (a bye per round), one and two
lanes' worth of rows per wave -- over the seven families of eigen_oracle (a Gram matrix, cond 1e6, cond 1e12, indefinite on
[-1, 1], rank m / 3, the identity, eigenvalues repeated in fours).  lda, ldv > m; NaN in A's strict upper triangle and pad
columns (never read: one that was read would reach w, V or info[0]); sentinels in V's pad columns and behind w (intact
afterwards).  Acceptance in float64 against the rounded input, u = 2^-24:
    || A V - V diag(w) ||_F / || A ||_F        <= 2 (m + 4) u
    || V^T V - I ||_F                          <= 8 m u
    max |w - eigvalsh| / max |eigvalsh|        <= 2 (m + 4) u
    info == (0, sweeps <= 32, m)
The float32 restatement (eigen_oracle.jacobi_f32: the same ordering, thresholds, sort and sign rule) is held to the same three
bounds on the same inputs, so a bound float32 Jacobi cannot reach fails the test by itself.  w descending; the sign rule; two
runs the same bits; max_sweeps = 1 on the Gram family: info[0] == 1 with finite outputs; a NaN on the diagonal: info[0] == 2,
w and V untouched; every TNT_BADARG.

Whiten: Z (200 x m), m in {5, 64, 128}, nearly orthogonal columns graded 1 .. 1e-6, S = Z^T Z formed in float64 and rounded:
    || (Z M)^T (Z M) - I ||_F <= 8 m u + m 2^-23 (the rounding of S),  info == (0, s, m);
with a duplicated and a zero column: everything finite, rank m - 2, the eigenvalues of (Z M)^T (Z M) (the squared singular
values of Z M in float64) within [0, 1 + that bound].

MEASURED on an MI355X, the worst ratio over the seven families of each error to m u (the float32 restatement on the host in
brackets; the bounds are 2 (m + 4) / m, 8 and 2 (m + 4) / m on this scale), and the largest sweep count:
  m = 1     residual 0.00 (0.00)   orthogonality 0.00 (0.00)   eigenvalues 0.00 (0.00)   sweeps 1
  m = 2     residual 0.31 (0.31)   orthogonality 0.51 (0.51)   eigenvalues 0.24 (0.24)   sweeps 2
  m = 3     residual 0.55 (0.58)   orthogonality 0.93 (1.16)   eigenvalues 0.29 (0.29)   sweeps 4
  m = 5     residual 0.41 (0.41)   orthogonality 2.04 (1.92)   eigenvalues 0.30 (0.30)   sweeps 5
  m = 63    residual 0.27 (0.30)   orthogonality 2.57 (2.78)   eigenvalues 0.31 (0.33)   sweeps 11
  m = 64    residual 0.26 (0.30)   orthogonality 2.43 (2.78)   eigenvalues 0.21 (0.17)   sweeps 12
  m = 65    residual 0.27 (0.30)   orthogonality 2.40 (2.75)   eigenvalues 0.30 (0.21)   sweeps 12
  m = 127   residual 0.20 (0.24)   orthogonality 2.69 (3.27)   eigenvalues 0.17 (0.20)   sweeps 15
  m = 128   residual 0.22 (0.26)   orthogonality 2.67 (3.33)   eigenvalues 0.16 (0.18)   sweeps 15
The kernel's sweep counts equal the restatement's on every input but one (m = 128, fours: 10 against 11); its FMA rotations
leave the errors a little below the restatement's multiply-and-add.
Whiten, || (Z M)^T (Z M) - I ||_F: m = 5 3.9e-07 (restatement 4.9e-07, bound 3.0e-06), m = 64 9.0e-06 (1.0e-05, 3.8e-05),
m = 128 2.0e-05 (2.3e-05, 7.6e-05), rank m, 5 / 8 / 9 sweeps.  With the two defects: rank m - 2, the largest eigenvalue
1 + 1.9e-07, 1 + 2.1e-06, 1 + 5.1e-06, the smallest 0.
"""
import functools

import numpy as np
import pytest
import torch

import eigen_oracle as EO

gpu = pytest.mark.gpu
U = EO.U
SENT = -777.25
ORDERS = [1, 2, 3, 5, 63, 64, 65, 127, 128]


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


@functools.lru_cache(maxsize=None)
def reference(name, m):
    """the restatement's (w, V, info) of a family: computed once"""
    return EO.jacobi_f32(EO.family(name, m))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def r4(v):
    return (v + 3) // 4 * 4


def lower_buffer(A, ld):
    """the lower triangle of A at stride ld; NaN everywhere else"""
    m = len(A)
    buf = np.full((m, ld), np.nan, np.float32)
    low = np.tril_indices(m)
    buf[low] = A[low]
    return dev(buf)


def solve(be, A, max_sweeps=64):
    m = len(A)
    lda, ldv = r4(m) + 4, r4(m) + 8
    Ad = lower_buffer(A, lda)
    w = torch.full((m + 2,), SENT, dtype=torch.float32, device="cuda")
    V = torch.full((m, ldv), SENT, dtype=torch.float32, device="cuda")
    info = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
    be.syev_jacobi(Ad, lda, m, w, V, ldv, info, max_sweeps=max_sweeps)
    w, V, info = w.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()
    low = np.tril_indices(m)
    assert np.array_equal(Ad.cpu().numpy()[low].view(np.int32), A[low].view(np.int32)), "A was written"
    assert np.all(w[m:] == SENT) and np.all(V[:, m:] == SENT) and info[3] == 12345, "a pad column or a word behind w / info was written"
    return w[:m], V[:, :m], tuple(int(x) for x in info[:3])


def check_order_and_sign(w, V):
    assert np.all(np.diff(w) <= 0), "w is not descending"
    for i in range(len(w)):
        assert V[np.argmax(np.abs(V[:, i])), i] > 0, f"column {i}: the entry of largest magnitude is not positive"


@gpu
@pytest.mark.parametrize("m", ORDERS)
def test_eigenpairs_reach_the_float64_bounds(m, be):
    bounds = EO.bounds(m)
    worst, worst_ref, sweeps = [0.0] * 3, [0.0] * 3, 0
    for name in EO.FAMILIES:
        A = EO.family(name, m)
        wr, Vr, info_r = reference(name, m)
        ref = EO.errors(A, wr, Vr)
        assert info_r[0] == 0 and all(e <= b for e, b in zip(ref, bounds)), ("the float32 restatement misses a bound", name, ref, bounds)
        w, V, info = solve(be, A)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(V)), "a NaN of A's upper triangle or pad was read"
        got = EO.errors(A, w, V)
        print(f"m={m} {name}: residual {got[0]:.3e} orthogonality {got[1]:.3e} eigenvalues {got[2]:.3e} (restatement "
              f"{ref[0]:.3e} {ref[1]:.3e} {ref[2]:.3e}) bounds {bounds[0]:.3e} {bounds[1]:.3e} {bounds[2]:.3e} info {info} "
              f"(restatement {info_r})")
        worst = [max(a, b / (m * U)) for a, b in zip(worst, got)]
        worst_ref = [max(a, b / (m * U)) for a, b in zip(worst_ref, ref)]
        sweeps = max(sweeps, info[1])
        assert info[0] == 0 and 1 <= info[1] <= 32 and info[2] == m, info
        assert all(e <= b for e, b in zip(got, bounds)), (name, got, bounds)
        check_order_and_sign(w, V)
    print(f"m={m} worst ratios to m u: {worst[0]:.2f} {worst[1]:.2f} {worst[2]:.2f} (restatement {worst_ref[0]:.2f} "
          f"{worst_ref[1]:.2f} {worst_ref[2]:.2f}) sweeps <= {sweeps}")


@gpu
def test_ties_keep_the_order_of_their_columns(be):
    """a diagonal matrix needs no rotation: w is its diagonal sorted, equal entries in ascending order of their column, and V
    the matching columns of the identity"""
    d = np.array([2.0, 5.0, 2.0, -1.0, 5.0, 2.0], np.float32)
    w, V, info = solve(be, np.diag(d))
    assert info == (0, 1, 6)
    assert np.array_equal(w, [5, 5, 2, 2, 2, -1])
    assert np.array_equal(np.argmax(V, axis=0), [1, 4, 0, 2, 5, 3]) and np.array_equal(V.sum(0), np.ones(6)) and np.all((V == 0) | (V == 1))


@gpu
@pytest.mark.parametrize("m", [65, 128])
def test_two_runs_give_the_same_bits(m, be):
    A = EO.family("cond1e6", m)
    a, b = solve(be, A), solve(be, A)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert a[2] == b[2]


@gpu
def test_one_sweep_is_reported_as_not_converged(be):
    A = EO.family("gram", 64)
    w, V, info = solve(be, A, max_sweeps=1)
    assert info == (1, 1, 64)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    check_order_and_sign(w, V)


@gpu
def test_a_nan_on_the_diagonal_leaves_the_outputs_alone(be):
    A = EO.family("gram", 65).copy()
    A[40, 40] = np.nan
    w, V, info = solve(be, A)
    assert info == (2, 0, 65)
    assert np.all(w == SENT) and np.all(V == SENT)


@gpu
def test_refusals(be):
    m, ld = 8, 8
    t = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    A, V, w = t(m, ld) + torch.eye(m, device="cuda"), t(m, ld), t(m + 1)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    s = be._s()
    syev = lambda A_=p(A), lda=ld, m_=m, w_=p(w), V_=p(V), ldv=ld, sw=30, i=p(info): be.lib.tnt_syev_jacobi_f32(
        A_, lda, m_, w_, V_, ldv, sw, i, s)
    whiten = lambda S_=p(A), lds=ld, m_=m, M_=p(V), ldm=ld, tau=2.0 ** -20, w_=p(w), i=p(info): be.lib.tnt_gram_whiten_f32(
        S_, lds, m_, M_, ldm, tau, w_, i, s)
    code = lambda k: -1000 - k
    assert syev() == 0 and whiten() == 0
    assert syev(w_=p(w) + 4, i=p(info) + 4) == 0 and whiten(w_=p(w) + 4, i=p(info) + 4) == 0      # 4-byte alignment suffices
    assert syev(A_=None) == code(1) and syev(A_=p(A) + 4) == code(1)
    assert syev(lda=4) == code(2) and syev(lda=10) == code(2)
    assert syev(m_=0) == code(3) and syev(m_=-1) == code(3) and syev(m_=129, lda=132, ldv=132) == code(3)
    assert syev(w_=None) == code(4) and syev(w_=p(w) + 2) == code(4)
    assert syev(V_=None) == code(5) and syev(V_=p(V) + 4) == code(5)
    assert syev(ldv=4) == code(6) and syev(ldv=10) == code(6)
    assert syev(sw=0) == code(7) and syev(sw=65) == code(7) and syev(sw=-3) == code(7)
    assert syev(i=None) == code(8) and syev(i=p(info) + 2) == code(8)
    assert syev(V_=p(A)) == code(9)
    assert whiten(S_=None) == code(1) and whiten(S_=p(A) + 4) == code(1)
    assert whiten(lds=4) == code(2) and whiten(lds=10) == code(2)
    assert whiten(m_=0) == code(3) and whiten(m_=129, lds=132, ldm=132) == code(3)
    assert whiten(M_=None) == code(4) and whiten(M_=p(V) + 4) == code(4)
    assert whiten(ldm=4) == code(5) and whiten(ldm=10) == code(5)
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert whiten(tau=bad) == code(6)
    assert whiten(w_=None) == code(7) and whiten(w_=p(w) + 2) == code(7)
    assert whiten(i=None) == code(8) and whiten(i=p(info) + 2) == code(8)
    assert whiten(M_=p(A)) == code(9)
    torch.cuda.synchronize()
    assert be.lib.tnt_version() >= 139


# ---------------------------------------------------------------------------------------------------- whiten
TAU = 2.0 ** -20


@functools.lru_cache(maxsize=None)
def graded(m, defects):
    """Z (200, m) float64 with nearly orthogonal columns graded 1 .. 1e-6; ``defects``: column 1 copied into column 3 and
    column 2 zeroed"""
    rng = np.random.default_rng(500 + m)
    q, _ = np.linalg.qr(rng.standard_normal((200, m)))
    Z = (q + 1e-3 * rng.standard_normal((200, m))) * np.logspace(0, -6, m)
    if defects:
        Z[:, 3] = Z[:, 1]
        Z[:, 2] = 0
    return Z


def run_whiten(be, S):
    m = len(S)
    lds, ldm = r4(m) + 4, r4(m) + 8
    Sd = lower_buffer(S, lds)
    w = torch.full((m + 2,), SENT, dtype=torch.float32, device="cuda")
    M = torch.full((m, ldm), SENT, dtype=torch.float32, device="cuda")
    info = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
    be.gram_whiten(Sd, lds, m, M, ldm, TAU, w, info)
    w, M, info = w.cpu().numpy(), M.cpu().numpy(), info.cpu().numpy()
    assert np.all(w[m:] == SENT) and np.all(M[:, m:] == SENT) and info[3] == 12345
    return M[:, :m], w[:m], tuple(int(x) for x in info[:3])


@gpu
@pytest.mark.parametrize("m", [5, 64, 128])
def test_whiten_orthonormalises_graded_columns(m, be):
    Z = graded(m, False)
    S = (Z.T @ Z).astype(np.float32)
    bound = 8 * m * U + m * 2.0 ** -23
    Mr, _, info_r = EO.whiten_f32(S, TAU)
    ZMr = Z @ Mr.astype(np.float64)
    ref = np.linalg.norm(ZMr.T @ ZMr - np.eye(m))
    assert ref <= bound and info_r[0] == 0 and info_r[2] == m, ("the float32 restatement misses the bound", ref, bound, info_r)
    M, w, info = run_whiten(be, S)
    ZM = Z @ M.astype(np.float64)
    err = np.linalg.norm(ZM.T @ ZM - np.eye(m))
    print(f"whiten m={m}: ||(ZM)^T ZM - I|| {err:.3e} (restatement {ref:.3e}) bound {bound:.3e} info {info} w {w[0]:.4f} .. {w[-1]:.4f}")
    assert info[0] == 0 and info[2] == m and err <= bound
    assert np.all(np.diff(w) <= 0)


@gpu
@pytest.mark.parametrize("m", [5, 64, 128])
def test_whiten_drops_a_duplicated_and_a_zero_column(m, be):
    Z = graded(m, True)
    S = (Z.T @ Z).astype(np.float32)
    bound = 8 * m * U + m * 2.0 ** -23
    M, w, info = run_whiten(be, S)
    assert np.all(np.isfinite(M)) and np.all(np.isfinite(w))
    assert info[0] == 0 and info[2] == m - 2, info
    sv = np.linalg.svd(Z @ M.astype(np.float64), compute_uv=False) ** 2
    print(f"whiten with defects m={m}: eigenvalues of (ZM)^T ZM in [{sv.min():.3e}, {sv.max():.9f}] bound 1 + {bound:.3e} info {info}")
    assert sv.min() >= 0 and sv.max() <= 1 + bound
    assert np.sum(sv > 0.5) == m - 2
