"""Timing of PCA of the scans (masters_thesis_amd/pca.py, csrc/eigen.hip) at the reference's sizes: n = 9000 scans,
N = 20 000 voxels (config 2), k = 100 components, 28 oversamples (m = 128).  One process, tools/semantic_bench.py's windows
(device events around windows that end in a synchronise, every window warmed first, medians of alternating windows):

  1. the Gram product (ridge.gram);
  2. one tnt_syev_jacobi_f32 on a Ritz matrix taken from the run, with its sweep count, barriers and microseconds per round,
     beside torch.linalg.eigh on the same 128 x 128 matrix on the device; one tnt_gram_whiten_f32 on a block Gram matrix
     from the run;
  3. the Kc Q and Z^T Z products (gemm3, unsplit: no exchange buffer, as ridge's sweeps);
  4. the whole fit, beside torch.pca_lowrank(q = 128, niter = 8) on the same tensor, and the fit with gram= handed in;
  5. transform of 64 scans;
  6. residual_ and the variance captured on a power-law spectrum, singular values i^-0.7 over 1000 directions.

Every expectation is stated before its measurement and marked held or missed after it.

    python tools/pca_bench.py [n N k oversamples]      # prints, and writes profiles/pca_bench.txt

Nothing here is a pass / fail threshold."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semantic_bench as SB  # noqa: E402
from masters_thesis_amd import ops, pca, ridge  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "pca_bench.txt")
say = SB.say


def verdict(what, ok):
    say(f"  expectation {'HELD' if ok else 'MISSED'}: {what}")


def main():
    n, N, k, over = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (9000, 20000, 100, 28)
    m = min(n, k + over)
    be = ops.backend()
    say(f"tools/pca_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {be.lib.tnt_version()}: n = {n}, N = {N}, "
        f"k = {k}, oversamples = {over} (m = {m})")
    g = torch.Generator(device="cuda").manual_seed(1)
    r = min(1000, n, N)
    def ortho(rows):
        f = torch.randn(rows, r, device="cuda", generator=g)
        try:
            return torch.linalg.qr(f)[0]
        except Exception:           # a torch build without a device QR
            return torch.linalg.qr(f.cpu())[0].cuda()

    a, b = ortho(n), ortho(N)
    sv = torch.arange(1, r + 1, device="cuda", dtype=torch.float32) ** -0.7
    X = ((a * sv) @ b.t()).contiguous()
    X -= X.mean(0)
    del a, b
    ldn, ldm = (n + 3) // 4 * 4, (m + 3) // 4 * 4
    zeros = lambda *s: torch.zeros(*s, device="cuda")

    say()
    say("1. the Gram product: windows of 3, 5 alternating windows, median ms")
    say("  expected: ridge_bench's figure for the same shape (about 15 ms)")
    res = SB.alternate({"ridge.gram (gemm3, lower 2048-row tiles + mirror copies)": lambda: ridge.gram(X)}, 3, warm=2)
    med = SB.report({q: [t / 1e3 for t in v] for q, v in res.items()})
    verdict("within 10 % of 14.84 ms", abs(list(med.values())[0] - 14.84) <= 1.5)

    # ---- a Ritz matrix and a block Gram matrix from the run: the first pass of the iteration, by hand
    p = pca.PCA(k, n_oversamples=over, n_iter=8)
    K = ridge.gram(X)
    be.gram_center(K, ldn, n, zeros(n + 1))
    info = torch.zeros(8, 3, dtype=torch.int32, device="cuda")
    G = zeros(n, ldm)
    G[:, :m] = torch.randn(n, m, generator=torch.Generator().manual_seed(0)).cuda()
    Q = p._orth(be, p._orth(be, G, n, m, info[0]), n, m, info[1])
    Z, T, S, W, M, th = zeros(n, ldm), zeros(m, ldm), zeros(m, ldm), zeros(m, ldm), zeros(m, ldm), zeros(m)
    kq = lambda: ridge._product(be, K, Q, Z, n, m, n, ldn, ldm, ldm)
    ztz = lambda: ridge._product(be, Z, Z, S, m, m, n, ldm, ldm, ldm, transA=True)
    kq()
    ridge._product(be, Q, Z, T, m, m, n, ldm, ldm, ldm, transA=True)
    T[:, :m] = 0.5 * (T[:, :m] + T[:, :m].t())
    ztz()
    Tt = T[:, :m].contiguous()
    syev = lambda: be.syev_jacobi(T, ldm, m, th, W, ldm, info[2])
    whiten = lambda: be.gram_whiten(S, ldm, m, M, ldm, pca.TAU, th, info[3])
    syev(); whiten()
    words = info.cpu().numpy()
    sweeps, wsweeps = int(words[2, 1]), int(words[3, 1])
    rounds = m - 1 + (m & 1)
    say()
    say(f"2. one decomposition of order {m}: windows of 10, 5 alternating windows, median us")
    say("  expected: LDS traffic of a round is 3 x m x m / 2 rotations x 16 bytes = 393 KB at m = 128, about 1.3 us at 128 bytes per")
    say("  clock, plus three barriers of 16 waves and the float64 phase of one wave: 2 to 3 us per round, 3 to 5 ms for a solve of")
    say("  10 to 12 sweeps; and no slower than torch.linalg.eigh on the same matrix")
    arms = {f"tnt_syev_jacobi_f32 on the first Ritz matrix ({sweeps} sweeps)": syev,
            f"tnt_gram_whiten_f32 on the first Z^T Z ({wsweeps} sweeps)": whiten}
    note = None
    try:
        torch.linalg.eigh(Tt)
        torch.cuda.synchronize()
        arms["torch.linalg.eigh (same matrix, same device)"] = lambda: torch.linalg.eigh(Tt)
    except Exception as e:      # a torch build without a device eigensolver
        note = f"  torch.linalg.eigh on this build raised {type(e).__name__}: {str(e).splitlines()[0][:200]}"
    res = SB.alternate(arms, 10, warm=2)
    med = SB.report(res, width=66)
    keys = list(arms)
    per_round = med[keys[0]] / (sweeps * rounds)
    say(f"  {sweeps} sweeps x {rounds} rounds, 3 barriers per round with a rotation (1 without): {per_round:.2f} us per round; "
        f"whiten {med[keys[1]] / (wsweeps * rounds):.2f} us per round")
    verdict("2 to 3 us per round", 2.0 <= per_round <= 3.0)
    verdict("3 to 5 ms per solve", 3e3 <= med[keys[0]] <= 5e3)
    if note:
        say(note)
    else:
        verdict("no slower than torch.linalg.eigh", med[keys[0]] <= med[keys[2]])

    say()
    say("3. the products of a pass: windows of 20, 5 alternating windows, median us")
    say(f"  expected: Kc Q ({n} x {m} x {n}, {2.0 * n * n * m / 1e9:.1f} GFLOP) near the rate of the Gram product; Z^T Z ({m} x {m} over")
    say(f"  K = {n}) is one to four tiles on 256 CUs when unsplit -- chosen all the same: no exchange buffer, no workgroup waiting for")
    say("  a peer, as ridge's sweeps -- so short of tiles: above 100 us for 0.3 GFLOP")
    res = SB.alternate({"Kc Q": kq, "Z^T Z (unsplit)": ztz}, 20, warm=2)
    med = SB.report(res)
    verdict("Z^T Z above 100 us", med["Z^T Z (unsplit)"] > 100.0)

    say()
    say("4. the whole fit, n_iter = 8: windows of 1, 3 windows, median ms")
    say(f"  expected: the Gram product + {3 * 8 + 3} decompositions at the figure above + {5 * 8 + 8} thin products; slower than")
    say("  torch.pca_lowrank, which never forms the n x n matrix, unless the Gram matrix is shared with ridge (gram=)")
    fit = lambda: pca.PCA(k, n_oversamples=over, n_iter=8).fit(X)
    fit_g = lambda: pca.PCA(k, n_oversamples=over, n_iter=8).fit(X, gram=K0)
    K0 = ridge.gram(X)
    model = fit()
    arms = {"PCA.fit": fit, "PCA.fit(gram=)": fit_g}
    note = None
    try:
        torch.pca_lowrank(X, q=m, center=True, niter=8)
        torch.cuda.synchronize()
        arms[f"torch.pca_lowrank(q = {m}, niter = 8)"] = lambda: torch.pca_lowrank(X, q=m, center=True, niter=8)
    except Exception as e:
        note = f"  torch.pca_lowrank on this build raised {type(e).__name__}: {str(e).splitlines()[0][:200]}"
    res = SB.alternate(arms, 1, reps=3, warm=0)
    med = SB.report({q: [t / 1e3 for t in v] for q, v in res.items()})
    say(f"  n_sweeps_ {model.n_sweeps_}, rank_ {model.rank_}, converged_ {model.converged_}")
    if note:
        say(note)
    else:
        verdict("slower than torch.pca_lowrank", med["PCA.fit"] > med[list(arms)[2]])

    Xq = X[:64].contiguous()
    say()
    say("5. transform of 64 scans: windows of 200, 5 alternating windows, median us")
    say("  expected: one product 64 x 100 x 20000 with its bias, as ridge's predict_embedding (about 320 us at 512 columns)")
    med = SB.report(SB.alternate({"transform (one product with -mean components^T as bias)": lambda: model.transform(Xq)}, 200))
    verdict("at most 320 us", list(med.values())[0] <= 320.0)

    say()
    say("6. the power-law spectrum, singular values i^-0.7 over 1000 directions, n_iter = 8")
    say("  expected: a slowly decaying spectrum leaves the last components short of convergence: residual_ rising from rounding")
    say("  level at the first component to 1e-3 .. 1e-2 at the 100th; the variance captured within 1e-3 of the exact share")
    lam = (sv.double() ** 2)
    exact = float(lam[:k].sum() / lam.sum())
    got = float(model.explained_variance_ratio_.double().sum())
    res_ = model.residual_
    say(f"  residual_: first {res_[0]:.2e}, median {sorted(res_)[k // 2]:.2e}, last {res_[-1]:.2e}, max {res_.max():.2e}")
    say(f"  variance captured by {k} components: {got:.6f}; exact {exact:.6f}")
    verdict("the last residual within 1e-3 .. 1e-2", 1e-3 <= float(res_[-1]) <= 1e-2)
    verdict("variance captured within 1e-3 of the exact share", abs(got - exact) <= 1e-3)
    with open(OUT, "w") as f:
        f.write("\n".join(SB.LINES) + "\n")


if __name__ == "__main__":
    main()
