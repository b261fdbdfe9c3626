"""Timing of ridge decoding (masters_thesis_amd/ridge.py, csrc/cholesky.hip) at the reference's sizes: n = 9000 training
scans, N = 20 000 voxels (config 2), G = 512.  One process, tools/semantic_bench.py's windows (device events around windows
that end in a synchronise, every window warmed first, medians of alternating windows):

  1. the Gram product X X^T (ridge.gram: the lower triangle of 2048-row tiles);
  2. one factorisation (tnt_cholesky_f32), beside the same sequence of block-column products issued alone -- the share of the
     factorisation spent in product launches; the rest is the panel launches -- and beside two yardsticks: a single
     n x n x (n / 3) gemm3 product, the flop-equivalent of the factorisation, and torch.linalg.cholesky on the same device;
  3. one solve with G right-hand sides (tnt_cholesky_solve_f32) beside torch.cholesky_solve;
  4. a full RidgeDecoder fit with cv = 5 over 8 alphas (41 factorisations and solves on one Gram matrix);
  5. predict_embedding for 64 scans.

    python tools/ridge_bench.py [n N G]      # prints, and writes profiles/ridge_bench.txt

Nothing here is a pass / fail threshold."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semantic_bench as SB  # noqa: E402
from masters_thesis_amd import _lib, ops, ridge  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ridge_bench.txt")
say = SB.say


def main():
    n, N, G = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (9000, 20000, 512)
    be = ops.backend()
    say(f"tools/ridge_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {be.lib.tnt_version()}: n = {n}, N = {N}, G = {G}")
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, N, device="cuda", generator=g)
    W = torch.randn(N, G, device="cuda", generator=g) / N ** 0.5
    Y = X @ W + 0.5 * torch.randn(n, G, device="cuda", generator=g)
    alpha = 100.0
    ldn = (n + 3) // 4 * 4
    K = ridge.gram(X)
    L = torch.zeros(n, ldn, device="cuda")
    work = torch.zeros(max(ops.cholesky_work_floats(n), ops.cholesky_solve_work_floats(G)), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    A = torch.zeros(n, G, device="cuda")
    third = torch.zeros(n, ldn, device="cuda")

    def products():
        for j0 in range(64, n, 64):
            ridge._product(be, L[j0:], L[j0:], work, n - j0, min(64, n - j0), j0, ldn, ldn, 64, transB=True)

    def solve():
        A.copy_(Y)
        be.cholesky_solve(L, ldn, n, A, G, G, work, status)

    say()
    say("1. the Gram product: windows of 3, 5 alternating windows, median ms")
    res = SB.alternate({"ridge.gram (gemm3, lower 2048-row tiles + mirror copies)": lambda: ridge.gram(X)}, 3, warm=2)
    SB.report({k: [t / 1e3 for t in v] for k, v in res.items()})
    say(f"  {n} x {n} x {N}: {2.0 * n * n * N / 1e12:.2f} TFLOP in full, half of it computed")

    arms = {
        "tnt_cholesky_f32": lambda: be.cholesky(K, ldn, L, ldn, n, alpha, work, status),
        "its block-column products alone, issued one by one": products,
        f"one gemm3 product {n} x {n} x {n // 3} (the factorisation's flops)": lambda: ridge._product(
            be, K, K, third, n, n, n // 3, ldn, ldn, ldn, transB=True),
        "tnt_cholesky_solve_f32 (with the copy of the right-hand sides)": solve,
    }
    torch_note = []
    try:
        Kt = K[:, :n].clone()
        Kt.diagonal().add_(alpha)
        Lt = torch.linalg.cholesky(Kt)
        torch.cholesky_solve(Y, Lt)
        torch.cuda.synchronize()
        arms["torch.linalg.cholesky (same device)"] = lambda: torch.linalg.cholesky(Kt)
        arms["torch.cholesky_solve (same device)"] = lambda: torch.cholesky_solve(Y, Lt)
    except Exception as e:      # a torch build without a device solver
        torch_note.append(f"  torch.linalg.cholesky / cholesky_solve on this build raised {type(e).__name__}: {str(e).splitlines()[0][:200]}")
    say()
    say(f"2./3. one factorisation and one solve, alpha = {alpha}: windows of 3, 5 alternating windows, median ms")
    res = SB.alternate(arms, 3, warm=2)
    med = SB.report({k: [t / 1e3 for t in v] for k, v in res.items()}, width=66)
    assert int(status.item()) == 0
    for line in torch_note:
        say(line)
    keys = list(arms)
    chol, prod, yard = med[keys[0]], med[keys[1]], med[keys[2]]
    ncol = (n + 63) // 64
    say(f"  {ncol} block columns: products {prod:.2f} ms ({100 * prod / chol:.0f} % of the factorisation), panels and the rest "
        f"{chol - prod:.2f} ms = {1e3 * (chol - prod) / ncol:.1f} us per block column; the factorisation is {chol / yard:.1f} x its "
        "flop-equivalent product")
    say(f"  the solve: {2 * ncol - 1} products and {2 * ncol} triangular launches, {1e3 * med[keys[3]] / (2 * ncol):.1f} us per block step")

    say()
    alphas = [1.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7]
    fit = lambda: ridge.RidgeDecoder(alphas=alphas, cv=5).fit(X, Y)
    model = fit()
    say(f"4. RidgeDecoder(alphas = 8 values, cv = 5).fit: windows of 1, 3 windows, median ms (alpha_ = {model.alpha_})")
    res = SB.alternate({"fit, cv = 5 x 8 alphas + the refit": fit}, 1, reps=3, warm=0)
    SB.report({k: [t / 1e3 for t in v] for k, v in res.items()})
    Xq = X[:64].contiguous()
    say()
    say("5. predict_embedding for 64 scans: windows of 200, 5 alternating windows, median us")
    SB.report(SB.alternate({"predict_embedding (one product with the intercept as bias)": lambda: model.predict_embedding(Xq)}, 200))
    with open(OUT, "w") as f:
        f.write("\n".join(SB.LINES) + "\n")


if __name__ == "__main__":
    main()
