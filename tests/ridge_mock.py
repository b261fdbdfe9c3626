"""CPU stand-in for the three entries of csrc/cholesky.hip -- TEST INFRASTRUCTURE ONLY -- on top of the mock of the
sentence-embedding entries: float32 storage, float64 arithmetic, the semantics of include/tnt_hip.h (only the lower triangle
of K read, only the lower triangle of L written, the status word, a nonzero status leaving X alone).  ``gemm3`` /
``gemm3_plan`` stand in for the unsplit gemm3 route that ridge.py takes where the strides allow it."""
import numpy as np

from mock_backend import flat, mat
from semantic_oracle import SemanticMockBackend


class RidgeMockBackend(SemanticMockBackend):
    force_status = 0          # tests: the value every factorisation files instead of its own

    def gemm3_plan(self, M, N, K, transA=False, transB=False, batch=1, allow_split=True):
        assert not allow_split, "ridge.py asks for the unsplit plan: no exchange buffer"
        return 7, 1

    def gemm3(self, A, B, C, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, colsum=None, A2=None, C2=None,
              tile=1, splitk=1, work=None, sync=None, live=None, live_mode=0):
        assert lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and splitk == 1 and work is None and sync is None
        assert colsum is None and A2 is None and live is None
        self.gemm(A, B, C, M, N, K, lda, ldb, ldc, transA=transA, transB=transB, bias=bias)

    def cholesky(self, K, ldk, L, ldl, n, shift, work, status):
        assert 1 <= n <= 32768 and ldk >= n and ldl >= n and ldk % 4 == 0 and ldl % 4 == 0
        assert work is not None and work.numel() >= 64 * n and status is not None
        a = np.tril(mat(K, n, n, ldk).astype(np.float64))
        a[np.diag_indices(n)] += np.float64(np.float32(shift))
        flat(status)[0] = self.force_status
        if self.force_status:
            return
        out = np.zeros((n, n))
        for k in range(n):                       # row by row: the first bad pivot in row order
            d = a[k, k] - out[k, :k] @ out[k, :k]
            if not (d > 0) or not np.isfinite(d):
                flat(status)[0] = 1 + k
                return
            out[k, k] = np.sqrt(d)
            out[k + 1:, k] = (a[k + 1:, k] - out[k + 1:, :k] @ out[k, :k]) / out[k, k]
        l = mat(L, n, n, ldl)
        low = np.tril_indices(n)
        l[low] = out[low]

    def cholesky_solve(self, L, ldl, n, X, ldx, G, work, status):
        assert 1 <= n <= 32768 and ldl >= n and ldl % 4 == 0 and G >= 1 and ldx >= G and ldx % 4 == 0
        assert work is not None and work.numel() >= 64 * ldx and status is not None
        if flat(status)[0] != 0:
            return
        l = np.tril(mat(L, n, n, ldl).astype(np.float64))
        x = mat(X, n, G, ldx)
        x[...] = np.linalg.solve(l.T, np.linalg.solve(l, x.astype(np.float64)))

    def gram_center(self, K, ldk, n, mean):
        assert 1 <= n <= 32768 and ldk >= n and ldk % 4 == 0 and mean.numel() >= n + 1
        k = mat(K, n, n, ldk)
        m = (k.astype(np.float64).sum(1) / n).astype(np.float32)
        g = m.astype(np.float64).sum() / n
        flat(mean)[:n] = m
        flat(mean)[n] = g
        k[...] = k.astype(np.float64) - m.astype(np.float64)[:, None] - m.astype(np.float64)[None, :] + g
