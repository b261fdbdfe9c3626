"""CPU stand-in for the two entries of csrc/eigen.hip -- TEST INFRASTRUCTURE ONLY -- on top of the mock of the ridge entries:
float32 storage, float64 ``eigh``, and the semantics of include/tnt_hip.h (only the lower triangle read, w descending, the
sign rule, the three info words, a non-finite entry leaving w and V alone, the whiten scaling and its numerical rank)."""
import numpy as np

from mock_backend import flat, mat
from ridge_mock import RidgeMockBackend


def _eig(a):
    """(w descending, V with the sign rule) of the symmetric float64 matrix a"""
    w, V = np.linalg.eigh(a)
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    for i in range(len(w)):
        if V[np.argmax(np.abs(V[:, i])), i] < 0:
            V[:, i] = -V[:, i]
    return w, V


def _lower(A, m, ld):
    a = np.tril(mat(A, m, m, ld).astype(np.float64))
    return a + np.tril(a, -1).T, bool(np.all(np.isfinite(a)))


class PcaMockBackend(RidgeMockBackend):
    force_info = 0            # tests: the info[0] every decomposition reports in place of 0

    def syev_jacobi(self, A, lda, m, w, V, ldv, info, max_sweeps=64):
        assert 1 <= m <= 128 and lda >= m and ldv >= m and lda % 4 == 0 and ldv % 4 == 0 and 1 <= max_sweeps <= 64
        assert info.numel() >= 3 and w.numel() >= m
        a, finite = _lower(A, m, lda)
        if not finite:
            flat(info)[:3] = (2, 0, m)
            return
        ev, vec = _eig(a)
        flat(w)[:m] = ev
        mat(V, m, m, ldv)[...] = vec
        flat(info)[:3] = (self.force_info, 1, m)

    def gram_whiten(self, S, lds, m, M, ldm, tau, w, info):
        assert 1 <= m <= 128 and lds >= m and ldm >= m and lds % 4 == 0 and ldm % 4 == 0 and 0 < tau < 1
        assert info.numel() >= 3 and w.numel() >= m
        s, finite = _lower(S, m, lds)
        if not finite:
            flat(info)[:3] = (2, 0, 0)
            return
        d = np.diag(s)
        r = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), 0.0)
        ev, vec = _eig((s * r[:, None] * r[None, :]).astype(np.float32).astype(np.float64))
        ev = ev.astype(np.float32).astype(np.float64)
        cut = np.float64(np.float32(tau)) * ev[0]
        den = np.maximum(ev, cut)
        scale = np.where(den > 0, 1 / np.sqrt(np.where(den > 0, den, 1)), 0.0)
        flat(w)[:m] = ev
        mat(M, m, m, ldm)[...] = r[:, None] * vec * scale[None, :]
        flat(info)[:3] = (self.force_info, 1, int(np.sum(ev > cut)))
