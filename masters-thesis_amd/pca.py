"""PCA of the scans on the device: the reference reduces a subject's 9000 x 327 684 betas before anything else
(AttemptFour/pca.py: TruncatedSVD / PCA, the singular values, the explained variance and its ratio, the components).  Here
the leading eigenpairs of the n x n Gram matrix give the same quantities without ever copying or centring the scans:

    Kc = H K H,  K = X X^T,  H = I - 11^T/n      (ridge.gram, then tnt_gram_center_f32; K itself with center=False)
    m  = min(n, n_components + n_oversamples)    (<= 128: the order tnt_syev_jacobi_f32 takes)
    Q  = orth(orth(G)),  G (n, m) standard normal from torch.Generator(seed) on the host
    repeat n_iter + 1 times:
        Z = Kc Q;  T = Q^T Z, symmetrised;  (theta, W) = tnt_syev_jacobi_f32(T)
        last pass: U = Q W, stop
        Q = orth(orth(Z W))
    orth(Z):  S = Z^T Z;  M = tnt_gram_whiten_f32(S, tau = 2^-20);  Z M

-- block subspace iteration with a Rayleigh-Ritz step in every pass.  Every product is a launch of the library's gemm3
family (ridge._product), every decomposition one launch of csrc/eigen.hip (definitions in include/tnt_hip.h); means, the
sign rule and the symmetrisation of the m x m Ritz matrix are torch (plumbing).  Nothing synchronises during a fit: the info
words of all decompositions and the residuals cross the bus once, after the last launch.

    singular_values_           s = sqrt(max(theta, 0))[:k]
    components_ (k, N)         diag(1/s) (H U)^T X: one product; unit rows; the sign is that of U's columns, each negated
                               where needed so that its entry of largest magnitude (the first on ties) is positive
    mean_ (N,)                 the column means (zeros with center=False)
    explained_variance_        s^2 / (n - 1)
    explained_variance_ratio_  against trace(Kc) / (n - 1)
    residual_ (k,)             ||Kc u_i - theta_i u_i|| / theta_0, from one more product: how far n_iter got (numpy)
    n_sweeps_, rank_           the largest sweep count and the smallest numerical rank any decomposition reported
    converged_                 False (with a warning) when a decomposition ran out of sweeps

With center=False singular_values_ and components_ are TruncatedSVD's; the variance attributes keep the formulas above
(second moments about zero), which differ from scikit-learn's TruncatedSVD (variances of the transformed columns).

Limits.  m <= 128 (a block Jacobi over 128-wide sub-problems on the same kernel is the known next step).  float32.  And
z-scored inputs: centring the Gram matrix of UNCENTRED scans cancels in float32 when the column means dwarf the variation
about them (a CPU prototype lost every digit at mean 3, standard deviation 0.05).  The reference's betas are z-scored per
voxel, which is the intended case; other data should be centred first.
"""
import os
import warnings

import numpy as np
import torch

from . import ops, ridge
from .ridge import _device, _product, _r4, _rows4, _tensor

M_MAX = 128              # tnt_syev_jacobi_f32 / tnt_gram_whiten_f32
N_MAX = ridge.N_MAX      # tnt_gram_center_f32
TAU = 2.0 ** -20         # the relative floor of tnt_gram_whiten_f32's eigenvalues
FILES = {"singular_values_": "pca_sing_values.npy", "explained_variance_ratio_": "pca_expl_var_ratio.npy",
         "explained_variance_": "pca_expl_var.npy", "components_": "pca_components.npy", "mean_": "pca_mean.npy"}


class PCAError(RuntimeError):
    """A decomposition met a non-finite entry: the scans (or the Gram matrix handed in) hold a NaN or an Inf."""


def _int(v, name, low):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
        raise ValueError(f"{name} must be an integer >= {low}, got {v!r}")
    return int(v)


class PCA:
    """Principal components of the rows of X (n, N) by block subspace iteration on the centred Gram matrix (module text).
    ``n_components`` = k; ``n_oversamples`` extra columns carried by the iteration (k + n_oversamples <= 128); ``n_iter``
    passes after the first Rayleigh-Ritz step; ``center=False``: the uncentred decomposition (TruncatedSVD); ``whiten``:
    transform divides by sqrt(explained_variance_); ``seed``: the start block.  The attributes are device tensors."""

    def __init__(self, n_components, n_oversamples=10, n_iter=8, center=True, whiten=False, seed=0, device=None):
        self.n_components = _int(n_components, "n_components", 1)
        self.n_oversamples = _int(n_oversamples, "n_oversamples", 0)
        self.n_iter = _int(n_iter, "n_iter", 0)
        if self.n_components + self.n_oversamples > M_MAX:
            raise ValueError(f"n_components + n_oversamples must not exceed {M_MAX} (the order tnt_syev_jacobi_f32 takes), got "
                             f"{self.n_components} + {self.n_oversamples}")
        self.center, self.whiten, self.seed = bool(center), bool(whiten), _int(seed, "seed", 0)
        self.device = _device(device)
        self.components_ = self.mean_ = self.singular_values_ = None
        self.explained_variance_ = self.explained_variance_ratio_ = self.residual_ = None
        self.n_sweeps_ = self.rank_ = self.converged_ = None

    # ------------------------------------------------------------------------------------------------ pieces of a fit
    def _orth(self, be, Z, n, m, info):
        """Z M with M = tnt_gram_whiten_f32(Z^T Z): two products and one decomposition; info: its three words"""
        ldm = Z.shape[1]
        dev = Z.device
        S = torch.zeros(m, ldm, dtype=torch.float32, device=dev)
        _product(be, Z, Z, S, m, m, n, ldm, ldm, ldm, transA=True)
        M = torch.zeros(m, ldm, dtype=torch.float32, device=dev)
        be.gram_whiten(S, ldm, m, M, ldm, TAU, torch.zeros(m, dtype=torch.float32, device=dev), info)
        Q = torch.zeros(n, ldm, dtype=torch.float32, device=dev)
        _product(be, Z, M, Q, n, m, m, ldm, ldm, ldm)
        return Q

    def _set(self, comp, mean, s, ev, ratio, N):
        """the state transform / inverse_transform work from: components and mean in the library's layout"""
        k, dev = self.n_components, self.device
        ldN, ldk = _r4(N), _r4(k)
        C = torch.zeros(k, ldN, dtype=torch.float32, device=dev)
        C[:, :N] = comp
        mu = torch.zeros(1, ldN, dtype=torch.float32, device=dev)
        mu[0, :N] = mean
        scale = torch.ones(k, dtype=torch.float32, device=dev)
        if self.whiten:
            sd = ev.double().sqrt()
            scale = torch.where(sd > 0, 1.0 / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.zeros_like(sd)).float()
        T = C * scale[:, None]                                  # what transform multiplies by
        shift = torch.zeros(1, ldk, dtype=torch.float32, device=dev)
        _product(ops.backend(), mu, T, shift, 1, k, N, ldN, ldN, ldk, transB=True)
        self._C, self._T, self._mu, self._bias = C, T, mu[0], -shift[0]
        self._N, self._ldN, self._ldk = N, ldN, ldk
        self.components_, self.mean_ = C[:, :N], mu[0, :N]
        self.singular_values_, self.explained_variance_, self.explained_variance_ratio_ = s, ev, ratio

    # ------------------------------------------------------------------------------------------------ fit
    def _fit(self, X, gram):
        dev, k = self.device, self.n_components
        X = _tensor(X, dev)
        if X.dim() != 2 or X.shape[1] < 1:
            raise ValueError(f"X is a 2-D array (n, N), got shape {tuple(X.shape)}")
        n, N = int(X.shape[0]), int(X.shape[1])
        if not 2 <= n <= N_MAX:
            raise ValueError(f"the number of rows must lie in [2, {N_MAX}] (tnt_gram_center_f32), got {n}")
        if k > min(n - 1, N):
            raise ValueError(f"n_components must not exceed min(n - 1, N) = {min(n - 1, N)}, got {k}")
        ldn = _r4(n)
        if gram is not None:
            gram = _tensor(gram, dev)
            if gram.dim() != 2 or gram.shape[0] != n or gram.shape[1] not in (n, ldn):
                raise ValueError(f"gram must be the ({n}, {ldn}) matrix of ridge.gram(X), got shape {tuple(gram.shape)}")
        be = ops.backend()
        X4, ldx = _rows4(X)
        if gram is None:
            K = ridge.gram(X4[:, :N], ldx, be)
        else:                                                  # a copy: the centring is in place and the caller keeps theirs
            K = torch.zeros(n, ldn, dtype=torch.float32, device=dev)
            K[:, :n] = gram[:, :n]
        if self.center:
            be.gram_center(K, ldn, n, torch.zeros(n + 1, dtype=torch.float32, device=dev))
            mean = X.mean(0, dtype=torch.float64).to(torch.float32)
        else:
            mean = torch.zeros(N, dtype=torch.float32, device=dev)
        trace = torch.diagonal(K[:, :n]).sum(dtype=torch.float64)

        m = min(n, k + self.n_oversamples)
        ldm = _r4(m)
        ncalls = 3 * self.n_iter + 3
        info = torch.zeros(ncalls, 3, dtype=torch.int32, device=dev)
        rows = iter(info)
        G = torch.zeros(n, ldm, dtype=torch.float32)
        G[:, :m] = torch.randn(n, m, generator=torch.Generator().manual_seed(self.seed), dtype=torch.float32)
        Q = self._orth(be, self._orth(be, G.to(dev), n, m, next(rows)), n, m, next(rows))
        theta = torch.zeros(m, dtype=torch.float32, device=dev)
        Z = torch.zeros(n, ldm, dtype=torch.float32, device=dev)
        T = torch.zeros(m, ldm, dtype=torch.float32, device=dev)
        W = torch.zeros(m, ldm, dtype=torch.float32, device=dev)
        for it in range(self.n_iter + 1):
            _product(be, K, Q, Z, n, m, n, ldn, ldm, ldm)
            _product(be, Q, Z, T, m, m, n, ldm, ldm, ldm, transA=True)
            T[:, :m] = 0.5 * (T[:, :m] + T[:, :m].t())
            be.syev_jacobi(T, ldm, m, theta, W, ldm, next(rows))
            Y = torch.zeros(n, ldm, dtype=torch.float32, device=dev)
            if it == self.n_iter:
                _product(be, Q, W, Y, n, m, m, ldm, ldm, ldm)                  # U = Q W
                break
            _product(be, Z, W, Y, n, m, m, ldm, ldm, ldm)
            Q = self._orth(be, self._orth(be, Y, n, m, next(rows)), n, m, next(rows))
        U = Y
        # the kernel's sign rule on U's columns: the entry of largest magnitude, the first on ties, is positive
        mag = U[:, :m].abs()
        first = torch.where(mag == mag.max(0).values, torch.arange(n, device=dev)[:, None], n - 1).min(0).values    # (n - 1: a NaN column matches nowhere)
        sign = torch.where(U[first, torch.arange(m, device=dev)] < 0, -1.0, 1.0).to(torch.float32)
        U[:, :m] *= sign
        KU = torch.zeros(n, ldm, dtype=torch.float32, device=dev)
        _product(be, K, U, KU, n, m, n, ldn, ldm, ldm)                         # the residuals' product
        th = theta.double()
        resid = (KU[:, :k].double() - U[:, :k].double() * th[:k]).norm(dim=0) / th[0]

        s64 = th.clamp_min(0).sqrt()[:k]
        inv = torch.where(s64 > 0, 1.0 / torch.where(s64 > 0, s64, torch.ones_like(s64)), torch.zeros_like(s64))
        ldk = _r4(k)
        HU = torch.zeros(n, ldk, dtype=torch.float32, device=dev)
        Uk = U[:, :k].double()
        if self.center:
            Uk = Uk - Uk.mean(0)
        HU[:, :k] = (Uk * inv).to(torch.float32)
        comp = torch.zeros(k, ldx, dtype=torch.float32, device=dev)
        _product(be, HU, X4, comp, k, N, n, ldk, ldx, ldx, transA=True)       # diag(1/s) (H U)^T X

        host = torch.cat([info.reshape(-1).double(), resid]).cpu().numpy()     # the one transfer of the fit
        words = host[:3 * ncalls].astype(np.int64).reshape(ncalls, 3)
        if (words[:, 0] == 2).any():
            raise PCAError("a decomposition met a non-finite entry: the scans or the Gram matrix hold a NaN or an Inf")
        self.converged_ = not (words[:, 0] == 1).any()
        if not self.converged_:
            warnings.warn("pca.PCA: a Jacobi decomposition did not converge within its sweeps; the results are what the "
                          "last sweep left", RuntimeWarning, stacklevel=3)
        self.n_sweeps_ = int(words[:, 1].max())
        self.rank_ = int(words[:, 2].min())
        s = s64.to(torch.float32)
        ev = (s64 * s64 / (n - 1)).to(torch.float32)
        ratio = (s64 * s64 / trace).to(torch.float32)
        self._set(comp[:, :N], mean, s, ev, ratio, N)
        self.residual_ = host[3 * ncalls:].astype(np.float32)             # (numpy: it came over with the info words)
        return U[:, :k] * s

    def fit(self, X, gram=None):
        """fit on the rows of X (n, N), numpy or a device tensor (used in place where it has the library's layout, as
        ridge._rows4 says); ``gram``: the UNCENTRED matrix of ridge.gram(X) where the caller already has it"""
        self._fit(X, gram)
        return self

    def fit_transform(self, X, gram=None):
        """the scores of the training rows, U diag(s) (n, k), from the fit itself: no product over N"""
        scores = self._fit(X, gram)
        if self.whiten:
            scores = scores / self.explained_variance_.sqrt()
        return scores

    # ------------------------------------------------------------------------------------------------ use
    def _fitted(self):
        if self.components_ is None:
            raise ValueError("fit the PCA first")

    def transform(self, X):
        """(B, k) device tensor: (X - mean_) components_^T, one product with -mean_ components_^T as its bias"""
        self._fitted()
        X = _tensor(X, self.device)
        if X.dim() != 2 or X.shape[1] != self._N or X.shape[0] < 1:
            raise ValueError(f"X of shape {tuple(X.shape)} for a PCA fitted on {self._N} columns")
        X4, ldx = _rows4(X)
        B, k = int(X.shape[0]), self.n_components
        out = torch.zeros(B, self._ldk, dtype=torch.float32, device=self.device)
        _product(ops.backend(), X4, self._T, out, B, k, self._N, ldx, self._ldN, self._ldk, transB=True, bias=self._bias)
        return out[:, :k]

    def inverse_transform(self, Z):
        """(B, N) device tensor: Z components_ + mean_ (Z scaled back first with whiten=True)"""
        self._fitted()
        Z = _tensor(Z, self.device)
        k = self.n_components
        if Z.dim() != 2 or Z.shape[1] != k or Z.shape[0] < 1:
            raise ValueError(f"Z of shape {tuple(Z.shape)} for a PCA of {k} components")
        if self.whiten:
            Z = Z * self.explained_variance_.sqrt()
        Z4, ldz = _rows4(Z)
        B = int(Z.shape[0])
        out = torch.zeros(B, self._ldN, dtype=torch.float32, device=self.device)
        _product(ops.backend(), Z4, self._C, out, B, self._N, k, ldz, self._ldN, self._ldN, bias=self._mu)
        return out[:, :self._N]

    def save(self, directory):
        """the reference's files (AttemptFour/pca.py) plus the mean: pca_sing_values.npy, pca_expl_var_ratio.npy,
        pca_expl_var.npy, pca_components.npy, pca_mean.npy"""
        self._fitted()
        os.makedirs(directory, exist_ok=True)
        for attr, name in FILES.items():
            np.save(os.path.join(directory, name), getattr(self, attr).cpu().numpy())

    @classmethod
    def load(cls, directory, whiten=False, device=None):
        """a PCA that transforms as the saved one did (residual_, n_sweeps_ and rank_ are not kept)"""
        a = {attr: np.load(os.path.join(directory, name)) for attr, name in FILES.items()}
        comp = a["components_"]
        if comp.ndim != 2 or a["mean_"].shape != (comp.shape[1],) or any(a[x].shape != (comp.shape[0],) for x in (
                "singular_values_", "explained_variance_", "explained_variance_ratio_")):
            raise ValueError(f"the files under {directory!r} do not fit together")
        p = cls(int(comp.shape[0]), n_oversamples=0, whiten=whiten, device=device)
        t = lambda x: _tensor(x, p.device)
        p._set(t(comp), t(a["mean_"]), t(a["singular_values_"]), t(a["explained_variance_"]),
               t(a["explained_variance_ratio_"]), int(comp.shape[1]))
        return p


class project:
    """A DataGenerator / SyntheticGenerator whose betas are replaced by ``p.transform(betas)``: the same length, every other
    array of a batch as it was, the components in the array type the wrapped generator yields -- so nic.NIC trains on
    components and ridge.stack(pca.project(gen, p)) feeds principal-component regression."""

    def __init__(self, generator, p):
        p._fitted()
        self.generator, self.pca = generator, p

    def __len__(self):
        return len(self.generator)

    def on_epoch_end(self):
        self.generator.on_epoch_end()

    def __getitem__(self, index):
        x, y = self.generator[index]
        betas = x[0]
        z = self.pca.transform(betas)
        z = z.to(betas.device) if isinstance(betas, torch.Tensor) else z.cpu().numpy()
        return (z,) + tuple(x[1:]), y
