"""Ridge decoding of sentence embeddings: the linear baseline of the fMRI-decoding literature -- ridge regression from the
voxels straight to the caption's sentence embedding -- on the device, in its dual form.

    mu_x, mu_y   the column means of the training rows (0 with fit_intercept=False)
    Kc           the Gram matrix of the centred rows, H X X^T H, H = I - 11^T/n    (n x n; one product, centred in place)
    A            solves (Kc + alpha I) A = Y - mu_y                                 (dual_coef_)
    coef_        X^T (H A)                                                          (N x G; one product)
    intercept_   mu_y - mu_x coef_
    prediction   x coef_ + intercept_

The Gram matrix is a product of the library's gemm3 family (through the backend, as evaluate.semantic_retrieve calls it
without a model); the factorisation, the triangular solves and the centring are csrc/cholesky.hip (tnt_cholesky_f32,
tnt_cholesky_solve_f32, tnt_gram_center_f32; definitions in include/tnt_hip.h).  Choosing alpha -- by k folds or by a held-out
set -- reuses the ONE uncentred Gram matrix: a fold's training block and its cross block are index gathers, centred with that
fold's means; nothing is recomputed from the scans.  Gathers, means and the score arithmetic are torch (plumbing); every
product, factorisation and solve is a HIP launch.  The status words of all factorisations travel to the host once, with the
scores; nothing synchronises per launch.

A RidgeDecoder has ``predict_embedding`` (the name nic.NIC uses) and ``gemm_sk``, so evaluate.semantic_retrieve and
evaluate.semantic_identification take it in place of a trained network.
"""
import math

import numpy as np
import torch

from . import ops

N_MAX = 32768            # tnt_cholesky_f32
_G3_REACH = 1 << 29      # gemm3 addresses an operand with 32-bit offsets: rows * stride stays below this
_GRAM_BLOCK = 2048       # rows per Gram tile: 32 x 32 tiles of 64 at the most, a grid the gemm3 plan accepts


class RidgeError(RuntimeError):
    """A factorisation met a pivot that is not a positive finite number: K + alpha I is not positive definite in float32 (or
    the data hold a NaN / Inf).  ``pivot`` is the 0-based row of that pivot."""

    def __init__(self, pivot, what):
        super().__init__(f"Cholesky factorisation failed at pivot {pivot} ({what}): K + alpha I is not positive definite in "
                         "float32, or the inputs are not finite")
        self.pivot = int(pivot)


def _r4(v):
    return (int(v) + 3) // 4 * 4


def _device(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _tensor(a, dev):
    """a float32 tensor on ``dev``; a tensor that already is one is returned as it is (no copy)"""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, np.float32))
    return t.to(device=dev, dtype=torch.float32)


def _rows4(X):
    """(buffer, stride) of a 2-D tensor in the library's layout: contiguous rows at a stride that is a multiple of 4, zeros in
    the pad columns, 16-byte aligned.  A tensor that already has it is used in place."""
    rows, cols = X.shape
    if X.is_contiguous() and cols % 4 == 0 and X.data_ptr() % 16 == 0:
        return X, cols
    buf = torch.zeros(rows, _r4(cols), dtype=torch.float32, device=X.device)
    buf[:, :cols] = X
    return buf, _r4(cols)


def _product(be, A, B, C, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None):
    """C = op(A) op(B) (+ bias): gemm3 at the unsplit tile of its cost model where its layout contract holds (strides that
    are multiples of 4, operands within its 32-bit reach), the tiled tnt_gemm_f32 otherwise"""
    rows_a, rows_b = (K if transA else M), (N if transB else K)
    if (hasattr(be, "gemm3") and lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and rows_a * lda < _G3_REACH
            and rows_b * ldb < _G3_REACH):
        tile, _ = be.gemm3_plan(M, N, K, transA, transB, 1, False)
        be.gemm3(A, B, C, M, N, K, lda, ldb, ldc, transA=transA, transB=transB, bias=bias, tile=tile, splitk=1)
    else:
        be.gemm(A, B, C, M, N, K, lda, ldb, ldc, transA=transA, transB=transB, bias=bias)


def gram(X, ldx=None, be=None):
    """The uncentred Gram matrix X X^T of the rows of X (n, N) as an (n, roundup4(n)) float32 tensor, pad columns zero.  One
    product where it fits; above 2048 rows (or where rows * stride passes gemm3's reach) the lower triangle of 2048-row tiles,
    one launch each, the upper tiles copied from their mirror images -- so K is symmetric to the bit."""
    be = be or ops.backend()
    if ldx is None:
        X, ldx = _rows4(X)
    n, N = int(X.shape[0]), int(X.shape[1])
    ldn = _r4(n)
    K = torch.zeros(n, ldn, dtype=torch.float32, device=X.device)
    blk = min(_GRAM_BLOCK, max(1, (_G3_REACH - 1) // ldx))
    if blk < n:
        blk = max(64, blk // 64 * 64)
    for r0 in range(0, n, blk):
        r1 = min(n, r0 + blk)
        for c0 in range(0, r0 + 1, blk):
            c1 = min(n, c0 + blk)
            _product(be, X[r0:], X[c0:], K[r0:, c0:], r1 - r0, c1 - c0, N, ldx, ldx, ldn, transB=True)
            if c0 < r0:
                K[c0:c1, r0:r1] = K[r0:r1, c0:c1].t()
    return K


def kfold(n, k, groups=None):
    """fold index (n,) int64 of every row.  Without groups: scikit-learn's unshuffled KFold -- contiguous folds, the first
    n % k of them one row longer.  With groups (n,): fold = rank(group id) % k, rank over the sorted distinct ids, so the
    rows of a group (the three trials of one image) never straddle a fold."""
    if groups is None:
        sizes = np.full(k, n // k, np.int64)
        sizes[:n % k] += 1
        return np.repeat(np.arange(k, dtype=np.int64), sizes)
    _, rank = np.unique(np.asarray(groups), return_inverse=True)
    return (rank.reshape(-1) % k).astype(np.int64)


def stack(generator, steps=None, device=None):
    """(betas (n, N), embeddings (n, G)) of an epoch of a DataGenerator(load_guse=) / SyntheticGenerator(guse_dim=), as two
    float32 device tensors: the first and the fifth input of every batch, in batch order; ``steps``: the first batches only."""
    total = len(generator)
    if steps is not None:
        if isinstance(steps, bool) or int(steps) != steps or not 1 <= steps <= total:
            raise ValueError(f"steps must be None or an integer in [1, {total}], got {steps!r}")
        total = int(steps)
    if total < 1:
        raise ValueError("the generator holds no batch")
    dev = _device(device)
    xs, gs = [], []
    for i in range(total):
        x = generator[i][0]
        if len(x) < 5:
            raise ValueError("the generator yields no sentence embedding: build it with load_guse= (DataGenerator) or "
                             "guse_dim= (SyntheticGenerator)")
        xs.append(_tensor(x[0], dev))
        gs.append(_tensor(x[4], dev))
    return torch.cat(xs, 0), torch.cat(gs, 0)


def _check_alpha(a, name):
    if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not math.isfinite(a) or a <= 0:
        raise ValueError(f"{name} must be a finite number > 0, got {a!r}")
    return float(a)


class RidgeDecoder:
    """Ridge regression from scans (n, N) to sentence embeddings (n, G) in the dual form (module text).  ``alpha``: the
    regularisation strength; ``alphas``: candidates, one of which is chosen by ``cv`` = k folds (``groups`` (n,) keeps the rows
    of a group in one fold) or by ``validation`` = (betas_v, targets_v), scored by ``score`` = "cosine" (the mean over the
    validation rows of cos(prediction, target), tnt_cosine_loss_f32's cos_row: an all-zero row counts with cos = 0) or "r2"
    (the mean over the columns of R^2); the first maximiser in the order given wins and the model is refitted on all rows.
    After fit: coef_ (N, G), intercept_ (G,), dual_coef_ (n, G) as device tensors, alpha_, cv_scores_ (len(alphas),) numpy."""

    def __init__(self, alpha=1.0, alphas=None, cv=None, groups=None, validation=None, score="cosine", fit_intercept=True,
                 device=None):
        self.alpha = _check_alpha(alpha, "alpha")
        self.alphas = None
        if alphas is not None:
            self.alphas = [_check_alpha(a, "every entry of alphas") for a in list(alphas)]
            if not self.alphas:
                raise ValueError("alphas is empty")
        if score not in ("cosine", "r2"):
            raise ValueError(f"score must be 'cosine' or 'r2', got {score!r}")
        if cv is not None and (isinstance(cv, bool) or not isinstance(cv, (int, np.integer)) or cv < 2):
            raise ValueError(f"cv must be an integer in [2, n], got {cv!r}")
        if validation is not None and (not isinstance(validation, (tuple, list)) or len(validation) != 2):
            raise ValueError("validation must be a pair (betas, targets)")
        if self.alphas is None:
            if cv is not None or validation is not None or groups is not None:
                raise ValueError("cv, groups and validation choose among alphas: give alphas= as well")
        else:
            if (cv is None) == (validation is None):
                raise ValueError("alphas needs exactly one of cv= and validation= to choose by")
            if groups is not None and cv is None:
                raise ValueError("groups assigns rows to folds: it needs cv=")
        self.cv = None if cv is None else int(cv)
        self.groups, self.validation, self.score = groups, validation, score
        self.fit_intercept = bool(fit_intercept)
        self.device = _device(device)
        self.coef_ = self.intercept_ = self.dual_coef_ = self.alpha_ = self.cv_scores_ = None

    # ------------------------------------------------------------------------------------------------ pieces of a fit
    def _solve_all(self, be, Kc, n, Yc, alphas, status):
        """for every alpha: factor Kc + alpha I and solve for the centred targets; yields (index, A (n, ldg)).  ``status``:
        one int32 word per alpha."""
        ldn, ldg = Kc.shape[1], Yc.shape[1]
        G = self._G
        L = torch.zeros(n, ldn, dtype=torch.float32, device=Kc.device)
        work = torch.zeros(max(ops.cholesky_work_floats(n), ops.cholesky_solve_work_floats(ldg)), dtype=torch.float32,
                           device=Kc.device)
        for i, a in enumerate(alphas):
            st = status[i:i + 1]
            be.cholesky(Kc, ldn, L, ldn, n, a, work, st)
            A = Yc.clone()
            be.cholesky_solve(L, ldn, n, A, ldg, G, work, st)
            yield i, A

    def _centre(self, be, K, n):
        """K <- H K H in place; (row means (n,), grand mean) or (None, None) without an intercept"""
        if not self.fit_intercept:
            return None, None
        mean = torch.zeros(n + 1, dtype=torch.float32, device=K.device)
        be.gram_center(K, K.shape[1], n, mean)
        return mean[:n], mean[n]

    def _targets(self, Y):
        """(mu_y (G,), the centred targets in an (n, roundup4(G)) buffer)"""
        G = self._G
        mu = Y.mean(0, dtype=torch.float64).to(torch.float32) if self.fit_intercept else torch.zeros(G, dtype=torch.float32,
                                                                                                  device=Y.device)
        Yc = torch.zeros(Y.shape[0], _r4(G), dtype=torch.float32, device=Y.device)
        Yc[:, :G] = Y - mu
        return mu, Yc

    def _score(self, be, pred, ldp, Yv):
        """the score of predictions (nv, ldp) against targets (nv, G): a 0-d device tensor"""
        nv, G = int(Yv.shape[0]), self._G
        if self.score == "cosine":
            Yv4, ldg = _rows4(Yv)
            loss_row = torch.zeros(nv, dtype=torch.float32, device=pred.device)
            cos_row = torch.zeros(nv, dtype=torch.float32, device=pred.device)
            be.cosine_loss(pred, ldp, Yv4, ldg, None, loss_row, cos_row, None, nv, G, 0.0)
            return cos_row.mean(dtype=torch.float64)
        p, y = pred[:, :G].double(), Yv.double()
        num = ((y - p) ** 2).sum(0)
        den = ((y - y.mean(0)) ** 2).sum(0)
        r2 = torch.where(den > 0, 1.0 - num / torch.where(den > 0, den, torch.ones_like(den)),
                         torch.where(num > 0, torch.zeros_like(num), torch.ones_like(num)))
        return r2.mean()

    def _validate(self, be, Ktr, ntr, Kva, Ytr, Yva, scores, status):
        """one training / validation split: Ktr (ntr, ld) the uncentred training Gram (centred in place here), Kva (nv, ntr)
        the uncentred cross-Gram; scores (len(alphas),) and status (len(alphas),) are filled"""
        G, nv = self._G, int(Kva.shape[0])
        m, g = self._centre(be, Ktr, ntr)
        if m is not None:
            Kva = Kva - Kva.mean(1, keepdim=True, dtype=torch.float64).to(torch.float32) - m[None, :] + g
        Kva4, ldv = _rows4(Kva)
        mu, Yc = self._targets(Ytr)
        ldg = Yc.shape[1]
        bias = torch.zeros(ldg, dtype=torch.float32, device=Ktr.device)
        bias[:G] = mu
        for i, A in self._solve_all(be, Ktr, ntr, Yc, self.alphas, status):
            pred = torch.zeros(nv, ldg, dtype=torch.float32, device=Ktr.device)
            _product(be, Kva4, A, pred, nv, G, ntr, ldv, ldg, ldg, bias=bias)
            scores[i] = self._score(be, pred, ldg, Yva)

    def _raise_on(self, status, what):
        bad = np.flatnonzero(status)
        if bad.size:
            raise RidgeError(int(status[bad[0]]) - 1, what(int(bad[0])))

    # ------------------------------------------------------------------------------------------------ fit
    def fit(self, betas, targets):
        dev = self.device
        X, Y = _tensor(betas, dev), _tensor(targets, dev)
        if X.dim() != 2 or Y.dim() != 2 or X.shape[1] < 1 or Y.shape[1] < 1:
            raise ValueError(f"betas (n, N) and targets (n, G) are 2-D arrays, got shapes {tuple(X.shape)} and {tuple(Y.shape)}")
        n, N, G = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
        if Y.shape[0] != n:
            raise ValueError(f"{n} rows of betas against {int(Y.shape[0])} rows of targets")
        if not 2 <= n <= N_MAX:
            raise ValueError(f"the number of training rows must lie in [2, {N_MAX}] (tnt_cholesky_f32), got {n}")
        if self.score == "cosine" and self.alphas is not None and G > 2048:
            raise ValueError(f"score='cosine' takes embeddings of at most 2048 columns (tnt_cosine_loss_f32), got {G}")
        fold = None
        if self.cv is not None:
            if self.cv > n:
                raise ValueError(f"cv must be an integer in [2, n = {n}], got {self.cv}")
            if self.groups is not None and len(self.groups) != n:
                raise ValueError(f"groups holds {len(self.groups)} entries for {n} rows")
            fold = kfold(n, self.cv, self.groups)
            if np.unique(fold).size < self.cv:
                raise ValueError(f"cv = {self.cv} folds over {np.unique(fold).size} groups: a fold would be empty")
        Xv = Yv = None
        if self.validation is not None:
            Xv, Yv = _tensor(self.validation[0], dev), _tensor(self.validation[1], dev)
            if Xv.dim() != 2 or Yv.dim() != 2 or Xv.shape[1] != N or Yv.shape[1] != G or Xv.shape[0] != Yv.shape[0] \
                    or Xv.shape[0] < 1:
                raise ValueError(f"validation of shapes {tuple(Xv.shape)}, {tuple(Yv.shape)} against training data of shapes "
                                 f"{tuple(X.shape)}, {tuple(Y.shape)}")
        be = ops.backend()
        self._G = G
        X4, ldx = _rows4(X)
        K0 = gram(X4[:, :N], ldx, be)                # the one Gram matrix of this fit
        ldn = K0.shape[1]

        self.alpha_, self.cv_scores_ = self.alpha, None
        if self.alphas is not None:
            na = len(self.alphas)
            nsplit = self.cv if fold is not None else 1
            scores = torch.zeros(nsplit, na, dtype=torch.float64, device=dev)
            status = torch.zeros(nsplit, na, dtype=torch.int32, device=dev)
            if fold is not None:
                fold_t = torch.as_tensor(fold, device=dev)
                for f in range(self.cv):
                    tr, va = torch.nonzero(fold_t != f).reshape(-1), torch.nonzero(fold_t == f).reshape(-1)
                    ntr = int(tr.numel())
                    Ktr = torch.zeros(ntr, _r4(ntr), dtype=torch.float32, device=dev)
                    rows = K0[tr]
                    Ktr[:, :ntr] = rows[:, tr]
                    self._validate(be, Ktr, ntr, K0[va][:, tr], Y[tr], Y[va], scores[f], status[f])
            else:
                Xv4, ldv = _rows4(Xv)
                nv = int(Xv.shape[0])
                Kva = torch.zeros(nv, ldn, dtype=torch.float32, device=dev)
                _product(be, Xv4, X4, Kva, nv, n, N, ldv, ldx, ldn, transB=True)
                self._validate(be, K0.clone(), n, Kva[:, :n], Y, Yv, scores[0], status[0])
            st, sc = status.cpu().numpy(), scores.cpu().numpy()          # the one transfer of the selection
            self._raise_on(st.reshape(-1), lambda i: f"split {i // na}, alpha = {self.alphas[i % na]!r}")
            self.cv_scores_ = sc.mean(0)
            self.alpha_ = self.alphas[int(np.argmax(self.cv_scores_))]   # numpy's argmax: the first maximiser

        # ---- the model on all rows at alpha_
        self._centre(be, K0, n)
        mu_y, Yc = self._targets(Y)
        ldg = Yc.shape[1]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        (_, A), = self._solve_all(be, K0, n, Yc, [self.alpha_], status)
        HA = A.clone()
        if self.fit_intercept:
            HA[:, :G] -= A[:, :G].mean(0, dtype=torch.float64).to(torch.float32)
        coef = torch.zeros(N, ldg, dtype=torch.float32, device=dev)
        _product(be, X4, HA, coef, N, G, n, ldx, ldg, ldg, transA=True)
        if self.fit_intercept:
            mu_x = X.mean(0, dtype=torch.float64)
            icpt = (mu_y.double() - mu_x @ coef[:, :G].double()).to(torch.float32)
        else:
            icpt = torch.zeros(G, dtype=torch.float32, device=dev)
        self._raise_on(status.cpu().numpy(), lambda i: f"the fit on all rows, alpha = {self.alpha_!r}")
        self._coef, self._ldg, self._N = coef, ldg, N
        self._bias = torch.zeros(ldg, dtype=torch.float32, device=dev)
        self._bias[:G] = icpt
        self.coef_, self.intercept_, self.dual_coef_ = coef[:, :G], self._bias[:G], A[:, :G]
        return self

    # ------------------------------------------------------------------------------------------------ prediction
    def predict_embedding(self, betas):
        """(B, G) float32 device tensor: betas coef_ + intercept_, one product with the intercept as its bias"""
        if self.coef_ is None:
            raise RuntimeError("fit the decoder first")
        X = _tensor(betas, self.device)
        if X.dim() != 2 or X.shape[1] != self._N or X.shape[0] < 1:
            raise ValueError(f"betas of shape {tuple(X.shape)} for a decoder fitted on {self._N} voxels")
        X4, ldx = _rows4(X)
        B = int(X.shape[0])
        out = torch.zeros(B, self._ldg, dtype=torch.float32, device=self.device)
        _product(ops.backend(), X4, self._coef, out, B, self._G, self._N, ldx, self._ldg, self._ldg, bias=self._bias)
        return out[:, :self._G]

    def predict(self, betas):
        return self.predict_embedding(betas).cpu().numpy()

    def gemm_sk(self, A, B, C, M, N, K, lda, ldb, ldc, ws=0, **kw):
        """the product route evaluate.semantic_retrieve asks of a model"""
        _product(ops.backend(), A, B, C, M, N, K, lda, ldb, ldc, transA=kw.get("transA", False), transB=kw.get("transB", False),
                 bias=kw.get("bias"))
