"""Float64 references and launch arithmetic of csrc/rowops.hip, shared by tests/test_gpu_rowop_paths.py (which compares the
kernels with them) and tests/test_host_rowop_edges.py (which checks them against oracle.ops on dense copies, and the
arithmetic against the constants in the source).  numpy only.

A strided reference is the dense reference applied to the live columns: `live(a, C)` drops the pad columns of a matrix held
at a row stride above C, the oracle.ops function runs on that, and `into(before, ref)` lays the result back over the live
columns of the output's initial contents, so that one comparison covers the values and the untouched pad columns."""
import numpy as np

from oracle import ops as O
from oracle.philox import keep_mask

# the constants of csrc/rowops.hip these mirrors were written against (test_host_rowop_edges.py reads them from the source)
MAX_CHUNKS, CHUNK_MIN_ROWS, LANES = 128, 64, 64
DIRECT_ROWS = 2048              # tnt_colsum_f32 / tnt_colsum4_f32 / tnt_bias_act_drop_bwd_f32: one launch up to here
EW_CAP, EW_BLOCK = 2048, 256    # ew_blocks: workgroups of 256 threads, at most 2048 of them
MASK4_CAP = 8192                # tnt_dropout_mask4_u8's own cap
ET_CW, ET_RG, ET_MAXR = 32, 32, 8
NARROW_COLS = 1024              # tnt_bias_act_drop_bwd_f32: cols <= 1024 takes the one-quad-per-workgroup form
EW_CAP_ELEMS, MASK4_CAP_GROUPS = EW_CAP * EW_BLOCK, MASK4_CAP * EW_BLOCK


def chunk_count(rows):
    n = (rows + CHUNK_MIN_ROWS - 1) // CHUNK_MIN_ROWS
    return MAX_CHUNKS if n > MAX_CHUNKS else max(n, 1)


def chunk_rows(rows):
    n = chunk_count(rows)
    return (rows + n - 1) // n


def chunk_plan(rows):
    """what bn_finalize_kernel / col_finalize_kernel see for `rows` rows: number of chunks, rows per chunk, nj of the last chunk
    as bn_finalize_kernel computes it (min(rows, (k + 1) crows) - k crows: zero or negative for an empty chunk), the number of
    empty chunks, and the trips of the 64-lane loop over the chunks"""
    n, cr = chunk_count(rows), chunk_rows(rows)
    nj = [min(rows, (k + 1) * cr) - k * cr for k in range(n)]
    return dict(nchunk=n, crows=cr, nj_last=nj[-1], empty=sum(1 for v in nj if v <= 0), trips=(n + LANES - 1) // LANES)


def ew_trips(total, cap=EW_CAP):
    """trips of an elementwise kernel's grid-stride loop over `total` work items"""
    blocks = min(max((total + EW_BLOCK - 1) // EW_BLOCK, 1), cap)
    return (total + blocks * EW_BLOCK - 1) // (blocks * EW_BLOCK)


def live(a, C):
    return np.asarray(a)[..., :C]


def into(before, ref):
    """`ref` over the live columns of a copy of `before` (the output buffer's initial contents at its row stride)"""
    out = np.array(before, copy=True)
    out[..., :ref.shape[-1]] = ref
    return out


# ------------------------------------------------------------------------------------------------ dropout
def drop_keep(rows, cols, tB, lwidth, lcol0, rows_per_site, rate, seed, site, step):
    """keep mask [rows][cols] of a BUFFER in tnt_dropout_f32's layout arguments: buffer row r belongs to site + r // rows_per_site
    (local row r % rows_per_site) when rows_per_site > 0, its logical row is (r % tB) * T + r // tB for a time-major buffer
    (T = rows / tB), and column c is logical element lrow * lwidth + lcol0 + c"""
    r = np.arange(rows)
    k = np.zeros(rows, np.int64)
    nl = rows
    if rows_per_site > 0:
        k, r, nl = r // rows_per_site, r % rows_per_site, rows_per_site
    lrow = (r % tB) * (rows // tB) + r // tB if tB > 0 else r
    out = np.empty((rows, cols), bool)
    for s in np.unique(k):
        m = keep_mask((nl, lwidth), rate, seed, site + int(s), step)
        out[k == s] = m[lrow[k == s], lcol0:lcol0 + cols]
    return out


def drop32(x32, keep, rate):
    """the device's float32 arithmetic: kept values times float32(1 / (1 - float32(rate))), bit for bit"""
    x32 = np.asarray(x32, np.float32)
    if rate <= 0:
        return x32.copy()
    return np.where(keep, x32 * np.float32(1.0 / (1.0 - np.float32(rate))), np.float32(0)).astype(np.float32)


def drop64(x, keep, rate):
    return O.dropout_fwd(np.asarray(x, np.float64), keep, rate)


def mask4_bytes(n, nsites, rate, seed, site0, step):
    """tnt_dropout_mask4_u8: [nsites][n / 4] bytes, bit j of byte g = element 4 g + j of site site0 + k kept"""
    out = np.empty((nsites, n // 4), np.uint8)
    w = np.array([1, 2, 4, 8], np.uint8)
    for k in range(nsites):
        out[k] = (keep_mask((n // 4, 4), rate, seed, site0 + k, step) * w).sum(1)
    return out


def metric_partials(alpha):
    """attention metric partials of alpha [T][B][R]: partial[t * nc + c] = sum over the 64 regions of chunk c of
    (1 - sum_b alpha[t][b][r])^2"""
    T, B, R = alpha.shape
    nc = (R + 63) // 64
    q = np.zeros((T, nc * 64))
    q[:, :R] = (1.0 - alpha.sum(1)) ** 2
    return q.reshape(T, nc, 64).sum(2).reshape(T * nc)


# ------------------------------------------------------------------------------------------------ norms at a row stride
def bn_fwd(x, gamma, beta, mm, mv, training, eps, momentum):
    return O.batchnorm_fwd(x, gamma, beta, mm, mv, training, eps, momentum)


def bn_bwd_strided(dy_ld, C, gamma, cache):
    return O.batchnorm_bwd(live(dy_ld, C), gamma, cache)


def ln_bwd_strided(dy_ld, C, gamma, cache):
    return O.layernorm_bwd(live(dy_ld, C), gamma, cache)


def bn_bwd_total(dy_ld, C, gamma, xhat, inv, dgamma_sum, dbeta_sum, n_total):
    """tnt_batchnorm_dx_f32: the training input gradient of these rows from sums taken over all n_total rows"""
    return gamma * inv / n_total * (n_total * live(dy_ld, C) - dbeta_sum - xhat * dgamma_sum)


def bn_two_pass_f32(x32, eps):
    """plain float32 two-pass BatchNorm statistics, oracle.ops.batchnorm_fwd's own expressions on a float32 array: (mean, var,
    xhat) -- the yardstick of the ill-conditioned case, not a reference.  numpy adds the rows of a [rows][C] array one after
    the other (its pairwise summation only runs along a contiguous axis), so this is the sequential float32 sum."""
    x32 = np.asarray(x32, np.float32)
    mean = x32.mean(0, dtype=np.float32)
    d = x32 - mean
    var = (d * d).mean(0, dtype=np.float32)
    return mean, var, d * (np.float32(1) / np.sqrt(var + np.float32(eps)))


def bn_two_pass_f32_pairwise(x32, eps):
    """the same two passes with every column summed pairwise (numpy on a contiguous row): printed beside the yardstick for the
    record, never asserted against"""
    xt = np.ascontiguousarray(np.asarray(x32, np.float32).T)
    mean = xt.mean(1, dtype=np.float32)
    d = xt - mean[:, None]
    var = (d * d).mean(1, dtype=np.float32)
    return mean, var, (d * (np.float32(1) / np.sqrt(var + np.float32(eps)))[:, None]).T


# ------------------------------------------------------------------------------------------------ fused backward / tail
def bias_act_drop_bwd(dy_ld, pre_ld, cols, keep, rate, act, slope):
    """dx = dropout'(dy) * act'(pre), dbias = its column sums"""
    dx = O.act_bwd(live(pre_ld, cols), drop64(live(dy_ld, cols), keep, rate), act, slope)
    return dx, dx.sum(0)


def enc_tail_fwd(y, gamma, beta, mm, mv, training, eps, momentum, r_feat, r_lstm, seed, s_feat, s_lstm, step):
    """Dropout(features) -> BatchNorm -> the LSTM layer's input dropout; both masks over element r * C + c.
    Returns out, xhat, inv_std, new moving mean / variance"""
    rows, C = y.shape
    x = drop64(y, keep_mask((rows, C), r_feat, seed, s_feat, step), r_feat) if training else y
    out, (xhat, inv, _), nmm, nmv = O.batchnorm_fwd(x, gamma, beta, mm, mv, training, eps, momentum)
    if training:
        out = drop64(out, keep_mask((rows, C), r_lstm, seed, s_lstm, step), r_lstm)
    return out, xhat, inv, nmm, nmv


def enc_tail_bwd(dout_ld, C, xhat, gamma, inv, pre, slope, r_feat, r_lstm, seed, s_feat, s_lstm, step):
    """its backward with LeakyReLU'(pre) and the bias sum: dpre, dgamma, dbeta, dbias"""
    rows = xhat.shape[0]
    g = drop64(live(dout_ld, C), keep_mask((rows, C), r_lstm, seed, s_lstm, step), r_lstm)
    dx, dgamma, dbeta = O.batchnorm_bwd(g, gamma, (xhat, inv, True))
    dx = drop64(dx, keep_mask((rows, C), r_feat, seed, s_feat, step), r_feat)
    dpre = np.where(pre > 0, dx, dx * slope)
    return dpre, dgamma, dbeta, dpre.sum(0)
