"""The launch arithmetic and the float64 references that tests/test_gpu_rowop_paths.py relies on, checked without a GPU.

The GPU file picks its row counts and sizes for one property each (an empty last chunk, a second lane trip, one element past a
grid cap, the last narrow width).  Those properties follow from constants in csrc/rowops.hip; this file reads the constants out
of the source, compares them and tnt_bn_nchunk (host code) with the Python mirror in rowop_oracle.py, and asserts the named
property of every named size -- a retuned constant fails here instead of letting the GPU cases slide off their edges.  It also
checks each strided / fused float64 reference of rowop_oracle.py against the oracle.ops function on a dense copy."""
import ctypes
import os
import re

import numpy as np
import pytest

import rowop_oracle as RO
from oracle import ops as O
from oracle.philox import keep_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "masters-thesis_amd", "csrc", "rowops.hip")).read()


def const(pattern):
    m = re.findall(pattern, SRC)
    assert m, f"csrc/rowops.hip no longer matches {pattern!r}"
    return m


def test_constants_of_the_source_are_the_mirrors():
    assert int(const(r"constexpr int MAX_CHUNKS = (\d+);")[0]) == RO.MAX_CHUNKS
    assert const(r"int n = \(rows \+ (\d+)\) / (\d+); return n > MAX_CHUNKS")[0] == ("63", "64")
    et = const(r"constexpr int ET_CW = (\d+), ET_RG = (\d+), ET_MAXR = (\d+);")[0]
    assert tuple(map(int, et)) == (RO.ET_CW, RO.ET_RG, RO.ET_MAXR) and RO.ET_RG * RO.ET_MAXR == 256
    assert const(r"return \(int\)\(b > (\d+) \? (\d+) : \(b < 1 \? 1 : b\)\);")[0] == (str(RO.EW_CAP),) * 2
    assert const(r"long b = \(total \+ 255\) / (\d+);")[0] == str(RO.EW_BLOCK)
    assert const(r"if \(blocks > (\d+)\) blocks = (\d+);")[0] == (str(RO.MASK4_CAP),) * 2
    assert int(const(r"const bool narrow = cols <= (\d+);")[0]) == RO.NARROW_COLS
    # the 2048-row caps: the direct column sum, the multi-job column sum, the fused backward and its rider
    assert int(const(r"if \(rows <= (\d+)\) \{\s*hipLaunchKernelGGL\(col_sum_direct_kernel")[0]) == RO.DIRECT_ROWS
    assert int(const(r"rs\[k\] > (\d+) \|\| outs\[k\] == nullptr")[0]) == RO.DIRECT_ROWS
    assert int(const(r"rows <= 0 \|\| cols <= 0 \|\| rows > (\d+) \|\|")[0]) == RO.DIRECT_ROWS
    assert int(const(r"rows1 > (\d+) \|\| out1 == nullptr")[0]) == RO.DIRECT_ROWS
    # the lane loops of the two finalize kernels step by the wave width
    assert len(const(r"for \(int k = lane; k < nchunk; k \+= 64\)")) == 3


def test_every_kernel_is_in_the_gpu_files_table():
    """the table at the top of test_gpu_rowop_paths.py names every __global__ of the source (but stage_batch_kernel, which has a
    file of its own) beside a test that exists"""
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_rowop_paths.py")).read()
    table = gpu[gpu.index("arguments that select it"):gpu.index("Protocol (")]
    kernels = set(re.findall(r"__global__.*?\bvoid (\w+)\(", SRC))
    assert len(kernels) == 23 and "stage_batch_kernel" in kernels, sorted(kernels)
    for k in kernels - {"stage_batch_kernel"}:
        assert re.search(rf"\b{k}\b", table), f"{k} is missing from the table"
    for form in ("<0,32>", "<0,64>", "<1,32> / <1,64>", "<2,32> / <2,64>", "col_finalize_kernel<true>", "col_finalize_kernel<false>",
                 "bias_act_drop_bwd_kernel<true>", "bias_act_drop_bwd_kernel<false>", "enc_tail_fwd_kernel<false>", "enc_tail_fwd_kernel<true>"):
        assert form in table, form
    defined = set(re.findall(r"^def (test_\w+)\(", gpu, flags=re.M))
    named = set(re.findall(r"\b(test_\w+)", table))
    assert named and named <= defined, sorted(named - defined)


def test_chunk_mirror_agrees_with_the_library():
    from masters_thesis_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.tnt_bn_nchunk.argtypes, lib.tnt_bn_nchunk.restype = [ctypes.c_int32], ctypes.c_int32
    for rows in list(range(-2, 9000)) + [23040, 10 ** 6, 2 ** 31 - 64]:
        assert lib.tnt_bn_nchunk(rows) == RO.chunk_count(rows), rows


# rows -> (chunks, empty chunks, nj of the last chunk, lane trips): the property each row count of the GPU file is named for
CHUNK_EDGES = {1: (1, 0, 1, 1), 63: (1, 0, 63, 1), 65: (2, 0, 32, 1), 2048: (32, 0, 64, 1), 2049: (33, 0, 33, 1),
               4097: (65, 0, 1, 2), 8193: (128, 1, -62, 2), 8255: (128, 1, 0, 2), 8256: (128, 0, 1, 2)}


@pytest.mark.parametrize("rows", sorted(CHUNK_EDGES))
def test_row_counts_sit_on_their_edges(rows):
    p = RO.chunk_plan(rows)
    assert (p["nchunk"], p["empty"], p["nj_last"], p["trips"]) == CHUNK_EDGES[rows], p
    # the chunks cover every row exactly once: no row beyond the last non-empty chunk
    assert sum(max(0, min(rows, (k + 1) * p["crows"]) - k * p["crows"]) for k in range(p["nchunk"])) == rows
    assert (rows > RO.DIRECT_ROWS) == (rows in (2049, 4097, 8193, 8255, 8256))


def test_sizes_past_the_grid_caps():
    assert 8255 * 65 == 536575 and RO.ew_trips(8255 * 65) == 2          # dropout_kernel
    assert 8256 * 256 // 4 == 528384 and RO.ew_trips(8256 * 64) == 2    # dropout4_kernel, dropout4x2_kernel, the metric form
    assert RO.EW_CAP_ELEMS == 524288 and RO.ew_trips(524289) == 2 and RO.ew_trips(524288) == 1      # act_bwd_kernel
    assert RO.ew_trips(8255 * 65) == 2 and RO.ew_trips(8256 * 256 // 4) == 2     # bn_apply_kernel / bn_dx_kernel, bn_apply4_kernel
    n, sites = 2800000, 3
    total = n // 4 * sites
    assert total > RO.MASK4_CAP_GROUPS == 2097152 and RO.ew_trips(total, RO.MASK4_CAP) == 2
    # the site index changes inside one thread's strided loop: thread 0's second group lies in another site
    assert RO.MASK4_CAP_GROUPS // (n // 4) != 0
    assert RO.NARROW_COLS == 1024 and 1028 % 32 == 4                    # the wide form's last column block: one live quad
    for rows in (1, 31, 33, 255, 256):
        assert rows <= RO.ET_RG * RO.ET_MAXR
    for n in (1, 63, 64, 1023, 1024, 1025, 2049, 5000):                 # sum_kernel's 1024-thread stride
        assert (n + 1023) // 1024 == {1: 1, 63: 1, 64: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3, 5000: 5}[n]


# ------------------------------------------------------------------------------------------------ references
def test_drop_keep_is_keep_mask_of_the_logical_tensor():
    rate, seed, site, step = 0.3, 1234567890123, 40, 9
    B, T, E, W, c0 = 4, 3, 5, 11, 3
    logical = keep_mask((B, T, W), rate, seed, site, step)[:, :, c0:c0 + E]
    rm = RO.drop_keep(B * T, E, 0, W, c0, 0, rate, seed, site, step)
    assert np.array_equal(rm.reshape(B, T, E), logical)
    tm = RO.drop_keep(T * B, E, B, W, c0, 0, rate, seed, site, step)
    assert np.array_equal(tm.reshape(T, B, E).transpose(1, 0, 2), logical)
    ps = RO.drop_keep(T * B, E, 0, W, c0, B, rate, seed, site, step)
    for t in range(T):
        assert np.array_equal(ps[t * B:(t + 1) * B], keep_mask((B, W), rate, seed, site + t, step)[:, c0:c0 + E])
    # the per-step use: logical width T * H, this step's columns
    H = 4
    whole = keep_mask((B, T * H), rate, seed, site, step)
    for t in range(T):
        assert np.array_equal(RO.drop_keep(B, H, 0, T * H, t * H, 0, rate, seed, site, step), whole[:, t * H:(t + 1) * H])
    assert RO.drop_keep(3, 4, 0, 4, 0, 0, 0.0, seed, site, step).all()


def test_drop32_and_mask4_follow_the_oracle():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 8)).astype(np.float32)
    keep = keep_mask((6, 8), 0.2, 5, 6, 7)
    assert np.array_equal(RO.drop32(x, keep, 0.2), O.dropout_fwd(x, keep, 0.2))
    assert RO.drop32(x, keep, 0.2).dtype == np.float32 and np.array_equal(RO.drop32(x, keep, 0.0), x)
    assert np.array_equal(RO.drop32(x, keep, 0.5), np.where(keep, 2 * x, 0))
    m = RO.mask4_bytes(16, 2, 0.4, 11, 3, 2)
    for k in range(2):
        bits = keep_mask((16,), 0.4, 11, 3 + k, 2)
        assert [(int(m[k, g]) >> j) & 1 for g in range(4) for j in range(4)] == list(bits.astype(int))


def test_strided_norm_references_are_the_dense_ones():
    rng = np.random.default_rng(1)
    rows, C, ld = 9, 5, 8
    x, dy = rng.standard_normal((rows, C)), rng.standard_normal((rows, C))
    gam, bet, mm, mv = rng.standard_normal(C), rng.standard_normal(C), rng.standard_normal(C), rng.random(C) + 0.5
    dy_ld = np.full((rows, ld), 1e6)
    dy_ld[:, :C] = dy
    for training in (True, False):
        y, cache, nmm, nmv = RO.bn_fwd(x, gam, bet, mm, mv, training, 1e-3, 0.99)
        for a, b in zip(RO.bn_bwd_strided(dy_ld, C, gam, cache), O.batchnorm_bwd(dy, gam, cache)):
            assert np.array_equal(a, b)
        before = np.full((rows, ld), np.nan)
        got = RO.into(before, y)
        assert np.array_equal(got[:, :C], y) and np.isnan(got[:, C:]).all() and np.isnan(before).all()
    y, cache, _, _ = RO.bn_fwd(x, gam, bet, mm, mv, True, 1e-3, 0.99)
    dx, dg, db = O.batchnorm_bwd(dy, gam, cache)
    np.testing.assert_allclose(RO.bn_bwd_total(dy_ld, C, gam, cache[0], cache[1], dg, db, rows), dx, rtol=1e-12, atol=1e-14)
    # two replicas: the gradient of the whole batch, replica by replica
    x2, dy2 = rng.standard_normal((2 * rows, C)), rng.standard_normal((2 * rows, C))
    _, c2, _, _ = RO.bn_fwd(x2, gam, bet, mm, mv, True, 1e-3, 0.99)
    dx2, dg2, db2 = O.batchnorm_bwd(dy2, gam, c2)
    for k in range(2):
        s = slice(k * rows, (k + 1) * rows)
        np.testing.assert_allclose(RO.bn_bwd_total(dy2[s], C, gam, c2[0][s], c2[1], dg2, db2, 2 * rows), dx2[s], rtol=1e-12,
                                   atol=1e-14)
    yl, cl = O.layernorm_fwd(x, gam, bet, 1e-3)
    for a, b in zip(RO.ln_bwd_strided(dy_ld, C, gam, cl), O.layernorm_bwd(dy, gam, cl)):
        assert np.array_equal(a, b)


def test_two_pass_float32_yardstick_is_batchnorm():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((300, 4)).astype(np.float32)
    mean, var, xhat = RO.bn_two_pass_f32(x, 1e-3)
    _, (xh, inv, _), _, _ = O.batchnorm_fwd(x.astype(np.float64), np.ones(4), np.zeros(4), np.zeros(4), np.ones(4), True, 1e-3, 0.99)
    np.testing.assert_allclose(xhat, xh, atol=1e-5)
    np.testing.assert_allclose(mean, x.astype(np.float64).mean(0), atol=1e-6)


def test_fused_references_are_compositions_of_the_oracle():
    rng = np.random.default_rng(3)
    rows, C, ld = 7, 8, 12
    seed, sf, sl, step = 99, 4, 5, 2
    y, dout, pre = rng.standard_normal((rows, C)), rng.standard_normal((rows, C)), rng.standard_normal((rows, C))
    gam, bet, mm, mv = rng.standard_normal(C), rng.standard_normal(C), rng.standard_normal(C), rng.random(C) + 0.5
    kf, kl = keep_mask((rows, C), 0.2, seed, sf, step), keep_mask((rows, C), 0.3, seed, sl, step)
    out, xhat, inv, nmm, nmv = RO.enc_tail_fwd(y, gam, bet, mm, mv, True, 1e-3, 0.99, 0.2, 0.3, seed, sf, sl, step)
    yo, (xh, iv, _), mmo, mvo = O.batchnorm_fwd(O.dropout_fwd(y, kf, 0.2), gam, bet, mm, mv, True, 1e-3, 0.99)
    assert np.array_equal(out, O.dropout_fwd(yo, kl, 0.3)) and np.array_equal(xhat, xh) and np.array_equal(nmv, mvo)
    out_i, _, _, nmm_i, _ = RO.enc_tail_fwd(y, gam, bet, mm, mv, False, 1e-3, 0.99, 0.2, 0.3, seed, sf, sl, step)
    assert np.array_equal(out_i, O.batchnorm_fwd(y, gam, bet, mm, mv, False, 1e-3, 0.99)[0]) and np.array_equal(nmm_i, mm)
    dout_ld = np.full((rows, ld), 1e6)
    dout_ld[:, :C] = dout
    dpre, dg, db, dbias = RO.enc_tail_bwd(dout_ld, C, xhat, gam, inv, pre, 0.2, 0.2, 0.3, seed, sf, sl, step)
    dx, dgo, dbo = O.batchnorm_bwd(O.dropout_fwd(dout, kl, 0.3), gam, (xh, iv, True))
    want = O.act_bwd(pre, O.dropout_fwd(dx, kf, 0.2), O.ACT_LEAKY, 0.2)
    assert np.array_equal(dpre, want) and np.array_equal(dg, dgo) and np.array_equal(db, dbo)
    assert np.array_equal(dbias, want.sum(0))
    for act in (O.ACT_NONE, O.ACT_LEAKY, O.ACT_RELU, O.ACT_TANH):
        dxa, dba = RO.bias_act_drop_bwd(dout_ld, dout_ld * 0 + np.pad(pre, ((0, 0), (0, ld - C))), C, kl, 0.3, act, 0.2)
        assert np.array_equal(dxa, O.act_bwd(pre, O.dropout_fwd(dout, kl, 0.3), act, 0.2)) and np.array_equal(dba, dxa.sum(0))
    alpha = rng.random((2, 3, 70))
    part = RO.metric_partials(alpha)
    q = (1 - alpha.sum(1)) ** 2
    np.testing.assert_allclose(part.reshape(2, 2), np.stack([q[:, :64].sum(1), q[:, 64:].sum(1)], 1), rtol=1e-13)
