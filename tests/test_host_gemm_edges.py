"""The launch arithmetic, the sizes and the float64 references that tests/test_gpu_gemm_paths.py relies on, checked without a GPU.

The GPU file picks every size for one property (a last chunk shorter than BK, a split that collapses, fewer K stages than the
ring is deep, splits that own no row, ...).  Those properties follow from constants and tables in csrc/gemm.hip and
csrc/gemm3.hip; this file reads them out of the sources, compares them with the mirrors in gemm_oracle.py and asserts the named
property of every named size -- a retuned table fails here instead of letting the GPU cases slide off their edges.  It checks the
references of gemm_oracle.py against oracle.ops on dense copies, that the GPU file's table names every kernel and configuration
beside a test that exists, and the refusals of the three entry points that return before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import gemm_oracle as G
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "masters-thesis_amd", "csrc")
GEMM = open(os.path.join(CSRC, "gemm.hip")).read()
GEMM3 = open(os.path.join(CSRC, "gemm3.hip")).read()
GPU = open(os.path.join(ROOT, "tests", "test_gpu_gemm_paths.py")).read()


def const(src, pattern):
    m = re.findall(pattern, src)
    assert m, f"the source no longer matches {pattern!r}"
    return m


# ------------------------------------------------------------------------------------------------ mirrors
def test_constants_of_the_sources_are_the_mirrors():
    assert int(const(GEMM, r"constexpr int BK = (\d+);")[0]) == G.BK
    cand = const(GEMM, r"const int cand\[4\]\[2\] = \{\{(\d+), (\d+)\}, \{(\d+), (\d+)\}, \{(\d+), (\d+)\}, \{(\d+), (\d+)\}\};")[0]
    assert sorted(zip(map(int, cand[0::2]), map(int, cand[1::2]))) == sorted(G.TILED)
    table = {}
    for cfg, kern, bm, bn, wgm, wgn, pd in const(GEMM, r"case (\d+): return launch_(1r|2)_cfg<(\d+), (\d+), (\d+), (\d+)(?:, (\d+))?>"):
        table[int(cfg)] = ("gemm1r" if kern == "1r" else "gemm2", int(bm), int(bn), int(wgm), int(wgn), int(pd or 2))
    assert table == G.CFG_1R
    assert const(GEMM, r"constexpr int R1_BM = (\d+), R1_BN = (\d+);")[0] == ("160", "128") and G.CFG_1R[1][1:3] == (160, 128)
    g3 = {int(r[0]): tuple(map(int, r[1:])) for r in
          const(GEMM3, r"case (\d+): return g3_layout<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>")}
    assert g3 == G.G3 and all(v[5] == G.NS for v in g3.values())
    tiles = {int(t): (int(bm), int(bn)) for t, bm, bn in const(GEMM3, r"case (\d+): o = \{(\d+), (\d+),")}
    assert tiles == {t: G.g3_tile(t)[:2] for t in G.G3}
    assert const(GEMM3, r"const int bk = tile >= 9 \? (\d+) : (\d+);")[0] == ("64", "32")
    assert all(G.g3_tile(t)[2] == (64 if t >= 9 else 32) for t in G.G3)
    assert int(const(GEMM3, r"if \(splitk > 1 && units > (\d+)\) return 1e30;")[0]) == G.G3_UNITS
    assert int(const(GEMM3, r"constexpr int G3_SENTINEL = (0x[0-9A-Fa-f]+);")[0], 16) == 0x7FC5EED5
    assert np.array([G.NAN]).view(np.uint32)[0] == 0x7FC00000        # the fill is the plain quiet NaN, not that pattern
    assert const(GEMM3, r"\(wave \* TM \+ tm\) % S == z")               # the ownership rule g3_ownerless mirrors


def test_split_mirrors_agree_with_the_library():
    from masters_thesis_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for tile in G.G3:
        for M, N, S, batch in ((65, 69, 2, 1), (161, 133, 8, 2), (1, 3, 3, 1), (257, 85, 12, 1), (70, 40, 1, 1)):
            assert lib.tnt_gemm3_work_floats(M, N, tile, S, batch) == G.g3_work_floats(tile, M, N, S, batch), (tile, M, N, S)
    for lay, (M, N, K) in G.FUSED_AUTO.items():
        tA, tB = G.LAYOUTS[lay]
        assert lib.tnt_gemm_fused_cfg(M, N, K, int(tA), int(tB), 1) in G.CFG_1R
    assert lib.tnt_gemm_fused_cfg(64, 64, 64, 0, 1, 1) == 0 and lib.tnt_gemm_fused_cfg(1000, 500, 33, 0, 1, 1) == 0


# ------------------------------------------------------------------------------------------------ the sizes sit on their edges
def test_tiled_sizes_sit_on_their_edges():
    assert [G.k_tiles(K) for K in G.TILED_K] == [1, 1, 1, 2, 3] and [K % G.BK for K in G.TILED_K] == [1, 31, 0, 1, 3]
    # (kchunk, splits that run, last chunk): two last chunks shorter than BK, a requested 8 that runs as 4, a last chunk of 1
    assert [G.tiled_split(K, S) for K, S in G.TILED_SPLITS] == [(96, 3, 8), (64, 4, 8), (32, 4, 4), (32, 2, 1)]
    assert all(G.tiled_split(K, S)[2] < G.BK for K, S in G.TILED_SPLITS)
    for bm, bn in G.TILED:
        shapes = G.tiled_shapes(bm, bn)
        assert len(shapes) == 30 >= 4 * len(G.TILED_EPILOGUES)
        assert {s[0] for s in shapes} == {1, bm - 1, bm + 1} and {s[1] for s in shapes} == {3, bn + 1}
    for form, (front, extra) in G.TILED_FORMS.items():
        vec = front % 4 == 0 and extra % 4 == 0
        assert vec == (form == "vec") and (front > 0 or extra > 0)
    assert len(G.TILED_EPILOGUES) == 7 and len(set(G.TILED_EPILOGUES)) == 7


def test_one_round_sizes_sit_on_their_edges():
    assert [G.k_tiles(K) for K in G.FUSED_K] == [1, 1, 2, 2, 3, 4, 5, 6]
    assert sum(1 for K in G.FUSED_K if K % 4) >= 4
    assert {G.k_tiles(K) for K in G.FUSED_K} == set(range(1, 7))
    # the 3-deep register ring of cfg 9: fewer, as many and more k tiles than it prefetches; gemm2's odd trailing step
    assert G.CFG_1R[9][5] == 3 and {1, 3, 5} <= {G.k_tiles(K) for K in G.FUSED_K if G.k_tiles(K) % 2}
    assert set(G.CFG_1R) == {1, 9, 21, 22, 24, 25, 26, 28}


def test_gemm3_sizes_sit_on_their_edges():
    for tile in G.G3:
        bm, bn, bk = G.g3_tile(tile)
        ks = G.g3_ks(bk)
        assert [G.g3_split(tile, K, 1)[0] for K in ks] == [1, 2, 3, 4] and min(G.g3_split(tile, K, 1)[0] for K in ks) < G.NS
        assert ks[0] % 4 and ks[0] // 4 == (bk - 4) // 4                  # ends inside the last 4-chunk of the first stage
        assert (ks[1] % bk) < 4 and (ks[2] % bk) % 16 and ks[2] % bk > 16 and ks[3] % bk == 0
        cases = {c[0]: c for c in G.g3_split_cases(tile)}
        assert G.g3_split(tile, *cases["S2"][1:3]) == (3, 2, 2, 1)          # the last split has fewer stages
        assert G.g3_split(tile, *cases["S3"][1:3]) == (5, 2, 3, 1)
        assert G.g3_split(tile, *cases["S8 clamped"][1:3]) == (2, 1, 2, 1)  # S above the stage count
        assert cases["S2 A2"][3] == 2 and cases["S2 bias"][4]
        for name, K, S, batch, _ in cases.values():                         # the residency rule, by the REQUESTED split
            for N in (3, bn + 5):
                assert G.g3_units(tile, bm + 1, N, S, batch) <= G.G3_UNITS, (tile, name)
            assert G.g3_work_floats(tile, bm + 1, bn + 5, S, batch) == 4 * S * batch * bm * bn
        assert not G.g3_ownerless(tile, 2) and not G.g3_ownerless(tile, 3)
    tile, M, N, K, S = G.G3_OWNERLESS
    assert G.g3_acc_rows(tile) == 8 and G.g3_ownerless(tile, S) == [8, 9, 10, 11]
    assert G.g3_split(tile, K, S) == (48, 4, 12, 4) and G.g3_units(tile, M, N, S) == 48 <= G.G3_UNITS
    c = G.G3_EMBEDDED
    for tile in c["tiles"]:
        bm, bn, bk = G.g3_tile(tile)
        K = bk + 5
        ld = G.roundup4(K) + c["ld_extra"]
        # the second stage of a row covers k in [bk, 2 bk): the live tail, the zero pads, the gap, and the next row's first floats
        assert G.g3_split(tile, K, 1)[0] == 2 and 2 * bk > ld and c["M"] > bm
        assert G.g3_units(tile, c["M"], c["N"], 1) == 2


# ------------------------------------------------------------------------------------------------ the table
def test_every_kernel_and_configuration_is_in_the_gpu_files_table():
    table = GPU[GPU.index("arguments that select it"):GPU.index("Protocol (")]
    kernels = set(re.findall(r"__global__.*?\bvoid (\w+)\(", GEMM + GEMM3))
    assert kernels == {"gemm_kernel", "splitk_reduce_kernel", "gemm1r_kernel", "gemm2_kernel", "gemm3_kernel", "gemm3_pair_kernel",
                       "g3_arm_kernel"}, sorted(kernels)
    for k in kernels:
        assert re.search(rf"\b{k}\b", table), f"{k} is missing from the table"
    for cfg in G.CFG_1R:
        assert re.search(rf"cfg[ =,\d]*\b{cfg}\b", table), f"cfg {cfg} is missing from the table"
    assert "tiles 1 .. 11" in table and len(G.G3) == 11
    for bm, bn in G.TILED:
        assert f"{bm}x{bn}" in table
    for form in ("VEC=true", "VEC=false", "PD=1", "PD=3", "LIVE=false", "LIVE=true", "cfg = 0"):
        assert form in table, form
    ops_tests = set(re.findall(r"^def (test_\w+)\(", open(os.path.join(ROOT, "tests", "test_gpu_ops.py")).read(), flags=re.M))
    defined = set(re.findall(r"^def (test_\w+)\(", GPU, flags=re.M))
    named = set(re.findall(r"\b(test_\w+)", table)) - {"test_gpu_ops"}
    assert named and named <= defined | {"test_gemm3_pair"} and "test_gemm3_pair" in ops_tests, sorted(named - defined)
    assert defined <= named, sorted(defined - named)


# ------------------------------------------------------------------------------------------------ references
def test_references_are_the_oracles():
    rng = np.random.default_rng(0)
    A, B, b = rng.standard_normal((7, 9)), rng.standard_normal((9, 5)), rng.standard_normal(5)
    for kind, code in G.ACTS.items():
        y, pre = O.dense_fwd(A, B, b, code, 0.2)
        assert np.array_equal(G.product(A, B, b), pre)
        if kind == "leaky":             # the device multiplies by float32(0.2)
            np.testing.assert_allclose(G.act(pre, kind, 0.2), y, rtol=1e-7)
        else:
            assert np.array_equal(G.act(pre, kind, 0.2), y)
    assert np.array_equal(G.product(A, B), O.dense_fwd(A, B, None)[1])
    dy = rng.standard_normal((9, 5))
    assert np.array_equal(G.colsum(dy), O.dense_bwd(A.T, None, None, dy, need_dx=False)[2])
    # the float32 forms: what tnt_act computes from a float32 pre
    p = np.array([-1.5, -0.0, 0.0, 2.25, -3.0], np.float32)
    assert np.array_equal(G.act(p, "none"), p) and np.array_equal(G.act(p, "relu"), np.array([0, 0, 0, 2.25, 0], np.float32))
    lk = G.act(p, "leaky", 0.2)
    assert lk.dtype == np.float32 and np.array_equal(lk, np.array([np.float32(-1.5) * np.float32(0.2), -0.0, 0.0, 2.25, np.float32(-3.0) * np.float32(0.2)], np.float32))
    assert G.act(p, "tanh").dtype == np.float64 and np.array_equal(G.act(p, "tanh"), np.tanh(p.astype(np.float64)))
    # the bound: (K + 2) u (|A| |B| + |bias|), and a float32 dot product of any order stays inside it
    bound = G.fp32_dot_bound(A, B, b)
    assert np.array_equal(bound, 11 * 2.0 ** -24 * (np.abs(A) @ np.abs(B) + np.abs(b)))
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    seq = np.zeros((7, 5), np.float32)
    for k in reversed(range(9)):
        seq += A32[:, k:k + 1] * B32[k:k + 1]
    want = G.product(A32, B32)
    assert (np.abs(seq - want) <= G.fp32_dot_bound(A32, B32)).all() and (np.abs(seq - want) > 0).any()
    ints = G.ints(rng, 50, 40)
    assert np.array_equal(ints, np.round(ints)) and ints.min() == -3 and ints.max() == 3
    assert 9 * 161 < 2 ** 24 and 9 * 1536 < 2 ** 24                    # every partial sum of the exact cases is an exact float32


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("front,ld_extra,zero_pad", [(0, 0, False), (1, 0, False), (8, 4, True), (0, 1, False), (4, 8, True)])
def test_embed_round_trips(trans, front, ld_extra, zero_pad):
    rng = np.random.default_rng(1)
    op = rng.standard_normal((6, 5))
    e = G.embed(op, trans, ld_extra, front, zero_pad=zero_pad)
    rows, width = (5, 6) if trans else (6, 5)
    assert e.ld == G.roundup4(width) + ld_extra and e.buf.dtype == np.float32 and len(e.buf) == front + rows * e.ld + G.TAIL
    assert np.shares_memory(e.view, e.buf) and len(e.buf) - len(e.view) == front
    assert np.array_equal(e.logical, op.astype(np.float32).astype(np.float64)) and e.logical.shape == op.shape
    assert np.array_equal(G.extract(e, op.shape, trans), e.logical)
    body = e.view[:rows * e.ld].reshape(rows, e.ld)
    pads = body[:, width:G.roundup4(width)]
    assert (pads == 0).all() if zero_pad else np.isnan(pads).all()
    assert np.isnan(body[:, G.roundup4(width):]).all() and np.isnan(e.buf[:front]).all() and np.isnan(e.view[rows * e.ld:]).all()
    assert np.isnan(e.buf).sum() == len(e.buf) - rows * width - (pads.size if zero_pad else 0)
    assert (e.buf.view(np.uint32)[np.isnan(e.buf)] == 0x7FC00000).all()
    f = G.embed(op, trans, ld_extra, front, fill=5.0)
    assert (f.buf[:front] == 5.0).all() and np.array_equal(f.logical, e.logical)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_refusals_that_return_before_any_launch():
    """argument combinations the three entry points refuse in host code (TNT_BADARG(k) = -1000 - k): nothing is launched, so no
    GPU is needed and the pointers are never followed"""
    # The pointers below are made up.  This file also runs where a GPU is present, so a combination belongs here only if the
    # entry point returns in host code before any launch (read the check order in gemm_dispatch, tnt_gemm_fused_f32, g3_fill and
    # g3_prepare before adding one): anything that got through would launch a kernel on these addresses.
    from masters_thesis_amd import _lib
    lib = _lib.load()
    p, odd = 0x10000, 0x10004                # "device pointers": 16-byte aligned, and not
    bad = lambda k: -1000 - k
    tiled = lambda **kw: lib.tnt_gemm_f32_tile(p, p, p, None, None, 64, 64, 64, 64, 64, 64, kw.get("tA", 0), kw.get("tB", 0), 0, 0.2, 0,
                                               kw.get("S", 1), None, 64, 64, None)
    assert tiled(tA=1, tB=1) == bad(12)                                                    # both transposes
    assert tiled(S=2) == bad(18)                                                           # split without work
    assert lib.tnt_gemm_f32(p, p, p, None, None, 64, 64, 64, 64, 64, 64, 1, 1, 0, 0.2, 0, 1, None, None) == bad(12)
    assert lib.tnt_gemm_f32(p, p, p, None, None, 64, 64, 0, 64, 64, 64, 0, 0, 0, 0.2, 0, 1, None, None) == bad(6)

    def fused(A=p, B=p, colsum=None, A2=None, C2=None, lda=64, ldb=64, tA=0, tB=0, cfg=21):
        return lib.tnt_gemm_fused_f32(A, B, p, None, colsum, A2, C2, 64, 64, 64, lda, ldb, 64, tA, tB, cfg, None)
    assert fused(tA=1, tB=1) == bad(14)
    assert fused(lda=62) == bad(1) and fused(ldb=66) == bad(1) and fused(A=odd) == bad(1) and fused(A2=odd, C2=p) == bad(1)   # ld % 4, alignment
    assert fused(colsum=p) == bad(5) and fused(colsum=p, tB=1) == bad(5)                   # column sums off TN
    assert fused(cfg=99) == bad(91) and fused(cfg=22, tA=1, tB=1) == bad(14)               # an unknown cfg
    assert fused(A2=p) == bad(6) and fused(C2=p) == bad(6)                                 # A2 without C2, C2 without A2
    assert fused(cfg=0, tB=1) == bad(92)                                                   # no configuration serves NT

    def g3(A=p, B=p, C=p, colsum=None, A2=None, C2=None, lda=64, ldb=64, ldc=64, tA=0, tB=0, tile=7, S=1, work=None, sync=None):
        return lib.tnt_gemm3_f32(A, B, C, None, colsum, A2, C2, 64, 64, 64, lda, ldb, ldc, tA, tB, tile, S, work, sync, None, 0, None)
    assert g3(tA=1, tB=1) == bad(15)
    assert g3(lda=62) == bad(1) and g3(ldb=62) == bad(1) and g3(ldc=66) == bad(1) and g3(B=odd) == bad(1) and g3(C=odd) == bad(1)
    assert g3(S=2) == bad(17) and g3(S=2, work=p) == bad(17) and g3(S=2, sync=p) == bad(17)   # split without work / sync
    assert g3(S=2, work=odd, sync=p) == bad(15)
    assert g3(colsum=p) == bad(5) and g3(colsum=p, tB=1) == bad(5)
    assert g3(colsum=p, tA=1, S=2, work=p, sync=p) == bad(7)                               # the rider needs the whole K
    assert g3(tile=0) == bad(13) and g3(tile=12) == bad(13) and g3(tile=99, tA=1) == bad(13)
    assert g3(A2=p) == bad(6) and g3(C2=p) == bad(6) and g3(A2=odd, C2=p) == bad(6)
