"""gemm3's device-side unit map (live_mode 3, ops.LIVE_ROWS_M_MAP; csrc/gemm3.hip, G3Cfg::body<true>) against float64.

A split NT product whose device word leaves fewer row tiles than M has deals its grid over the live row tiles only, with the
largest split that fits the grid.  Shape (both tiles): M = 256 -- four row tiles of 64 --, N = 200 -- a ragged last column tile
of either tile --, K = 328 -- ten full 32-deep stages and a tail of 8 --, planned with split 2 (6 + 5 stages).  The live words
and the map each one gives on the 64 x 128 tile (16 units) / the 64 x 64 tile (32 units):

    0            no live tile: every workgroup leaves
    1, 63, 64    one row tile:    2 / 4 tiles, S' = 6 (2 stages each, the last split 1) -- the split is bounded by the grid
    65, 128      two row tiles:   4 / 8 tiles, S' = 4 (3 stages each, the last split 2)
    129          three row tiles: 6 / 12 tiles, S' = 2 -- the host's split on fewer tiles, units left over on some XCDs
    255, 256     four row tiles: today's map (255: the last tile ragged)
    300          past M: clamped, today's map

Checked per word, on exact (integer) and random data: rows below the word against float64 (bit for bit / gemm3's bound,
gemm_oracle.g3_bound -- the tolerances tests/test_gpu_gemm_paths.py uses for split products); rows at or past it keep the NaN
they were poisoned with (as do the pad columns and the guard bands); the error word is 0; the whole work buffer holds the
sentinel afterwards; a second launch on the same work buffer gives identical bits; words 256 and 300 give the bits of the
launch without the map (live_mode 1).  The rows of A at or past the word are NaN: they do not exist and must not be read.

The pair form runs the same sweep through tnt_gemm3_pair_f32 the way the vocabulary head's backward uses it: dlogits
[256][328] is the B operand of a TN product under LIVE_ROWS_K (dW = Out^T dlogits with the column sums as a rider) and the A
operand of the NT product under the map (dX = dlogits W^T), one live word for both; U = 200 on the benchmark's tiles (128 x 80
TN, 64 x 128 NT) and U = 128 on the 64 x 64 pair."""
import numpy as np
import pytest
import torch

import gemm_oracle as G
from test_gpu_gemm_paths import KINDS, SENTINEL, compare, g3_operands, pads_kept, put
from test_gpu_lstm_paths import Guards
from test_gpu_ops import dev
from test_gpu_rowop_paths import Report, bits

pytestmark = pytest.mark.gpu

M, N, K, S = 256, 200, 328, 2
LIVES = (0, 1, 63, 64, 65, 128, 129, 255, 256, 300)
LIVE_ROWS_M, LIVE_ROWS_K, LIVE_ROWS_M_MAP = 1, 2, 3


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    assert (ops.LIVE_ROWS_M, ops.LIVE_ROWS_K, ops.LIVE_ROWS_M_MAP) == (LIVE_ROWS_M, LIVE_ROWS_K, LIVE_ROWS_M_MAP)
    return ops.backend()


def device_map(tile, Mv, units, nst):
    """the unit map body<true> derives: (live units, split, stages per split)"""
    bm, bn, _ = G.g3_tile(tile)
    mt, mtv, ntl = -(-M // bm), -(-Mv // bm), -(-N // bn)
    if mtv >= mt:
        return units, S, -(-nst // S)
    if mtv == 0:
        return 0, 0, 0
    s0 = min(units // (mtv * ntl), nst)
    per = -(-nst // s0)
    s = -(-nst // per)
    return mtv * ntl * s, s, per


def test_the_sweep_reaches_every_map():
    """the live words of this file give, on both tiles: no unit, a split bounded by the grid, a split above the host's, the
    host's split on fewer tiles with units left over, and today's map"""
    for tile, units in ((5, 16), (7, 32)):
        nst = G.g3_split(tile, K, S)[0]
        assert nst == 11 and G.g3_units(tile, M, N, S) == units
        maps = {lv: device_map(tile, min(lv, M), units, nst) for lv in LIVES}
        assert maps[0][0] == 0
        assert maps[1] == maps[63] == maps[64] == (units * 6 // 8, 6, 2)
        assert maps[65] == maps[128] == (units, 4, 3)
        assert maps[129] == (units * 6 // 8, 2, 6)
        assert maps[255] == maps[256] == maps[300] == (units, 2, 6)


def poisoned_rows(Ad, ld, rows, width, lv):
    """a copy of the embedded operand whose rows at or past `lv` hold NaN"""
    out = Ad.clone()
    torch.as_strided(out, (rows, width), (ld, 1))[lv:] = float("nan")
    return out


def rows_kept(C, lv):
    want = torch.full_like(C[lv:], float("nan")).contiguous()
    assert torch.equal(bits(C[lv:].contiguous()), bits(want)), "a row at or past the live extent was written"


def armed(work, sync):
    torch.cuda.synchronize()
    assert bool((work.view(torch.int32) == SENTINEL).all()), "the exchange buffer is not re-armed"
    assert int(sync.sum()) == 0, "the error word is set"


@pytest.mark.parametrize("tile", [5, 7])
def test_gemm3_live_map(be, tile):
    rep = Report(f"gemm3 live map tile {tile}")
    ldc = G.roundup4(N) + 4
    wf = be.gemm3_work_floats(M, N, tile, S)
    assert wf == G.g3_work_floats(tile, M, N, S)
    for kind in KINDS:
        rng = np.random.default_rng([tile, KINDS.index(kind), 31])
        (opA, opB), es = g3_operands(rng, kind, "NT", M, N, K, 4)
        Ad, Bd = put(es[0]), put(es[1])
        want = G.product(opA, opB)
        for lv in LIVES:
            Mv = min(lv, M)
            live = torch.tensor([lv], dtype=torch.int32, device="cuda")
            Al = poisoned_rows(Ad, es[0].ld, M, K, Mv)
            gs = Guards()
            work, sync = gs.new("work", wf), torch.zeros(1, dtype=torch.int32, device="cuda")
            be.gemm3_work_arm(work)

            def launch(mode):
                C = gs.new("C", M, ldc)
                be.gemm3(Al, Bd, C, M, N, K, es[0].ld, es[1].ld, ldc, transB=True, tile=tile, splitk=S, work=work, sync=sync,
                         live=live, live_mode=mode)
                armed(work, sync)
                return C
            C, again = launch(LIVE_ROWS_M_MAP), launch(LIVE_ROWS_M_MAP)
            gs.check()
            assert torch.equal(bits(C), bits(again)), f"live {lv}: a second launch on the same buffers gave other bits"
            pads_kept(C, N)
            rows_kept(C, Mv)
            if Mv:
                compare(rep, kind, f"{kind} live {lv} C", C[:Mv, :N], want[:Mv], G.g3_bound(want[:Mv], K))
            if lv >= M:
                assert torch.equal(bits(C), bits(launch(LIVE_ROWS_M))), f"live {lv}: not the bits of the launch without the map"
    rep.check()


@pytest.mark.parametrize("tn_tile,nt_tile,U", [(4, 5, 200), (7, 7, 128)])
def test_gemm3_pair_live_map(be, tn_tile, nt_tile, U):
    rep = Report(f"gemm3 pair live map TN {tn_tile} + NT {nt_tile}, U {U}")
    V, R = K, M                       # dlogits [R][V]; Out [R][U]; W [U][V]
    ldv, ldu = G.roundup4(V) + 4, G.roundup4(U) + 4
    assert be.gemm3_pair_supported(tn_tile, True, False, nt_tile, False, True)
    wf = be.gemm3_work_floats(R, U, nt_tile, S)
    for kind in KINDS:
        rng = np.random.default_rng([tn_tile, nt_tile, U, KINDS.index(kind), 32])
        (dl, wT), es = g3_operands(rng, kind, "NT", R, U, V, 4)             # dlogits (K-contiguous A), W^T
        out_rows = (G.ints(rng, R, U) if kind == "exact" else rng.standard_normal((R, U))).astype(np.float32)
        Dd, Wd = put(es[0]), put(es[1])
        for lv in LIVES:
            Rv = min(lv, R)
            live = torch.tensor([lv], dtype=torch.int32, device="cuda")
            Dl = poisoned_rows(Dd, es[0].ld, R, V, Rv)
            o = out_rows.copy()
            o[Rv:] = np.nan
            Od = dev(np.pad(o, ((0, 0), (0, ldu - U)), constant_values=np.nan))
            gs = Guards()
            work, sync = gs.new("work", wf), torch.zeros(1, dtype=torch.int32, device="cuda")
            be.gemm3_work_arm(work)

            def launch(mode):
                dW, db, dX = gs.new("dW", U, ldv), gs.new("db", ldv), gs.new("dX", R, ldu)
                d1 = be.gemm3_desc(Od, Dl, dW, U, V, R, ldu, es[0].ld, ldv, transA=True, colsum=db, tile=tn_tile,
                                   live=live, live_mode=LIVE_ROWS_K)
                d2 = be.gemm3_desc(Dl, Wd, dX, R, U, V, es[0].ld, es[1].ld, ldu, transB=True, tile=nt_tile, splitk=S,
                                   work=work, sync=sync, live=live, live_mode=mode)
                be.gemm3_pair(d1, d2)
                armed(work, sync)
                return dW, db, dX
            first, again = launch(LIVE_ROWS_M_MAP), launch(LIVE_ROWS_M_MAP)
            gs.check()
            for a, b in zip(first, again):
                assert torch.equal(bits(a), bits(b)), f"live {lv}: a second launch on the same buffers gave other bits"
            dW, db, dX = first
            pads_kept(dW, V), pads_kept(db, V), pads_kept(dX, U)
            rows_kept(dX, Rv)
            tag = f"{kind} live {lv} "
            w_dw = G.product(out_rows[:Rv].astype(np.float64).T, dl[:Rv])
            compare(rep, kind, tag + "dW", dW[:, :V], w_dw, G.g3_bound(w_dw, max(Rv, 1)) + 1e-30)
            compare(rep, kind, tag + "db", db[:V], G.colsum(dl[:Rv]), (Rv + 2) * G.U24 * np.abs(dl[:Rv]).sum(0) + 1e-30)
            if Rv:
                w_dx = G.product(dl, wT)[:Rv]
                compare(rep, kind, tag + "dX", dX[:Rv, :U], w_dx, G.g3_bound(w_dx, V))
            if lv >= R:
                for a, b in zip(first, launch(LIVE_ROWS_M)):
                    assert torch.equal(bits(a), bits(b)), f"live {lv}: not the bits of the launch without the map"
    rep.check()
