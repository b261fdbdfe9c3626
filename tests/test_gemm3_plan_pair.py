"""tnt_gemm3_plan_pair (csrc/gemm3.hip), the joint plan of a pair launch, on the host: for the pair shapes a training step of
both bench workloads launches and a sweep of live extents it returns tiles the pair kernel has, grids whose workgroups are
all resident together where a product is split, and a modelled makespan not above that of the two independent
tnt_gemm3_plan picks.  No compute call is made (runs without a GPU)."""
import ctypes as C
import os

import pytest

TILES = {1: (160, 128, 32), 2: (128, 160, 32), 3: (128, 128, 32), 4: (128, 80, 32), 5: (64, 128, 32), 6: (128, 64, 32), 7: (64, 64, 32),
         8: (256, 80, 32), 9: (64, 64, 64), 10: (64, 128, 64), 11: (128, 64, 64)}
NOSPLIT, MAP, SMALL = 1, 2, 4
# (name, product 1, product 2, the extent a live word bounds or None); a product = (M, N, K, transA, transB, batch, flags)
PAIRS = [
    ("dense head", (512, 5001, 960, 1, 0, 1, NOSPLIT), (960, 512, 5001, 0, 1, 1, MAP), 960),
    ("dense lstm", (512, 2048, 1024, 1, 0, 2, NOSPLIT), (1024, 512, 2048, 0, 1, 1, 0), None),
    ("attention head", (256, 5001, 960, 1, 0, 1, 0), (960, 256, 5001, 0, 1, 1, 0), None),
    ("attention lstm", (512, 2048, 960, 1, 0, 2, NOSPLIT), (960, 512, 2048, 0, 1, 1, 0), None),
    ("attention head, compacted", (256, 5001, 960, 1, 0, 1, NOSPLIT), (960, 256, 5001, 0, 1, 1, MAP), 960),
]
LIVES = (0, 1, 63, 64, 65, 300, 480, 600, 700, 736, 752, 760, 784, 800, 896, 897, 959, 960, 2000)


@pytest.fixture(scope="module")
def lib():
    from masters_thesis_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the kernel library first: __graft_entry__.build()"
    return C.CDLL(_lib.LIB_PATH)


def plan_pair(lib, p1, p2, live1, live2):
    a = (C.c_int32 * 8)(*p1[:6], live1, p1[6])
    b = (C.c_int32 * 8)(*p2[:6], live2, p2[6])
    out, span = (C.c_int32 * 8)(), (C.c_double * 2)()
    rc = lib.tnt_gemm3_plan_pair(a, b, out, span)
    return rc, list(out), list(span)


def independent(lib, p):
    t, s = C.c_int32(0), C.c_int32(0)
    assert lib.tnt_gemm3_plan(p[0], p[1], p[2], p[3], p[4], p[5], 0 if p[6] & NOSPLIT else 1, C.byref(t), C.byref(s)) == 0
    return t.value, s.value


@pytest.mark.parametrize("case", PAIRS, ids=[c[0] for c in PAIRS])
def test_plan_pair(lib, case):
    _, p1, p2, extent = case
    for lv in (LIVES if extent is not None else (0,)):
        rc, out, span = plan_pair(lib, p1, p2, lv, lv)
        assert rc == 0, (case[0], lv, rc)
        (t1, s1, n1), (t2, s2, n2), resident = out[0:3], out[3:6], out[6]
        assert lib.tnt_gemm3_pair_supported(t1, p1[3], p1[4], t2, p2[3], p2[4]) == 1, (lv, out)
        for p, t, s, n in ((p1, t1, s1, n1), (p2, t2, s2, n2)):
            bm, bn, bk = TILES[t]
            nst = -(-p[2] // bk)
            per = -(-nst // s)
            assert s >= 1 and -(-nst // per) == s, (lv, out)                    # no split without K stages
            assert n == -(-p[0] // bm) * -(-p[1] // bn) * s * p[5], (lv, out)   # the grid covers the FULL shape
            if p[6] & NOSPLIT:
                assert s == 1, (lv, out)
            if s > 1:
                assert per >= 4 and lib.tnt_gemm3_work_floats(p[0], p[1], t, s, p[5]) == n * bm * bn, (lv, out)
        if s1 > 1 or s2 > 1:                                                    # the splits of a tile are resident together
            assert 1 <= resident and n1 + n2 <= min(1024, 256 * resident), (lv, out)
        assert span[0] <= span[1] < 1e29, (lv, span)
        if case[0] == "dense head" and (lv == 0 or lv >= extent):      # the flagship pair without a shorter extent: today's plan
            assert (t1, s1) == independent(lib, p1) and (t2, s2) == independent(lib, p2), (lv, out)


def test_the_map_shortens_the_modelled_head_pair(lib):
    """the bench's head pair at the live counts its batches have (736 to 760 of 960 rows): with the device-side map the
    modelled makespan is below the one without it, and it never is above"""
    _, p1, p2, _ = PAIRS[0]
    for lv in LIVES:
        with_map = plan_pair(lib, p1, p2, lv, lv)[2][0]
        without = plan_pair(lib, p1, p2[:6] + (0,), lv, lv)[2][0]
        assert with_map <= without + 1e-9, (lv, with_map, without)
        if 700 <= lv <= 768:
            assert with_map < without - 3.0, (lv, with_map, without)


def test_plan_pair_refuses(lib):
    out, span = (C.c_int32 * 8)(), (C.c_double * 2)()
    good = (C.c_int32 * 8)(512, 5001, 960, 1, 0, 1, 0, NOSPLIT)
    bad = (C.c_int32 * 8)(0, 5001, 960, 1, 0, 1, 0, 0)
    assert lib.tnt_gemm3_plan_pair(None, good, out, span) != 0 and lib.tnt_gemm3_plan_pair(good, bad, out, span) != 0
    nn = (C.c_int32 * 8)(960, 5001, 512, 0, 0, 1, 0, 0)                          # NN + NN has no pair form
    assert lib.tnt_gemm3_plan_pair(nn, nn, out, span) != 0
    assert lib.tnt_gemm3_plan_pair(good, (C.c_int32 * 8)(960, 512, 5001, 0, 1, 1, 0, 0), out, None) == 0     # span is optional
