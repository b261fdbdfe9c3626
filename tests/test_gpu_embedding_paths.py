"""Every kernel the Embedding entry points of csrc/seqops.hip launch, on a real MI355X against plain float64 numpy, on every
launch path, at ragged sizes, with padded rows, misaligned bases and ids outside [0, V).

Which test launches which kernel -- read against tnt_embedding_fwd_f32, tnt_embedding_fwd_drop{,2}_f32, tnt_embedding_bwd_f32,
tnt_embedding_bwd_sparse_f32 and tnt_step_finalize_f32:

    kernel                       test                        arguments that select it
    emb_fwd_kernel               test_fwd                    always; B T = 1, 21 and 5 leave a row tail (4 rows per workgroup), 5 x 11520 is
                                                             the gather use (T = 1, V = B, repeated and permuted ids)
    emb_fwd_drop_kernel          test_fwd_drop[*-one]        tnt_embedding_fwd_drop_f32 (rate2 = 0); out null and given, rate 0 and 0.3
                                 test_fwd_drop[*-two]        tnt_embedding_fwd_drop2_f32 with rate2 = 0.4: the second mask
    rowsq_kernel                 test_bwd_dense              sq_norm given (every other launch of a case; null on the others)
    sum_accum_kernel             test_bwd_dense              sq_norm given; n = 1190 is its second trip at 1024 threads
    zero_fill_kernel             test_bwd_dense              always: dtable starts as NaN, so a row it skips fails
    emb_bwd_kernel               test_bwd_dense[scalar-*]    E % 4 != 0: E in 1 63 65 70 (65, 70: a second 64-column block, 1 and 6 lanes);
                                                             E = 64 with ldd = 67; E = 64 with drows or dtable one float off 16 bytes
    emb_bwd4_kernel              test_bwd_dense[vec-*]       E in 4 252 256 260 512, ldd in E, E + 4, aligned (260: a second 256-column
                                                             block with one live lane)
    emb_bwd_sparse_kernel<16>    test_bwd_sparse[w16-*]      zero_id = -1
    emb_bwd_sparse_kernel<4>     test_bwd_sparse[w4-*]       zero_id >= 0 (0 where ldd = E, V - 1 where ldd = E + 4)
    step_finalize_kernel         test_bwd_sparse,            ids_src / ids_dst / n_ids (the id hand-off) and extra_part / extra / n_extra
                                 test_alternation            (the sum of the norm partials)
    both dense and both sparse   test_alternation            dense -> sparse -> sparse -> dense -> sparse on one table, ids handed on as
                                                             ModelBase._embedding_bwd does

Boundaries (test_boundaries_match_the_source reads them from csrc/seqops.hip): a workgroup's wave w scans the 64 positions
k+1+64w .. k+64+64w behind its own position k = b*T + t, then steps by NT = 256 (both dense kernels, sparse<4>) or 1024
(sparse<16>); the hits of one 64-wide ballot are consumed NF at a time, NF = 16 in emb_bwd_kernel and 8 in emb_bwd4_kernel and
the sparse kernel; a workgroup owns 64 columns (scalar) or 256 (float4, sparse).

Row counts n = B T (ROWS): 1, 21 = 7 x 3, 63 = 9 x 7, 65 = 13 x 5, 257 = 1 x 257, 1190 = 70 x 17.  257 is a prime, so that case
cannot tell row t*B + b from b*T + t; the others do.  257 is a second trip of the "earlier occurrence" scan and of the duplicate
scan at 256 threads, 1190 at 1024.

Id layouts (layouts()): a = all distinct (neither 0 nor V-1), b = one id everywhere, c = boundary: an owner at position k and
exactly m copies inside ONE ballot window k+1+64w+trip*NT .. +63, for m in NF-1, NF, NF+1, 2NF+1 at w = 0, the same four at a
wave w > 0, and two in the second trip; every other id distinct (packed into as few id arrays as hold them, what does not fit
n is left out; at n = 1190 all ten fit, asserted), d = the pad-heavy random layout of test_gpu_ops.test_embedding, e1 / e2 = stray ids -1, -7,
INT32_MIN, V, V+5, INT32_MAX among genuine 0 and V-1, the stray occurrence of a row first (e1) or the in-range one first (e2),
e3 = stray ids and neither 0 nor V-1 itself.

Reference: numpy float64, ids clamped (include/tnt_hip.h: an id counts as clip(id, 0, V-1)): forward table[clip(ids)], backward
np.add.at over the clamped ids, norm sum(rows ** 2) over the un-merged rows; inputs rounded to float32 first.  Two kinds of data:
  * exact: drows integers in [-3, 3], dropout rate 0.5 (scale 2).  Every float32 sum of such terms below 2^24 is exact in any
    order, so the table, EVERY sq_part entry (the owner's share of the norm per 256-column block, zero for a non-owner) and the
    norm must EQUAL the reference: no tolerance hides a dropped, doubled or misplaced row.  The worst-case norm with dropout,
    36 * 1190 * 512, is above 2^24; the drawn data stay far below (a mean of 8 per element), which exact_total() asserts.
  * gaussian: the bounds of test_gpu_ops.py: table 1e-5 of the reference's largest magnitude, norm 1e-5 relative.
The sparse form's mask is keep_mask((B, T, E)) of oracle/philox.py, the pattern test_fwd_drop finds in tnt_embedding_fwd_drop_f32's
output at ldo > E; it is applied here at ldd > E, so a mask indexed by ldd fails.

Every launch runs twice on fresh buffers and must give the same bits (twice() of test_gpu_encoder_paths.py); outputs sit in POISON
bands (Guards of test_gpu_lstm_paths.py); pad columns of the inputs hold 1e6, pad columns of `out` must keep their bits; sq_part
starts as NaN and every entry must end finite; dtable starts as NaN in the dense form."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle.philox import keep_mask
from test_gpu_lstm_paths import r32
from test_gpu_encoder_paths import twice, refuse, untouched, padded
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

KEEP = -77.25                                   # pad columns and unwritten rows of an output
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ROWS = [(1, 1), (7, 3), (9, 7), (13, 5), (1, 257), (70, 17)]          # (B, T)
NF_SCALAR, NF_VEC, NT_DENSE, NT_SPARSE = 16, 8, 256, {16: 1024, 4: 256}
SEED, SITE = 91, 49
F32 = np.float32


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def vocab(n):
    return n + 40


# ------------------------------------------------------------------------------------------------ id layouts
def stray_seq(V, kind):
    if kind == "e1":
        return [-1, 0, -7, I32_MIN, V, V - 1, V + 5, I32_MAX, 0, V - 1, -1, V]
    if kind == "e2":
        return [0, V - 1, -1, -7, I32_MIN, V, V + 5, I32_MAX, 0, V - 1]
    return [-7, V + 5, I32_MIN, I32_MAX, -7, V]              # e3: rows 0 and V-1 through stray ids only


def boundary_specs(NF, NT):
    """(m, w, trip): m copies of the owner's id in the ballot window of wave w in scan trip `trip`"""
    W = NT // 64
    ms = (NF - 1, NF, NF + 1, 2 * NF + 1)
    ws = sorted({1, W // 2, W - 1})
    trip2 = [(NF + 1, 0, 1), (NF, 1, 1)]                    # 1190 rows hold the second trip of waves 0 and 1 only at NT = 1024
    return trip2 + [(m, ws[i % len(ws)], 0) for i, m in enumerate(ms)] + [(m, 0, 0) for m in ms]


def boundary_layouts(n, V, NF, NT, rng):
    """-> [(ids[n], [(spec, owner position, id)])]: the specs that fit n, packed greedily; ids 1..19 mark the groups"""
    arrays = []

    def fresh():
        return dict(ids=np.zeros(n, np.int64), used=np.zeros(n, bool), cursor=0, groups=[])

    def place(st, spec):
        m, w, trip = spec
        k = st["cursor"]
        while k < n and st["used"][k]:
            k += 1
        s = k + 1 + 64 * w + trip * NT
        if s + 64 > n:
            return False
        free = [i for i in range(s, s + 64) if not st["used"][i]]
        if len(free) < m:
            return False
        pick, gid = rng.choice(free, m, replace=False), len(st["groups"]) + 1
        st["ids"][k] = st["ids"][pick] = gid
        st["used"][k] = st["used"][pick] = True
        st["groups"].append((spec, k, gid))
        st["cursor"] = s + 64 if (w == 0 and trip == 0) else k + 1
        return True

    for spec in boundary_specs(NF, NT):
        if not (arrays and place(arrays[-1], spec)):
            st = fresh()
            if place(st, spec):
                arrays.append(st)
    out = []
    for st in arrays:
        rest = np.flatnonzero(~st["used"])
        st["ids"][rest] = rng.permutation(np.arange(20, V - 1))[:len(rest)]
        for (m, w, trip), k, gid in st["groups"]:                 # what the docstring promises, recounted
            s = k + 1 + 64 * w + trip * NT
            hits = np.flatnonzero(st["ids"] == gid)
            assert hits[0] == k and len(hits) == m + 1 and (hits[1:] >= s).all() and (hits[1:] < s + 64).all()
        out.append((st["ids"], st["groups"]))
    return out


@functools.lru_cache(maxsize=None)
def layouts(B, T, NF, NT):
    """-> [(name, ids (B, T) int64)] for n = B T rows, in the order the sparse sequences consume them"""
    n, V = B * T, vocab(B * T)
    rng = np.random.default_rng(1000 * n + NF + NT)
    d = rng.integers(0, V, (B, T))
    d[0, :] = 3
    d[:, T // 2:] = np.where(rng.random((B, T - T // 2)) < 0.7, 0, d[:, T // 2:])
    out = [("d", d), ("b", np.full((B, T), 5)), ("a", rng.permutation(np.arange(1, V - 1))[:n].reshape(B, T))]
    for name in ("e1", "e2", "e3"):
        seq = stray_seq(V, name)[:n]
        ids = rng.permutation(np.arange(20, V - 1))[:n]
        ids[np.sort(rng.choice(n, len(seq), replace=False))] = seq
        out.append((name, ids.reshape(B, T)))
    cs = boundary_layouts(n, V, NF, NT, rng)
    if n == 1190:
        assert sorted(g[0] for _, groups in cs for g in groups) == sorted(boundary_specs(NF, NT)), "a boundary case does not fit"
    out += [(f"c{i}", ids.reshape(B, T)) for i, (ids, _) in enumerate(cs)]
    return out


# ------------------------------------------------------------------------------------------------ reference
def clamp(ids, V):
    return np.clip(np.asarray(ids, np.int64), 0, V - 1)


def ref_bwd(rows, ids, V, zero_id=-1):
    """rows (T, B, E) float64, ids (B, T) -> (table (V, E), rows in position order k = b*T + t with the zero_id rows at 0,
    clamped ids [n])"""
    T, B, E = rows.shape
    c = clamp(ids, V).reshape(-1)
    r = rows.transpose(1, 0, 2).reshape(B * T, E)
    if zero_id >= 0:
        r = np.where((c == zero_id)[:, None], 0.0, r)
    g = np.zeros((V, E))
    np.add.at(g, c, r)
    return g, r, c


def ref_parts(r, c):
    """sq_part[k * ny + y]: the first occurrence of an id holds the squares of all its rows in column block y, others hold 0"""
    n, E = r.shape
    ny = (E + 255) // 256
    sqb = np.stack([(r[:, 256 * y:256 * (y + 1)] ** 2).sum(1) for y in range(ny)], 1)
    first = {}
    owner = np.array([first.setdefault(int(v), k) for k, v in enumerate(c)])
    out = np.zeros((n, ny))
    np.add.at(out, owner, sqb)
    return out.reshape(-1)


def draw_rows(rng, T, B, E, exact):
    return rng.integers(-3, 4, (T, B, E)).astype(np.float64) if exact else r32(rng.standard_normal((T, B, E)))


def dropped(rows, rate, step):
    """the rows behind the mask tnt_embedding_fwd_drop_f32 applied: element (b*T + t) * E + e of stream (SEED, SITE, step)"""
    T, B, E = rows.shape
    keep = keep_mask((B, T, E), rate, SEED, SITE, step).transpose(1, 0, 2)
    scale = float(F32(1) / (F32(1) - F32(rate)))
    return np.where(keep, rows * scale, 0.0)


def exact_total(r):
    total = float((r ** 2).sum())
    assert total < 2 ** 24, "the exact data are not exact in float32 at this size"
    return total


def upload_rows(rows, ldd, off=0, nan_rows=None):
    """(T, B, E) -> device view [T*B][ldd], pad columns at 1e6, the base `off` floats behind a 16-byte boundary; nan_rows: a
    (T, B) mask of rows the kernel must not read"""
    T, B, E = rows.shape
    host = padded(rows.reshape(T * B, E), ldd)
    if nan_rows is not None:
        host[nan_rows.reshape(-1)] = np.nan
    flat = torch.zeros(T * B * ldd + 4, device="cuda")
    view = flat[off:off + T * B * ldd]
    view.copy_(dev(host).reshape(-1))
    return view


def same(got, want):
    """float32 values equal to the float64 reference: not one bit of rounding, no NaN"""
    want = np.asarray(want, np.float64)
    assert np.array_equal(want.astype(F32).astype(np.float64), want), "the reference is not a float32 number"
    return np.array_equal(got.detach().cpu().numpy().reshape(want.shape), want.astype(F32))


# ------------------------------------------------------------------------------------------------ (a) forward
FWD_CASES = [(1, 1, 1, 1, 1), (7, 3, 70, 75, 23), (9, 4, 36, 40, 11), (5, 1, 11520, 11520, 5), (64, 15, 512, 512, 5001)]


def fwd_ids(B, T, V, variant, rng):
    if (B, T) == (5, 1):
        return np.array([[3], [3], [0], [4], [1]]) if variant == 0 else np.array([[4], [0], [4], [2], [0]])
    ids = rng.integers(0, V, (B, T))
    if variant == 1:
        seq = stray_seq(V, "e1")[:B * T]
        ids.reshape(-1)[np.sort(rng.choice(B * T, len(seq), replace=False))] = seq
    return ids


@pytest.mark.parametrize("B,T,E,ldo,V", FWD_CASES, ids=lambda v: str(v))
def test_fwd(be, B, T, E, ldo, V):
    """tnt_embedding_fwd_f32: out[t*B + b][:E] = table[clip(ids[b][t])], bit for bit, pad columns untouched; ids in range and
    with strays; (5, 1, 11520): the row gather of beam search and consensus decoding"""
    rng = np.random.default_rng(B * T + E)
    table = r32(rng.standard_normal((V, E)))
    td = dev(table)
    for variant in (0, 1):
        ids = fwd_ids(B, T, V, variant, rng)
        idd = dev(ids, torch.int32)
        want = table[clamp(ids, V)].transpose(1, 0, 2).reshape(T * B, E)

        def launch(gs):
            out = gs.new("out", T * B, ldo, fill=KEEP)
            be.embedding_fwd(td, idd, out, B, T, E, ldo, V)
            return (out,)
        out, = twice(launch)
        assert same(out[:, :E], want), f"variant {variant}"
        assert bool((out[:, E:] == KEEP).all()), "pad columns written"


DROP_CASES = [(7, 3, 72, 76, 23), (9, 4, 36, 36, 11)]


@pytest.mark.parametrize("masks", ["one", "two"])
@pytest.mark.parametrize("B,T,E,ldo,V", DROP_CASES, ids=lambda v: str(v))
def test_fwd_drop(be, B, T, E, ldo, V, masks):
    """tnt_embedding_fwd_drop_f32 / _drop2_f32: the bits of embedding_fwd followed by be.dropout (and be.dropout with
    rows_per_site = B for the second mask), the keep pattern of oracle/philox.py, `out` (when given) the plain rows, pads kept"""
    rng = np.random.default_rng(B + E)
    table = r32(rng.standard_normal((V, E)))
    assert (table != 0).all()
    td, step, sdv, D = dev(table), 2, 3, 8
    sd = torch.tensor([sdv], dtype=torch.int32, device="cuda")
    r2, s2 = 0.4, 48
    mask2 = (r2, s2, D + E, D) if masks == "two" else None
    for variant, rate, with_out in [(0, 0.3, True), (1, 0.3, False), (1, 0.0, True), (0, 0.0, False)]:
        ids = fwd_ids(B, T, V, variant, rng)
        idd = dev(ids, torch.int32)
        plain = torch.full((T * B, ldo), KEEP, device="cuda")
        be.embedding_fwd(td, idd, plain, B, T, E, ldo, V)
        want = torch.full((T * B, ldo), KEEP, device="cuda")
        be.dropout(plain, want, T * B, E, ldo, B, E, 0, rate, SEED, SITE, step, sd)
        if mask2:
            be.dropout(want, want, T * B, E, ldo, 0, D + E, D, r2, SEED, s2, step, sd, rows_per_site=B)

        def launch(gs):
            out = gs.new("out", T * B, ldo, fill=KEEP) if with_out else None
            od = gs.new("out_drop", T * B, ldo, fill=KEEP)
            be.embedding_fwd_drop(td, idd, out, od, B, T, E, ldo, V, rate, SEED, SITE, step, sd, mask2=mask2)
            return (od, out) if with_out else (od,)
        got = twice(launch)
        assert torch.equal(got[0].view(torch.int32), want.view(torch.int32)), (rate, with_out)
        if with_out:
            assert torch.equal(got[1].view(torch.int32), plain.view(torch.int32))
        keep = keep_mask((B, T, E), rate, SEED, SITE, step + sdv).transpose(1, 0, 2)
        if mask2:
            keep = keep & np.stack([keep_mask((B, D + E), r2, SEED, s2 + t, step + sdv)[:, D:] for t in range(T)])
        assert np.array_equal(got[0][:, :E].cpu().numpy().reshape(T, B, E) != 0, keep), "not the oracle's keep pattern"
        # one mask: the float64 statement of it, rounded once
        if not mask2:
            rows = table[clamp(ids, V)].transpose(1, 0, 2)
            scale = F32(1) / (F32(1) - F32(rate))
            assert np.array_equal(got[0][:, :E].cpu().numpy().reshape(T, B, E), np.where(keep, rows.astype(F32) * scale, F32(0)))


def test_fwd_drop_refusals(be):
    """tnt_embedding_fwd_drop2_f32 refuses E % 4, ldo % 4, a misaligned table / out / out_drop, a rate outside [0, 1) and every
    clause of the second mask's geometry, and writes nothing"""
    import masters_thesis_amd.ops as ops
    B, T, E, V = 3, 2, 8, 5
    n = B * T
    tabf = torch.full((V * 12 + 4,), 7.0, device="cuda")
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    of, df = torch.full((n * 12 + 4,), 7.0, device="cuda"), torch.full((n * 12 + 4,), 7.0, device="cuda")
    good = (0.3, 48, 16, 8)

    def call(E=E, ldo=E, t_off=0, o_off=0, d_off=0, rate=0.3, mask2=None):
        be.embedding_fwd_drop(tabf[t_off:], ids, of[o_off:], df[d_off:], B, T, E, ldo, V, rate, SEED, SITE, 0, None, mask2=mask2)
    for kw in [dict(E=6, ldo=8), dict(E=8, ldo=10), dict(t_off=1), dict(o_off=1), dict(d_off=1), dict(rate=-0.1), dict(rate=1.0),
               dict(mask2=(1.0,) + good[1:]), dict(mask2=(0.3, 48, 18, 8)), dict(mask2=(0.3, 48, 16, 6)),
               dict(mask2=(0.3, 48, 16, -4)), dict(mask2=(0.3, 48, 12, 8)), dict(t_off=1, mask2=good), dict(rate=1.5, mask2=good)]:
        refuse(lambda: call(**kw))
    # a negative second rate does not pass the Python wrapper's "mask2 given" test: straight at the entry point
    refuse(lambda: be._call(be.lib.tnt_embedding_fwd_drop2_f32, "tnt_embedding_fwd_drop2_f32", ops._p(tabf), ops._p(ids), ops._p(of),
                            ops._p(df), B, T, E, E, V, 0.3, SEED, SITE, 0, None, -0.1, 48, 16, 8, be._s()))
    untouched(of, df)
    call(mask2=good)                                                              # and the unmodified arguments pass
    torch.cuda.synchronize()
    assert bool((df[:n * E] != 7.0).any())


# ------------------------------------------------------------------------------------------------ (b) dense backward
DENSE_CASES = ([pytest.param("scalar", E, E, 0, 0, id=f"scalar-E{E}") for E in (1, 63, 65, 70)]
               + [pytest.param("scalar", 64, 67, 0, 0, id="scalar-E64-ldd67"),
                  pytest.param("scalar", 64, 64, 1, 0, id="scalar-E64-drows+1"),
                  pytest.param("scalar", 64, 64, 0, 1, id="scalar-E64-dtable+1")]
               + [pytest.param("vec", E, E + p, 0, 0, id=f"vec-E{E}-ldd{E + p}") for E in (4, 252, 256, 260, 512) for p in (0, 4)])


def run_dense(be, rows, ids, V, ldd, sq_given, off_d=0, off_t=0):
    T, B, E = rows.shape
    dr, idd = upload_rows(rows, ldd, off_d), dev(ids, torch.int32)

    def launch(gs):
        full = gs.new("dtable", V * E + 4)
        sq = gs.new("sq_norm", 1) if sq_given else None
        work = gs.new("rowsq_work", B * T) if sq_given else None
        be.embedding_bwd(dr, idd, full[off_t:off_t + V * E], sq, work, B, T, E, ldd, V)
        return (full, sq) if sq_given else (full,)
    got = twice(launch)
    full = got[0]
    assert bool(torch.isnan(full[:off_t]).all()) and bool(torch.isnan(full[off_t + V * E:]).all()), "written around dtable"
    return full[off_t:off_t + V * E].view(V, E), (got[1] if sq_given else None)


@pytest.mark.parametrize("kernel,E,ldd,off_d,off_t", DENSE_CASES)
def test_bwd_dense(be, kernel, E, ldd, off_d, off_t):
    """tnt_embedding_bwd_f32 on both scatter kernels: every row count, every id layout, exact data -- table and norm EQUAL the
    float64 scatter over the clamped ids -- then gaussian data at 63 and 1190 rows within the existing bounds; sq_norm given on
    every other launch, null on the rest"""
    assert (kernel == "vec") == (E % 4 == 0 and ldd % 4 == 0 and off_d == 0 and off_t == 0)          # the dispatch's condition
    NF = NF_VEC if kernel == "vec" else NF_SCALAR
    rng = np.random.default_rng(E * 7 + ldd)
    launches = 0
    for B, T in ROWS:
        V = vocab(B * T)
        for name, ids in layouts(B, T, NF, NT_DENSE):
            for exact in (True, False) if (name == "d" and B * T in (63, 1190)) else (True,):
                rows = draw_rows(rng, T, B, E, exact)
                sq_given = launches % 2 == 0
                launches += 1
                tab, sq = run_dense(be, rows, ids, V, ldd, sq_given, off_d, off_t)
                g, r, _ = ref_bwd(rows, ids, V)
                what = f"n = {B * T}, layout {name}, {'exact' if exact else 'gaussian'}"
                if exact:
                    assert same(tab, g), f"table differs from the scatter over the clamped ids: {what}"
                    assert sq is None or float(sq) == exact_total(r), f"norm {float(sq)} != {exact_total(r)}: {what}"
                else:
                    close(tab, g, atol=1e-5 * np.abs(g).max())
                    assert sq is None or abs(float(sq) - (r ** 2).sum()) <= 1e-5 * (r ** 2).sum(), what


# ------------------------------------------------------------------------------------------------ (c) sparse backward
def int_guarded(n, fill):
    flat = torch.full((n + 16,), 12345, dtype=torch.int32, device="cuda")
    flat[8:8 + n] = fill
    return flat, flat[8:8 + n]


def run_sparse_steps(be, B, T, E, ldd, V, steps, zero_id, dense_at=()):
    """steps: [(ids (B, T), rows (T, B, E), rate, drop step)] on ONE table from zero; after a sparse call tnt_step_finalize_f32 hands
    the ids on and sums the partials, after a dense call (positions dense_at) the ids are copied as ModelBase._embedding_bwd does.
    -> per step (table, sq_part or None, norm, prev_ids), from the first of two bit-identical runs"""
    n = B * T
    nparts = be.embedding_bwd_parts(B, T, E)
    assert nparts == n * ((E + 255) // 256)
    none = torch.zeros(1, device="cuda")
    ups = []
    for ids, rows, rate, dstep in steps:
        nan_rows = (clamp(ids, V) == zero_id).T if zero_id >= 0 else None
        ups.append((upload_rows(rows, ldd, nan_rows=nan_rows), dev(ids, torch.int32),
                    torch.tensor([dstep], dtype=torch.int32, device="cuda")))

    def launch(gs):
        tab = gs.new("dtable", V, E, fill=0.0)
        pflat, prev = int_guarded(n, -1)
        outs = []
        for i, ((dr, idd, sd), (ids, rows, rate, dstep)) in enumerate(zip(ups, steps)):
            sq = gs.new("sq_norm", 1)
            if i in dense_at:
                parts = None
                be.embedding_bwd(dr, idd, tab, sq, gs.new("rowsq_work", n), B, T, E, ldd, V)
                prev.copy_(idd.reshape(-1))
            else:
                parts = gs.new("sq_part", nparts)
                be.embedding_bwd_sparse(dr, idd, prev, tab, parts, B, T, E, ldd, V, drop_rate=rate, drop_seed=SEED, drop_site=SITE,
                                        drop_step_dev=sd if rate > 0 else None, zero_id=zero_id)
                be.step_finalize(none, None, None, None, None, None, 0, extra_part=parts, extra=sq, n_extra=nparts, ids_src=idd,
                                 ids_dst=prev, n_ids=n)
            outs += [tab.clone(), sq, prev.clone()] + ([parts] if parts is not None else [])
        return tuple(outs) + (pflat,)
    got = list(twice(launch))
    pflat = got.pop()
    assert bool((pflat[:8] == 12345).all()) and bool((pflat[8 + n:] == 12345).all()), "written around prev_ids"
    res = []
    for i in range(len(steps)):
        tab, sq, prev = got[:3]
        got = got[3:]
        res.append((tab, None if i in dense_at else got.pop(0), sq, prev))
    return res


def check_steps(res, steps, V, zero_id, exact, what):
    """after every step the table is THAT step's scatter alone, zero where the reference is; the partials are finite and the
    owner's share each; the norm is the un-merged rows'; prev_ids holds the step's ids as given"""
    for i, ((tab, parts, sq, prev), (ids, rows, rate, dstep)) in enumerate(zip(res, steps)):
        msg = f"{what}, step {i}"
        eff = dropped(rows, rate, dstep) if rate > 0 else rows
        g, r, c = ref_bwd(eff, ids, V, zero_id)
        total = (r ** 2).sum()
        assert torch.equal(prev.cpu(), torch.tensor(np.asarray(ids).reshape(-1).astype(np.int32))), f"prev_ids != ids: {msg}"
        if parts is not None:
            assert bool(torch.isfinite(parts).all()), f"a norm partial was not written: {msg}"
        if exact:
            assert same(tab, g), f"table differs from this step's scatter over the clamped ids: {msg}"
            assert float(sq) == exact_total(r), f"norm {float(sq)} != {total}: {msg}"
            if parts is not None:
                assert same(parts, ref_parts(r, c)), f"sq_part is not the owner's share: {msg}"
        else:
            close(tab, g, atol=1e-5 * np.abs(g).max())
            assert abs(float(sq) - total) <= 1e-5 * total, msg
        assert np.array_equal(tab.cpu().numpy() == 0, g == 0), f"zero pattern: {msg}"


SPARSE_CASES = [pytest.param(W, E, E + p, id=f"w{W}-E{E}-ldd{E + p}") for W in (16, 4) for E in (4, 36, 256, 260, 512) for p in (0, 4)]


@pytest.mark.parametrize("W,E,ldd", SPARSE_CASES)
def test_bwd_sparse(be, W, E, ldd):
    """tnt_embedding_bwd_sparse_f32 at 16 and at 4 waves over sequences of three consecutive steps per row count: the layouts in
    sequences d b a (ids vanish; d carries zero_id = 0, b has it in prev_ids only, a nowhere), e1 e2 c0 (stray ids reach prev_ids),
    e3 a e2 (rows 0 and V-1 written through stray ids ONLY, then a step that touches neither: the cleanup has to clamp) and the
    remaining boundary layouts; dropout on every other step with rate 0.5 (exact) / 0.3 (gaussian), at ldd = E and E + 4"""
    rng = np.random.default_rng(E + ldd + W)
    for B, T in ROWS:
        V = vocab(B * T)
        zero_id = -1 if W == 16 else (0 if ldd == E else V - 1)
        lay = dict(layouts(B, T, NF_VEC, NT_SPARSE[W]))
        cs = [nm for nm in lay if nm[0] == "c"]
        names = ([["d", "b", "a"], ["e1", "e2", cs[0] if cs else "d"], ["e3", "a", "e2"]]
                 + [(cs[i:i + 3] + ["d", "b"])[:3] for i in range(1, len(cs), 3)])
        seqs = [[(nm, lay[nm]) for nm in seq] for seq in names]
        runs = [(s, True) for s in seqs] + ([(seqs[0], False)] if B * T in (63, 1190) else [])
        for q, (seq, exact) in enumerate(runs):
            steps = [(ids, draw_rows(rng, T, B, E, exact), (0.5 if exact else 0.3) if (i + q) % 2 else 0.0, 3 + i + q)
                     for i, (_, ids) in enumerate(seq)]
            res = run_sparse_steps(be, B, T, E, ldd, V, steps, zero_id)
            check_steps(res, steps, V, zero_id, exact, f"n = {B * T}, layouts {[nm for nm, _ in seq]}, zero_id {zero_id}")


@pytest.mark.parametrize("B,T", [(13, 5), (70, 17)], ids=lambda v: str(v))
def test_alternation(be, B, T):
    """dense (d) -> sparse (e3) -> sparse (a) -> dense (e2) -> sparse (b) on one table: whichever form ran last, the table is
    zero outside the CLAMPED rows of prev_ids, so after every call it equals that call's scatter alone"""
    E, ldd, V = 36, 40, vocab(B * T)
    rng = np.random.default_rng(B)
    lay = dict(layouts(B, T, NF_VEC, NT_SPARSE[16]))
    steps = [(lay[nm], draw_rows(rng, T, B, E, True), 0.0, 0) for nm in ("d", "e3", "a", "e2", "b")]
    res = run_sparse_steps(be, B, T, E, ldd, V, steps, -1, dense_at=(0, 3))
    check_steps(res, steps, V, -1, True, f"alternation, n = {B * T}")


def test_bwd_sparse_refusals(be):
    """every refusal of tnt_embedding_bwd_sparse_f32 leaves the table (and the partials) untouched"""
    B, T, E, V = 3, 2, 8, 5
    n = B * T
    rowf = torch.ones(n * 12 + 4, device="cuda")
    tabf, parts = torch.full((V * 12 + 4,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
    ids, prev = torch.ones(n, dtype=torch.int32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def call(B=B, T=T, E=E, V=V, ldd=E, r_off=0, t_off=0, prev=prev, parts=parts, **kw):
        be.embedding_bwd_sparse(rowf[r_off:], ids, prev, tabf[t_off:], parts, B, T, E, ldd, V, **kw)
    for kw in [dict(B=0), dict(T=0), dict(E=0, ldd=8), dict(V=0), dict(B=-1), dict(T=-2), dict(E=-4, ldd=8), dict(V=-1),
               dict(E=6, ldd=8), dict(ldd=10), dict(r_off=1), dict(t_off=1), dict(prev=None), dict(parts=None), dict(prev=ids),
               dict(zero_id=V), dict(zero_id=V + 3), dict(drop_rate=-0.1), dict(drop_rate=1.0)]:
        refuse(lambda: call(**kw))
    untouched(tabf, parts)
    call(zero_id=V - 1, drop_rate=0.5)                                             # and the unmodified arguments pass
    torch.cuda.synchronize()
    assert float(tabf[E]) != 7.0


# ------------------------------------------------------------------------------------------------ the docstring's constants
def test_boundaries_match_the_source():
    """NF, the columns per workgroup and the scan steps this file's layouts are built around, read from csrc/seqops.hip"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "masters-thesis_amd", "csrc", "seqops.hip")).read()

    def body(name):
        m = re.search(r"void " + name + r"\(.*?(?=__global__|\Z)", src, re.S)
        assert m, name
        return m.group(0)
    s, v, p = body("emb_bwd_kernel"), body("emb_bwd4_kernel"), body("emb_bwd_sparse_kernel")
    assert f"constexpr int NF = {NF_SCALAR};" in s and f"constexpr int NF = {NF_VEC};" in v and f"constexpr int NF = {NF_VEC};" in p
    for b in (s, v):
        assert f"base = k + 1 + 64 * w; base < n; base += {NT_DENSE})" in b and f"i < k; i += {NT_DENSE})" in b
    assert "constexpr int NT = 64 * EBS_W;" in p and "base = k + 1 + 64 * w; base < n; base += NT)" in p and "i < k; i += NT)" in p
    assert "blockIdx.y * 64 + lane" in s and "blockIdx.y * 256 + lane * 4" in v and "blockIdx.y * 256 + lane * 4" in p
    for fwd in ("emb_fwd_kernel", "emb_fwd_drop_kernel"):
        assert "blockIdx.x * 4 + (threadIdx.x >> 6)" in body(fwd)
    assert re.search(r"emb_bwd_sparse_kernel<4>, dim3\(2 \* B \* T, \(E \+ 255\) / 256\), dim3\(256\)", src)
    assert re.search(r"emb_bwd_sparse_kernel<16>, dim3\(2 \* B \* T, \(E \+ 255\) / 256\), dim3\(1024\)", src)
    assert {W: 64 * W for W in NT_SPARSE} == NT_SPARSE
    assert "sum_accum_kernel, dim3(1), dim3(1024)" in src and "i < n; i += 1024) s += x[i];" in src
