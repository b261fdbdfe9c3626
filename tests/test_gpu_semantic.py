"""tnt_cosine_loss_f32, tnt_row_inv_norm_f32 and tnt_cosine_topk_f32 on a real MI355X against tests/semantic_oracle.py (float64
for the loss, its gradient and the norms; the float32 restatement of the similarity and the selection's total order, which the
selection must reproduce bit for bit).

Loss shapes (B, G): (1, 1), (3, 5) scalar tail only, (5, 63), (4, 64) one float4 per 16 lanes, (7, 65), (2, 512) config 2's
width, (64, 512), (65, 516) more rows than waves, (3, 2048) the widest; once with row strides above G, once without dz, once
with dz in place of z, once on pointers that are not 16-byte aligned (the single-float walk).

Bounds, derived: inputs lie in [-1, 1].  A G-term float32 sum is within G 2^-24 times the sum of the absolute terms of exact;
behind the normalisation that sum is at most 1, so
  |cos - ref| <= 4 (G + 8) 2^-24                              (three sums, two roots, two divisions)
  |dz - ref|  <= 8 (G + 8) 2^-24 gscale / nz   per element    (nz = sqrt(max(sum z^2, 1e-12)) of the reference)
  |inv - ref| <= (G + 8) 2^-24 |ref|
Run-to-run identity and row independence are bit comparisons."""
import ctypes

import numpy as np
import pytest
import torch

import semantic_oracle as SO
from test_gpu_ops import dev
from test_gpu_attention_paths import guarded, SENT

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24
LOSS_SHAPES = [(1, 1), (3, 5), (5, 63), (4, 64), (7, 65), (2, 512), (64, 512), (65, 516), (3, 2048)]
TOPK_SHAPES = [(1, 1, 1), (3, 7, 7), (2, 64, 5), (5, 65, 64), (4, 1000, 10), (64, 4099, 32)]
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def rows(B, G, ld, seed, off=0):
    """(host float32 [B][G], device buffer [B][ld] with NaN in the pad columns, its first element ``off`` floats into a
    16-byte aligned allocation)"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1, 1, (B, G)).astype(np.float32)
    flat = torch.full((B * ld + off,), float("nan"), device="cuda")
    d = flat[off:].view(B, ld)
    d[:, :G] = dev(h)
    return h, d


def run_loss(be, z, g, B, G, ldz, ldg, gscale, mode="dz"):
    """mode: "dz" (its own buffer), "none", "alias" (in place of z).  Returns (loss, cos, mean, dz or None)"""
    loss, t1 = guarded(B)
    cos, t2 = guarded(B)
    out, t3 = guarded(1)
    zz = z.clone()
    dz, t4 = guarded(B, ldz, fill=7.0)
    arg = dict(dz=dz, none=None, alias=zz)[mode]
    be.cosine_loss(zz, ldz, g, ldg, arg, loss, cos, out, B, G, gscale)
    torch.cuda.synchronize()
    for t in (t1, t2, t3, t4):
        assert (t == SENT).all()
    if mode == "dz":
        assert (dz[:, G:] == 7.0).all()                 # the pad columns are not written
        assert torch.equal(zz[:, :G], z[:, :G])
    d = None if mode == "none" else (dz if mode == "dz" else zz)[:, :G].clone()
    return loss.clone(), cos.clone(), out.clone(), d


def check_loss(got, z, g, B, G, gscale):
    loss, cos, out, dz = got
    wl, wc, wd = SO.cosine_loss(z, g, gscale)
    f64 = lambda t: t.cpu().double().numpy()
    ec = np.abs(f64(cos) - wc).max() / (4 * (G + 8) * UNIT)
    el = np.abs(f64(loss) - wl).max() / (4 * (G + 8) * UNIT)
    em = abs(float(out[0]) - wl.mean()) / (4 * (G + 8) * UNIT)
    print(f"  ({B}, {G}): cos error / bound {ec:.3f}, loss {el:.3f}, mean {em:.3f}", end="")
    assert ec <= 1 and el <= 1 and em <= 1, (ec, el, em)
    if dz is not None:
        nz = np.sqrt(np.maximum((z.astype(np.float64) ** 2).sum(1), 1e-12))
        ed = (np.abs(f64(dz) - wd) / (8 * (G + 8) * UNIT * gscale / nz[:, None])).max()
        print(f", dz {ed:.3f}", end="")
        assert np.isfinite(f64(dz)).all() and ed <= 1, ed
    print()


@pytest.mark.parametrize("B,G", LOSS_SHAPES, ids=ids(LOSS_SHAPES))
def test_cosine_loss_against_float64(be, B, G):
    ld = (G + 3) // 4 * 4
    z, zd = rows(B, G, ld, 10 * B + G)
    g, gd = rows(B, G, ld, 10 * B + G + 1)
    gscale = 0.7 / B
    got = run_loss(be, zd, gd, B, G, ld, ld, gscale)
    check_loss(got, z, g, B, G, gscale)
    again = run_loss(be, zd, gd, B, G, ld, ld, gscale)
    for a, b in zip(got, again):                         # two runs: the same bits
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["strides", "none", "alias", "unaligned"])
def test_cosine_loss_argument_forms(be, mode):
    B, G = 7, 65
    ldz, ldg, off = (72, 80, 0) if mode == "strides" else (65, 65, 1) if mode == "unaligned" else (68, 68, 0)
    z, zd = rows(B, G, ldz, 3, off)
    g, gd = rows(B, G, ldg, 4, off)
    gscale = 0.25
    got = run_loss(be, zd, gd, B, G, ldz, ldg, gscale, mode if mode in ("none", "alias") else "dz")
    check_loss(got, z, g, B, G, gscale)
    if mode == "alias":                                  # in place: the gradient's bits are those of the separate buffer
        assert torch.equal(got[3], run_loss(be, zd, gd, B, G, ldz, ldg, gscale)[3])


def test_cosine_loss_zero_rows(be):
    """an all-zero target row: cos = 0, loss = 1, dz = 0; an all-zero prediction row: cos = 0 and the below-epsilon gradient
    -gscale gn / 1e-6, finite"""
    B, G, ld = 4, 24, 24
    z, zd = rows(B, G, ld, 5)
    g, gd = rows(B, G, ld, 6)
    g[1] = 0; gd[1] = 0
    z[2] = 0; zd[2] = 0
    gscale = 0.5
    got = run_loss(be, zd, gd, B, G, ld, ld, gscale)
    check_loss(got, z, g, B, G, gscale)
    loss, cos, out, dz = got
    assert float(cos[1]) == 0 and float(loss[1]) == 1 and not dz[1].any()
    assert float(cos[2]) == 0 and float(loss[2]) == 1 and torch.isfinite(dz[2]).all() and dz[2].abs().max() > 1e4
    gn = g[2].astype(np.float64) / np.linalg.norm(g[2].astype(np.float64))
    assert np.abs(dz[2].cpu().double().numpy() + gscale * gn * 1e6).max() <= 8 * (G + 8) * UNIT * gscale * 1e6


def test_cosine_loss_row_bits_do_not_depend_on_the_batch(be):
    B, G, ld = 65, 516, 516
    z, zd = rows(B, G, ld, 7)
    g, gd = rows(B, G, ld, 8)
    all_ = run_loss(be, zd, gd, B, G, ld, ld, 0.125)
    one = run_loss(be, zd[:1].clone(), gd[:1].clone(), 1, G, ld, ld, 0.125)
    last = run_loss(be, zd[64:].clone(), gd[64:].clone(), 1, G, ld, ld, 0.125)
    for k in (0, 1, 3):
        assert torch.equal(all_[k][:1], one[k]) and torch.equal(all_[k][64:], last[k])
    assert float(one[2][0]) == float(one[0][0])


def test_cosine_loss_mean_above_one_workgroup(be):
    """B > 256: several workgroups and the second, one-thread launch that forms the mean in ascending row order"""
    B, G, ld = 300, 20, 20
    z, zd = rows(B, G, ld, 9)
    g, gd = rows(B, G, ld, 10)
    got = run_loss(be, zd, gd, B, G, ld, ld, 1.0 / B)
    check_loss(got, z, g, B, G, 1.0 / B)
    s = np.float32(0)
    for v in got[0].cpu().numpy():
        s = np.float32(s + v)
    assert float(got[2][0]) == float(np.float32(s / np.float32(B)))


def test_cosine_loss_bad_arguments(be):
    from masters_thesis_amd._lib import KernelLibraryError
    z, zd = rows(2, 8, 8, 1)
    loss, t = guarded(2, fill=3.0)
    for args in ((None, 8, zd, 8, None, loss, loss, None, 2, 8, 1.0), (zd, 8, None, 8, None, loss, loss, None, 2, 8, 1.0),
                 (zd, 8, zd, 8, None, None, loss, None, 2, 8, 1.0), (zd, 8, zd, 8, None, loss, None, None, 2, 8, 1.0),
                 (zd, 8, zd, 8, None, loss, loss, None, 0, 8, 1.0), (zd, 8, zd, 8, None, loss, loss, None, 2, 0, 1.0),
                 (zd, 8, zd, 8, None, loss, loss, None, 2, 2049, 1.0), (zd, 4, zd, 8, None, loss, loss, None, 2, 8, 1.0),
                 (zd, 8, zd, 4, None, loss, loss, None, 2, 8, 1.0)):
        with pytest.raises(KernelLibraryError, match="tnt_cosine_loss_f32 failed with code -10"):
            be.cosine_loss(*args)
    torch.cuda.synchronize()
    assert (loss == 3.0).all() and (t == SENT).all()


# ---------------------------------------------------------------------------------------------------- inverse norms
@pytest.mark.parametrize("G", sorted({g for _, g in LOSS_SHAPES}))
def test_row_inv_norm(be, G):
    rws = 9
    for ld, off in (((G + 3) // 4 * 4, 0), (G + 1, 1)):
        x, xd = rows(rws, G, ld, 100 + G, off)
        x[3] = 0; xd[3] = 0
        inv, t = guarded(rws)
        be.row_inv_norm(xd, ld, inv, rws, G)
        torch.cuda.synchronize()
        want = SO.row_inv_norm(x)
        err = np.abs(inv.cpu().double().numpy() - want) / want
        assert err.max() <= (G + 8) * UNIT and float(inv[3]) == 1e6 and (t == SENT).all(), err.max()
        one, _ = guarded(1)
        be.row_inv_norm(xd[5:6].clone(), ld, one, 1, G)
        assert torch.equal(one, inv[5:6])               # a row's bits are its own


# ---------------------------------------------------------------------------------------------------- selection
def select(be, S, qinv, binv, B, M, k, lds):
    Sd = torch.full((B, lds), float("inf"), device="cuda")         # the pad would win every rank if it were read
    Sd[:, :M] = dev(S)
    idx = torch.full((B * k + 64,), -7, dtype=torch.int32, device="cuda")
    sim, t = guarded(B, k)
    be.cosine_topk(Sd, lds, dev(qinv), dev(binv), idx, sim, B, M, k)
    torch.cuda.synchronize()
    assert (idx[B * k:] == -7).all() and (t == SENT).all()
    return idx[:B * k].view(B, k).cpu().numpy(), sim.cpu().numpy()


def check_select(be, S, B, M, k, lds, seed):
    rng = np.random.default_rng(seed)
    qinv = rng.uniform(0.5, 2.0, B).astype(np.float32)
    binv = rng.uniform(0.5, 2.0, M).astype(np.float32)
    S = np.asarray(S, np.float32)
    idx, sim = select(be, S, qinv, binv, B, M, k, lds)
    c = SO.similarity_f32(S, qinv, binv)
    wi, wv = SO.topk(c, k)
    assert np.array_equal(idx, wi), (idx[0], wi[0])
    assert np.array_equal(sim.view(np.uint32), wv.view(np.uint32))


@pytest.mark.parametrize("B,M,k", TOPK_SHAPES, ids=ids(TOPK_SHAPES))
@pytest.mark.parametrize("kind", ["ties", "gauss", "special", "stride"])
def test_cosine_topk_bits(be, B, M, k, kind):
    rng = np.random.default_rng(B * 1000 + M + k)
    lds = (M + 3) // 4 * 4
    if kind == "ties":
        S = rng.integers(-3, 4, (B, M)).astype(np.float32)
        qinv, binv = np.ones(B, np.float32), np.ones(M, np.float32)          # integer similarities: ties everywhere
        idx, sim = select(be, S, qinv, binv, B, M, k, lds)
        wi, wv = SO.topk(S, k)
        assert np.array_equal(idx, wi) and np.array_equal(sim.view(np.uint32), wv.view(np.uint32))
        S[:, ::3] *= -0.0                                                    # signed zeros tie with each other
    else:
        S = rng.standard_normal((B, M)).astype(np.float32)
    if kind == "special":
        r = B - 1
        for j, v in zip(rng.permutation(M)[:5], (np.nan, -np.inf, np.inf, np.nan, -np.inf)):
            S[r, j] = v
    if kind == "stride":
        lds = M + 9                                      # odd stride: the single-float walk
    check_select(be, S, B, M, k, lds, 7 * B + M)


def test_cosine_topk_long_row(be):
    """a row that does not fit in LDS: M = 65 536 + 3, with the winners planted at both ends and across the float4 tail"""
    B, M, k = 2, 65539, 8
    rng = np.random.default_rng(12)
    S = rng.standard_normal((B, M)).astype(np.float32)
    S[0, [0, M - 1, M - 2, 4096, 65536]] = 50.0
    S[1, [M - 1, 17]] = np.nan
    check_select(be, S, B, M, k, M + 1, 13)
    check_select(be, S, B, M, k, (M + 3) // 4 * 4, 13)


def test_cosine_topk_bad_arguments(be):
    B, M = 2, 16
    S, q, b = torch.zeros(B, M, device="cuda"), torch.ones(B, device="cuda"), torch.ones(M, device="cuda")
    idx = torch.full((B * 64,), -7, dtype=torch.int32, device="cuda")
    sim = torch.full((B * 64,), SENT, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda S_, q_, b_, i_, s_, M_, k_, lds=M: be.lib.tnt_cosine_topk_f32(p(S_), lds, p(q_), p(b_), p(i_), p(s_), B, M_, k_, None)
    assert call(S, q, b, idx, sim, M, 17) == -1009                  # k > M
    assert call(S, q, b, idx, sim, 16, 65, lds=128) == -1009         # k > 64
    assert call(S, q, b, idx, sim, M, 0) == -1009
    for args in ((None, q, b, idx, sim), (S, None, b, idx, sim), (S, q, None, idx, sim), (S, q, b, None, sim),
                 (S, q, b, idx, None)):
        assert call(*args, M, 4) == -1001
    assert call(S, q, b, idx, sim, M, 4, lds=8) == -1002
    torch.cuda.synchronize()
    assert (idx == -7).all() and (sim == SENT).all()               # nothing was launched
    assert be.lib.tnt_version() >= 135
