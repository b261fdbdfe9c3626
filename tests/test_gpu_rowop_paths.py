"""Every kernel of csrc/rowops.hip (but stage_batch_kernel: tests/test_gpu_stage_forward.py) on a real MI355X against plain
float64 numpy, at row strides above the width, at the chunk edges of the two-level column reductions and past the grid caps.

Which test launches which kernel -- read against the dispatch in the tnt_* entry points of csrc/rowops.hip:

    kernel                              test                                  arguments that select it
    dropout_kernel                      test_dropout_layouts[scalar-*]        cols = 37, lcol0 = 3 (anything % 4 != 0); and
                                        test_dropout_past_the_grid_cap[scalar]    8255 x 65: 536 575 elements, a second trip
    dropout4_kernel                     test_dropout_layouts[float4-*]        cols = 36, ld, lwidth, lcol0 % 4 == 0, aligned; and
                                        test_dropout_past_the_grid_cap[float4]    8256 x 256: 528 384 quads
    dropout4x2_kernel                   test_dropout2                         tnt_dropout2_f32, also at 8256 x 256
    dropout4_metric_kernel              test_dropout_metric                   tnt_dropout_metric_f32: R in 1 64 65 129, B in 1 3 4 5
    dropout_mask4_kernel                test_dropout_mask4                    3 sites x 2 800 000 elements (past 8192 x 256 groups), 2 x 36
    act_bwd_kernel                      test_act_bwd                          act in leaky relu tanh none, n in 1 255 257 524 289
    col_partial_kernel<0,32>            test_batchnorm (training forward)     C <= 32: rows in 1 2048 2049 8193 8256 ...
    col_partial_kernel<0,64>            test_batchnorm (training forward)     C > 32: C in 33 36 64 65 130
                                        test_sync_batchnorm_pieces            tnt_batchnorm_stats_f32, both forms
                                        test_batchnorm_ill_conditioned        means 1e3, deviation 0.1: the shifted sums
    col_partial_kernel<1,32> / <1,64>   test_batchnorm (backward sums),       dgamma / dbeta given; C <= 32 / C > 32
                                        test_layernorm (backward sums)
    col_partial_kernel<2,32> / <2,64>   test_colsum                           tnt_colsum_f32 above 2048 rows; C <= 32 / C > 32
    bn_finalize_kernel                  test_batchnorm, test_sync_batchnorm_pieces (nrep = 2), test_batchnorm_ill_conditioned
                                                                              rows 4097: second lane trip; 8193 / 8255: empty last chunk
    bn_infer_prep_kernel                test_batchnorm (training = 0)
    bn_apply_kernel                     test_batchnorm                        C or ldy % 4 != 0 (C in 1 5 33 65 130); and
                                        test_batchnorm_alignment_forms_agree      x, y or xhat one float off 16 bytes at C in 32 36 64
    bn_apply4_kernel                    test_batchnorm                        C, ldy % 4 == 0, aligned (C in 4 32 36 64)
    col_finalize_kernel<true>           test_batchnorm, test_layernorm        backward sums; 4097 rows and up: second lane trip
    col_finalize_kernel<false>          test_colsum                           rows > 2048
    bn_dx_kernel                        test_batchnorm                        training with sums, with act_pre, inference with null sums
                                        test_sync_batchnorm_pieces            tnt_batchnorm_dx_f32, n_total = 2 rows
    ln_fwd_kernel, ln_dx_kernel         test_layernorm                        C in 1 5 32 33 64 65 130 (second lane trip above 64)
    sum_kernel, sum2_kernel             test_sums                             n in 1 63 64 1023 1024 1025 2049 5000
    col_sum_direct_kernel               test_colsum                           rows <= 2048
    col_sum_multi_kernel                test_colsum_multi                     tnt_colsum2_f32 / tnt_colsum4_f32, holes at slot 0, 1 and 3
    bias_act_drop_bwd_kernel<true>      test_bias_act_drop_bwd                cols <= 1024: 4, 256, 1024
    bias_act_drop_bwd_kernel<false>     test_bias_act_drop_bwd                cols = 1028
    enc_tail_fwd_kernel<false>          test_enc_tail                         tnt_enc_tail_fwd_f32
    enc_tail_fwd_kernel<true>           test_enc_tail                         tnt_enc_tail_fwd_sk_f32 and _sk_emb_f32 (the Embedding rider)
    enc_tail_bwd_kernel                 test_enc_tail                         tnt_enc_tail_bwd_f32 and _bwd_drop_f32 (the dropout rider)

Protocol (as tests/test_gpu_encoder_paths.py): inputs are rounded to float32 before the float64 reference sees them; pad columns
of strided inputs hold PAD = 1e6; outputs start as NaN inside POISON bands (Guards) and their pad columns must still be NaN
afterwards; every launch runs twice on fresh buffers and must give the same bits.  xhat and dx are dense by contract.  A strided
reference is the dense reference on the live columns (rowop_oracle.py, checked on the host by test_host_rowop_edges.py, which
also pins every size used here to the edge it is named for).

Bounds.  Exact where the arithmetic is: dropout outputs (bit for bit float32(x * float32(1 / (1 - float32(rate))))), LeakyReLU'
and ReLU', every sum of integer data in [-3, 3] (all float32 partial sums are exact in any order) -- with dropout rate 0.5 the
scale is exactly 2, so dbeta / dbias of integer gradients stay exact.  Elsewhere ETOL = 1e-5 of the reference's largest
magnitude, the bound of the embedding and encoder path files; every test prints its worst error / bound ratios (Report).  The
ill-conditioned BatchNorm case derives its bound from a float32 two-pass numpy BatchNorm (see its docstring)."""
import functools

import numpy as np
import pytest
import torch

import rowop_oracle as RO
from oracle import ops as O
from oracle.philox import keep_mask
from test_gpu_encoder_paths import padded, refuse, twice, untouched
from test_gpu_lstm_paths import Guards, r32
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

NAN = float("nan")
ETOL = 1e-5
EPS, MOM = 1e-3, 0.99
SEED, STEP_HOST, STEP_DEV = 1234567890123, 3, 4
STEP = STEP_HOST + STEP_DEV


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def step_dev():
    return torch.tensor([STEP_DEV], dtype=torch.int32, device="cuda")


def gin(gs, name, a):
    """a guarded device copy of an input that the launch updates in place"""
    a = np.asarray(a)
    v = gs.new(name, *a.shape)
    v.copy_(dev(a))
    return v


def off_view(flat, off, *shape):
    """a view of `shape` that starts `off` floats into `flat` (off = 1: one float off 16-byte alignment)"""
    n = int(np.prod(shape))
    v = flat[off:off + n].view(*shape)
    assert v.data_ptr() % 16 == 4 * off
    return v


def pads_nan(out, C):
    """the pad columns of a NaN-initialised output kept their bits"""
    if out.shape[-1] > C:
        pad = out[..., C:]
        assert torch.equal(bits(pad), bits(torch.full_like(pad, NAN))), "a pad column of an output was written"


def ints(rng, *shape):
    """integer-valued data in [-3, 3]: sums of it are exact in float32 in any order"""
    return rng.integers(-3, 4, shape).astype(np.float64)


def with_zeros(rng, *shape):
    """pre-activations of both signs with exact zeros among them"""
    a = r32(rng.standard_normal(shape))
    a.reshape(-1)[::7] = 0.0
    return a


class Report:
    """collects error / bound ratios, prints them, fails on any above 1 (or not finite)"""
    def __init__(self, case):
        self.case, self.rows = case, []

    def near(self, name, got, want, rtol=ETOL):
        got = host(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
        want = np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bound = rtol * (np.abs(want).max() + 1e-30)
        self.rows.append((name, float(np.abs(got - want).max() / bound)))

    def within(self, name, err, bound):
        self.rows.append((name, float(err / bound)))

    def exact(self, name, got, want):
        got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
        want = np.asarray(want)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want.astype(got.dtype), equal_nan=got.dtype.kind == "f"), f"{self.case}: {name} is not exact: {int((got != want).sum())} elements differ"

    def check(self):
        worst = sorted(self.rows, key=lambda r: -r[1] if np.isfinite(r[1]) else -np.inf)
        print(f"\n[{self.case}] worst error / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in worst[:8]))
        bad = [(n, r) for n, r in self.rows if not r <= 1.0]
        assert not bad, (self.case, bad)


@functools.lru_cache(maxsize=8)
def kmask(shape, rate, site, step=STEP):
    """oracle keep mask of stream (SEED, site, step), shared between the tests of one size; never modified"""
    m = keep_mask(shape, rate, SEED, site, step)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------------------------------------ (a) BatchNorm
# (rows, C, pad): every row count of the chunk edges once at a small C, every C once at a small row count; pad 4 / 0 where the
# float4 form is wanted (C % 4 == 0), pad 3 for the scalar form
BN_CASES = [(1, 5, 0), (63, 36, 4), (65, 33, 3), (2048, 4, 0), (2049, 5, 3), (4097, 36, 4), (8193, 5, 0), (8255, 65, 3),
            (8256, 32, 4), (7, 1, 3), (130, 32, 0), (67, 64, 4), (9, 130, 3), (66, 36, 0), (12, 65, 0)]


@functools.lru_cache(maxsize=None)
def bn_data(rows, C):
    rng = np.random.default_rng([rows, C, 1])
    d = dict(x=r32(rng.standard_normal((rows, C)) * 2 + 1.5), gam=r32(1 + 0.3 * rng.standard_normal(C)),
             bet=r32(rng.standard_normal(C)), mm=r32(rng.standard_normal(C)), mv=r32(rng.random(C) + 0.5),
             dy=ints(rng, rows, C), pre=with_zeros(rng, rows, C))
    for v in d.values():
        v.setflags(write=False)
    return d


def bn_forward(be, d, rows, C, ld, training, rate=0.0, site=21, xd=None, offs=(0, 0)):
    """one guarded forward launch pair; returns y [rows][ld], xhat, inv_std, moving mean, moving variance"""
    xd = dev(d["x"]) if xd is None else xd
    gd, bd = dev(d["gam"]), dev(d["bet"])
    sd = step_dev()
    nwork = C * (2 * RO.chunk_count(rows) + 1)

    def launch(gs):
        yf, xf = gs.new("y", rows * ld + 4), gs.new("xhat", rows * C + 4)
        y, xhat = off_view(yf, offs[0], rows, ld), off_view(xf, offs[1], rows, C)
        inv, mm, mv, work = gs.new("inv_std", C), gin(gs, "mov_mean", d["mm"]), gin(gs, "mov_var", d["mv"]), gs.new("work", nwork)
        be.batchnorm_fwd(xd, gd, bd, mm, mv, y, xhat, inv, rows, C, ld, training, EPS, MOM, work,
                         drop=(rate, SEED, site, sd) if rate > 0 else None)
        return yf, xf, inv, mm, mv
    yf, xf, inv, mm, mv = twice(launch)
    for flat, off, n in ((yf, offs[0], rows * ld), (xf, offs[1], rows * C)):
        assert bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + n:]).all()), "written around the view"
    y, xhat = off_view(yf, offs[0], rows, ld), off_view(xf, offs[1], rows, C)
    pads_nan(y, C)
    return y, xhat, inv, mm, mv


@pytest.mark.parametrize("rows,C,pad", BN_CASES)
def test_batchnorm(be, rows, C, pad):
    """tnt_batchnorm_fwd_f32 (training and inference), tnt_batchnorm_fwd_drop_f32, tnt_batchnorm_bwd_f32 and _bwd_act_f32 at
    ldy = lddy = C + pad: y, xhat, inv_std and the moving statistics against float64; the dropped y bit for bit from the undropped
    one and the oracle mask over element r * C + c; backward with sums (dbeta of integer dy exact), with LeakyReLU'(act_pre), sums
    only (dx null), and the inference gradient with null sums"""
    d, ld, rep = bn_data(rows, C), C + pad, Report(f"batchnorm {rows}x{C} ld {C + pad}")
    x, gam, bet, dy, pre = d["x"], d["gam"], d["bet"], d["dy"], d["pre"]
    caches = {}
    for training in (True, False):
        y, xhat, inv, mm, mv = bn_forward(be, d, rows, C, ld, training)
        yo, cache, mmo, mvo = RO.bn_fwd(x, gam, bet, d["mm"], d["mv"], training, EPS, MOM)
        caches[training] = cache
        t = "train" if training else "infer"
        rep.near(f"y/{t}", y[:, :C], yo); rep.near(f"xhat/{t}", xhat, cache[0]); rep.near(f"inv_std/{t}", inv, cache[1])
        rep.near(f"mov_mean/{t}", mm, mmo); rep.near(f"mov_var/{t}", mv, mvo)
        if training:
            rate = 0.3
            yd, xh2, inv2, _, _ = bn_forward(be, d, rows, C, ld, True, rate)
            rep.exact("y/dropout", yd[:, :C], RO.drop32(host(y[:, :C]), kmask((rows, C), rate, 21, STEP_DEV), rate))
            assert torch.equal(bits(xh2), bits(xhat)) and torch.equal(bits(inv2), bits(inv)), "dropout changed xhat / inv_std"
    dyd, gd, pred = dev(padded(dy, ld)), dev(gam), dev(pre)
    nwork = C * (2 * RO.chunk_count(rows) + 1)
    for training in (True, False):
        xh, iv = r32(caches[training][0]), r32(caches[training][1])          # the backward's inputs, rounded like the device's
        xhd, ivd = dev(xh), dev(iv)
        dxo, dgo, dbo = RO.bn_bwd_strided(padded(dy, ld), C, gam, (xh, iv, training))
        t = "train" if training else "infer"
        for act in (False, True):
            def launch(gs):
                dx, dg, db, work = gs.new("dx", rows, C), gs.new("dgamma", C), gs.new("dbeta", C), gs.new("work", nwork)
                be.batchnorm_bwd(dyd, xhd, gd, ivd, dx, dg, db, rows, C, ld, training, work, act_pre=pred if act else None, slope=0.25)
                return dx, dg, db
            dx, dg, db = twice(launch)
            rep.near(f"dx/{t}{'/act' if act else ''}", dx, dxo * np.where(pre > 0, 1.0, 0.25) if act else dxo)
            rep.near(f"dgamma/{t}", dg, dgo)
            rep.exact(f"dbeta/{t}", db, dbo)

        def sums_only(gs):
            dg, db, work = gs.new("dgamma", C), gs.new("dbeta", C), gs.new("work", nwork)
            be.batchnorm_bwd(dyd, xhd, gd, ivd, None, dg, db, rows, C, ld, training, work)
            return dg, db
        dg, db = twice(sums_only)
        rep.near(f"dgamma/{t}/sums only", dg, dgo); rep.exact(f"dbeta/{t}/sums only", db, dbo)
    # inference with null sums: dx = gamma * inv_std * dy needs none
    def infer_dx(gs):
        dx = gs.new("dx", rows, C)
        be.batchnorm_bwd(dyd, xhd, gd, ivd, dx, None, None, rows, C, ld, False, None)
        return (dx,)
    dx, = twice(infer_dx)
    rep.near("dx/infer/null sums", dx, gam * iv * dy)
    rep.check()


@pytest.mark.parametrize("C", [32, 36, 64])
def test_batchnorm_alignment_forms_agree(be, C):
    """C % 4 == 0 at ldy = C + 4: with x, y or xhat one float off 16 bytes the launch takes bn_apply_kernel, aligned it takes
    bn_apply4_kernel; both must give the same bits (with the dropout behind the normalisation on), and match float64"""
    rows, ld, rate = 67, C + 4, 0.3
    d = bn_data(rows, C)
    base = bn_forward(be, d, rows, C, ld, True, rate)
    xf = torch.zeros(rows * C + 4, device="cuda")
    x_off = off_view(xf, 1, rows, C)
    x_off.copy_(dev(d["x"]))
    for name, kw in (("x", dict(xd=x_off)), ("y", dict(offs=(1, 0))), ("xhat", dict(offs=(0, 1)))):
        got = bn_forward(be, d, rows, C, ld, True, rate, **kw)
        for k, (a, b) in enumerate(zip(base, got)):
            assert torch.equal(bits(a[:, :C]) if k == 0 else bits(a), bits(b[:, :C]) if k == 0 else bits(b)), \
                f"{name} misaligned: output {k} differs from the aligned launch"
    yo, cache, _, _ = RO.bn_fwd(d["x"], d["gam"], d["bet"], d["mm"], d["mv"], True, EPS, MOM)
    rep = Report(f"batchnorm alignment C {C}")
    rep.near("y", base[0][:, :C], RO.drop64(yo, kmask((rows, C), rate, 21, STEP_DEV), rate)); rep.near("xhat", base[1], cache[0])
    rep.check()


@pytest.mark.parametrize("rows,C,pad", [(65, 5, 3), (4097, 36, 4), (8193, 33, 0)])
def test_sync_batchnorm_pieces(be, rows, C, pad):
    """tnt_batchnorm_stats_f32 on two replicas -> concatenated partials -> tnt_batchnorm_apply_stats_f32(nrep = 2) on each ->
    tnt_batchnorm_bwd_f32(dx null) sums, added -> tnt_batchnorm_dx_f32(n_total = 2 rows): everything against the float64
    statistics and gradient of the whole 2 rows batch (not against tnt_batchnorm_fwd_f32)"""
    ld, rep = C + pad, Report(f"sync batchnorm 2 x {rows}x{C} ld {C + pad}")
    rng = np.random.default_rng([rows, C, 2])
    x = r32(rng.standard_normal((2 * rows, C)) * 2 + np.where(np.arange(2 * rows)[:, None] < rows, 1.0, -0.5))    # replicas differ
    gam, bet, mm0, mv0 = r32(1 + 0.3 * rng.standard_normal(C)), r32(rng.standard_normal(C)), r32(rng.standard_normal(C)), r32(rng.random(C) + 0.5)
    dy = ints(rng, 2 * rows, C)
    nch = RO.chunk_count(rows)
    assert be.bn_nchunk(rows) == nch
    xs, gd, bd = [dev(x[k * rows:(k + 1) * rows]) for k in range(2)], dev(gam), dev(bet)

    def stats(gs):
        allp = gs.new("part_all", 2, nch * 2 * C)
        for k in range(2):
            be.batchnorm_stats(xs[k], rows, C, allp[k])
        return (allp,)
    allp, = twice(stats)
    yo, (xho, ivo, _), mmo, mvo = RO.bn_fwd(x, gam, bet, mm0, mv0, True, EPS, MOM)
    outs = []
    for k in range(2):
        def apply(gs):
            y, xhat, inv, mean = gs.new("y", rows, ld), gs.new("xhat", rows, C), gs.new("inv_std", C), gs.new("mean_work", C)
            mm, mv = gin(gs, "mov_mean", mm0), gin(gs, "mov_var", mv0)
            be.batchnorm_apply_stats(allp, 2, xs[k], gd, bd, mm, mv, y, xhat, inv, rows, C, ld, EPS, MOM, mean)
            return y, xhat, inv, mm, mv, mean
        y, xhat, inv, mm, mv, mean = twice(apply)
        pads_nan(y, C)
        s = slice(k * rows, (k + 1) * rows)
        rep.near(f"y/{k}", y[:, :C], yo[s]); rep.near(f"xhat/{k}", xhat, xho[s]); rep.near(f"inv_std/{k}", inv, ivo)
        rep.near(f"mean/{k}", mean, x.mean(0)); rep.near(f"mov_mean/{k}", mm, mmo); rep.near(f"mov_var/{k}", mv, mvo)
        outs.append((xhat, inv))
    assert torch.equal(bits(outs[0][1]), bits(outs[1][1])), "the replicas disagree on inv_std"
    xh, iv = r32(xho), r32(ivo)
    dxo, dgo, dbo = O.batchnorm_bwd(dy, gam, (xh, iv, True))
    nwork = C * (2 * nch + 1)
    dyds, xhds, ivd = [dev(padded(dy[k * rows:(k + 1) * rows], ld)) for k in range(2)], [dev(xh[k * rows:(k + 1) * rows]) for k in range(2)], dev(iv)

    def sums(gs):
        loc = gs.new("sums", 2, 2, C)
        for k in range(2):
            be.batchnorm_bwd(dyds[k], xhds[k], gd, ivd, None, loc[k, 0], loc[k, 1], rows, C, ld, True, gs.new("work", nwork))
        return (loc,)
    loc, = twice(sums)
    tot = loc[0] + loc[1]                     # the all-reduce
    rep.near("dgamma", tot[0], dgo); rep.exact("dbeta", tot[1], dbo)
    for k in range(2):
        def dx_(gs):
            dx = gs.new("dx", rows, C)
            be.batchnorm_dx(dyds[k], ld, xhds[k], gd, ivd, tot[0], tot[1], dx, rows, C, 2 * rows)
            return (dx,)
        dx, = twice(dx_)
        rep.near(f"dx/{k}", dx, dxo[k * rows:(k + 1) * rows])
    rep.check()


@pytest.mark.parametrize("rows,C", [(4097, 36), (8193, 5)])
def test_batchnorm_ill_conditioned(be, rows, C):
    """Column means of about 1e3 with a standard deviation of about 0.1: col_partial_kernel<0>'s shifted sums must survive what
    a naive S2 - S1^2 / n does not (there var = 0.01 is the difference of two sums near 1e6 n, each rounded to 6e-8 of itself:
    float32 numpy gives "variances" between -97 and 106 on these inputs, an inv_std error of the order of inv_std itself, 9.5).
    The bound is not fixed beforehand: the test measures the error of a plain float32 two-pass numpy BatchNorm (oracle.ops'
    expressions on the float32 array: mean over the rows, then the mean of the squared deviations) against float64 on the same
    rounded inputs and allows the kernel 4 x that, because its summation order differs (8 or 4 row lanes merged by Chan's
    formula, then up to 128 chunks).  Measured on the CPU for these inputs, float32 two-pass against float64 (max abs):
        4097 x 36: mean 7.6e-3, inv_std 2.4e-2, xhat 8.0e-2     -> bounds 3.0e-2, 9.7e-2, 3.2e-1
        8193 x 5:  mean 4.2e-2, inv_std 6.6e-1, xhat 6.8e-1     -> bounds 1.7e-1, 2.6, 2.7
    numpy adds the rows of a [rows][C] array sequentially, which is why this yardstick is as coarse as it is.  With every column
    summed pairwise the same two passes give mean 9.4e-5 / 1.4e-4, inv_std 4.2e-6 / 9.0e-6, xhat 9.1e-4 / 1.4e-3; the test prints
    the kernel's error against those figures as well, for the record, and asserts nothing on them."""
    rng = np.random.default_rng([rows, C, 3])
    x = r32(1e3 * (1 + 0.2 * rng.random(C)) + 0.1 * rng.standard_normal((rows, C)))
    d = dict(x=x, gam=np.ones(C), bet=np.zeros(C), mm=np.zeros(C), mv=np.ones(C))
    _, (xho, ivo, _), _, _ = RO.bn_fwd(x, d["gam"], d["bet"], d["mm"], d["mv"], True, EPS, MOM)
    m32, v32, xh32 = RO.bn_two_pass_f32(x, EPS)
    iv32 = np.float32(1) / np.sqrt(v32 + np.float32(EPS))
    ref_err = dict(mean=np.abs(m32 - x.mean(0)).max(), inv_std=np.abs(iv32 - ivo).max(), xhat=np.abs(xh32 - xho).max())
    print(f"\n[ill-conditioned {rows}x{C}] float32 two-pass error: " + ", ".join(f"{k} {v:.3e}" for k, v in ref_err.items()))
    assert all(v > 0 for v in ref_err.values())
    mp, vp, xhp = RO.bn_two_pass_f32_pairwise(x, EPS)
    pw_err = dict(mean=np.abs(mp - x.mean(0)).max(), inv_std=np.abs(np.float32(1) / np.sqrt(vp + np.float32(EPS)) - ivo).max(),
                  xhat=np.abs(xhp - xho).max())
    xd, gd, bd = dev(x), dev(d["gam"]), dev(d["bet"])
    nwork = C * (2 * RO.chunk_count(rows) + 1)

    def launch(gs):
        y, xhat, inv, work = gs.new("y", rows, C), gs.new("xhat", rows, C), gs.new("inv_std", C), gs.new("work", nwork)
        mm, mv = gin(gs, "mov_mean", d["mm"]), gin(gs, "mov_var", d["mv"])
        be.batchnorm_fwd(xd, gd, bd, mm, mv, y, xhat, inv, rows, C, C, True, EPS, MOM, work)
        return xhat, inv, work
    xhat, inv, work = twice(launch)
    rep = Report(f"ill-conditioned batchnorm {rows}x{C}")
    rep.within("xhat", np.abs(host(xhat) - xho).max(), 4 * ref_err["xhat"])
    rep.within("inv_std", np.abs(host(inv) - ivo).max(), 4 * ref_err["inv_std"])
    rep.within("mean", np.abs(host(work[:C]) - x.mean(0)).max(), 4 * ref_err["mean"])        # the batch mean: work's first C floats
    got_err = dict(mean=np.abs(host(work[:C]) - x.mean(0)).max(), inv_std=np.abs(host(inv) - ivo).max(), xhat=np.abs(host(xhat) - xho).max())
    print(f"[ill-conditioned {rows}x{C}] kernel error: " + ", ".join(f"{k} {v:.3e}" for k, v in got_err.items())
          + "; pairwise float32 two-pass: " + ", ".join(f"{k} {v:.3e}" for k, v in pw_err.items()))
    rep.check()


# ------------------------------------------------------------------------------------------------ (b) LayerNorm
LN_CASES = [(1, 5, 0), (65, 33, 3), (4097, 32, 4), (8193, 5, 3), (7, 1, 0), (6, 64, 0), (9, 65, 3), (5, 130, 0), (63, 36, 4)]


@pytest.mark.parametrize("rows,C,pad", LN_CASES)
def test_layernorm(be, rows, C, pad):
    """tnt_layernorm_fwd_f32 at ldy = C + pad and tnt_layernorm_bwd_f32 at lddy = C + pad: with sums (col_partial_kernel<1> at the
    chunk edges), dx only (null sums) and sums only (null dx)"""
    ld, rep = C + pad, Report(f"layernorm {rows}x{C} ld {C + pad}")
    rng = np.random.default_rng([rows, C, 4])
    x, gam, bet, dy = r32(rng.standard_normal((rows, C)) * 2 + 1.5), r32(1 + 0.3 * rng.standard_normal(C)), r32(rng.standard_normal(C)), ints(rng, rows, C)
    xd, gd, bd = dev(x), dev(gam), dev(bet)

    def fwd(gs):
        y, xhat, inv = gs.new("y", rows, ld), gs.new("xhat", rows, C), gs.new("inv_std", rows)
        be.layernorm_fwd(xd, gd, bd, y, xhat, inv, rows, C, ld, EPS)
        return y, xhat, inv
    y, xhat, inv = twice(fwd)
    pads_nan(y, C)
    yo, (xho, ivo) = O.layernorm_fwd(x, gam, bet, EPS)
    rep.near("y", y[:, :C], yo); rep.near("xhat", xhat, xho); rep.near("inv_std", inv, ivo[:, 0])
    xh, iv = r32(xho), r32(ivo)
    dxo, dgo, dbo = RO.ln_bwd_strided(padded(dy, ld), C, gam, (xh, iv))
    dyd, xhd, ivd = dev(padded(dy, ld)), dev(xh), dev(iv[:, 0])
    nwork = C * (2 * RO.chunk_count(rows) + 1)
    for want_dx, want_sums in ((True, True), (True, False), (False, True)):
        def bwd(gs):
            dx = gs.new("dx", rows, C) if want_dx else None
            dg, db, work = (gs.new("dgamma", C), gs.new("dbeta", C), gs.new("work", nwork)) if want_sums else (None, None, None)
            be.layernorm_bwd(dyd, xhd, gd, ivd, dx, dg, db, rows, C, ld, work)
            return tuple(t for t in (dx, dg, db) if t is not None)
        out = list(twice(bwd))
        if want_dx:
            rep.near(f"dx{'' if want_sums else '/null sums'}", out.pop(0), dxo)
        if want_sums:
            rep.near(f"dgamma{'' if want_dx else '/null dx'}", out[0], dgo); rep.exact("dbeta", out[1], dbo)
    rep.check()


# ------------------------------------------------------------------------------------------------ (c) sums
@pytest.mark.parametrize("n", [1, 63, 64, 1023, 1024, 1025, 2049, 5000])
def test_sums(be, n):
    """tnt_sum_f32 and tnt_sum2_f32: integer data must give the exact sum (a dropped or doubled element cannot hide), Gaussian
    data the float64 sum within ETOL of its magnitude; the floats behind n hold PAD"""
    rng = np.random.default_rng([n, 5])
    rep = Report(f"sums n {n}")
    for kind in ("int", "gauss"):
        a, b = (ints(rng, n), ints(rng, n)) if kind == "int" else (r32(rng.standard_normal(n)), r32(rng.standard_normal(n) + 0.5))
        ad, bd = dev(np.concatenate([a, [1e6] * 3])), dev(np.concatenate([b, [1e6] * 3]))

        def launch(gs):
            o, o2 = gs.new("out", 1), gs.new("out2", 2)
            be.sum(ad, o, n, 0.5)
            be.sum2(ad, o2[0:1], bd, o2[1:2], n, 0.25)
            return o, o2
        o, o2 = twice(launch)
        want = np.array([0.5 * a.sum(), 0.25 * a.sum(), 0.25 * b.sum()])
        got = np.concatenate([host(o), host(o2)])
        if kind == "int":
            rep.exact("sum, sum2 (integers)", got, want)
        else:
            for k, name in enumerate(("sum", "sum2[0]", "sum2[1]")):
                rep.near(name, got[k:k + 1], want[k:k + 1])
    rep.check()


COLSUM_CASES = [(1, 5, 0), (63, 36, 3), (65, 33, 3), (2048, 5, 3), (2049, 5, 3), (4097, 36, 0), (8193, 5, 0), (8255, 65, 3),
                (8256, 32, 4), (7, 1, 0), (2049, 33, 0), (2050, 64, 3), (2051, 130, 0), (40, 130, 3), (2048, 65, 0)]


@pytest.mark.parametrize("rows,C,pad", COLSUM_CASES)
def test_colsum(be, rows, C, pad):
    """tnt_colsum_f32: the direct kernel up to 2048 rows, partials + finalize above, at ld = C + pad with PAD in the pad columns;
    integer data, so the column sums are exact"""
    rng = np.random.default_rng([rows, C, 6])
    x = ints(rng, rows, C)
    xd = dev(padded(x, C + pad))

    def launch(gs):
        out, work = gs.new("out", C), gs.new("work", C * RO.chunk_count(rows))
        be.colsum(xd, out, rows, C, C + pad, work)
        return (out,)
    out, = twice(launch)
    Report(f"colsum {rows}x{C}").exact("out", out, x.sum(0))


# jobs (rows, C, pad) or None for a hole; the first three are tnt_colsum4_f32, the last two tnt_colsum2_f32
MULTI_CASES = [[None, (1, 32, 0), (2048, 33, 3), (7, 63, 1)], [(2048, 31, 1), None, (1, 1, 0), (65, 64, 0)],
               [(5, 95, 0), (2048, 64, 4), (33, 1, 3), None], [(1, 33, 0), (2048, 63, 1)], [(2048, 32, 0), (1, 31, 2)]]


@pytest.mark.parametrize("jobs", MULTI_CASES, ids=lambda j: "-".join("hole" if k is None else f"{k[0]}x{k[1]}" for k in j))
def test_colsum_multi(be, jobs):
    """tnt_colsum4_f32 with a hole at slot 0, 1 or 3 and tnt_colsum2_f32: a job of 1 row, a job of 2048 rows, C % 32 in 0, 1, 31;
    integer data, exact sums"""
    rng = np.random.default_rng([len(jobs), 7] + [0 if j is None else j[0] + j[1] for j in jobs])
    xs = [None if j is None else ints(rng, j[0], j[1]) for j in jobs]
    xds = [None if j is None else dev(padded(x, j[1] + j[2])) for j, x in zip(jobs, xs)]

    def launch(gs):
        outs = [None if j is None else gs.new(f"out{k}", j[1]) for k, j in enumerate(jobs)]
        args = [(None, None, 0, 0, 0) if j is None else (xd, o, j[0], j[1], j[1] + j[2]) for j, xd, o in zip(jobs, xds, outs)]
        if len(jobs) == 2:
            be.colsum2(*args[0], *args[1])
        else:
            be.colsum_multi(args)
        return tuple(o for o in outs if o is not None)
    outs = twice(launch)
    rep = Report("colsum multi")
    for o, x in zip(outs, [x for x in xs if x is not None]):
        rep.exact(f"job {x.shape}", o, x.sum(0))


# ------------------------------------------------------------------------------------------------ (d) activation backward
@pytest.mark.parametrize("n", [1, 255, 257, 524289])
@pytest.mark.parametrize("act", [O.ACT_LEAKY, O.ACT_RELU, O.ACT_TANH, O.ACT_NONE], ids=["leaky", "relu", "tanh", "none"])
def test_act_bwd(be, act, n):
    """tnt_act_bwd_f32 out of place and in place (dx == dy); pre holds exact zeros and both signs; n = 524 289 is one element past
    the 2048 x 256 grid.  LeakyReLU' (slope 0.25), ReLU' and the pass-through are exact, tanh' is held to ETOL"""
    rng = np.random.default_rng([n, act, 8])
    pre, dy = with_zeros(rng, n), r32(rng.standard_normal(n))
    pd, dyd = dev(pre), dev(dy)
    want = O.act_bwd(pre, dy, act, 0.25)
    rep = Report(f"act_bwd act {act} n {n}")
    for inplace in (False, True):
        def launch(gs):
            dx = gin(gs, "dy", dy) if inplace else gs.new("dx", n)
            be.act_bwd(pd, dx if inplace else dyd, dx, n, act, 0.25)
            return (dx,)
        dx, = twice(launch)
        if act == O.ACT_TANH:
            rep.near(f"dx{'/in place' if inplace else ''}", dx, want)
        else:
            rep.exact(f"dx{'/in place' if inplace else ''}", dx, want)
    rep.check()


# ------------------------------------------------------------------------------------------------ (e) dropout
DB, DT = 6, 5
# layout -> (rows, tmajor_B, rows_per_site, lwidth - lcol0 - cols as a multiple of cols): row-major, time-major, a stack of T
# per-step tensors, and one step's columns of a (B, T * H) logical tensor (lwidth > cols, lcol0 > 0)
LAYOUTS = {"row-major": (DB * DT, 0, 0, 0), "time-major": (DT * DB, DB, 0, 0), "rows-per-site": (DT * DB, 0, DB, 0), "step-of-T": (DB, 0, 0, 2)}
FORMS = {"scalar": (37, 3, 3), "float4": (36, 4, 4)}       # cols, lcol0, pad


def drop_case(layout, form, seedk=0):
    rows, tB, rps, extra = LAYOUTS[layout]
    cols, c0, pad = FORMS[form]
    lwidth = c0 + cols + extra * (cols + (0 if form == "float4" else 1))
    rng = np.random.default_rng([rows, cols, tB, rps, 9 + seedk])
    return rows, cols, pad, tB, rps, lwidth, c0, r32(rng.standard_normal((rows, cols)))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dropout_layouts(be, layout, form):
    """tnt_dropout_f32: every logical layout in the scalar and in the float4 form, at ld = cols and ld > cols, out of place and in
    place; bit-exact against the oracle mask (pad columns of x hold PAD: in place they must keep it)"""
    rows, cols, pad, tB, rps, lwidth, c0, x = drop_case(layout, form)
    rate, site = 0.2, 49
    want = RO.drop32(x, RO.drop_keep(rows, cols, tB, lwidth, c0, rps, rate, SEED, site, STEP), rate)
    sd = step_dev()
    rep = Report(f"dropout {layout} {form}")
    for ld in (cols, cols + pad):
        xp = padded(x, ld)
        xd = dev(xp)
        for inplace in (False, True):
            def launch(gs):
                y = gin(gs, "x", xp) if inplace else gs.new("y", rows, ld)
                be.dropout(y if inplace else xd, y, rows, cols, ld, tB, lwidth, c0, rate, SEED, site, STEP_HOST, sd, rows_per_site=rps)
                return (y,)
            y, = twice(launch)
            rep.exact(f"y ld {ld}{' in place' if inplace else ''}", y, RO.into(xp if inplace else np.full((rows, ld), np.nan), want))
            if not inplace:
                pads_nan(y, cols)


BIG = {"scalar": (8255, 65, 3), "float4": (8256, 256, 0)}


@pytest.mark.parametrize("form", BIG)
def test_dropout_past_the_grid_cap(be, form):
    """one case past the 2048-workgroup cap per kernel: 8255 x 65 elements (dropout_kernel, ld 68), 8256 x 256 / 4 quads
    (dropout4_kernel): the grid-stride loop takes a second trip"""
    rows, cols, pad = BIG[form]
    assert RO.ew_trips(rows * cols // (4 if form == "float4" else 1)) == 2
    rate, site, ld = 0.3, 50, cols + pad
    rng = np.random.default_rng([rows, cols, 10])
    x = r32(rng.standard_normal((rows, cols)))
    xd, sd = dev(padded(x, ld)), step_dev()

    def launch(gs):
        y = gs.new("y", rows, ld)
        be.dropout(xd, y, rows, cols, ld, 0, cols, 0, rate, SEED, site, STEP_HOST, sd)
        return (y,)
    y, = twice(launch)
    pads_nan(y, cols)
    Report(f"dropout {rows}x{cols}").exact("y", y[:, :cols], RO.drop32(x, kmask((rows, cols), rate, site), rate))


@pytest.mark.parametrize("big", [False, True], ids=["small", "8256x256"])
def test_dropout2(be, big):
    """tnt_dropout2_f32 against the product of two oracle masks (not two device launches): mask a a stack of per-step tensors with
    lcol0 > 0, mask b time-major; ld = cols and cols + 4, in place and out of place; 8256 x 256 is past the grid cap"""
    if big:
        rows, cols, B, ca = 8256, 256, 64, 0
    else:
        rows, cols, B, ca = DT * DB, 36, DB, 4
    ra, rb, sa, sb = 0.4, 0.25, 48, 7
    rng = np.random.default_rng([rows, cols, 11])
    x = r32(rng.standard_normal((rows, cols)))
    if big:
        ka, kb = kmask((rows, cols), ra, sa), RO.drop_keep(rows, cols, B, cols, 0, 0, rb, SEED, sb, STEP)
        mask_a = (0, cols, 0, 0, ra, sa)
    else:
        ka, kb = RO.drop_keep(rows, cols, 0, ca + cols, ca, B, ra, SEED, sa, STEP), RO.drop_keep(rows, cols, B, cols, 0, 0, rb, SEED, sb, STEP)
        mask_a = (0, ca + cols, ca, B, ra, sa)
    want = RO.drop32(RO.drop32(x, ka, ra), kb, rb)
    sd = step_dev()
    rep = Report(f"dropout2 {rows}x{cols}")
    for ld in ((cols,) if big else (cols, cols + 4)):
        xp = padded(x, ld)
        xd = dev(xp)
        for inplace in ((False,) if big else (False, True)):
            def launch(gs):
                y = gin(gs, "x", xp) if inplace else gs.new("y", rows, ld)
                be.dropout2(y if inplace else xd, y, rows, cols, ld, mask_a, (B, cols, 0, 0, rb, sb), SEED, STEP_HOST, sd)
                return (y,)
            y, = twice(launch)
            rep.exact(f"y ld {ld}{' in place' if inplace else ''}", y, RO.into(xp if inplace else np.full((rows, ld), np.nan), want))


@pytest.mark.parametrize("R,B,big", [(1, 1, False), (64, 3, False), (65, 4, False), (129, 5, False), (65, 5, True)])
def test_dropout_metric(be, R, B, big):
    """tnt_dropout_metric_f32: the dropout (float4 form, time-major, ld = cols + 4; once at 8256 x 256, past the grid cap) bit-exact,
    and the attention metric's partials of alpha [T][B][R] against float64 at R = 1, 64, 65, 129 (one and a partly filled second
    or third region block) and B = 1, 3, 4, 5 (four row lanes)"""
    T = 2
    rows, cols, tB, ld = (8256, 256, 0, 256) if big else (DT * DB, 36, DB, 40)
    rate, site = 0.3, 50 if big else 51
    rng = np.random.default_rng([R, B, 12])
    x, alpha = r32(rng.standard_normal((rows, cols))), r32(rng.random((T, B, R)) / B)
    keep = kmask((rows, cols), rate, site) if big else RO.drop_keep(rows, cols, tB, cols, 0, 0, rate, SEED, site, STEP)
    xd, ad, sd = dev(padded(x, ld)), dev(alpha), step_dev()
    nc = (R + 63) // 64

    def launch(gs):
        y, part = gs.new("y", rows, ld), gs.new("partial", T * nc)
        be.dropout_metric(xd, y, rows, cols, ld, tB, cols, 0, rate, SEED, site, STEP_HOST, sd, ad, part, T, B, R)
        return y, part
    y, part = twice(launch)
    pads_nan(y, cols)
    rep = Report(f"dropout_metric R {R} B {B}")
    rep.exact("y", y[:, :cols], RO.drop32(x, keep, rate))
    rep.near("partial", part, RO.metric_partials(alpha))
    rep.check()


@pytest.mark.parametrize("n,sites", [(36, 2), (2800000, 3)])
def test_dropout_mask4(be, n, sites):
    """tnt_dropout_mask4_u8: 3 sites of 2 800 000 elements are 2 100 000 groups, past the 8192 x 256 cap, and the site index changes
    inside a thread's strided loop; every byte against the oracle's bits"""
    rate, site0 = 0.35, 60
    sd = step_dev()
    if n > 1000:
        assert RO.ew_trips(n // 4 * sites, RO.MASK4_CAP) == 2
    runs = []
    for _ in range(2):
        buf = torch.full((sites * (n // 4) + 512,), 0xAB, dtype=torch.uint8, device="cuda")
        be.dropout_mask4(buf[256:256 + sites * (n // 4)], n, sites, rate, SEED, site0, STEP_HOST, sd)
        torch.cuda.synchronize()
        assert bool((buf[:256] == 0xAB).all()) and bool((buf[-256:] == 0xAB).all()), "written around the mask buffer"
        runs.append(buf)
    assert torch.equal(runs[0], runs[1])
    got = host(runs[0][256:-256]).reshape(sites, n // 4)
    assert np.array_equal(got, RO.mask4_bytes(n, sites, rate, SEED, site0, STEP))


# ------------------------------------------------------------------------------------------------ (f) fused bias / act / dropout backward
# (rows, cols, pad, act, rate, tmajor_B, rider): narrow at cols 4, 256, 1024 (the last narrow width), wide at 1028 (its last
# 32-column block has one live quad); rows around the wide form's 128 row lanes and the narrow form's 1024; rider = the second
# column-sum job: none, 1 row, or 2048 rows of 33 columns
BAD_CASES = [(1, 4, 0, O.ACT_RELU, 0.5, 0, None), (127, 1028, 4, O.ACT_LEAKY, 0.5, 0, 1), (129, 1028, 0, O.ACT_TANH, 0.0, 3, None),
             (1023, 256, 4, O.ACT_RELU, 0.5, 3, 2048), (1025, 1024, 0, O.ACT_LEAKY, 0.0, 5, None), (2048, 1028, 0, O.ACT_RELU, 0.5, 64, 2048),
             (2048, 4, 4, O.ACT_NONE, 0.5, 0, 1), (129, 256, 0, O.ACT_TANH, 0.5, 0, None), (128, 1028, 4, O.ACT_NONE, 0.5, 0, None)]


@pytest.mark.parametrize("rows,cols,pad,act,rate,tB,rider", BAD_CASES)
def test_bias_act_drop_bwd(be, rows, cols, pad, act, rate, tB, rider):
    """tnt_bias_act_drop_bwd_f32 against float64 built from the oracle mask (lwidth = cols + 4, lcol0 = 4), dy and pre at
    ld = cols + pad; integer dy, so with rate 0 / 0.5 dx and dbias are exact for every activation but tanh; the riding column sums
    of integer data are exact"""
    ld, site = cols + pad, 33
    rng = np.random.default_rng([rows, cols, 13])
    dy, pre = ints(rng, rows, cols), with_zeros(rng, rows, cols)
    keep = RO.drop_keep(rows, cols, tB, cols + 4, 4, 0, rate, SEED, site, STEP_DEV)
    dxo, dbo = RO.bias_act_drop_bwd(padded(dy, ld), padded(pre, ld), cols, keep, rate, act, 0.25)
    dyp = padded(dy, ld)
    dyd, pd, sd = dev(dyp), dev(padded(pre, ld)), step_dev()
    x1 = ints(rng, rider, 33) if rider else None
    x1d = dev(padded(x1, 36)) if rider else None
    rep = Report(f"bias_act_drop_bwd {rows}x{cols} ld {ld}")
    for inplace in (False, True):
        def launch(gs):
            dx = gin(gs, "dy", dyp) if inplace else gs.new("dx", rows, ld)
            db = gs.new("dbias", cols)
            out1 = gs.new("out1", 33) if rider else None
            be.bias_act_drop_bwd(dx if inplace else dyd, pd, dx, db, rows, cols, ld, act, 0.25, tB, cols + 4, 4, rate, SEED, site, sd,
                                 extra=(x1d, out1, rider, 33, 36) if rider else None)
            return (dx, db, out1) if rider else (dx, db)
        out = twice(launch)
        dx, db = out[0], out[1]
        tag = " in place" if inplace else ""
        if inplace:
            rep.exact("pad columns" + tag, dx[:, cols:], dyp[:, cols:])
        else:
            pads_nan(dx, cols)
        if act == O.ACT_TANH:
            rep.near("dx" + tag, dx[:, :cols], dxo); rep.near("dbias" + tag, db, dbo)
        else:
            rep.exact("dx" + tag, dx[:, :cols], dxo); rep.exact("dbias" + tag, db, dbo)
        if rider:
            rep.exact("rider" + tag, out[2], x1.sum(0))
    rep.check()


# ------------------------------------------------------------------------------------------------ (g) encoder tail
# (rows, C, pad, nsplit, training, r_feat, r_lstm): rows around the 32 row groups x 8 rows per thread
ET_CASES = [(1, 4, 0, 1, True, 0.2, 0.3), (31, 32, 4, 3, True, 0.2, 0.0), (33, 36, 0, 1, True, 0.0, 0.5), (255, 96, 4, 3, True, 0.2, 0.3),
            (256, 32, 0, 1, True, 0.5, 0.5), (256, 96, 4, 3, False, 0.2, 0.3), (33, 4, 4, 1, False, 0.0, 0.0), (256, 36, 4, 3, True, 0.3, 0.5)]
ET_SITES = (2, 48, 49, 50)      # feature dropout, LSTM-input dropout, Embedding rider, dropout rider


@pytest.mark.parametrize("rows,C,pad,ns,training,r_feat,r_lstm", ET_CASES)
def test_enc_tail(be, rows, C, pad, ns, training, r_feat, r_lstm):
    """tnt_enc_tail_fwd_f32, _fwd_sk_f32, _fwd_sk_emb_f32 against float64 dropout -> BatchNorm (training / inference) -> dropout,
    and tnt_enc_tail_bwd_f32, _bwd_drop_f32 against its float64 backward with LeakyReLU' and the bias sum, all from oracle masks;
    out and dout at ldo = C + pad; the Embedding rider and the dropout rider work on the rows behind the feature rows of the same
    buffers (exact); dbeta of integer dout is exact where the LSTM-input rate is 0 or 0.5"""
    ld, rep = C + pad, Report(f"enc_tail {rows}x{C} ld {C + pad} ns {ns} {'train' if training else 'infer'}")
    sf, sl, se, sx = ET_SITES
    rng = np.random.default_rng([rows, C, ns, 14])
    part, bias = r32(rng.standard_normal((ns, rows, C)) * 0.5), r32(0.1 * rng.standard_normal(C))
    gam, bet, mm0, mv0 = r32(1 + 0.1 * rng.standard_normal(C)), r32(0.1 * rng.standard_normal(C)), r32(0.1 * rng.standard_normal(C)), r32(1 + 0.1 * rng.random(C))
    pre64 = part.sum(0) + bias
    y64 = np.where(pre64 > 0, pre64, 0.2 * pre64)
    y_in = r32(y64)                                                         # the plain entry point's input
    eB, eT, V = 3, 2, 11
    table, ids = r32(rng.standard_normal((V, C))), rng.integers(0, V, (eB, eT)).astype(np.int32)
    emb_rate = 0.5
    pd, bd, gd, btd, yd, sd = dev(part), dev(bias), dev(gam), dev(bet), dev(y_in), step_dev()
    td, idd = dev(table), dev(ids, torch.int32)
    ke = keep_mask((eB, eT, C), emb_rate, SEED, se, STEP_DEV)
    emb_want = RO.drop32(table[ids], ke, emb_rate).transpose(1, 0, 2).reshape(eT * eB, C)         # rows t * B + b

    def fwd(kind):
        def launch(gs):
            out = gs.new("out", rows + eT * eB, ld)
            xhat, inv, mm, mv = gs.new("xhat", rows, C), gs.new("inv_std", C), gin(gs, "mov_mean", mm0), gin(gs, "mov_var", mv0)
            tail = (gd, btd, mm, mv, out, xhat, inv, rows, C, ld, training, EPS, MOM, r_feat, r_lstm, SEED, sf, sl, sd)
            if kind == "plain":
                be.enc_tail_fwd(yd, *tail)
                return out, xhat, inv, mm, mv
            pre = gs.new("pre", rows, C)
            if kind == "sk":
                be.enc_tail_fwd_sk(pd, ns, bd, pre, 0.2, *tail)
            else:
                be.enc_tail_fwd_sk_emb(pd, ns, bd, pre, 0.2, *tail, td, idd, out[rows:], eB, eT, V, emb_rate, se)
            return out, xhat, inv, mm, mv, pre
        return twice(launch)

    for kind in ("plain", "sk", "sk_emb"):
        res = fwd(kind)
        out, xhat, inv, mm, mv = res[:5]
        oo, xho, ivo, mmo, mvo = RO.enc_tail_fwd(y_in if kind == "plain" else y64, gam, bet, mm0, mv0, training, EPS, MOM, r_feat, r_lstm,
                                                 SEED, sf, sl, STEP_DEV)
        pads_nan(out, C)
        rep.near(f"out/{kind}", out[:rows, :C], oo); rep.near(f"xhat/{kind}", xhat, xho); rep.near(f"inv_std/{kind}", inv, ivo)
        rep.near(f"mov_mean/{kind}", mm, mmo); rep.near(f"mov_var/{kind}", mv, mvo)
        if kind != "plain":
            rep.near(f"pre/{kind}", res[5], pre64)
        if kind == "sk_emb":
            rep.exact("embedding rider", out[rows:, :C], emb_want)
        else:
            assert bool(torch.isnan(out[rows:]).all()), "rows behind the feature rows were written without a rider"

    # backward: the inputs are the float64 forward's, rounded
    _, xho, ivo, _, _ = RO.enc_tail_fwd(y64, gam, bet, mm0, mv0, True, EPS, MOM, r_feat, r_lstm, SEED, sf, sl, STEP_DEV)
    xh, iv, pre = r32(xho), r32(ivo), with_zeros(rng, rows, C)
    dR, dtB = 6, 3                                                           # the dropout rider's rows, time-major (T = 2)
    dbuf = padded(np.concatenate([ints(rng, rows, C), r32(rng.standard_normal((dR, C)))]), ld)
    dpo, dgo, dbo, dbio = RO.enc_tail_bwd(dbuf[:rows], C, xh, gam, iv, pre, 0.2, r_feat, r_lstm, SEED, sf, sl, STEP_DEV)
    drop_rate = 0.5
    kx = RO.drop_keep(dR, C, dtB, C + 4, 4, 0, drop_rate, SEED, sx, STEP_DEV)
    xhd, ivd, prd = dev(xh), dev(iv), dev(pre)
    for ride in (False, True):
        def launch(gs):
            dout = gin(gs, "dout", dbuf)
            dpre, dg, db, dbias = gs.new("dpre", rows, C), gs.new("dgamma", C), gs.new("dbeta", C), gs.new("dbias", C)
            args = (dout, xhd, gd, ivd, prd, dpre, dg, db, dbias, rows, C, ld, r_feat, r_lstm, 0.2, SEED, sf, sl, sd)
            if ride:
                be.enc_tail_bwd_drop(*args, dout[rows:], dR, C, ld, dtB, C + 4, 4, drop_rate, sx)
            else:
                be.enc_tail_bwd(*args)
            return dout, dpre, dg, db, dbias
        dout, dpre, dg, db, dbias = twice(launch)
        t = "/rider" if ride else ""
        rep.near("dpre" + t, dpre, dpo); rep.near("dgamma" + t, dg, dgo); rep.near("dbias" + t, dbias, dbio)
        if r_lstm in (0.0, 0.5):
            rep.exact("dbeta" + t, db, dbo)
        else:
            rep.near("dbeta" + t, db, dbo)
        want = dbuf.copy()
        if ride:
            want[rows:, :C] = RO.drop32(dbuf[rows:, :C], kx, drop_rate)
        rep.exact("dout buffer" + t, dout, want)
    rep.check()


# ------------------------------------------------------------------------------------------------ (h) refusals
def sevens(*shape):
    return torch.full(shape, 7.0, device="cuda")


def test_batchnorm_refusals(be):
    """tnt_batchnorm_bwd_f32 / _bwd_act_f32 refuse the training input gradient without its sums (the kernel would read them
    through null pointers); every BatchNorm entry refuses rows <= 0, C <= 0 and a stride below C; nothing is written.  Each of
    these is a host check in front of the first launch."""
    rows, C = 8, 12
    m, v, w, sd = sevens(rows, C), sevens(C), sevens(C * 3), step_dev()
    dy, xhat, dx, y, pre = sevens(rows, C), sevens(rows, C), sevens(rows, C), sevens(rows, C), sevens(rows, C)
    gam, inv, dg, db, mm, mv, part = sevens(C), sevens(C), sevens(C), sevens(C), sevens(C), sevens(C), sevens(4 * C)
    refuse(lambda: be.batchnorm_bwd(dy, xhat, gam, inv, dx, None, None, rows, C, C, True, None))
    refuse(lambda: be.batchnorm_bwd(dy, xhat, gam, inv, dx, None, None, rows, C, C, True, w, act_pre=pre, slope=0.2))
    refuse(lambda: be.batchnorm_bwd(dy, xhat, gam, inv, dx, dg, None, rows, C, C, True, w))
    for r_, c_, ld_ in ((0, C, C), (-1, C, C), (rows, 0, C), (rows, C, C - 1)):
        refuse(lambda: be.batchnorm_fwd(m, gam, v, mm, mv, y, xhat, inv, r_, c_, ld_, True, EPS, MOM, w))
        refuse(lambda: be.batchnorm_fwd(m, gam, v, mm, mv, y, xhat, inv, r_, c_, ld_, False, EPS, MOM, w, drop=(0.2, 1, 2, sd)))
        refuse(lambda: be.batchnorm_bwd(dy, xhat, gam, inv, dx, dg, db, r_, c_, ld_, True, w))
        refuse(lambda: be.batchnorm_bwd(dy, xhat, gam, inv, dx, dg, db, r_, c_, ld_, False, w, act_pre=pre, slope=0.2))
        refuse(lambda: be.batchnorm_apply_stats(part, 1, m, gam, v, mm, mv, y, xhat, inv, r_, c_, ld_, EPS, MOM, w))
        refuse(lambda: be.batchnorm_dx(dy, ld_, xhat, gam, inv, dg, db, dx, r_, c_, max(r_, 1)))
    refuse(lambda: be.batchnorm_fwd(m, gam, v, mm, mv, y, xhat, inv, rows, C, C, True, EPS, MOM, w, drop=(1.0, 1, 2, sd)))
    refuse(lambda: be.batchnorm_stats(m, 0, C, part))
    untouched(m, v, w, dy, xhat, dx, y, pre, gam, inv, dg, db, mm, mv, part)


def test_layernorm_refusals(be):
    """tnt_layernorm_fwd_f32 / _bwd_f32: rows <= 0, C <= 0, ldy / lddy < C, one sum without the other: an error code, nothing written"""
    rows, C = 8, 12
    x, y, xhat, dx, dy = sevens(rows, C), sevens(rows, C), sevens(rows, C), sevens(rows, C), sevens(rows, C)
    gam, bet, inv, dg, db, w = sevens(C), sevens(C), sevens(rows), sevens(C), sevens(C), sevens(3 * C)
    for r_, c_, ld_ in ((0, C, C), (-3, C, C), (rows, 0, C), (rows, -1, C), (rows, C, C - 1)):
        refuse(lambda: be.layernorm_fwd(x, gam, bet, y, xhat, inv, r_, c_, ld_, EPS))
        refuse(lambda: be.layernorm_bwd(dy, xhat, gam, inv, dx, dg, db, r_, c_, ld_, w))
        refuse(lambda: be.layernorm_bwd(dy, xhat, gam, inv, dx, None, None, r_, c_, ld_, None))
    refuse(lambda: be.layernorm_bwd(dy, xhat, gam, inv, dx, dg, None, rows, C, C, w))
    untouched(x, y, xhat, dx, dy, gam, bet, inv, dg, db, w)


def test_dropout_refusals(be):
    """ld < cols and a rate outside [0, 1) in tnt_dropout_f32, _dropout2_f32, _dropout_metric_f32, _dropout_mask4_u8 and
    tnt_bias_act_drop_bwd_f32: an error code, nothing written"""
    rows, cols = 6, 8
    x, y, alpha, part, db, pre = sevens(rows, cols), sevens(rows, cols), sevens(2, 3, 5), sevens(2), sevens(cols), sevens(rows, cols)
    mk = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    sd = step_dev()
    for ld, rate in ((cols - 4, 0.2), (cols, 1.0), (cols, -0.1), (cols, 1.5), (cols, float("nan"))):
        refuse(lambda: be.dropout(x, y, rows, cols, ld, 0, cols, 0, rate, 1, 2, 3, sd))
        refuse(lambda: be.dropout_metric(x, y, rows, cols, ld, 0, cols, 0, rate, 1, 2, 3, sd, alpha, part, 2, 3, 5))
        refuse(lambda: be.dropout2(x, y, rows, cols, ld, (0, cols, 0, 0, rate, 4), (0, cols, 0, 0, 0.3, 5), 1, 3, sd))
        refuse(lambda: be.bias_act_drop_bwd(x, pre, y, db, rows, cols, ld, O.ACT_RELU, 0.2, 0, cols, 0, rate, 1, 2, sd))
        if ld == cols:
            refuse(lambda: be.dropout_mask4(mk, 64, 1, rate, 1, 2, 3, sd))
    untouched(x, y, alpha, part, db, pre)
    assert bool((mk == 7).all())


def test_enc_tail_refusals(be):
    """the encoder-tail forward and backward entries refuse r_feat / r_lstm outside [0, 1), ldo < C, and a dropout rider with
    drop_ld < drop_cols: an error code, nothing written"""
    rows, C, ns = 5, 8, 2
    part, bias, pre, y = sevens(ns, rows, C), sevens(C), sevens(rows, C), sevens(rows, C)
    gam, bet, mm, mv, inv = sevens(C), sevens(C), sevens(C), sevens(C), sevens(C)
    out, xhat, dpre, dg, db, dbias = sevens(rows + 4, C), sevens(rows, C), sevens(rows, C), sevens(C), sevens(C), sevens(C)
    sd = step_dev()
    for ld, rf, rl in ((C, 1.0, 0.2), (C, 0.2, 1.0), (C, -0.5, 0.2), (C, 0.2, float("nan")), (C - 4, 0.2, 0.2)):
        tail = (gam, bet, mm, mv, out, xhat, inv, rows, C, ld, True, EPS, MOM, rf, rl, 1, 2, 3, sd)
        refuse(lambda: be.enc_tail_fwd(y, *tail))
        refuse(lambda: be.enc_tail_fwd_sk(part, ns, bias, pre, 0.2, *tail))
        refuse(lambda: be.enc_tail_fwd_sk_emb(part, ns, bias, pre, 0.2, *tail, None, None, None, 0, 0, 0, 0.0, 0))
        bwd = (out, xhat, gam, inv, pre, dpre, dg, db, dbias, rows, C, ld, rf, rl, 0.2, 1, 2, 3, sd)
        refuse(lambda: be.enc_tail_bwd(*bwd))
        refuse(lambda: be.enc_tail_bwd_drop(*bwd, out[rows:], 4, C, C, 0, C, 0, 0.2, 4))
    good = (out, xhat, gam, inv, pre, dpre, dg, db, dbias, rows, C, C, 0.2, 0.2, 0.2, 1, 2, 3, sd)
    refuse(lambda: be.enc_tail_bwd_drop(*good, out[rows:], 4, C, C - 4, 0, C, 0, 0.2, 4))
    untouched(part, bias, pre, y, gam, bet, mm, mv, inv, out, xhat, dpre, dg, db, dbias)
