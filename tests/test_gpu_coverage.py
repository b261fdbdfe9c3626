"""tnt_attention_coverage_f32 and the external-gradient rider of the attention backward kernels (tnt_attention_step_bwd_ext_f32,
tnt_lc_seq_bwd_ext_f32) on a real MI355X against float64 numpy (tests/coverage_oracle.py, itself checked against central
differences in tests/test_host_coverage.py).

Coverage kernel: both axes at (T, B, R) = (1, 1, 1), (3, 5, 129), (15, 3, 65), (33, 2, 64) -- one element, a one-row tail
past 128, a tail past 64, the longest caption the step supports -- and once with a step stride larger than B R.
  ext: |got - ref| <= |coef| (n + 2) 2^-24 max(s, 1) per element, n the number of summands: an in-order float32 sum of n
       values in [0, 1] is within (n - 1) 2^-24 s of the exact sum of the float32 inputs, the subtraction and the product add
       one rounding each (of a value <= max(s, 1));
  out: RTOL (tests/test_gpu_ops.py) of the float64 value; bit-identical with ext = NULL; 64 sentinel floats behind ext, out
       and work untouched.

Rider: every STEP_CASES and CHAIN_CASES shape of tests/test_gpu_attention_paths.py (the smallest shapes that select each of
the 4 + 8 backward kernels; its inputs, planted peaks and helpers are imported), both stride layouts -- (ext_ts, ext_bs) =
(0, R), one row per sample, and (R, 0), one row per step -- with a random ext of the size of the step's own dalpha = dctx . F.
Bounds as in that file: RTOL of the tensor's largest magnitude against float64; the chain against the per-step launches
within 3e-5 max(1e-3, |ref|).  The same launches through the _ext entries with ext = NULL are bit-identical to the old
entries.  Each case asserts on the CPU that dropping ext moves dP by at least 100 times the tolerance."""
import types

import numpy as np
import pytest
import torch

import coverage_oracle as CO
from oracle import ops as O
from test_gpu_ops import RTOL, dev
from test_gpu_attention_paths import (STEP_CASES, CHAIN_CASES, Report, guarded, r32, step_inputs, chain_case, chain_dev, SLOPE,
                                      NAN, SENT, RATE_A, RATE_IN, SEED, SITE_A, SITE_I, STEP, STEP_DEV, C_RATE_A, C_RATE_IN,
                                      C_RATE_OUT, C_SEED, C_SITE_A, C_SITE_I, C_SITE_O)

pytestmark = pytest.mark.gpu

LAYOUTS = ("time", "batch")


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


# ---------------------------------------------------------------------------------------------------- coverage kernel
COV_SHAPES = [(1, 1, 1, 0), (3, 5, 129, 0), (15, 3, 65, 0), (33, 2, 64, 0), (3, 5, 129, 5 * 129 + 7)]


@pytest.mark.parametrize("axis", CO.AXES)
@pytest.mark.parametrize("T,B,R,tstride", COV_SHAPES, ids=[f"{t}x{b}x{r}" + ("-strided" if s else "") for t, b, r, s in COV_SHAPES])
def test_coverage_kernel_against_float64(be, T, B, R, tstride, axis):
    from masters_thesis_amd.ops import attention_coverage_work_floats
    rng = np.random.default_rng(1000 * T + 10 * B + R)
    alpha = rng.random((T, B, R)) ** 3                       # in [0, 1], a few regions carry most of the weight
    alpha = r32(alpha / np.maximum(alpha.sum(-1, keepdims=True), 1e-3))
    assert alpha.min() >= 0 and alpha.max() <= 1
    ts = tstride or B * R
    buf = torch.full((T * ts + 3,), NAN, device="cuda")      # the gaps between the steps are never read
    a_dev = torch.as_strided(buf, (T, B, R), (ts, R, 1))
    a_dev.copy_(dev(alpha))
    ax = CO.AXES.index(axis)
    rows, n = (B, T) if axis == "time" else (T, B)
    nwork = attention_coverage_work_floats(T, B, R, ax)
    assert nwork == rows * -(-R // 256)
    coef = np.float32(2 * 0.7 / (rows * R))
    ext, t_ext = guarded(rows, R)
    out, t_out = guarded(1)
    work, t_work = guarded(nwork)
    be.attention_coverage(a_dev, T, B, R, ax, float(coef), ext, out, work, tstride=tstride)
    out2, t_out2 = guarded(1)
    work2, t_work2 = guarded(nwork)
    be.attention_coverage(a_dev, T, B, R, ax, float(coef), None, out2, work2, tstride=tstride)
    ext3, t_ext3 = guarded(rows, R)
    work3, t_work3 = guarded(nwork)
    be.attention_coverage(a_dev, T, B, R, ax, float(coef), ext3, None, work3, tstride=tstride)
    torch.cuda.synchronize()
    s = CO.sums(alpha, axis)
    want = np.float64(coef) * (s - 1.0)
    err = np.abs(ext.cpu().double().numpy() - want)
    bound = abs(np.float64(coef)) * (n + 2) * 2.0 ** -24 * np.maximum(s, 1.0)
    print(f"\n[coverage {T}x{B}x{R} {axis}] worst ext error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), (np.max(err / bound),)
    val = CO.coverage(alpha, axis)
    assert abs(float(out) - val) <= RTOL * val + 1e-30, (float(out), val)
    assert torch.equal(out, out2) and torch.equal(work, work2) and torch.equal(ext, ext3) and torch.equal(work, work3)
    for t in (t_ext, t_out, t_work, t_out2, t_work2, t_ext3, t_work3):
        assert float(t.min()) == SENT == float(t.max())


def test_coverage_kernel_refuses_bad_arguments(be):
    from masters_thesis_amd._lib import KernelLibraryError
    z = lambda *s: torch.zeros(*s, device="cuda")
    al, ext, out, work = z(2, 3, 4), torch.full((12,), SENT, device="cuda"), torch.full((1,), SENT, device="cuda"), z(8)
    for args, kw, code in (((al, 0, 3, 4, 0), {}, -1003), ((al, 2, 3, 4, 2), {}, -1006), ((al, 2, 3, 4, 0), dict(tstride=11), -1002)):
        with pytest.raises(KernelLibraryError, match=rf"code {code}$"):
            be.attention_coverage(*args, 1.0, ext, out, work, **kw)
    with pytest.raises(KernelLibraryError, match=r"code -1010$"):
        be.attention_coverage(al, 2, 3, 4, 0, 1.0, ext, out, None)
    torch.cuda.synchronize()
    assert float(ext.min()) == SENT == float(ext.max()) and float(out) == SENT


# ---------------------------------------------------------------------------------------------------- rider: step kernels
def make_ext(rng, layout, T, B, R, scale):
    """a random rider in the kernel's layout: (flat float32-valued buffer, ext_ts, ext_bs, the [T][B][R] gradient it stands for)"""
    ts, bs = CO.strides(layout, R)
    rows = B if layout == "time" else T
    buf = r32(rng.standard_normal(rows * R) * scale)
    return buf, ts, bs, CO.ext_view(buf, ts, bs, T, B, R)


def step_ref(x, dctx_d, ext, coef=0.0):
    """float64 step backward with dalpha += coef (alpha - 1) + ext: dh, dP, dF, dvb [B][A], dqpre"""
    dctx = O.dropout_bwd(dctx_d, x.keep_in, RATE_IN)
    e = coef * (x.alpha - 1) + ext
    dh, dF, dsum, _, _, _, _ = O.attention_step_bwd(dctx, x.F, x.W2, x.v[:, None], x.cache, SLOPE, dalpha_ext=e)
    dalpha = (dctx[:, None, :] * x.F).sum(axis=2) + e
    de = x.alpha * (dalpha - (x.alpha * dalpha).sum(axis=1, keepdims=True))
    return types.SimpleNamespace(dh=dh, dP=dsum, dF=dF, dvb=(x.sd * de[:, :, None]).sum(axis=1),
                                 dq=O.act_bwd(x.qpre, dsum.sum(axis=1), O.ACT_LEAKY, SLOPE))


def step_bwd_ext_entry(be, ext, ext_bs, dctx_d, F, P, W2, v, qpre, alpha, dP, dF, dvb, dqpre, dh, B, R, D, A, U, slope, rate_attn,
                       rate_in, in_lwidth, seed, site_attn, site_in, step, step_dev, keep4=None, alpha_mse=0.0, fresh=False):
    """tnt_attention_step_bwd_ext_f32 itself, also with ext = NULL (HipBackend.attention_step_bwd takes the old entry then)"""
    from masters_thesis_amd.ops import _p
    be._call(be.lib.tnt_attention_step_bwd_ext_f32, "tnt_attention_step_bwd_ext_f32", _p(dctx_d), _p(F), _p(P), _p(W2), _p(v),
             _p(qpre), _p(alpha), _p(dP), _p(dF), _p(dvb), _p(dqpre), _p(dh), B, R, D, A, U, slope, rate_attn, rate_in, in_lwidth,
             seed, site_attn, site_in, step, _p(step_dev), None, None, None, 0, _p(keep4), float(alpha_mse), int(fresh), _p(ext),
             int(ext_bs), be._s())


@pytest.mark.parametrize("name,B,R,D,A,U,nparts,vs,poff", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_rider_against_float64(be, name, B, R, D, A, U, nparts, vs, poff):
    """tnt_attention_step_bwd_ext_f32 at the shape of every step-backward kernel: per layout one launch onto filled
    accumulators with alpha_mse = 0.37 beside the rider and one fresh launch over NaN accumulators, against float64 at
    RTOL; ext = NULL through the new entry against the old entry, bit for bit; nothing written behind any output."""
    x = step_inputs(name, B, R, D, A, U, vs)
    rep, tails = Report(name), []

    def out(*shape, fill=NAN):
        view, tail = guarded(*shape, fill=fill)
        tails.append(tail)
        return view
    Pbuf = torch.zeros(B * R * A + 4, device="cuda")
    Pd = Pbuf[poff:poff + B * R * A].view(B, R, A)
    Pd.copy_(dev(x.P))
    Fd, W2d, vd, qd, ald, dcd = dev(x.F), dev(x.W2), dev(x.v), dev(x.qpre), dev(x.alpha), dev(x.dctx_d)
    step_dev = torch.tensor([STEP_DEV], dtype=torch.int32, device="cuda")
    tail_args = (B, R, D, A, U, SLOPE, RATE_A, RATE_IN, x.lw, SEED, SITE_A, SITE_I, STEP, step_dev)
    dctx = O.dropout_bwd(x.dctx_d, x.keep_in, RATE_IN)
    scale = np.abs((dctx[:, None, :] * x.F).sum(axis=2)).std()          # the size of the step's own dalpha
    rng = np.random.default_rng(7)
    plain = step_ref(x, x.dctx_d, 0.0)
    acc = tuple(r32(t) for t in (x.dP0 * np.abs(plain.dP).max() / 0.05, x.dF0, x.dvb0))

    def launch(entry, fresh, acc_, **kw):
        fill = NAN if fresh else 0.0
        dP, dF, dvb, dq, dh = out(B, R, A, fill=fill), out(B, R, D, fill=fill), out(B, A + 1, fill=fill), out(B, A), out(B, U)
        if acc_ is not None:
            dP.copy_(dev(acc_[0])); dF.copy_(dev(acc_[1])); dvb.copy_(dev(acc_[2]))
        entry(dcd, Fd, Pd, W2d, vd, qd, ald, dP, dF, dvb, dq, dh, *tail_args, fresh=fresh, **kw)
        return dP, dF, dvb, dq, dh
    for layout in LAYOUTS:
        buf, ts, bs, ext = make_ext(rng, layout, 1, B, R, scale)
        ext_d = dev(buf)
        for tag, fresh, coef in ((f"{layout} acc", False, 0.37), (f"{layout} fresh", True, 0.0)):
            ref, off = step_ref(x, x.dctx_d, ext[0], coef), step_ref(x, x.dctx_d, 0.0, coef)
            moved = np.abs(ref.dP - off.dP).max()
            assert moved >= 100 * RTOL * np.abs(ref.dP).max(), (tag, moved, np.abs(ref.dP).max())    # a dead rider cannot pass
            base = (0.0, 0.0, np.zeros((B, A + 1))) if fresh else acc
            dP, dF, dvb, dq, dh = launch(be.attention_step_bwd, fresh, None if fresh else acc, alpha_mse=coef, ext=ext_d, ext_bs=bs)
            rep.add(tag + " dh", dh, ref.dh); rep.add(tag + " dP", dP, base[0] + ref.dP); rep.add(tag + " dF", dF, base[1] + ref.dF)
            rep.add(tag + " dvb", dvb[:, :A], base[2][:, :A] + ref.dvb); rep.add(tag + " dqpre", dq, ref.dq)
            assert np.abs(dvb[:, A].cpu().double().numpy() - base[2][:, A]).max() < 1e-4
    # ext = NULL through the new entry: the bits of the old entry
    for fresh, coef in ((False, 0.37), (True, 0.0)):
        old = launch(be.attention_step_bwd, fresh, None if fresh else acc, alpha_mse=coef)
        new = launch(lambda *a, **k: step_bwd_ext_entry(be, None, 0, *a, **k), fresh, None if fresh else acc, alpha_mse=coef)
        for a_, b_ in zip(old, new):
            assert torch.equal(a_, b_), (name, fresh)
    torch.cuda.synchronize()
    assert all(float(t.min()) == SENT == float(t.max()) for t in tails)
    assert float(Pbuf[:poff].abs().sum()) == 0 and float(Pbuf[poff + B * R * A:].abs().sum()) == 0
    rep.check()


def test_ext_entries_refuse_bad_strides(be):
    from masters_thesis_amd._lib import KernelLibraryError
    B, R, D, A, U = 2, 16, 8, 8, 32
    z = lambda *s: torch.zeros(*s, device="cuda")
    outs = [torch.full(s, SENT, device="cuda") for s in ((B, R, A), (B, R, D), (B, A + 1), (B, A), (B, U))]
    with pytest.raises(KernelLibraryError, match=r"code -1035$"):
        be.attention_step_bwd(z(B, D), z(B, R, D), z(B, R, A), z(U, A), z(A), z(B, A), z(B, R), *outs, B, R, D, A, U, SLOPE, 0.0, 0.0,
                              D + 20, 7, 16, 48, 0, None, ext=z(B * R), ext_bs=-1)
    torch.cuda.synchronize()
    assert all(float(o.min()) == SENT == float(o.max()) for o in outs)


# ---------------------------------------------------------------------------------------------------- rider: chain kernels
def lc_seq_bwd_ext_entry(be, ext, ts, bs, F, P, W2, v, qpre, alpha, keep4, keep_stride, dP, dF, dvb, dqpre, Ur, Wc, dout, gates, cs,
                         dz, work, T, B, R, D, A, U, slope, rate_attn, rate_in, in_lwidth, seed, site_attn0, site_in0, step_dev,
                         alpha_mse, sync, guard_out, out_drop=None):
    """tnt_lc_seq_bwd_ext_f32 itself, also with ext = NULL (HipBackend.lc_seq_bwd takes the old entries then)"""
    from masters_thesis_amd.ops import _p
    rate_out, site_out0 = out_drop if out_drop is not None else (0.0, 0)
    be._call(be.lib.tnt_lc_seq_bwd_ext_f32, "tnt_lc_seq_bwd_ext_f32", _p(F), _p(P), _p(W2), _p(v), _p(qpre), _p(alpha), _p(keep4),
             int(keep_stride), _p(dP), _p(dF), _p(dvb), _p(dqpre), _p(Ur), _p(Wc), _p(dout), _p(gates), _p(cs), _p(dz), _p(work), T, B,
             R, D, A, U, slope, rate_attn, rate_in, in_lwidth, int(seed), int(site_attn0), int(site_in0), _p(step_dev),
             float(alpha_mse), float(rate_out), int(site_out0), _p(ext), int(ts), int(bs), _p(sync), _p(guard_out), be._s())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [c[0] for c in CHAIN_CASES])
def test_chain_rider_against_float64_and_step_kernels(be, name, layout):
    """tnt_lc_seq_bwd_ext_f32, one case per compiled variant <G4, NP, RB> and stride layout, on the stored values of the
    float64 forward: layout "time" with the stored keep bits and the masked dout, layout "batch" with in-kernel Philox and
    the output Dropout' riding along -- dz, dqpre, dP, dF, dvb[:, :A] against coverage_oracle.chain_bwd_ext at RTOL and
    against the per-step sequence (tnt_lstm_step_bwd_f32 + tnt_attention_step_bwd_ext_f32 on the step's slab); then both
    forms with ext = NULL through the new entry against the old entries, bit for bit.  After every launch the error word
    sync[1024] and the guard are 0."""
    x = chain_case(name)
    T, B, R, D, A, U = x.T, x.B, x.R, x.D, x.A, x.U
    if not be.lstm_seq_supported(B, U):
        pytest.skip("persistent chain kernels not supported on this device")
    d = chain_dev(be, x)
    rep = Report(f"{name} {layout}")
    z = lambda *s: torch.zeros(*s, device="cuda")
    f = lambda *s: torch.full(s, NAN, device="cuda")
    stride = B * R * A // 4
    i_ = x.fwd_in
    st64 = x.stored
    # a rider of standard deviation 0.05, the size of the chains' own dalpha = dctx . F at these shapes (dout ~ 0.1): it moves
    # dP by 350 .. 2200 tolerances (asserted below at 100)
    rng = np.random.default_rng(sum(map(ord, name + layout)))
    scale = 0.05
    buf, ts, bs, ext = make_ext(rng, layout, T, B, R, scale)
    args = (i_["F"], i_["P"], i_["W2"], i_["v"], i_["Wc"], i_["Ur"], st64["qpre"], st64["alpha"], st64["gates"], st64["cs"], x.dout)
    kw = dict(r_attn=C_RATE_A, r_in=C_RATE_IN, masks=x.masks, alpha_mse_coef=x.mse, out_drop=(C_RATE_OUT, x.out_masks))
    ref = CO.chain_bwd_ext(*args, ext, **kw)
    moved = np.abs(ref["dP"] - x.b["dP"]).max()
    assert moved >= 100 * RTOL * np.abs(ref["dP"]).max(), (moved, np.abs(ref["dP"]).max())          # a dead rider cannot pass
    ext_d = dev(buf)
    st = types.SimpleNamespace(**{k: dev(a) for k, a in st64.items()})
    dout_raw = dev(x.dout)
    dout = torch.empty_like(dout_raw)
    be.dropout(dout_raw.view(T * B, U), dout.view(T * B, U), T * B, U, U, 0, U, 0, C_RATE_OUT, C_SEED, C_SITE_O, 0, d.step_dev,
               rows_per_site=B)
    # ---- the per-step sequence with the rider's slab of each step
    r_dz, r_dq, r_dP, r_dF, r_dvb = z(T, B, U, 4), z(T, B, A), z(B, R, A), z(B, R, D), z(B, A + 1)
    dh_att, dc, parts = z(B, U), z(B, U), z(U // 16, B, D)
    use_parts = (U // 16) * D <= 1024
    for i in range(T - 1, -1, -1):
        last = i == T - 1
        be.lstm_step_bwd(None if last else r_dz[i + 1], d.Ur, None, None if last else dh_att, None if last else dc, None,
                         dout[i], None, 0, 0, st.gates[i], st.cs[i + 1], st.cs[i], r_dz[i], None, dc, None, B, U,
                         Wc=d.Wc if use_parts else None, D=D, dctx_part=parts if use_parts else None)
        pk = dict(dctx_part=parts, nparts=U // 16) if use_parts else dict(dz=r_dz[i], Wc=d.Wc)
        be.attention_step_bwd(None, d.F, d.P, d.W2, d.v, st.qpre[i], st.alpha[i], r_dP, r_dF, r_dvb, r_dq[i], dh_att, B, R, D,
                              A, U, SLOPE, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A + i, C_SITE_I + i, 0, d.step_dev,
                              keep4=d.keep[i], alpha_mse=x.mse, fresh=last, ext=ext_d[i * ts:], ext_bs=bs, **pk)
    steps = dict(dz=r_dz, dqpre=r_dq, dP=r_dP, dF=r_dF, dvb=r_dvb[:, :A])
    work = torch.full((be.lc_seq_bwd_work_floats(B, U),), 7.0, device="cuda")
    stored, rider = (True, False) if layout == "time" else (False, True)

    def chain(entry, **kw_):
        g_dz, g_dq, g_dP, g_dF, g_dvb = f(T, B, U, 4), f(T, B, A), f(B, R, A), f(B, R, D), f(B, A + 1)
        entry(d.F, d.P, d.W2, d.v, st.qpre, st.alpha, d.keep if stored else None, stride if stored else 0, g_dP, g_dF, g_dvb, g_dq,
              d.Ur, d.Wc, dout_raw if rider else dout, st.gates, st.cs, g_dz, work, T, B, R, D, A, U, SLOPE, C_RATE_A, C_RATE_IN,
              x.lw, C_SEED, C_SITE_A, C_SITE_I, d.step_dev, x.mse, d.sync, d.guard,
              out_drop=(C_RATE_OUT, C_SITE_O) if rider else None, **kw_)
        torch.cuda.synchronize()
        assert int(d.sync[1024]) == 0 and float(d.guard) == 0.0
        return dict(dz=g_dz, dqpre=g_dq, dP=g_dP, dF=g_dF, dvb=g_dvb)
    got = chain(be.lc_seq_bwd, ext=(ext_d, ts, bs))
    assert got["dvb"][:, A].abs().max().item() < 1e-4
    got["dvb"] = got["dvb"][:, :A]
    for k in got:
        rep.add(k, got[k], ref[k])
        rep.add_abs(f"{k} vs steps", got[k], steps[k], 3e-5 * max(1e-3, steps[k].abs().max().item()))
    # ---- ext = NULL through the new entry: the bits of the old entries (plain and with the Dropout' rider)
    old = chain(be.lc_seq_bwd)
    new = chain(lambda *a, **k: lc_seq_bwd_ext_entry(be, None, 0, 0, *a, **k))
    for k in old:
        assert torch.equal(old[k], new[k]), (name, layout, k)
    rep.check()
