"""tnt_init_state_fwd_f32 / tnt_init_state_bwd_f32 and the initial-cell-state gradient of the persistent backward chain
(tnt_lc_seq_bwd_init_f32) on a real MI355X against float64 numpy on the same float32 inputs (tests/init_state_oracle.py,
tests/lc_chain_oracle.py; both checked against central differences on the CPU).

Shapes (B, R, D, U): (3, 4, 16, 16) the tiny test model; (2, 1, 4, 8) R = 1; (5, 129, 32, 512) the chain tests' width;
(3, 513, 64, 40) D at its limit, R past 512; (4, 37, 5, 24) D no multiple of 4.

Bounds: the componentwise running-error bound, no tuned number.  An n-term float32 sum or dot product is within
g(n) = n u / (1 - n u), u = 2^-24, of exact relative to the sum of the absolute terms, whatever the order.
  fmean    g(R + 2) mean_r|F|                                     (the sum and the division)
  h0, c0   g(R + D + 8) (mean_r|F| |W| + |b|)                      (tanh is 1-Lipschitz; 8 covers tanh and the fused operations)
  g = ds (1 - s^2) is formed in float32 from two terms ds and ds s^2: |g_fl - g| <= g(4) ga with ga = |ds| (1 + s^2), so
  dW       g(B + 4) sum_b |fmean| ga          db   g(B + 4) sum_b ga
  dm       g(2 U + 4) S,  S = gah |Wh|^T + gac |Wc|^T             (2 U terms)
  dF       g(2 U + 8) S / R + u |dF0|                              (the division, the add onto dF0 and its rounding)
Row independence and run-to-run identity are bit comparisons.  Worst observed error / bound on an MI355X: fmean 0.13,
h0 / c0 0.06, dW 0.31, db 0.24, dF 0.53; the chain's outputs 0.005.

Chain: T = 2, U = 512, R = 129, D = A = 32 at B = 5 (one partly filled 8-row block), 9 (two blocks) and 65 (the 16-row
instantiation), dropout 0.2 / 0.3 with the stored keep bits: dc0 and every other output against lc_chain_oracle.chain_bwd at
the tolerance tests/test_gpu_attention_paths.py applies to dz (RTOL of the tensor's largest magnitude); 64 sentinel floats
behind dc0 untouched; and with dc0 = NULL through the new entry every output is the old entry's, bit for bit."""
import types

import numpy as np
import pytest
import torch

import init_state_oracle as IO
import lc_chain_oracle as C
from test_gpu_ops import RTOL, dev
from test_gpu_attention_paths import (Report, guarded, r32, make_v, SLOPE, NAN, SENT, C_RATE_A, C_RATE_IN, C_RATE_OUT, C_SEED,
                                      C_SITE_A, C_SITE_I, C_SITE_O, C_STEP)

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24
SHAPES = [(3, 4, 16, 16), (2, 1, 4, 8), (5, 129, 32, 512), (3, 513, 64, 40), (4, 37, 5, 24)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def gamma(n):
    return n * UNIT / (1.0 - n * UNIT)


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def inputs(B, R, D, U, seed=0):
    rng = np.random.default_rng(1000 * B + 100 * D + R + U + seed)
    n = lambda *s, sc=1.0: r32(rng.standard_normal(s) * sc)
    return types.SimpleNamespace(F=r32(n(B, R, D) + 0.3), Wh=n(D, U, sc=D ** -0.5), bh=n(U, sc=0.1), Wc=n(D, U, sc=D ** -0.5),
                                 bc=n(U, sc=0.1))


def within(got, want, bound, what):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
    worst = float(np.nanmax(ratio)) if np.isfinite(got).all() else float("inf")
    print(f"  {what}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def forward(be, x, B, R, D, U):
    fm, t1 = guarded(B, D)
    h0, t2 = guarded(B, U)
    c0, t3 = guarded(B, U)
    be.init_state_fwd(dev(x.F), dev(x.Wh), dev(x.bh), dev(x.Wc), dev(x.bc), fm, h0, c0, B, R, D, U)
    torch.cuda.synchronize()
    assert all(float(t.min()) == SENT == float(t.max()) for t in (t1, t2, t3))
    return fm, h0, c0


@pytest.mark.parametrize("B,R,D,U", SHAPES, ids=IDS)
def test_forward_against_float64(be, B, R, D, U):
    x = inputs(B, R, D, U)
    h_ref, c_ref, m_ref = IO.init_fwd(x.F, x.Wh, x.bh, x.Wc, x.bc)
    fm, h0, c0 = forward(be, x, B, R, D, U)
    print()
    mabs = np.abs(x.F).mean(axis=1)
    within(fm, m_ref, gamma(R + 2) * mabs, "fmean")
    within(h0, h_ref, gamma(R + D + 8) * (mabs @ np.abs(x.Wh) + np.abs(x.bh)), "h0")
    within(c0, c_ref, gamma(R + D + 8) * (mabs @ np.abs(x.Wc) + np.abs(x.bc)), "c0")
    assert np.abs(h_ref).max() > 0.3 and np.abs(h_ref - c_ref).max() > 0.1          # neither trivial nor the same layer twice
    # fmean is optional (inference): the same states without it
    h2, c2 = torch.full((B, U), NAN, device="cuda"), torch.full((B, U), NAN, device="cuda")
    be.init_state_fwd(dev(x.F), dev(x.Wh), dev(x.bh), dev(x.Wc), dev(x.bc), None, h2, c2, B, R, D, U)
    assert torch.equal(h2, h0) and torch.equal(c2, c0)


def backward_inputs(B, R, D, U):
    x = inputs(B, R, D, U)
    rng = np.random.default_rng(7 + B + R + D + U)
    n = lambda *s, sc=1.0: r32(rng.standard_normal(s) * sc)
    h0, c0, m = IO.init_fwd(x.F, x.Wh, x.bh, x.Wc, x.bc)
    x.h0, x.c0, x.m = r32(h0), r32(c0), r32(m)
    x.dh0, x.dc0, x.dF0 = n(B, U, sc=0.1), n(B, U, sc=0.1), n(B, R, D, sc=0.05)
    return x


def backward(be, x, B, R, D, U, with_dF=True, with_dW=True):
    outs = [guarded(D, U), guarded(U), guarded(D, U), guarded(U)]
    dF, tF = guarded(B, R, D)
    dF.copy_(dev(x.dF0))
    grads = [o[0] for o in outs] if with_dW else [None] * 4
    be.init_state_bwd(dev(x.dh0), dev(x.dc0), dev(x.h0), dev(x.c0), dev(x.m), dev(x.Wh), dev(x.Wc), *grads,
                      dF if with_dF else None, B, R, D, U)
    torch.cuda.synchronize()
    assert all(float(t.min()) == SENT == float(t.max()) for _, t in outs) and float(tF.min()) == SENT == float(tF.max())
    return [o[0] for o in outs], dF


@pytest.mark.parametrize("B,R,D,U", SHAPES, ids=IDS)
def test_backward_against_float64(be, B, R, D, U):
    x = backward_inputs(B, R, D, U)
    ref = IO.init_bwd(x.dh0, x.dc0, x.h0, x.c0, x.m, x.Wh, x.Wc, R)
    (dWh, dbh, dWc, dbc), dF = backward(be, x, B, R, D, U)
    gah, gac = np.abs(x.dh0) * (1 + x.h0 ** 2), np.abs(x.dc0) * (1 + x.c0 ** 2)
    print()
    within(dWh, ref["dWh"], gamma(B + 4) * (np.abs(x.m).T @ gah), "dWh")
    within(dWc, ref["dWc"], gamma(B + 4) * (np.abs(x.m).T @ gac), "dWc")
    within(dbh, ref["dbh"], gamma(B + 4) * gah.sum(0), "dbh")
    within(dbc, ref["dbc"], gamma(B + 4) * gac.sum(0), "dbc")
    S = gah @ np.abs(x.Wh).T + gac @ np.abs(x.Wc).T
    want = x.dF0 + ref["dF_row"][:, None, :]
    within(dF, want, gamma(2 * U + 8) * S[:, None, :] / R + UNIT * np.abs(x.dF0), "dF")
    # the branch is far above the bound it is checked in: a launch that added nothing would not pass
    assert np.abs(ref["dF_row"]).max() >= 100 * (gamma(2 * U + 8) * S / R).max()
    # the nullable halves: parameter gradients alone leave dF as it was; dF alone writes no parameter gradient
    (w2, b2, w3, b3), dF2 = backward(be, x, B, R, D, U, with_dF=False)
    assert torch.equal(w2, dWh) and torch.equal(b2, dbh) and torch.equal(w3, dWc) and torch.equal(b3, dbc)
    assert torch.equal(dF2, dev(x.dF0))
    nans, dF3 = backward(be, x, B, R, D, U, with_dW=False)
    assert torch.equal(dF3, dF) and all(bool(torch.isnan(t).all()) for t in nans)


@pytest.mark.parametrize("B,R,D,U", SHAPES, ids=IDS)
def test_row_independence_and_run_to_run_bits(be, B, R, D, U):
    """the same scan at another row and in another batch size gives the same bits (beam search repeats rows, score_captions
    gathers them); two runs of either launch give the same bits"""
    x = inputs(B, R, D, U)
    fm, h0, c0 = forward(be, x, B, R, D, U)
    fm2, h02, c02 = forward(be, x, B, R, D, U)
    assert torch.equal(fm, fm2) and torch.equal(h0, h02) and torch.equal(c0, c02)
    B2 = 2 * B + 3
    perm = np.random.default_rng(3).integers(0, B, B2)
    perm[-1] = 0
    y = types.SimpleNamespace(**vars(x))
    y.F = x.F[perm]
    fmp, hp, cp = forward(be, y, B2, R, D, U)
    idx = torch.as_tensor(perm, device="cuda")
    assert torch.equal(fmp, fm[idx]) and torch.equal(hp, h0[idx]) and torch.equal(cp, c0[idx])
    xb = backward_inputs(B, R, D, U)
    a, dFa = backward(be, xb, B, R, D, U)
    b, dFb = backward(be, xb, B, R, D, U)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(dFa, dFb)


def test_entries_refuse_what_they_cannot_run(be):
    from masters_thesis_amd._lib import KernelLibraryError
    z = lambda *s: torch.zeros(*s, device="cuda")
    outs = [torch.full(s, SENT, device="cuda") for s in ((2, 65), (2, 8), (2, 8))]
    for B, R, D, U in ((2, 3, 65, 8), (2, 3, 0, 8), (0, 3, 4, 8), (2, 0, 4, 8), (2, 3, 4, 0)):
        with pytest.raises(KernelLibraryError, match="tnt_init_state_fwd_f32"):
            be.init_state_fwd(z(2, 3, 65), z(65, 8), z(8), z(65, 8), z(8), *outs, B, R, D, U)
        with pytest.raises(KernelLibraryError, match="tnt_init_state_bwd_f32"):
            be.init_state_bwd(z(2, 8), z(2, 8), z(2, 8), z(2, 8), z(2, 65), z(65, 8), z(65, 8), outs[0], outs[1], outs[0], outs[1],
                              None, B, R, D, U)
    with pytest.raises(KernelLibraryError, match="tnt_init_state_bwd_f32"):     # the parameter gradients: all four or none
        be.init_state_bwd(z(2, 8), z(2, 8), z(2, 8), z(2, 8), z(2, 4), z(4, 8), z(4, 8), outs[0], None, outs[0], outs[1], None,
                          2, 3, 4, 8)
    torch.cuda.synchronize()
    assert all(float(o.min()) == SENT == float(o.max()) for o in outs)
    assert be.lib.tnt_version() >= 134


# ---------------------------------------------------------------------------------------------------- the chain's dc0
def lc_seq_bwd_init_entry(be, dc0, F, P, W2, v, qpre, alpha, keep4, keep_stride, dP, dF, dvb, dqpre, Ur, Wc, dout, gates, cs, dz,
                          work, T, B, R, D, A, U, slope, rate_attn, rate_in, in_lwidth, seed, site_attn0, site_in0, step_dev,
                          alpha_mse, sync, guard_out, out_drop=None):
    """tnt_lc_seq_bwd_init_f32 itself, also with dc0 = NULL (HipBackend.lc_seq_bwd takes the old entries then)"""
    from masters_thesis_amd.ops import _p
    rate_out, site_out0 = out_drop if out_drop is not None else (0.0, 0)
    be._call(be.lib.tnt_lc_seq_bwd_init_f32, "tnt_lc_seq_bwd_init_f32", _p(F), _p(P), _p(W2), _p(v), _p(qpre), _p(alpha), _p(keep4),
             int(keep_stride), _p(dP), _p(dF), _p(dvb), _p(dqpre), _p(Ur), _p(Wc), _p(dout), _p(gates), _p(cs), _p(dz), _p(work), T,
             B, R, D, A, U, slope, rate_attn, rate_in, in_lwidth, int(seed), int(site_attn0), int(site_in0), _p(step_dev),
             float(alpha_mse), float(rate_out), int(site_out0), None, 0, 0, _p(dc0), _p(sync), _p(guard_out), be._s())


@pytest.mark.parametrize("B", [5, 9, 65])
def test_chain_initial_cell_gradient_against_float64(be, B):
    T, R, D, A, U = 2, 129, 32, 32, 512
    if not be.lstm_seq_supported(B, U):
        pytest.skip("persistent chain kernels not supported on this device")
    rng = np.random.default_rng(4000 + B)
    n = lambda *s, sc=1.0: r32(rng.standard_normal(s) * sc)
    lw = D + 20
    i = dict(F=n(B, R, D), P=n(B, R, A), W2=n(U, A, sc=U ** -0.5), b2=n(A, sc=0.1), v=make_v(rng, A, 0.6), bv=n(1),
             xz=n(T, B, U, 4, sc=0.5), Wc=n(D, U, 4, sc=D ** -0.5), Ur=n(U, U, 4, sc=U ** -0.5), zb=n(U, 4, sc=0.1),
             h0=n(B, U, sc=0.5), c0=n(B, U, sc=0.5))
    masks = C.chain_masks(T, B, R, D, A, C_RATE_A, C_RATE_IN, lw, C_SEED, C_SITE_A, C_SITE_I, C_STEP)
    omasks = C.out_masks(T, B, U, C_RATE_OUT, C_SEED, C_SITE_O, C_STEP)
    f = C.chain_fwd(**i, r_attn=C_RATE_A, r_in=C_RATE_IN, masks=masks)
    st64 = {k: r32(f[k]) for k in ("qpre", "alpha", "gates", "cs")}
    dout64 = n(T, B, U, sc=0.1)
    ref = C.chain_bwd(i["F"], i["P"], i["W2"], i["v"], i["Wc"], i["Ur"], st64["qpre"], st64["alpha"], st64["gates"], st64["cs"],
                      dout64, r_attn=C_RATE_A, r_in=C_RATE_IN, masks=masks, out_drop=(C_RATE_OUT, omasks))
    assert np.abs(ref["dc0"]).max() > 1e-3
    d = types.SimpleNamespace(**{k: dev(a) for k, a in i.items()})
    st = types.SimpleNamespace(**{k: dev(a) for k, a in st64.items()})
    step_dev = torch.tensor([C_STEP], dtype=torch.int32, device="cuda")
    keep = torch.zeros(T, B * R * A // 4, dtype=torch.uint8, device="cuda")
    be.dropout_mask4(keep, B * R * A, T, C_RATE_A, C_SEED, C_SITE_A, 0, step_dev)
    sync, guard = torch.zeros(1025, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    dout = dev(dout64)
    work = torch.full((be.lc_seq_bwd_work_floats(B, U),), 7.0, device="cuda")
    stride = B * R * A // 4
    nanf = lambda *s: torch.full(s, NAN, device="cuda")

    def chain(entry, **kw):
        g = dict(dz=nanf(T, B, U, 4), dqpre=nanf(T, B, A), dP=nanf(B, R, A), dF=nanf(B, R, D), dvb=nanf(B, A + 1))
        entry(d.F, d.P, d.W2, d.v, st.qpre, st.alpha, keep, stride, g["dP"], g["dF"], g["dvb"], g["dqpre"], d.Ur, d.Wc, dout,
              st.gates, st.cs, g["dz"], work, T, B, R, D, A, U, SLOPE, C_RATE_A, C_RATE_IN, lw, C_SEED, C_SITE_A, C_SITE_I,
              step_dev, 0.0, sync, guard, out_drop=(C_RATE_OUT, C_SITE_O), **kw)
        torch.cuda.synchronize()
        assert int(sync[1024]) == 0 and float(guard) == 0.0
        return g
    dc0, tail = guarded(B, U)
    got = chain(be.lc_seq_bwd, dc0=dc0)
    assert float(tail.min()) == SENT == float(tail.max())
    rep = Report(f"dc0 B={B}")
    rep.add("dc0", dc0, ref["dc0"])
    for k in ("dz", "dqpre", "dP", "dF"):
        rep.add(k, got[k], ref[k])
    rep.add("dvb", got["dvb"][:, :A], ref["dvb"])
    # dc0 = NULL through the new entry: the bits of the old entry; and the store changes no other output
    old = chain(be.lc_seq_bwd)
    new = chain(lambda *a, **k: lc_seq_bwd_init_entry(be, None, *a, **k))
    for k in old:
        assert torch.equal(old[k], new[k]), k
        assert torch.equal(old[k], got[k]), k
    rep.check()
