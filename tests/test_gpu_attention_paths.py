"""Every kernel of csrc/attention.hip's recurrent part on a real MI355X against float64 numpy: the 8 attention step
kernels in every backward mode (oracle/ops.py) and the 16 persistent chain kernels over several steps
(tests/lc_chain_oracle.py, itself checked against finite differences in tests/test_host_lc_chain_oracle.py).

Which case launches which kernel -- read against the dispatch at tnt_attention_step_{fwd,bwd}_f32 (wide_ok: A % 4 == D % 4
== 0 and R <= 6 * 1024 / G4 with G4 = 8 for A, D <= 32, else 16; every wide pointer 16-byte aligned; narrow<32> for
A, D <= 32, else narrow<64>) and at tnt_lc_seq_{fwd,bwd}_drop_f32 (G4 as above, NP = 3 for ceil(R / (1024 / G4)) <= 3,
else 6, RB = 8 for B <= 64, else 16).  Every case runs the forward and the backward kernel of its row.

    step kernel (fwd and bwd)        STEP_CASES id        (B, R, D, A)          row passes / why
    attention_*_wide_kernel<8>       wide8-4p             (2, 385, 32, 32)      4, the last holds one row
                                     wide8-6p             (2, 768, 8, 12)       6, the R bound; A != D
    attention_*_wide_kernel<16>      wide16-2p            (2, 65, 36, 8)        2, D alone selects G4 = 16; one-row tail
                                     wide16-6p-tail       (2, 321, 64, 64)      6, one-row tail
                                     wide16-6p-bound      (1, 384, 64, 64)      6, the R bound
    attention_*_kernel<32>           narrow32-769         (2, 769, 32, 32)      first R past wide<8>
                                     narrow32-maxr        (1, 2048, 4, 4)       MAXR
                                     narrow-fallback      (2, 100, 32, 32)      wide-eligible, P one float off alignment
    attention_*_kernel<64>           narrow64-odd         (3, 40, 33, 50)       A, D no multiples of 4
                                     narrow64-385         (2, 385, 36, 40)      first R past wide<16>
                                     narrow64-maxr        (1, 2048, 64, 64)     MAXR at full width

    chain kernel (fwd and bwd)       CHAIN_CASES id       (T, B, R, D, A)
    lc_seq_*_kernel<8, 3, 8>         8-3-8                (3, 5, 129, 32, 32)   two passes, one-row tail
    lc_seq_*_kernel<8, 3, 16>        8-3-16               (3, 65, 100, 32, 32)  five row blocks, the last with one sample
    lc_seq_*_kernel<8, 6, 8>         8-6-8                (3, 5, 385, 32, 32)
    lc_seq_*_kernel<8, 6, 16>        8-6-16               (4, 80, 512, 16, 32)  the R bound; two interior steps
    lc_seq_*_kernel<16, 3, 8>        16-3-8               (3, 9, 65, 36, 8)
    lc_seq_*_kernel<16, 3, 16>       16-3-16              (3, 65, 192, 64, 64)  the NP = 3 bound
    lc_seq_*_kernel<16, 6, 8>        16-6-8               (3, 8, 193, 48, 40)   first R that needs NP = 6
    lc_seq_*_kernel<16, 6, 16>       16-6-16              (3, 128, 384, 64, 64) every bound at once

Inputs: every operand is rounded to float32 before the reference sees it.  In every sample one region holds the softmax
peak -- the LAST region for odd samples, region 0 for even ones -- planted by adding a multiple of v to that row of P (the
multiple that makes the reference's attention weight of the row 0.75, in a chain's first step 0.9; asserted > 0.5 on the
CPU), so the first and the last row of a pass carry weight and a row dropped or read past the end moves every output by far more
than the tolerance, while the other regions still share the rest of the weight.  In the later steps of a chain the same
row meets another dropout mask and another query; its weight then scatters around that value (asserted > 0.5 on
average: a saturated row would hold it in every step, but at weight 1.0, which hides every other region).

Tolerance against float64: RTOL = 1e-4 of the reference tensor's largest magnitude, the bound of tests/test_gpu_ops.py for
these kernels, for every tensor of every case (no exception was needed; each test prints its worst error / bound
ratios).  Chain against the per-step launches: 2e-5 max(1, |ref|) forward, 3e-5 max(1e-3, |ref|) backward, the bounds of
test_lc_seq_{fwd,bwd}_equals_step_kernels."""
import functools
import types

import numpy as np
import pytest
import torch

import lc_chain_oracle as C
from oracle import ops as O
from oracle.philox import keep_mask
from test_gpu_ops import RTOL, dev

pytestmark = pytest.mark.gpu

SLOPE = 0.2
NAN = float("nan")
SENT = 1234.5                   # behind every guarded output: no kernel may write there


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def r32(a):
    """round to float32, keep float64: the reference and the device start from the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


def ratio(got, want, rtol=RTOL):
    """max |got - want| over the bound rtol * max |want| (NaN in got = inf)"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max()
    return float("inf") if not np.isfinite(err) else err / (rtol * (np.abs(want).max() + 1e-30))


class Report:
    """collects error / bound ratios, prints them, fails on the first above 1"""
    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, name, got, want, rtol=RTOL):
        self.rows.append((name, ratio(got, want, rtol)))

    def add_abs(self, name, got, ref, bound):
        d = (got - ref).abs().max().item()
        self.rows.append((name, d / bound if np.isfinite(d) else float("inf")))

    def check(self):
        worst = sorted(self.rows, key=lambda r: -r[1])
        print(f"\n[{self.case}] worst error / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in worst[:6]))
        bad = [(n, r) for n, r in self.rows if not r <= 1.0]
        assert not bad, (self.case, bad)


def guarded(*shape, fill=NAN):
    """an output buffer with 64 floats of SENT behind it; returns (view, tail)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 64,), SENT, device="cuda")
    flat[:n] = fill
    return flat[:n].view(*shape), flat[n:]


def keep_scale(keep, rate, shape):
    if keep is None or rate <= 0:
        return np.ones(shape)
    return keep / (1.0 - np.float64(np.float32(rate)))


def plant_peaks(P, q, v, bv, keep, rate, target=0.75):
    """Adds to row r_b of P[b] (r_b = R-1 for odd b, 0 for even b) the multiple of v that gives the row the attention
    weight ``target`` for the query q [B][A] and this keep mask (bisection on the float64 score, which grows with the
    multiple: every term v_a tanh(P + m v_a + q_a) does).  Returns the new P (rounded to float32) and the rows."""
    B, R, A = P.shape
    k = keep_scale(keep, rate, P.shape)
    e = (np.tanh(P + q[:, None, :]) * k) @ v + bv[0]
    P, rows = P.copy(), []
    for b in range(B):
        r = R - 1 if b % 2 else 0
        others = np.delete(e[b], r)
        want = np.log(target / (1 - target)) + others.max() + np.log(np.exp(others - others.max()).sum())
        score = lambda m: (np.tanh(P[b, r] + m * v + q[b]) * k[b, r]) @ v + bv[0]
        lo, hi = 0.0, 20.0 / np.abs(v).max()                 # |P| stays far inside the kernels' e^{2P} range (|P| <= 40)
        assert score(hi) > want, ("v too small to plant a peak", b, score(hi), want)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if score(mid) < want else (lo, mid)
        P[b, r] = r32(P[b, r] + hi * v)
        rows.append(r)
    return P, rows


def make_v(rng, A, vs):
    """|v_a| in vs * [0.5, 1.5): no component so small that the planted row needs a huge multiple"""
    return r32(rng.choice([-1.0, 1.0], A) * (0.5 + rng.random(A)) * vs)


# ----------------------------------------------------------------------------------------------- step kernels
#            id                 B  R     D   A   U   nparts  v scale  P offset (floats)
STEP_CASES = [("wide8-4p",        2, 385,  32, 32, 32, 32,     0.6,     0),
              ("wide8-6p",        2, 768,  8,  12, 48, 7,      1.5,     0),
              ("wide16-2p",       2, 65,   36, 8,  32, 3,      1.5,     0),
              ("wide16-6p-tail",  2, 321,  64, 64, 48, 16,     0.4,     0),
              ("wide16-6p-bound", 1, 384,  64, 64, 32, 5,      0.4,     0),
              ("narrow32-769",    2, 769,  32, 32, 32, 5,      0.6,     0),
              ("narrow32-maxr",   1, 2048, 4,  4,  48, 9,      4.0,     0),
              ("narrow64-odd",    3, 40,   33, 50, 32, 4,      0.4,     0),
              ("narrow64-385",    2, 385,  36, 40, 48, 3,      0.5,     0),
              ("narrow64-maxr",   1, 2048, 64, 64, 32, 16,     0.4,     0),
              ("narrow-fallback", 2, 100,  32, 32, 32, 5,      0.6,     1)]
RATE_A, RATE_IN, SEED, SITE_A, SITE_I, STEP, STEP_DEV = 0.2, 0.25, 77, 16 + 3, 48 + 3, 3, 2


def step_inputs(name, B, R, D, A, U, vs):
    rng = np.random.default_rng(sum(map(ord, name)))
    n = lambda *s, sc=1.0: r32(rng.standard_normal(s) * sc)
    x = types.SimpleNamespace(F=n(B, R, D), h=n(B, U, sc=0.5), W2=n(U, A, sc=U ** -0.5), b2=n(A, sc=0.1),
                              v=make_v(rng, A, vs), bv=n(1), P=n(B, R, A), lw=D + 20)
    x.keep = keep_mask((B, R, A), RATE_A, SEED, SITE_A, STEP + STEP_DEV)
    x.keep_in = keep_mask((B, x.lw), RATE_IN, SEED, SITE_I, STEP + STEP_DEV)[:, :D]
    q = O.act_fwd(x.h @ x.W2 + x.b2, O.ACT_LEAKY, SLOPE)
    x.P, x.rows = plant_peaks(x.P, q, x.v, x.bv, x.keep, RATE_A)
    (x.ctx, x.alpha, x.sd), x.cache = O.attention_step_fwd(x.h, x.F, x.P, x.W2, x.b2, x.v[:, None], x.bv, x.keep, RATE_A, SLOPE)
    x.ctx_d = O.dropout_fwd(x.ctx, x.keep_in, RATE_IN)
    x.qpre = x.cache[1]
    peak = x.alpha[np.arange(B), x.rows]
    assert (peak > 0.5).all() and (peak < 0.95).all(), peak
    x.dctx_d, x.dz = n(B, D), n(B, 4 * U, sc=0.3)
    x.Wc = n(D, 4 * U, sc=(4 * U) ** -0.5)
    x.dP0, x.dF0, x.dvb0 = n(B, R, A, sc=0.05), n(B, R, D, sc=0.3), n(B, A + 1, sc=0.3)
    return x


def step_bwd_ref(x, dctx_d, coef=0.0):
    """float64: dh, dsum (= dP of the step), dF, dvb [B][A], dqpre, dW2"""
    dctx = O.dropout_bwd(dctx_d, x.keep_in, RATE_IN)
    ext = coef * (x.alpha - 1) if coef else None
    dh, dF, dsum, dW2, _, dv, _ = O.attention_step_bwd(dctx, x.F, x.W2, x.v[:, None], x.cache, SLOPE, dalpha_ext=ext)
    dalpha = (dctx[:, None, :] * x.F).sum(axis=2) + (ext if ext is not None else 0)
    de = x.alpha * (dalpha - (x.alpha * dalpha).sum(axis=1, keepdims=True))
    dvb = (x.sd * de[:, :, None]).sum(axis=1)
    assert np.abs(dvb.sum(0) - dv[:, 0]).max() <= 1e-12 * (np.abs(dv).max() + 1)
    return types.SimpleNamespace(dh=dh, dP=dsum, dF=dF, dvb=dvb, dq=O.act_bwd(x.qpre, dsum.sum(axis=1), O.ACT_LEAKY, SLOPE),
                                 dW2=dW2)


@pytest.mark.parametrize("name,B,R,D,A,U,nparts,vs,poff", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_kernels_against_float64(be, name, B, R, D, A, U, nparts, vs, poff):
    """tnt_attention_step_fwd_f32 / _bwd_f32 at one shape per kernel and row-pass count (table above): qpre, alpha, ctx,
    ctx_d, s_out forward; dh, dP, dF, dvb, dqpre and dW2 = h^T dqpre backward, in each mode -- (a) dctx_d given, added to
    filled accumulators, (b) dz + Wc, (c) nparts unequal context-gradient parts, (d) alpha_mse_coef = 0.37, (e) fresh over
    NaN accumulators, (f) stored keep4 bits, bit-identical to in-kernel Philox (where A % 4 == 0, keep4's contract) --
    every one against float64 at RTOL; nothing written behind any output."""
    x = step_inputs(name, B, R, D, A, U, vs)
    rep, tails = Report(name), []

    def out(*shape, fill=NAN):
        view, tail = guarded(*shape, fill=fill)
        tails.append(tail)
        return view
    Pbuf = torch.zeros(B * R * A + 4, device="cuda")
    Pd = Pbuf[poff:poff + B * R * A].view(B, R, A)
    Pd.copy_(dev(x.P))
    assert Pd.data_ptr() % 16 == 4 * poff
    Fd, W2d, vd, hd, b2d, bvd = dev(x.F), dev(x.W2), dev(x.v), dev(x.h), dev(x.b2), dev(x.bv)
    step_dev = torch.tensor([STEP_DEV], dtype=torch.int32, device="cuda")
    keep4 = None
    if A % 4 == 0:
        keep4 = torch.zeros(B * R * A // 4, dtype=torch.uint8, device="cuda")
        be.dropout_mask4(keep4.view(1, -1), B * R * A, 1, RATE_A, SEED, SITE_A, STEP, step_dev)
    tail_args = (B, R, D, A, U, SLOPE, RATE_A, RATE_IN, x.lw, SEED, SITE_A, SITE_I, STEP, step_dev)

    def fwd(k4):
        o = [out(B, A), out(B, R), out(B, D), out(B, D), out(B, R, A)]
        be.attention_step_fwd(hd, Fd, Pd, W2d, b2d, vd, bvd, *o, *tail_args, keep4=k4)
        return o
    f0 = fwd(None)
    for nm, got, want in zip(("qpre", "alpha", "ctx", "ctx_d", "s_out"), f0, (x.qpre, x.alpha, x.ctx, x.ctx_d, x.sd)):
        rep.add(nm, got, want)
    assert torch.equal(f0[4] == 0, dev(~x.keep, torch.bool))             # exactly the oracle's mask was dropped
    if keep4 is not None:
        for a, b in zip(f0, fwd(keep4)):
            assert torch.equal(a, b)
    qd, ald = dev(x.qpre), dev(x.alpha)

    def bwd(tag, ref, acc=None, k4=None, fresh=False, **kw):
        """one backward launch; acc = None: zeroed accumulators (NaN-filled with fresh), else the (dP0, dF0, dvb0) to add to"""
        fill = NAN if fresh else 0.0
        dP, dF, dvb, dq, dh = out(B, R, A, fill=fill), out(B, R, D, fill=fill), out(B, A + 1, fill=fill), out(B, A), out(B, U)
        base = (0.0, 0.0, np.zeros((B, A + 1)))
        if acc is not None:
            dP.copy_(dev(acc[0])); dF.copy_(dev(acc[1])); dvb.copy_(dev(acc[2])); base = acc
        dctx_d = kw.pop("dctx_d", None)
        be.attention_step_bwd(dctx_d, Fd, Pd, W2d, vd, qd, ald, dP, dF, dvb, dq, dh, *tail_args, keep4=k4, fresh=fresh, **kw)
        rep.add(tag + " dh", dh, ref.dh); rep.add(tag + " dP", dP, base[0] + ref.dP); rep.add(tag + " dF", dF, base[1] + ref.dF)
        rep.add(tag + " dvb", dvb[:, :A], base[2][:, :A] + ref.dvb); rep.add(tag + " dqpre", dq, ref.dq)
        rep.add(tag + " dW2", x.h.T @ dq.cpu().double().numpy(), ref.dW2)
        # the softmax backward sums to zero over the regions: column A (the per-sample part of dbv) only rounds
        assert np.abs(dvb[:, A].cpu().double().numpy() - base[2][:, A]).max() < 1e-4
        return dP, dF, dvb, dq, dh
    ref_a = step_bwd_ref(x, x.dctx_d)
    acc = (x.dP0 * np.abs(ref_a.dP).max() / 0.05, x.dF0, x.dvb0)          # accumulators of the size of what is added
    acc = tuple(r32(t) for t in acc)
    a0 = bwd("(a)", ref_a, acc=acc, dctx_d=dev(x.dctx_d))
    bwd("(a0)", ref_a, dctx_d=dev(x.dctx_d))                              # the same onto zeros: the bound is the step's own scale
    if keep4 is not None:                                                 # (f)
        for a, b in zip(a0, bwd("(f)", ref_a, acc=acc, k4=keep4, dctx_d=dev(x.dctx_d))):
            assert torch.equal(a, b)
    bwd("(b)", step_bwd_ref(x, x.dz @ x.Wc.T), dz=dev(x.dz), Wc=dev(x.Wc))
    rng = np.random.default_rng(5)
    parts = rng.standard_normal((nparts, B, D)) * (0.2 + 1.8 * rng.random((nparts, 1, 1)))      # unequal parts ...
    parts[-1] += x.dctx_d - parts.sum(0)                                                        # ... that sum to dctx_d
    parts = r32(parts)
    assert nparts * D <= 1024
    bwd("(c)", step_bwd_ref(x, parts.sum(0)), dctx_part=dev(parts), nparts=nparts)
    bwd("(d)", step_bwd_ref(x, x.dctx_d, coef=0.37), dctx_d=dev(x.dctx_d), alpha_mse=0.37)
    e = bwd("(e)", ref_a, fresh=True, dctx_d=dev(x.dctx_d))
    assert float(e[2][:, A].abs().max()) < 1e-4
    torch.cuda.synchronize()
    assert all(float(t.min()) == SENT == float(t.max()) for t in tails)
    assert float(Pbuf[:poff].abs().sum()) == 0 and float(Pbuf[poff + B * R * A:].abs().sum()) == 0
    rep.check()


def test_step_kernels_refuse_what_they_cannot_run(be):
    """R = 2049, D = 65, A = 65, nparts * D = 1028 and dz with U = 24 come back with the ABI's argument code (-1000 - k, k the
    argument's number in the source) and nothing is launched: every output keeps its fill."""
    from masters_thesis_amd._lib import KernelLibraryError

    def call(B, R, D, A, U, code, fwd=True, **kw):
        z = lambda *s: torch.zeros(*s, device="cuda")
        outs = [torch.full(s, SENT, device="cuda") for s in ((B, A), (B, R), (B, D), (B, D), (B, R, A), (B, R, D), (B, A + 1), (B, U))]
        qpre, alpha, ctx, ctx_d, s_out, dF, dvb, dh = outs
        tail = (B, R, D, A, U, SLOPE, 0.2, 0.2, D + 20, 7, 16, 48, 0, None)
        if fwd:
            with pytest.raises(KernelLibraryError, match=rf"code {code}$"):
                be.attention_step_fwd(z(B, U), z(B, R, D), z(B, R, A), z(U, A), z(A), z(A), z(1), qpre, alpha, ctx, ctx_d, s_out, *tail)
        kw = {k: z(*s) if isinstance(s, tuple) else s for k, s in kw.items()}
        with pytest.raises(KernelLibraryError, match=rf"code {code}$"):
            be.attention_step_bwd(z(B, D), z(B, R, D), z(B, R, A), z(U, A), z(A), z(B, A), z(B, R), s_out, dF, dvb, qpre, dh,
                                  *tail, **kw)
        torch.cuda.synchronize()
        assert all(float(o.min()) == SENT == float(o.max()) for o in outs)
    call(2, 2049, 8, 8, 32, -1002)
    call(2, 16, 65, 8, 32, -1003)
    call(2, 16, 8, 65, 32, -1004)
    call(2, 16, 4, 8, 32, -1030, fwd=False, dctx_part=(257, 2, 4), nparts=257)
    call(2, 16, 8, 8, 24, -1027, fwd=False, dz=(2, 4 * 24), Wc=(8, 4 * 24))


# ---------------------------------------------------------------------------------------------- chain kernels
#             id         T  B    R    D   A   v scale  alpha_mse
CHAIN_CASES = [("8-3-8",   3, 5,   129, 32, 32, 0.6,     0.0),
               ("8-3-16",  3, 65,  100, 32, 32, 0.6,     0.01),
               ("8-6-8",   3, 5,   385, 32, 32, 0.6,     0.01),
               ("8-6-16",  4, 80,  512, 16, 32, 0.6,     0.0),
               ("16-3-8",  3, 9,   65,  36, 8,  1.5,     0.01),
               ("16-3-16", 3, 65,  192, 64, 64, 0.4,     0.0),
               ("16-6-8",  3, 8,   193, 48, 40, 0.5,     0.0),
               ("16-6-16", 3, 128, 384, 64, 64, 0.4,     0.01)]
U_SEQ = 512
C_RATE_A, C_RATE_IN, C_RATE_OUT, C_SEED, C_SITE_A, C_SITE_I, C_SITE_O, C_STEP = 0.2, 0.3, 0.3, 4711, 16, 48, 77, 3


@functools.lru_cache(maxsize=1)
def chain_case(name):
    """inputs (float32-valued float64), masks and the float64 forward / backward reference of one case; the forward and
    the backward test of a case run back to back and share it"""
    _, T, B, R, D, A, vs, mse = next(c for c in CHAIN_CASES if c[0] == name)
    U = U_SEQ
    rng = np.random.default_rng(sum(map(ord, name)) + 1000)
    n = lambda *s, sc=1.0: r32(rng.standard_normal(s) * sc)
    x = types.SimpleNamespace(T=T, B=B, R=R, D=D, A=A, U=U, mse=mse, lw=D + 20)
    x.fwd_in = dict(F=n(B, R, D), P=n(B, R, A), W2=n(U, A, sc=U ** -0.5), b2=n(A, sc=0.1), v=make_v(rng, A, vs), bv=n(1),
                    xz=n(T, B, U, 4, sc=0.5), Wc=n(D, U, 4, sc=D ** -0.5), Ur=n(U, U, 4, sc=U ** -0.5), zb=n(U, 4, sc=0.1),
                    h0=n(B, U, sc=0.5), c0=n(B, U, sc=0.5))
    i = x.fwd_in
    x.masks = C.chain_masks(T, B, R, D, A, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A, C_SITE_I, C_STEP)
    x.out_masks = C.out_masks(T, B, U, C_RATE_OUT, C_SEED, C_SITE_O, C_STEP)
    q0 = O.act_fwd(i["h0"] @ i["W2"] + i["b2"], O.ACT_LEAKY, SLOPE)
    i["P"], x.rows = plant_peaks(i["P"], q0, i["v"], i["bv"], x.masks[0][0], C_RATE_A, target=0.9)
    x.f = C.chain_fwd(**i, r_attn=C_RATE_A, r_in=C_RATE_IN, masks=x.masks)
    peak = x.f["alpha"][:, np.arange(B), x.rows]
    # 0.9 in step 0; later steps draw another dropout mask and another query, which move the row's score by a few units
    # either way (a fifth of its A terms is dropped), so there the weight is asserted on average only
    assert (peak[0] > 0.5).all() and peak[1:].mean() > 0.5, (name, peak[0].min(), peak[1:].mean())
    x.dout = n(T, B, U, sc=0.1)
    st = {k: r32(x.f[k]) for k in ("qpre", "alpha", "gates", "cs")}               # what the device is given as "stored"
    x.stored = st
    x.b = C.chain_bwd(i["F"], i["P"], i["W2"], i["v"], i["Wc"], i["Ur"], st["qpre"], st["alpha"], st["gates"], st["cs"], x.dout,
                      r_attn=C_RATE_A, r_in=C_RATE_IN, masks=x.masks, alpha_mse_coef=mse, out_drop=(C_RATE_OUT, x.out_masks))
    return x


def chain_dev(be, x):
    """device copies of a case's operands, the stored keep bits, and the exchange / state buffers (filled with 7.0: their
    contents must not matter)"""
    T, B, R, A, U = x.T, x.B, x.R, x.A, x.U
    d = types.SimpleNamespace(**{k: dev(a) for k, a in x.fwd_in.items()})
    d.step_dev = torch.tensor([C_STEP], dtype=torch.int32, device="cuda")
    d.keep = torch.zeros(T, B * R * A // 4, dtype=torch.uint8, device="cuda")
    be.dropout_mask4(d.keep, B * R * A, T, C_RATE_A, C_SEED, C_SITE_A, 0, d.step_dev)
    d.sync, d.guard = torch.zeros(1025, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    return d


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("name", [c[0] for c in CHAIN_CASES])
def test_chain_kernels_against_float64_and_step_kernels(be, name, direction):
    """tnt_lc_seq_fwd[_drop]_f32 / tnt_lc_seq_bwd[_drop]_f32, one case per compiled variant <G4, NP, RB> (table above), T = 3
    steps (a first, an interior and a last one; T = 4 once), attention dropout 0.2, context input dropout 0.3.
    Forward: four launches on one sync / exchange state -- stored keep4 bits, then in-kernel Philox, each first plain
    and then with the output Dropout riding along (hd bit-equal to tnt_dropout_f32 of hs[1:]) -- each compared with
    chain_fwd in float64 (hs, cs, gates, qpre, alpha, ctx, ctx_d at RTOL) and with the per-step launches.
    Backward, on the stored values of the float64 forward: the same four launches, the riders receiving the unmasked dout;
    dz, dqpre, dP, dF, dvb[:, :A] against chain_bwd at RTOL and against the per-step sequence; |dvb[:, A]| < 1e-4.
    After every launch the error word sync[1024] and the guard are 0."""
    x = chain_case(name)
    T, B, R, D, A, U = x.T, x.B, x.R, x.D, x.A, x.U
    if not be.lstm_seq_supported(B, U):
        pytest.skip("persistent chain kernels not supported on this device")
    d = chain_dev(be, x)
    rep = Report(f"{name} {direction}")
    z = lambda *s: torch.zeros(*s, device="cuda")
    stride = B * R * A // 4
    if direction == "fwd":
        def buffers():
            hs, cs = z(T + 1, B, U), z(T + 1, B, U)
            hs[0], cs[0] = d.h0, d.c0
            return dict(hs=hs, cs=cs, gates=z(T, B, U, 4), qpre=z(T, B, A), alpha=z(T, B, R), ctx=z(T, B, D), ctx_d=z(T, B, D))
        ref = buffers()
        for i in range(T):
            be.attention_step_fwd(ref["hs"][i], d.F, d.P, d.W2, d.b2, d.v, d.bv, ref["qpre"][i], ref["alpha"][i], ref["ctx"][i],
                                  ref["ctx_d"][i], None, B, R, D, A, U, SLOPE, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A + i,
                                  C_SITE_I + i, 0, d.step_dev, keep4=d.keep[i])
            be.lstm_step_fwd(d.xz[i], ref["hs"][i], ref["cs"][i], d.Ur, ref["ctx_d"][i], d.Wc, D, None, 0, 0, None,
                             ref["hs"][i + 1], ref["cs"][i + 1], None, ref["gates"][i], B, U, xz_bias=d.zb)
        work = torch.full((be.lc_seq_fwd_work_floats(B),), 7.0, device="cuda")
        for stored in (True, False):
            for rider in (False, True):
                tag = f"{'keep4' if stored else 'philox'}{'+hd' if rider else ''}"
                got, hd = buffers(), torch.full((T, B, U), NAN, device="cuda")
                be.lc_seq_fwd(d.F, d.P, d.W2, d.b2, d.v, d.bv, got["qpre"], got["alpha"], got["ctx"], got["ctx_d"],
                              d.keep if stored else None, stride if stored else 0, d.xz, d.Wc, d.Ur, d.zb, got["hs"], got["cs"],
                              got["gates"], T, B, R, D, A, U, SLOPE, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A, C_SITE_I,
                              d.step_dev, work, d.sync, d.guard, out_drop=(hd, C_RATE_OUT, C_SITE_O) if rider else None)
                torch.cuda.synchronize()
                assert int(d.sync[1024]) == 0 and float(d.guard) == 0.0, tag
                if rider:
                    hd_ref = z(T, B, U)
                    be.dropout(got["hs"][1:].view(T * B, U), hd_ref.view(T * B, U), T * B, U, U, 0, U, 0, C_RATE_OUT, C_SEED,
                               C_SITE_O, 0, d.step_dev, rows_per_site=B)
                    assert torch.equal(hd, hd_ref), tag
                    assert torch.equal(hd == 0, dev(~np.stack(x.out_masks), torch.bool)), tag
                for k in ref:
                    rep.add(f"{tag} {k}", got[k], x.f[k])
                    rep.add_abs(f"{tag} {k} vs steps", got[k], ref[k], 2e-5 * max(1.0, ref[k].abs().max().item()))
    else:
        st = types.SimpleNamespace(**{k: dev(a) for k, a in x.stored.items()})
        dout_raw = dev(x.dout)
        dout = torch.empty_like(dout_raw)                        # Dropout' behind the LSTM: one site per step
        be.dropout(dout_raw.view(T * B, U), dout.view(T * B, U), T * B, U, U, 0, U, 0, C_RATE_OUT, C_SEED, C_SITE_O, 0, d.step_dev,
                   rows_per_site=B)
        # ---- the per-step sequence (tnt_lstm_step_bwd_f32 + tnt_attention_step_bwd_f32)
        r_dz, r_dq, r_dP, r_dF, r_dvb = z(T, B, U, 4), z(T, B, A), z(B, R, A), z(B, R, D), z(B, A + 1)
        dh_att, dc, parts = z(B, U), z(B, U), z(U // 16, B, D)
        use_parts = (U // 16) * D <= 1024              # the per-step kernels' limit; else dctx = dz Wc^T inside the attention step
        for i in range(T - 1, -1, -1):
            last = i == T - 1
            be.lstm_step_bwd(None if last else r_dz[i + 1], d.Ur, None, None if last else dh_att, None if last else dc, None,
                             dout[i], None, 0, 0, st.gates[i], st.cs[i + 1], st.cs[i], r_dz[i], None, dc, None, B, U,
                             Wc=d.Wc if use_parts else None, D=D, dctx_part=parts if use_parts else None)
            kw = dict(dctx_part=parts, nparts=U // 16) if use_parts else dict(dz=r_dz[i], Wc=d.Wc)
            be.attention_step_bwd(None, d.F, d.P, d.W2, d.v, st.qpre[i], st.alpha[i], r_dP, r_dF, r_dvb, r_dq[i], dh_att, B, R, D,
                                  A, U, SLOPE, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A + i, C_SITE_I + i, 0, d.step_dev,
                                  keep4=d.keep[i], alpha_mse=x.mse, fresh=last, **kw)
        steps = dict(dz=r_dz, dqpre=r_dq, dP=r_dP, dF=r_dF, dvb=r_dvb[:, :A])
        work = torch.full((be.lc_seq_bwd_work_floats(B, U),), 7.0, device="cuda")
        for stored in (True, False):
            for rider in (False, True):
                tag = f"{'keep4' if stored else 'philox'}{'+drop' if rider else ''}"
                f = lambda *s: torch.full(s, NAN, device="cuda")
                g_dz, g_dq, g_dP, g_dF, g_dvb = f(T, B, U, 4), f(T, B, A), f(B, R, A), f(B, R, D), f(B, A + 1)
                be.lc_seq_bwd(d.F, d.P, d.W2, d.v, st.qpre, st.alpha, d.keep if stored else None, stride if stored else 0, g_dP,
                              g_dF, g_dvb, g_dq, d.Ur, d.Wc, dout_raw if rider else dout, st.gates, st.cs, g_dz, work, T, B, R, D,
                              A, U, SLOPE, C_RATE_A, C_RATE_IN, x.lw, C_SEED, C_SITE_A, C_SITE_I, d.step_dev, x.mse, d.sync,
                              d.guard, out_drop=(C_RATE_OUT, C_SITE_O) if rider else None)
                torch.cuda.synchronize()
                assert int(d.sync[1024]) == 0 and float(d.guard) == 0.0, tag
                got = dict(dz=g_dz, dqpre=g_dq, dP=g_dP, dF=g_dF, dvb=g_dvb[:, :A])
                for k in got:
                    rep.add(f"{tag} {k}", got[k], x.b[k])
                    rep.add_abs(f"{tag} {k} vs steps", got[k], steps[k], 3e-5 * max(1e-3, steps[k].abs().max().item()))
                assert g_dvb[:, A].abs().max().item() < 1e-4, tag
    rep.check()


def _chain_call(be, T, B, R, D, A, U, poff=0):
    """both chain entry points on buffers of the full size of the shape (were a refusal missing, the launch would stay
    inside them); returns the two error codes (0 = launched)"""
    from masters_thesis_amd._lib import KernelLibraryError
    z = lambda *s: torch.zeros(*s, device="cuda")
    P = z(B * R * A + 4)[poff:poff + B * R * A].view(B, R, A)
    sync, guard = torch.zeros(1025, dtype=torch.int32, device="cuda"), z(1)
    step_dev = torch.tensor([0], dtype=torch.int32, device="cuda")
    work = z(max(3 * B * 1024, 3 * ((B + 7) // 8) * 32 * 32 * 256 + 3 * B * U + 3 * ((B + 7) // 8) * 16 * 16 * 64))
    F, W2, v, Wc, Ur = z(B, R, D), z(U, A), z(A + 4), z(D, U, 4), z(U, U, 4)
    codes = []
    for fwd in (True, False):
        try:
            if fwd:
                be.lc_seq_fwd(F, P, W2, z(A), v, z(1), z(T, B, A), z(T, B, R), z(T, B, D), z(T, B, D), None, 0, z(T, B, U, 4), Wc, Ur,
                              z(U, 4), z(T + 1, B, U), z(T + 1, B, U), z(T, B, U, 4), T, B, R, D, A, U, SLOPE, 0.0, 0.0, D + 20, 7,
                              16, 48, step_dev, work, sync, guard)
            else:
                be.lc_seq_bwd(F, P, W2, v, z(T, B, A), z(T, B, R), None, 0, z(B, R, A), z(B, R, D), z(B, A + 1), z(T, B, A), Ur, Wc,
                              z(T, B, U), z(T, B, U, 4), z(T + 1, B, U), z(T, B, U, 4), work, T, B, R, D, A, U, SLOPE, 0.0, 0.0,
                              D + 20, 7, 16, 48, step_dev, 0.0, sync, guard)
            codes.append(0)
        except KernelLibraryError as e:
            codes.append(int(str(e).rsplit("code ", 1)[1]))
    return codes


def test_chain_contract(be):
    """What tnt_lc_seq_{fwd,bwd}_f32 refuse, by the ABI's argument code and with no launch: R = 513 at A = D = 32, R = 385
    at D = 36 (code 21), B = 129, U = 256 (24), A = 30 (21), P one float off 16-byte alignment (1); the work sizes are 0 for
    B = 0 and B = 129; and lc_nic.NIC._lc_seq_ok draws its line where the library does, at R = 512 | 513 (A = D = 32)
    and R = 384 | 385 (A = 40).  The library's answer for an admitted shape is read without a launch: its shape checks
    come before its alignment check, so with a misaligned P an admitted shape answers 1 and a refused one 21."""
    from masters_thesis_amd.lc_nic import NIC
    for shape, code in (((1, 2, 513, 32, 32, 512), -1021), ((1, 2, 385, 36, 32, 512), -1021), ((1, 129, 16, 32, 32, 512), -1024),
                        ((1, 2, 16, 32, 32, 256), -1024), ((1, 2, 16, 32, 30, 512), -1021)):
        assert _chain_call(be, *shape) == [code, code], shape
    assert _chain_call(be, 1, 2, 16, 32, 32, 512, poff=1) == [-1001, -1001]
    assert be.lc_seq_fwd_work_floats(0) == 0 and be.lc_seq_fwd_work_floats(129) == 0 and be.lc_seq_fwd_work_floats(128) > 0
    assert be.lc_seq_bwd_work_floats(0, 512) == 0 and be.lc_seq_bwd_work_floats(129, 512) == 0
    assert be.lc_seq_bwd_work_floats(128, 512) > 0 and be.lc_seq_bwd_work_floats(64, 256) == 0
    for R, D, A in ((512, 32, 32), (513, 32, 32), (384, 32, 40), (385, 32, 40), (384, 40, 32), (385, 40, 32)):
        model = types.SimpleNamespace(_seq_lstm=True, use_lc_seq=True, use_layer_norm=False, be=be, R=R, D=D, A=A)
        admitted = _chain_call(be, 1, 2, R, D, A, 512, poff=1) == [-1001, -1001]
        assert NIC._lc_seq_ok(model) == admitted == (R in (512, 384)), (R, D, A)
