"""Classifier-free guidance on the GPU, the kernel: tnt_guidance_mix_f32 against the float64 restatement
(tests/guidance_oracle.py) over vocabulary sizes, row counts, scales and plausibility masks, with wide rows and columns
banned in the null row, the conditional row or both; exact zeros, pad columns, read-only logits, the token on both slabs;
exact ties; a null slab equal to the conditional one; scale = 0 against softmax + argmax; the degenerate rows; a row wider
than the register path; every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import guidance_oracle as GO

pytestmark = pytest.mark.gpu

# |p - p64| <= REL * (1 + 2 * scale) * p64 + ABS.  REL, ABS are the consensus kernel test's (tests/test_gpu_consensus.py):
# float32 exp carries the rounding of its argument, lc and ln are each rounded to half an ulp of a magnitude up to ~160 on
# the wide rows, and the 5001-term float32 sums add a few 1e-7.  The rounding of lc enters g (1 + scale) times, that of ln
# scale times, hence the factor.
# Measured on the CPU with the float32 numpy restatement of the same formula (GO.mix(..., dtype=np.float32): numpy's
# summation order, no fused multiply-add) against the float64 one on exactly these inputs, worst error / bound per V over
# all Rm, scale, plaus:  V=1: 0.000  V=5: 0.014  V=63: 0.377  V=64: 0.139  V=65: 0.167  V=257: 0.137  V=5001: 0.606
# V=8200: 0.479.  A worst ratio above 1 on the GPU would be a finding about the kernel, not a reason to widen the bound.
REL, ABS = 2e-5, 1e-9
VS = (1, 5, 63, 64, 65, 257, 5001)
RMS = (1, 3, 7)
SCALES = (0.0, 0.5, 1.5, 8.0)
PLAUS = (0.0, 0.1)
NEAR = 1e-3             # no conditional log-probability of the inputs lies this close to the mask threshold
# V -> the seed of its logits, chosen on the CPU so that the float64 restatement has no lc_v within NEAR of
# log(plaus) + max lc (asserted below): a column that close could flip between masked and kept within rounding
SEED = {1: 1, 5: 5, 63: 63, 64: 64, 65: 65, 257: 2257, 5001: 8001, 8200: 15200}


def bound(want, scale):
    return REL * (1 + 2 * scale) * want + ABS


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_logits(rng, V, ld, Rm):
    """(x (2*Rm, ld) float32 with NaN in the pad columns, null_col, cond_col, both_col), after make_logits of
    tests/test_gpu_consensus.py: N(0, 3^2) logits; every third mixed row is wide in both members (uniform over [-80, 80]);
    column null_col is -inf in the null row only, cond_col in the conditional row only, both_col in both.  V < 4 has no room
    for three distinct columns and bans nothing (the columns come back as None)."""
    x = np.full((2 * Rm, ld), np.nan, np.float32)
    body = rng.standard_normal((2, Rm, V)) * 3
    wide = np.arange(Rm) % 3 == 1
    body[:, wide] = rng.uniform(-80, 80, (2, int(wide.sum()), V))
    null_col = cond_col = both_col = None
    if V >= 4:
        null_col, cond_col, both_col = 1, 2, (V * 3) // 5
        body[1, :, null_col] = -np.inf
        body[0, :, cond_col] = -np.inf
        body[:, :, both_col] = -np.inf
    x[:, :V] = body.reshape(2 * Rm, V)
    return x, null_col, cond_col, both_col


def cases(V):
    """the logits of every Rm for this V, from one generator seeded by SEED[V]"""
    rng = np.random.default_rng(SEED[V])
    return [(Rm, make_logits(rng, V, V + 3, Rm)) for Rm in RMS]


def threshold_distance(x, plaus):
    """the smallest |lc_v - (log(plaus) + max lc)| over the finite lc_v of the conditional rows, in float64"""
    xc = np.asarray(x[:x.shape[0] // 2], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = xc.max(axis=-1, keepdims=True)
        lc = (xc - m) - np.log(np.exp(xc - m).sum(axis=-1, keepdims=True))
        d = np.abs(lc - (np.log(plaus) + lc.max(axis=-1, keepdims=True)))
    return float(d[np.isfinite(d)].min()) if np.isfinite(d).any() else np.inf


def run_mix(be, x, V, ld, Rm, scale, plaus, with_token=True):
    """-> (mix (Rm, ld) with the sentinel -7 where nothing was written, token (2*Rm,) or None)"""
    xd = dev(x)
    mixd = torch.full((Rm, ld), -7.0, dtype=torch.float32, device="cuda")
    tok = torch.full((2 * Rm,), -9, dtype=torch.int32, device="cuda") if with_token else None
    be.guidance_mix(xd, ld, V, Rm, scale, plaus, mixd, ld, tok)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))          # the logits are read only
    return mixd.cpu().numpy(), None if tok is None else tok.cpu().numpy()


def check_against_float64(be, V):
    ld = V + 3
    worst = 0.0
    for Rm, (x, null_col, cond_col, both_col) in cases(V):
        for plaus in PLAUS:
            if plaus > 0:
                assert threshold_distance(x[:, :V], plaus) >= NEAR, (V, Rm)        # the inputs alone, in float64
            for scale in SCALES:
                got, tok = run_mix(be, x, V, ld, Rm, scale, plaus)
                want, _ = GO.mix(x[:, :V], scale, plaus)
                tag = (V, Rm, scale, plaus)
                p = got[:, :V]
                assert np.all(got[:, V:] == -7.0), tag                                   # pad columns keep the sentinel
                err, bnd = np.abs(p - want), bound(want, scale)
                worst = max(worst, float((err / bnd).max()))
                assert np.all(err <= bnd), (tag, float((err / bnd).max()))
                # exactly 0.0f: the masked columns (the restatement's zeros: every other g_v is finite) and the columns
                # banned in the conditional row; a column banned in the null row only keeps g = lc
                assert np.all(p[want == 0.0] == 0.0), tag
                if cond_col is not None:
                    assert np.all(p[:, cond_col] == 0.0) and np.all(p[:, both_col] == 0.0), tag
                    assert np.all(p[:, null_col][want[:, null_col] > 1e-30] > 0.0), tag
                assert np.all(p[want > 1e-30] > 0.0), tag
                # the token: equal in both slabs, the first max of the returned p, and a maximum of the restatement's p
                t = tok.reshape(2, Rm)
                assert np.array_equal(t[0], t[1]) and np.array_equal(t[0], GO.first_max(p)), tag
                pick, top = want[np.arange(Rm), t[0]], want.max(axis=1)
                assert np.all(pick >= top - 2 * bound(top, scale)), tag
    print(f"V={V}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("V", VS)
def test_mix_matches_float64(be, V):
    check_against_float64(be, V)


def test_rows_wider_than_the_register_path(be):
    """V > 8192: the kernel re-reads the logits in every pass and parks the guided logits in the mix row"""
    check_against_float64(be, 8200)


def test_exact_tie_goes_to_the_lower_index(be):
    rng = np.random.default_rng(3)
    V, ld, Rm = 5001, 5004, 3
    x = np.zeros((2 * Rm, ld), np.float32)
    x[:, :V] = rng.standard_normal((2 * Rm, V)).astype(np.float32)
    hi, lo = 4097, 130                             # columns of different threads in different waves
    x[:Rm, hi] = x[:Rm, lo] = rng.uniform(6, 8, Rm).astype(np.float32)        # equal in the conditional row, dominating it
    x[Rm:, hi] = x[Rm:, lo] = rng.uniform(-6, -5, Rm).astype(np.float32)      # equal and unlikely in the null row: the
    #                                                                           contrast of 12 beats any other column's (< 9)
    for scale, plaus in ((0.0, 0.0), (1.5, 0.1), (8.0, 0.0)):
        got, tok = run_mix(be, x, V, ld, Rm, scale, plaus)
        assert np.all(got[:, hi] == got[:, lo]) and np.all(got[:, lo] == got[:, :V].max(axis=1))
        assert np.all(tok == lo), (scale, plaus, tok)


def test_null_equal_to_conditional_is_the_unguided_row_bit_for_bit(be):
    rng = np.random.default_rng(4)
    for V in (65, 5001):
        ld, Rm = V + 3, 3
        x, _, _, _ = make_logits(rng, V, ld, Rm)
        x[Rm:] = x[:Rm]                            # lc - ln is exactly 0 in every column
        for plaus in PLAUS:
            base, btok = run_mix(be, x, V, ld, Rm, 0.0, plaus)
            for scale in SCALES[1:]:
                got, tok = run_mix(be, x, V, ld, Rm, scale, plaus)
                assert np.array_equal(got.view(np.int32), base.view(np.int32)), (V, scale, plaus)
                assert np.array_equal(tok, btok)


def test_scale_0_without_mask_is_softmax_and_argmax(be):
    rng = np.random.default_rng(5)
    for V, ld in ((5, 8), (257, 260), (5001, 5004)):
        Rm = 7
        x, _, _, _ = make_logits(rng, V, ld, Rm)
        x[:, V:] = 0.0
        got, tok = run_mix(be, x, V, ld, Rm, 0.0, 0.0)
        xd = dev(x[:Rm])
        ids = torch.zeros(Rm, dtype=torch.int32, device="cuda")
        be.argmax_rows(xd, ids, Rm, V, ld)
        be.softmax_cce(xd, None, xd, None, None, None, Rm, V, ld, 0.0)
        torch.cuda.synchronize()
        ref = xd.cpu().numpy()[:, :V].astype(np.float64)
        assert np.all(np.abs(got[:, :V] - ref) <= bound(ref, 0.0)), V
        top2 = np.sort(ref, axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * bound(top2[:, 1], 0.0)       # the top-two gap exceeds the bound
        assert clear.any() and np.array_equal(tok[:Rm][clear], ids.cpu().numpy()[clear]), V
        assert np.array_equal(tok[:Rm], tok[Rm:])


def test_degenerate_rows(be):
    V, ld, Rm = 257, 260, 3
    rng = np.random.default_rng(6)
    x = np.zeros((2 * Rm, ld), np.float32)
    x[:, :V] = rng.standard_normal((2 * Rm, V)).astype(np.float32) * 3
    x[1, :V] = -np.inf                             # mixed row 1: the conditional row is all -inf
    x[Rm + 2, :V] = -np.inf                        # mixed row 2: the null row is all -inf
    for scale, plaus in ((1.5, 0.0), (8.0, 0.1)):
        got, tok = run_mix(be, x, V, ld, Rm, scale, plaus)
        want, wtok = GO.mix(x[:, :V], scale, plaus)
        assert np.all(got[1, :V] == 0.0) and np.all(want[1] == 0.0) and tok[1] == 0 and tok[Rm + 1] == 0
        assert np.all(np.abs(got[:, :V] - want) <= bound(want, scale))
        assert np.array_equal(tok[:Rm], tok[Rm:]) and np.array_equal(tok[:Rm], GO.first_max(got[:, :V]))
        # the all -inf null row: the softmax of the conditional row (masked, if a mask is on), whatever the scale
        alone, _ = run_mix(be, x, V, ld, Rm, 0.0, plaus)
        assert np.array_equal(got[2].view(np.int32), alone[2].view(np.int32))
    got, _ = run_mix(be, x, V, ld, Rm, 8.0, 0.0)
    xd = dev(x[2:3])
    be.softmax_cce(xd, None, xd, None, None, None, 1, V, ld, 0.0)
    torch.cuda.synchronize()
    ref = xd.cpu().numpy()[0, :V].astype(np.float64)
    assert np.all(np.abs(got[2, :V] - ref) <= bound(ref, 0.0))


def test_token_is_optional(be):
    rng = np.random.default_rng(7)
    V, ld, Rm = 257, 257, 3
    x, _, _, _ = make_logits(rng, V, ld, Rm)
    a, _ = run_mix(be, x, V, ld, Rm, 1.5, 0.1, with_token=True)
    b, tok = run_mix(be, x, V, ld, Rm, 1.5, 0.1, with_token=False)
    assert tok is None and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    Rm, V, ld = 4, 12, 16
    buf = torch.randn(2 * Rm + Rm, ld, device="cuda")          # logits, and behind them a region a mix could overlap into
    x, tail = buf[:2 * Rm], buf[2 * Rm:]
    mixd = torch.full((Rm, ld), -7.0, device="cuda")
    tok = torch.full((2 * Rm,), -9, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def call(logits=x, ld=ld, V=V, Rm=Rm, scale=1.5, plaus=0.1, mix=mixd, ldm=ld, token=tok):
        return lib.tnt_guidance_mix_f32(p(logits), ld, V, Rm, scale, plaus, p(mix), ldm, p(token), None)
    bads = [dict(Rm=0), dict(Rm=-1), dict(V=0), dict(V=-3), dict(ld=11), dict(ldm=11), dict(scale=-0.5), dict(scale=nan),
            dict(scale=inf), dict(scale=-inf), dict(plaus=-0.1), dict(plaus=1.0), dict(plaus=1.5), dict(plaus=nan),
            dict(plaus=inf), dict(logits=None), dict(mix=None), dict(mix=x), dict(mix=x[Rm:]), dict(mix=buf[2 * Rm - 1:])]
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                   # TNT_BADARG
    torch.cuda.synchronize()
    assert bool((mixd == -7.0).all()) and bool((tok == -9).all())        # nothing was launched
    assert call() == 0 and call(token=None) == 0 and call(mix=tail) == 0 and call(scale=0.0, plaus=0.0) == 0
    torch.cuda.synchronize()
    assert bool((mixd[:, :V] >= 0).all()) and bool((mixd[:, V:] == -7.0).all()) and bool((tok >= 0).all())
    assert lib.tnt_version() >= 117
