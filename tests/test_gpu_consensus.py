"""Consensus decoding on the GPU, the kernels: tnt_consensus_mix_f32 against the float64 restatement
(tests/consensus_oracle.py) over vocabulary sizes, row counts, member counts, both modes, equal and unequal weights, wide
rows and banned columns; exact ties; G = 1 against softmax + argmax; the all -inf logmean row; pad columns; every refusal;
tnt_consensus_spread_i32 bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import consensus_oracle as CO

pytestmark = pytest.mark.gpu

# |p - p64| <= REL * p64 + ABS.  float32 exp carries the rounding of its argument: x - m_g is rounded to half an ulp of a
# magnitude up to ~30 (2^-20 = 9.5e-7) and so are l_v and l_v - L in logmean, each entering p relatively; the 5001-term
# float32 sums of s_g and Z add a few 1e-7 as pairwise partial sums; ABS covers the products that underflow float32.
REL, ABS = 2e-5, 1e-9


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_logits(rng, V, ld, Rm, G):
    """(x (G*Rm, ld) float32 with NaN in the pad columns, one_col, all_col): N(0, 3^2) logits; every third mixed row is wide
    in each member (uniform over [-80, 80]); column one_col is -inf in the last member only, all_col in every member"""
    x = np.full((G * Rm, ld), np.nan, np.float32)
    body = rng.standard_normal((G, Rm, V)) * 3
    wide = np.arange(Rm) % 3 == 1
    body[:, wide] = rng.uniform(-80, 80, (G, int(wide.sum()), V))
    one_col, all_col = 1 % V, (V * 3) // 5
    body[G - 1, :, one_col] = -np.inf
    body[:, :, all_col] = -np.inf
    x[:, :V] = body.reshape(G * Rm, V)
    return x, one_col, all_col


def run_mix(be, x, V, ld, Rm, G, w, mode, with_token=True):
    """-> (mix (Rm, ld) with the sentinel -7 where nothing was written, token (G*Rm,) or None)"""
    xd = dev(x)
    mixd = torch.full((Rm, ld), -7.0, dtype=torch.float32, device="cuda")
    tok = torch.full((G * Rm,), -9, dtype=torch.int32, device="cuda") if with_token else None
    be.consensus_mix(xd, ld, V, Rm, G, dev(w), CO.MODES.index(mode), mixd, ld, tok)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))          # the logits are read only
    return mixd.cpu().numpy(), None if tok is None else tok.cpu().numpy()


@pytest.mark.parametrize("V", [5, 257, 5001])
def test_mix_matches_float64(be, V):
    rng = np.random.default_rng(V)
    ld = V + 3
    worst = 0.0
    for Rm in (1, 3, 7):
        for G in (1, 2, 3, 8, 16):
            x, one_col, all_col = make_logits(rng, V, ld, Rm, G)
            unequal = rng.uniform(0.2, 2.0, G)
            for w in (None, (unequal / unequal.sum()).astype(np.float32)):
                for mode in CO.MODES:
                    got, tok = run_mix(be, x, V, ld, Rm, G, w, mode)
                    want, _ = CO.mix(x[:, :V], G, w, mode)
                    tag = (V, Rm, G, mode, w is not None)
                    p = got[:, :V]
                    assert np.all(got[:, V:] == -7.0), tag                                   # pad columns untouched
                    err, bound = np.abs(p - want), REL * want + ABS
                    worst = max(worst, float((err / bound).max()))
                    assert np.all(err <= bound), (tag, float((err / bound).max()))
                    # -inf: exactly 0 in all members' column; in one member's column only for logmean (G = 1: that member
                    # is the only one)
                    assert np.all(p[:, all_col] == 0.0), tag
                    if mode == "logmean" or G == 1:
                        assert np.all(p[:, one_col] == 0.0), tag
                    else:
                        assert np.all(p[:, one_col][want[:, one_col] > 1e-30] > 0.0), tag
                    # the token: no exclusions
                    t = tok.reshape(G, Rm)
                    assert np.all(t == t[0]), tag
                    pick = want[np.arange(Rm), t[0]]
                    assert np.all((t[0] >= 0) & (t[0] < V)) and np.all(pick >= want.max(axis=1) * (1 - 1e-5)), tag
                    assert np.array_equal(t[0], CO.first_max(p)), tag                        # and it is the first max of p
    print(f"V={V}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode", CO.MODES)
def test_exact_tie_goes_to_the_lower_index(be, mode):
    rng = np.random.default_rng(3)
    V, ld, Rm = 5001, 5004, 3
    for G in (1, 3, 16):
        x = np.zeros((G * Rm, ld), np.float32)
        x[:, :V] = rng.standard_normal((G * Rm, V)).astype(np.float32)
        hi, lo = 4097, 130                         # columns of different threads in different waves
        x[:, hi] = x[:, lo] = (rng.uniform(6, 8, G * Rm)).astype(np.float32)      # equal in every member, dominating the row
        got, tok = run_mix(be, x, V, ld, Rm, G, None, mode)
        assert np.all(got[:, hi] == got[:, lo]) and np.all(got[:, lo] == got[:, :V].max(axis=1))
        assert np.all(tok == lo), (G, tok)


def test_one_member_mean_is_softmax_and_argmax(be):
    rng = np.random.default_rng(4)
    for V, ld in ((5, 8), (257, 260), (5001, 5004)):
        Rm = 7
        x, _, _ = make_logits(rng, V, ld, Rm, 1)
        x[:, V:] = 0.0
        got, tok = run_mix(be, x, V, ld, Rm, 1, None, "mean")
        xd = dev(x)
        ids = torch.zeros(Rm, dtype=torch.int32, device="cuda")
        be.softmax_cce(xd, None, xd, None, None, None, Rm, V, ld, 0.0)
        be.argmax_rows(xd, ids, Rm, V, ld)
        torch.cuda.synchronize()
        ref = xd.cpu().numpy()[:, :V].astype(np.float64)
        assert np.array_equal(tok, ids.cpu().numpy()), V
        assert np.all(np.abs(got[:, :V] - ref) <= REL * ref + ABS), V


def test_all_banned_logmean_row_is_zero_with_token_zero(be):
    V, ld, Rm, G = 257, 260, 3, 2
    rng = np.random.default_rng(5)
    x = np.zeros((G * Rm, ld), np.float32)
    x[:, :V] = rng.standard_normal((G * Rm, V)).astype(np.float32)
    # mixed row 1: member 0 bans the even columns, member 1 the odd ones, so every l_v is -inf though every member has a
    # finite maximum; mixed row 2: both member rows are -inf throughout
    x[0 * Rm + 1, 0:V:2] = -np.inf
    x[1 * Rm + 1, 1:V:2] = -np.inf
    x[0 * Rm + 2, :V] = x[1 * Rm + 2, :V] = -np.inf
    got, tok = run_mix(be, x, V, ld, Rm, G, None, "logmean")
    want, wtok = CO.mix(x[:, :V], G, None, "logmean")
    assert np.all(got[1:, :V] == 0.0) and np.all(want[1:] == 0.0)
    assert np.array_equal(tok.reshape(G, Rm)[0], wtok) and np.all(tok.reshape(G, Rm)[:, 1:] == 0)
    assert np.all(np.abs(got[0, :V] - want[0]) <= REL * want[0] + ABS) and tok[0] == wtok[0]
    # mean: the members' supports are disjoint, nothing is lost; the all -inf members contribute nothing
    got, tok = run_mix(be, x, V, ld, Rm, G, None, "mean")
    want, wtok = CO.mix(x[:, :V], G, None, "mean")
    assert np.all(np.abs(got[:, :V] - want) <= REL * want + ABS) and np.all(got[2, :V] == 0.0)
    assert np.array_equal(tok.reshape(G, Rm)[0], wtok)


def test_token_is_optional(be):
    rng = np.random.default_rng(6)
    V, ld, Rm, G = 257, 257, 3, 3
    x, _, _ = make_logits(rng, V, ld, Rm, G)
    for mode in CO.MODES:
        a, _ = run_mix(be, x, V, ld, Rm, G, None, mode, with_token=True)
        b, tok = run_mix(be, x, V, ld, Rm, G, None, mode, with_token=False)
        assert tok is None and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    G, Rm, V, ld = 3, 4, 12, 16
    buf = torch.randn(G * Rm + Rm, ld, device="cuda")          # logits, and behind them a region a mix could overlap into
    x, tail = buf[:G * Rm], buf[G * Rm:]
    mixd = torch.full((Rm, ld), -7.0, device="cuda")
    tok = torch.full((G * Rm,), -9, dtype=torch.int32, device="cuda")
    w = torch.full((G,), 1 / 3, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(logits=x, ld=ld, V=V, Rm=Rm, G=G, w=w, mode=0, mix=mixd, ldm=ld, token=tok):
        return lib.tnt_consensus_mix_f32(p(logits), ld, V, Rm, G, p(w), mode, p(mix), ldm, p(token), None)
    bads = [dict(Rm=0), dict(Rm=-1), dict(V=0), dict(V=-3), dict(ld=11), dict(ldm=11), dict(G=0), dict(G=17), dict(G=-1),
            dict(mode=2), dict(mode=-1), dict(logits=None), dict(mix=None), dict(mix=x), dict(mix=x[Rm:]),
            dict(mix=buf[G * Rm - 1:])]
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                   # TNT_BADARG
    torch.cuda.synchronize()
    assert bool((mixd == -7.0).all()) and bool((tok == -9).all())        # nothing was launched
    assert call() == 0 and call(w=None, token=None) == 0 and call(mix=tail) == 0 and call(mode=1, G=1) == 0
    torch.cuda.synchronize()
    assert bool((mixd[:, :V] >= 0).all()) and bool((mixd[:, V:] == -7.0).all()) and bool((tok >= 0).all())

    i32 = dict(dtype=torch.int32, device="cuda")
    src, out = torch.ones(Rm, **i32), torch.full((G * Rm,), -9, **i32)

    def sp(token=src, parent=src, fin=src, Rm=Rm, G=G, token_out=out, parent_out=out, fin_out=out):
        return lib.tnt_consensus_spread_i32(p(token), p(parent), p(fin), Rm, G, p(token_out), p(parent_out), p(fin_out), None)
    for kw in [dict(Rm=0), dict(G=0), dict(G=17), dict(token_out=None), dict(parent_out=None), dict(fin_out=None)]:
        rc = sp(**kw)
        assert -1100 < rc <= -1000, (kw, rc)
    torch.cuda.synchronize()
    assert bool((out == -9).all())
    assert sp(token=None, parent=None, fin=None, token_out=None, parent_out=None, fin_out=None) == 0


@pytest.mark.parametrize("Rm,G", [(1, 1), (3, 2), (7, 16), (320, 3), (1000, 8)])
def test_spread_is_bitwise_and_every_output_is_optional(be, Rm, G):
    rng = np.random.default_rng(Rm * 31 + G)
    token = rng.integers(-5, 5001, Rm).astype(np.int32)
    parent = rng.integers(0, Rm, Rm).astype(np.int32)
    fin = rng.integers(0, 2, Rm).astype(np.int32)
    want = CO.spread(token, parent, fin, Rm, G)
    for mask in range(1, 8):
        srcs = [dev(a) if mask >> j & 1 else None for j, a in enumerate((token, parent, fin))]
        outs = [torch.full((G * Rm + 2,), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
        be.consensus_spread(*srcs, Rm, G, *[o if s is not None else None for o, s in zip(outs, srcs)])
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            o = o.cpu().numpy()
            assert np.all(o[G * Rm:] == -9), (mask, j)                                   # nothing behind the last row
            if mask >> j & 1:
                assert np.array_equal(o[:G * Rm], want[j]), (mask, j)
            else:
                assert np.all(o == -9), (mask, j)
