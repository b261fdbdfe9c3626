"""Per-variable learning-rate multipliers and frozen variables inside the update kernels on a real MI355X: the LM
instantiations of adam_fin_kernel (tnt_adam_fin_lrmul_f32), adam_kernel (tnt_adam_lrmul_f32), sgd_kernel
(tnt_sgd_lrmul_f32), the norm launches that do not read a frozen gradient (tnt_span_sqnorm_lrmul_f32,
tnt_seg_sqnorm_lrmul_f32) and the reduction that leaves the frozen variables out (tnt_global_sqnorm_lrmul_f32), against the
float64 restatement of the header's definition: the plain float64 update with the step and the decay scaled by the
variable's multiplier, a frozen variable untouched.

The arena is test_gpu_weight_decay's (ten variables of 1 ... 9 * 8192 + 3 elements: a scalar tail, an unaligned length,
exact and ragged spans, one variable of ten spans); the table freezes a single-span variable, the ten-span variable and the
last one.  Tolerances are test_gpu_optim_tail's (theta 1e-6, m / v 1e-5 relative per variable, the padding bit-identical),
the reduction's test_gpu_global_clip's.  With multipliers in {0.25, 0.5, 2, 10} a kernel that ignored the table misses
theta's bound by four orders of magnitude.  Where the definition promises bits (a frozen variable, a table of ones, a
tripped guard, non-finite values in a frozen gradient) the comparison is bit-exact.

The encoder's fused update takes its variable's multiplier as a scalar (tnt_dense_dw_adam_lrmul_f32 /
tnt_dense_dw_adam_fin_lrmul_f32), tested at test_gpu_weight_decay's ENC_SHAPES as test_dense_dw_adamw argues."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ops as O
from global_clip_oracle import global_sqnorm, gsq_rel_bound
from test_gpu_ops import close, dev
from test_gpu_optim_tail import B1, B2, EPS, EXTRA_SEG, LR, check_update, desc, host, lr_t_of, norm_launch, ref_adam, state
from test_gpu_weight_decay import ENC_SHAPES, SIDE, arena, be, enc_case, plain_state, ref_adamw, start  # noqa: F401  (fixtures)
from test_gpu_global_clip import MU, q_list, ref_update, ring_args, sgd_args

pytestmark = pytest.mark.gpu

LRM = np.float32([1, 0, 0.5, 10, 0, 1, 0.25, 0, 2, 0])
FROZEN = [s for s, m in enumerate(LRM) if m == 0]
GSQ, C, CS = 4.0, 1.0, 0.5            # a supplied global word: cs = c / max(sqrt(G), c) = 0.5


def mixed(A, before, after, lrm=LRM):
    """the definition on top of a plain float64 Adam update: theta moves by mul times the plain step (update and decay
    are both linear in the rate), the moments are the plain ones; a frozen variable keeps all three"""
    out = [x.copy() for x in after]
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        sl = slice(o, o + n)
        if lrm[s] == 0:
            for x, b in zip(out, before):
                x[sl] = b[sl]
        else:
            out[0][sl] = before[0][sl] + float(lrm[s]) * (after[0][sl] - before[0][sl])
    return out


def assert_frozen_bits(A, S, keys=("th", "m", "v"), lrm=LRM):
    for k, h in zip(keys, (A.theta, A.m0, A.v0)):
        got = S[k].cpu().numpy()
        for s in (s for s, m in enumerate(lrm) if m == 0):
            o, n = A.offs[s], A.lens[s]
            assert np.array_equal(got[o:o + n], h[o:o + n]), (k, s)


def lrm_norm_launch(be, A, S, lrm, skip=True):
    sp = A.sp
    be.span_sqnorm_lrmul(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], S["partial"], sp.nspan, lrm,
                         lr_job=(S["adam_t"], S["lr"], S["lr_t"], B1, B2), skip=S["ovr"] if skip else None)


def fin_lrmul(be, A, S, fin, clip, lrm, gsq=None, wd=None, **ring):
    sp = A.sp
    be.adam_fin_lrmul(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["ovr"], sp.nspan, EPS, clip, fin,
                      lrm, gsq=gsq, seg_wd=wd, **ring)


def poison(A, S, lrm=LRM):
    """non-finite values all over the gradients of the frozen variables"""
    g = S["gr"]
    for k, s in enumerate(s for s, m in enumerate(lrm) if m == 0):
        o, n = A.offs[s], A.lens[s]
        g[o:o + n] = float("nan") if k % 2 == 0 else float("inf")
        if n > 2:
            g[o + 1] = -float("inf")


# ------------------------------------------------------------------------------------------ the span kernel, fin form
@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("mode", ["clip", "noclip", "gclip"])
def test_adam_fin_lrmul_against_float64(be, arena, mode, decay):
    A = arena
    S = state(A)
    lrm, wd = dev(LRM), dev(A.wd) if decay else None
    gsq = dev([GSQ]) if mode == "gclip" else None
    clip = {"clip": 0.1, "noclip": 0.0, "gclip": C}[mode]
    poison(A, S)                                          # the frozen gradients hold NaN / inf throughout
    lrm_norm_launch(be, A, S, lrm)
    fin_lrmul(be, A, S, desc(be, A, S), clip, lrm, gsq=gsq, wd=wd)
    torch.cuda.synchronize()
    if mode == "gclip":
        after = ref_update(A, CS, "adam", wd=A.wd if decay else None)
    else:
        after = ref_adamw(A, *start(A), 7, clip, wd=A.wd if decay else np.zeros(A.nseg))
    check_update(A, host(S, "th", "m", "v"), mixed(A, start(A), after), before=[A.theta, A.m0, A.v0])
    assert_frozen_bits(A, S)
    # the counters tick once, the ticket is re-armed, every scalar the side workgroup files is finite
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41 and int(S["arrive"].abs().sum()) == 0
    assert abs(float(S["lr_t"]) - lr_t_of(7)) <= 1e-6 * lr_t_of(7)
    for k in ("partial", "sq", "wsq", "l2o", "o0", "o1", "o2", "extra"):
        assert bool(torch.isfinite(S[k]).all()), k
    sq, wsq = host(S, "sq", "wsq")
    for s in FROZEN:                                       # no norm of a frozen gradient; its L2 term stays in the metric
        o, n = A.offs[s], A.lens[s]
        want_w = 0.0 if A.l2[s] == 0 else (A.theta[o:o + n].astype(np.float64) ** 2).sum()
        assert sq[s] == 0.0 and abs(wsq[s] - want_w) <= 1e-5 * want_w, s
    want_l2 = sum(float(A.l2[s]) * (A.theta[o:o + n].astype(np.float64) ** 2).sum() for s, (o, n) in enumerate(zip(A.offs, A.lens)))
    assert abs(float(S["l2o"]) - want_l2) <= 1e-5 * want_l2


def test_non_finite_frozen_gradients_change_no_bit(be, arena):
    """the same launches with clean and with poisoned frozen gradients: every output is bit-equal, the global word included"""
    A = arena
    lrm = dev(LRM)
    out = []
    for dirty in (False, True):
        S = state(A)
        if dirty:
            poison(A, S)
        gsq = torch.full((1,), -7.0, device="cuda")
        lrm_norm_launch(be, A, S, lrm)
        be.global_sqnorm_lrmul(gsq, A.nseg, lrm, sq_override=S["ovr"], partial=S["partial"], seg_first=A.sp.seg_first,
                               extra_part=S["ep"], n_extra=len(A.extra_part), extra_seg=EXTRA_SEG)
        fin_lrmul(be, A, S, desc(be, A, S), 0.05, lrm, gsq=gsq, wd=dev(A.wd))
        torch.cuda.synchronize()
        S["gsq"] = gsq
        out.append(S)
    clean, dirty = out
    for k in ("th", "m", "v", "gsq") + SIDE:
        assert torch.equal(clean[k], dirty[k]), k
    assert bool(torch.isfinite(dirty["gsq"]).all()) and float(dirty["gsq"]) > 0 and int(dirty["adam_t"]) == 7
    assert_frozen_bits(A, dirty)


def test_a_table_of_ones_is_the_plain_launch(be, arena):
    A = arena
    sp = A.sp
    ones = torch.ones(A.nseg, device="cuda")
    # fin form: norm launch, reduction, update, with decay and the global word
    S, P = state(A), state(A)
    gs, gp = torch.full((1,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda")
    kw = dict(sq_override=S["ovr"], seg_first=sp.seg_first, n_extra=len(A.extra_part), extra_seg=EXTRA_SEG)
    lrm_norm_launch(be, A, S, ones)
    be.global_sqnorm_lrmul(gs, A.nseg, ones, partial=S["partial"], extra_part=S["ep"], **kw)
    fin_lrmul(be, A, S, desc(be, A, S), 0.05, ones, gsq=gs, wd=dev(A.wd))
    norm_launch(be, A, P)
    be.global_sqnorm(gp, A.nseg, partial=P["partial"], extra_part=P["ep"], **kw)
    be.adam_fin_gclip(P["th"], P["m"], P["v"], P["gr"], sp.span_seg, sp.span_off, sp.span_len, P["ovr"], sp.nspan, EPS, 0.05,
                      desc(be, A, P), gp, seg_wd=dev(A.wd))
    # ... and per-variable clipping without decay
    S2, P2 = state(A), state(A)
    lrm_norm_launch(be, A, S2, ones)
    fin_lrmul(be, A, S2, desc(be, A, S2), 0.1, ones)
    norm_launch(be, A, P2)
    be.adam_fin(P2["th"], P2["m"], P2["v"], P2["gr"], sp.span_seg, sp.span_off, sp.span_len, P2["ovr"], sp.nspan, EPS, 0.1,
                desc(be, A, P2))
    torch.cuda.synchronize()
    assert torch.equal(gs, gp)
    for X, Y in ((S, P), (S2, P2)):
        for k in ("th", "m", "v") + SIDE:
            assert torch.equal(X[k], Y[k]), k
    # the ring form, SGD and the table-form norm launch
    R, Q, G, H = (lrm_plain_state(be, A, ones) for _ in range(4))
    Rp, Gp = plain_state(be, A), plain_state(be, A)
    for k in ("partial", "sq", "wsq"):
        assert torch.equal(R[k], Rp[k]), k
    be.adam_lrmul(*ring_args(A, R, 0.1), ones, guard=R["guard"])
    be.adam(*ring_args(A, Rp, 0.1), guard=Rp["guard"])
    be.adam_lrmul(*ring_args(A, Q, 0.1), ones, lr=Q["lr"], seg_wd=dev(A.wd), guard=Q["guard"])
    Qp = plain_state(be, A)
    be.adamw(*ring_args(A, Qp, 0.1), Qp["lr"], dev(A.wd), guard=Qp["guard"])
    be.sgd_lrmul(*sgd_args(A, G), 0.0, G["lr"], MU, 0.1, ones, guard=G["guard"])
    be.sgd(*sgd_args(A, Gp), 0.0, Gp["lr"], MU, 0.1, guard=Gp["guard"])
    Hp = plain_state(be, A)
    be.sgd_lrmul(*sgd_args(A, H), 0.0, H["lr"], MU, 0.1, ones, seg_wd=dev(A.wd), guard=H["guard"])
    be.sgdw(*sgd_args(A, Hp), Hp["lr"], MU, 0.1, dev(A.wd), guard=Hp["guard"])
    torch.cuda.synchronize()
    for X, Y in ((R, Rp), (Q, Qp), (G, Gp), (H, Hp)):
        for k in ("th", "m", "v"):
            assert torch.equal(X[k], Y[k]), k


def test_metrics_ring_and_counters_once_per_launch(be, arena):
    """three launches with frozen spans present: one ring row, one tick of each counter and a re-armed ticket per launch"""
    A = arena
    S = state(A)
    lrm = dev(LRM)
    nmet = 5
    met = torch.zeros(nmet, device="cuda")
    ring = torch.full((2, nmet + 1), -7.0, device="cuda")
    ring_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    fin = desc(be, A, S)
    for k in range(3):
        vec = np.float32([k + 0.5, -k, 1e3 * k, 7, 0.25 * k])
        met.copy_(dev(vec))
        lrm_norm_launch(be, A, S, lrm)
        fin_lrmul(be, A, S, fin, 0.1, lrm, met=met, ring=ring, ring_t=ring_t)
        torch.cuda.synchronize()
        assert int(ring_t) == k + 1 and int(S["adam_t"]) == 7 + k and int(S["drop"]) == 41 + k
        assert int(S["arrive"].abs().sum()) == 0
        assert torch.equal(ring[k % 2], dev(np.append(vec, np.float32(k))))
    assert_frozen_bits(A, S)
    # the ring form files its row from a frozen first span's workgroup too
    frozen_first = dev(np.float32([0] + [1] * (A.nseg - 1)))
    R = lrm_plain_state(be, A, frozen_first)
    be.adam_lrmul(*ring_args(A, R, 0.1), frozen_first, guard=R["guard"], met=met, ring=ring, ring_t=ring_t)
    torch.cuda.synchronize()
    assert int(ring_t) == 4 and torch.equal(ring[1, :nmet], met)
    assert torch.equal(R["th"][:1], dev(A.theta[:1])) and not torch.equal(R["th"], dev(A.theta))


# ------------------------------------------------------------------------------------------ the plain forms
def lrm_plain_state(be, A, lrm):
    """test_gpu_weight_decay.plain_state with the norm launch that takes the table"""
    S = state(A)
    sp = A.sp
    be.seg_sqnorm_lrmul(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, S["l2"], S["partial"], S["sq"],
                        S["wsq"], None, sp.nspan, A.nseg, lrm)
    S["lr_t"].fill_(float(np.float32(lr_t_of(7))))
    return S


@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("mode", ["clip", "noclip", "gclip"])
def test_adam_lrmul_against_float64(be, arena, mode, decay):
    A = arena
    lrm = dev(LRM)
    S = state(A)
    poison(A, S)
    sp = A.sp
    be.seg_sqnorm_lrmul(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, S["l2"], S["partial"], S["sq"],
                        S["wsq"], S["l2o"], sp.nspan, A.nseg, lrm)
    lr_t = np.float32(lr_t_of(7))
    S["lr_t"].fill_(float(lr_t))
    clip = {"clip": 0.1, "noclip": 0.0, "gclip": C}[mode]
    kw = dict(lr=S["lr"], seg_wd=dev(A.wd)) if decay else {}
    be.adam_lrmul(*ring_args(A, S, clip), lrm, gsq=dev([GSQ]) if mode == "gclip" else None, guard=S["guard"], **kw)
    torch.cuda.synchronize()
    wd = A.wd if decay else None
    if mode == "gclip":
        after = ref_update(A, CS, "adam", lr_t=lr_t, wd=wd)
    else:
        th0 = start(A)[0]
        th1, m1, v1 = ref_adam(A, *start(A), 7, clip, extra=False)
        th1 = th0 + (th1 - th0) * (float(lr_t) / lr_t_of(7))               # lr_t is handed over as a float32
        for s, (o, n) in enumerate(zip(A.offs, A.lens)):
            th1[o:o + n] -= (float(LR) * float(wd[s] if decay else 0.0)) * th0[o:o + n]
        after = (th1, m1, v1)
    check_update(A, host(S, "th", "m", "v"), mixed(A, start(A), after), before=[A.theta, A.m0, A.v0])
    assert_frozen_bits(A, S)
    for k in ("partial", "sq", "wsq", "l2o"):
        assert bool(torch.isfinite(S[k]).all()), k
    assert all(float(S["sq"][s]) == 0.0 for s in FROZEN)


@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("mode", ["clip", "gclip"])
def test_sgd_lrmul_against_float64(be, arena, mode, decay):
    A = arena
    lrm = dev(LRM)
    S = lrm_plain_state(be, A, lrm)
    poison(A, S)
    clip = 0.1 if mode == "clip" else C
    be.sgd_lrmul(*sgd_args(A, S), 0.0, S["lr"], MU, clip, lrm, gsq=dev([GSQ]) if mode == "gclip" else None,
                 seg_wd=dev(A.wd) if decay else None, guard=S["guard"])
    torch.cuda.synchronize()
    th, mom = start(A)[:2]
    th1, mom1 = th.copy(), mom.copy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        if LRM[s] == 0:
            continue
        w = th[o:o + n]
        g = A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w
        if mode == "gclip":
            g = g * CS
        else:
            q = float(A.ovr[s]) if A.ovr[s] >= 0 else (g * g).sum()
            g = g * clip / max(np.sqrt(q), clip)
        rate = float(LRM[s]) * float(LR)
        t1, mom1[o:o + n] = O.sgd_momentum_update(w, mom[o:o + n], g, rate, MU)
        th1[o:o + n] = t1 - (rate * float(A.wd[s] if decay else 0.0)) * w
    check_update(A, host(S, "th", "m"), (th1, mom1), before=[A.theta, A.m0])
    assert_frozen_bits(A, S, keys=("th", "m"))


# ------------------------------------------------------------------------------------------ the reduction launch
@pytest.mark.parametrize("form", ["fin", "table"])
def test_global_sqnorm_lrmul_arena(be, arena, form):
    A = arena
    lrm = dev(LRM)
    if form == "fin":
        S = state(A)
        poison(A, S)
        lrm_norm_launch(be, A, S, lrm)
        kw = dict(partial=S["partial"], seg_first=A.sp.seg_first, extra_part=S["ep"], n_extra=len(A.extra_part), extra_seg=EXTRA_SEG)
    else:
        S = lrm_plain_state(be, A, lrm)
        S["sq"][FROZEN] = float("nan")                       # a frozen slot is not read, whatever it holds
        kw = dict(sq=S["sq"])
    g1, g2 = torch.full((1,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda")
    for g in (g1, g2):
        be.global_sqnorm_lrmul(g, A.nseg, lrm, sq_override=S["ovr"], **kw)
    torch.cuda.synchronize()
    q = q_list(A, form, extra_part=A.extra_part)
    want = global_sqnorm([q[s] for s in range(A.nseg) if LRM[s] != 0])
    assert want < 0.97 * global_sqnorm(q)                    # the frozen variables' share of the full norm: 3000 x the bound
    assert abs(float(g1) - want) <= gsq_rel_bound(A.nseg) * want, (float(g1), want)
    assert torch.equal(g1, g2)
    if form == "fin":                                        # a frozen Embedding: its extra partials are left out as well
        tab = LRM.copy(); tab[EXTRA_SEG] = 0
        g3 = torch.full((1,), -7.0, device="cuda")
        S["ep"].fill_(float("nan"))
        be.global_sqnorm_lrmul(g3, A.nseg, dev(tab), sq_override=S["ovr"], **kw)
        torch.cuda.synchronize()
        w3 = global_sqnorm([q[s] for s in range(A.nseg) if tab[s] != 0])
        assert abs(float(g3) - w3) <= gsq_rel_bound(A.nseg) * w3


@pytest.mark.parametrize("lens", [[5], [9 * 8192 + 3], [3] * 730, [3] * 255 + [11 * 8192] + [3] * 300 + [9 * 8192 + 1]],
                         ids=["one-small", "one-10-spans", "730-one-span", "556-two-large"])
def test_global_sqnorm_lrmul_shapes(be, lens):
    """test_gpu_global_clip.test_global_sqnorm_shapes' variable lists with every third variable frozen (variable 0 too: a
    list of one variable sums to 0), both forms from random span partials, non-finite partials in the frozen slots"""
    from masters_thesis_amd.arena import build_spans
    rng = np.random.default_rng(len(lens))
    offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in lens])])[:-1].tolist()
    sp = build_spans(offs, lens, device="cuda")
    nseg = len(lens)
    tab = np.ones(nseg, np.float32)
    tab[::3] = 0
    tab[1::3] = 0.5
    part = (rng.random(2 * sp.nspan) * 3).astype(np.float32)
    ovr = np.full(nseg, -1.0, np.float32)
    if nseg > 300:
        ovr[[7, 255, 300]] = [2.5, 11.0, 0.0]
    first = sp.seg_first.cpu().numpy()
    q = [float(ovr[s]) if ovr[s] >= 0 else float(part[2 * first[s]:2 * first[s + 1]:2].astype(np.float64).sum())
         for s in range(nseg)]
    want = global_sqnorm([q[s] for s in range(nseg) if tab[s] != 0])
    sq, wsq = torch.zeros(nseg, device="cuda"), torch.zeros(nseg, device="cuda")
    be.step_finalize(dev(part), sp.seg_first, torch.zeros(nseg, device="cuda"), sq, wsq, None, nseg)
    for s in range(0, nseg, 3):
        part[2 * first[s]:2 * first[s + 1]] = np.nan
    sq[::3] = float("inf")
    pd, od, td = dev(part), dev(ovr), dev(tab)
    g = [torch.full((1,), -7.0, device="cuda") for _ in range(4)]
    for out in g[:2]:
        be.global_sqnorm_lrmul(out, nseg, td, sq_override=od, partial=pd, seg_first=sp.seg_first)
    for out in g[2:]:
        be.global_sqnorm_lrmul(out, nseg, td, sq_override=od, sq=sq)
    torch.cuda.synchronize()
    assert abs(float(g[0]) - want) <= gsq_rel_bound(nseg) * want, (float(g[0]), want)
    for out in g[1:]:
        assert torch.equal(out, g[0])


# ------------------------------------------------------------------------------------------ the encoder kernel
@pytest.mark.parametrize("form", ["fin", "sq"])
@pytest.mark.parametrize("mode", ["clip", "override", "noclip", "gclip"])
@pytest.mark.parametrize("N,E,Bk,ldx", ENC_SHAPES)
def test_dense_dw_adam_lrmul(be, enc_case, N, E, Bk, ldx, mode, form):
    """both forms at a scalar multiplier, with and without decay: g is the kernel's own float32 product, everything behind
    it (L2, clip, Adam at lrm * lr_t, the decay at lrm * lr) float64.  lrm = 1 gives the plain, decaying and global-clip
    entries' bits, lrm = 0 and a tripped guard leave the state, a bad lrm is BADARG without a launch."""
    from masters_thesis_amd.arena import build_spans
    from masters_thesis_amd.ops import _p
    c = enc_case(N, E, Bk, ldx)
    F32 = lambda x: float(np.float32(x))
    lam, lr_t, lrm = F32(0.01), F32(3e-4), 0.25
    clip = {"clip": 0.1, "override": 0.1, "noclip": 0.0, "gclip": C}[mode]
    nslot, k0 = build_spans([0], [N * E], device="cpu").nspan, 3
    partial = torch.full((2 * (k0 + nslot + 5),), 7.0, device="cuda")
    be.dense_dw_sqnorm(c.xd, c.dd, dev(c.theta), lam, partial[2 * k0:], nslot, N, E, Bk, ldx)
    sq = partial[2 * k0:2 * (k0 + nslot):2].sum().reshape(1)
    ovr, lrt, lr = dev([4.0 if mode == "override" else -1.0]), dev([lr_t]), dev([LR])
    gsq = dev([GSQ]) if mode == "gclip" else None
    guard = torch.zeros(1, dtype=torch.int32, device="cuda")
    norm = (partial, k0, k0 + nslot) if form == "fin" else (sq,)
    tail = (ovr, lrt, B1, B2, EPS, clip, N, E, Bk, ldx)

    def run(mul, decay, tripped=False, entry="lrmul"):
        th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
        guard[0] = int(tripped)
        head = (c.xd, c.dd, th, m, v, lam) + norm
        kw = dict(lr=lr, wd=decay) if decay is not None else {}
        if entry == "lrmul" and form == "fin":
            be.dense_dw_adam_fin_lrmul(*head, *tail, mul, gsq=gsq, **kw, guard=guard)
        elif entry == "lrmul":
            be.dense_dw_adam_lrmul(*head, *tail, mul, gsq=gsq, **kw, guard=guard)
        elif mode == "gclip":
            (be.dense_dw_adam_fin_gclip if form == "fin" else be.dense_dw_adam_gclip)(*head, *tail, gsq, **kw, guard=guard)
        elif decay is not None:
            (be.dense_dw_adamw_fin if form == "fin" else be.dense_dw_adamw)(*head, *tail, lr, decay, guard=guard)
        else:
            (be.dense_dw_adam_fin if form == "fin" else be.dense_dw_adam)(*head, *tail, guard=guard)
        torch.cuda.synchronize()
        return th, m, v

    th64 = c.theta.astype(np.float64)
    ge = c.gk + 2 * lam * th64
    if mode == "gclip":
        ge = ge * CS
    elif clip > 0:
        q = 4.0 if mode == "override" else ((c.g64 + 2 * lam * th64) ** 2).sum()
        ge = ge * clip / max(np.sqrt(q), clip)
    _, mw, vw = O.adam_update(th64, c.m0.astype(np.float64), c.v0.astype(np.float64), ge, 1, 1.0, B1, B2, EPS)
    for wd in (None, 0.05):
        th, m, v = run(lrm, wd)
        tw = (th64 - (lrm * lr_t) * mw / (np.sqrt(vw) + EPS)) - (lrm * float(LR) * (wd or 0.0)) * th64
        close(m, mw, rtol=1e-5); close(v, vw, rtol=1e-5); close(th, tw, rtol=1e-6)
        for a, b in zip(run(1.0, wd), run(None, wd, entry="plain")):          # a multiplier of 1: the other entries' bits
            assert torch.equal(a, b)
        for a, h in zip(run(0.0, wd), (c.theta, c.m0, c.v0)):                  # frozen: no launch
            assert torch.equal(a, dev(h))
        for a, h in zip(run(lrm, wd, tripped=True), (c.theta, c.m0, c.v0)):
            assert torch.equal(a, dev(h))
    assert float(partial[:2 * k0].max()) == 7.0 and float(partial[2 * (k0 + nslot):].min()) == 7.0
    if mode == "clip":
        th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
        lib, s = be.lib, be._s()
        for bad in (-0.5, float("nan"), float("inf")):
            rcs = (lib.tnt_dense_dw_adam_lrmul_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(sq), None, _p(lrt), B1, B2, EPS,
                                                   0.1, None, N, E, Bk, ldx, bad, None, None, 0.0, s),
                   lib.tnt_dense_dw_adam_fin_lrmul_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(partial), k0, k0 + nslot,
                                                       None, _p(lrt), B1, B2, EPS, 0.1, None, N, E, Bk, ldx, bad, None, None, 0.0, s))
            assert all(rc <= -1000 for rc in rcs), (bad, rcs)
        torch.cuda.synchronize()
        assert torch.equal(th, dev(c.theta)) and torch.equal(m, dev(c.m0)) and torch.equal(v, dev(c.v0))


# ------------------------------------------------------------------------------------------ capture, guard, bad arguments
def test_a_captured_launch_follows_an_in_place_table_rewrite(be, arena):
    A = arena
    S = state(A)
    lrm = dev(LRM)
    fin = desc(be, A, S)
    pair = lambda: (lrm_norm_launch(be, A, S, lrm), fin_lrmul(be, A, S, fin, 0.1, lrm))
    pair()                                                   # warm-up outside the capture; it is step 7
    torch.cuda.synchronize()
    prev = host(S, "th", "m", "v")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    torch.cuda.synchronize()
    assert torch.equal(S["th"], dev(prev[0])) and int(S["adam_t"]) == 7          # capturing runs nothing
    tabs = (np.float32([0, 1, 1, 0, 2, 0, 1, 0.1, 0, 1]), np.ones(A.nseg, np.float32), LRM)
    for k, tab in enumerate(tabs):
        lrm.copy_(dev(tab))
        g.replay()
        torch.cuda.synchronize()
        got = host(S, "th", "m", "v")
        after = ref_adam(A, *prev, 8 + k, 0.1)
        want = mixed(A, prev, after, lrm=tab)
        check_update(A, got, want, before=prev)
        for x, b in zip(got, prev):                          # the variables frozen in THIS replay: bit for bit
            for s in (s for s, m in enumerate(tab) if m == 0):
                assert np.array_equal(x[A.offs[s]:A.offs[s] + A.lens[s]], b[A.offs[s]:A.offs[s] + A.lens[s]]), (k, s)
        assert int(S["adam_t"]) == 8 + k and int(S["arrive"].abs().sum()) == 0
        prev = got


def test_tripped_guard_leaves_the_state(be, arena):
    A = arena
    lrm, gsq = dev(LRM), dev([GSQ])
    S = state(A)
    S["guard"][0] = 1
    lrm_norm_launch(be, A, S, lrm)
    fin_lrmul(be, A, S, desc(be, A, S), C, lrm, gsq=gsq, wd=dev(A.wd))
    R, G = lrm_plain_state(be, A, lrm), lrm_plain_state(be, A, lrm)
    R["guard"][0] = 1; G["guard"][0] = 1
    be.adam_lrmul(*ring_args(A, R, C), lrm, gsq=gsq, lr=R["lr"], seg_wd=dev(A.wd), guard=R["guard"])
    be.sgd_lrmul(*sgd_args(A, G), 0.0, G["lr"], MU, 0.1, lrm, guard=G["guard"])
    torch.cuda.synchronize()
    for X in (S, R, G):
        for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
            assert torch.equal(X[k], dev(h)), k
    assert int(S["adam_t"]) == 6 and int(S["drop"]) == 40 and int(S["arrive"].abs().sum()) == 0


def test_bad_arguments_return_badarg_without_a_launch(be, arena):
    from masters_thesis_amd.ops import _p
    A, lib, s = arena, be.lib, be._s()
    sp = A.sp
    S = plain_state(be, A)
    fin, good, lrm = desc(be, A, S), dev([4.0]), dev(LRM)
    part0 = S["partial"].clone()
    spans = (_p(sp.span_seg), _p(sp.span_off), _p(sp.span_len))
    ring = lambda tab, g, cl, lr, wd: lib.tnt_adam_lrmul_f32(
        _p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]), _p(S["ovr"]), sp.nspan, 0.0,
        _p(S["lr_t"]), B1, B2, EPS, cl, None, None, 0, None, 0, None, tab, g, lr, wd, s)
    finl = lambda tab, g, cl: lib.tnt_adam_fin_lrmul_f32(
        _p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["ovr"]), sp.nspan, EPS, cl, ctypes.addressof(fin), None, 0,
        None, 0, None, tab, g, None, s)
    sgd = lambda tab, g, cl, lr, wd: lib.tnt_sgd_lrmul_f32(
        _p(S["th"]), _p(S["m"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]), _p(S["ovr"]), sp.nspan, 0.0, lr, 0.9, cl, None,
        tab, g, wd, s)
    norm = lambda tab: lib.tnt_span_sqnorm_lrmul_f32(_p(S["th"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["partial"]), sp.nspan,
                                                     None, None, None, 0.0, 0.0, None, tab, s)
    segn = lambda tab: lib.tnt_seg_sqnorm_lrmul_f32(_p(S["th"]), _p(S["gr"]), *spans, _p(sp.seg_first), _p(S["l2"]),
                                                    _p(S["partial"]), _p(S["sq"]), _p(S["wsq"]), None, sp.nspan, A.nseg, tab, s)
    red = lambda tab, out: lib.tnt_global_sqnorm_lrmul_f32(None, None, _p(S["sq"]), _p(S["ovr"]), None, 0, -1, A.nseg, out, tab, s)
    T, L, W = _p(lrm), _p(S["lr"]), _p(dev(A.wd))
    rcs = [ring(None, None, 0.1, None, None), finl(None, None, 0.1), sgd(None, None, 0.1, L, None), norm(None), segn(None),
           red(None, _p(good)), red(T, None),                                     # a null table; a reduction without an output
           ring(T, None, 0.1, None, W), sgd(T, None, 0.1, None, W)]               # a decay without its learning rate
    for cl in (0.0, -1.0, float("nan"), float("inf")):                            # a global word with a bad threshold
        rcs += [ring(T, _p(good), cl, None, None), finl(T, _p(good), cl), sgd(T, _p(good), cl, L, None)]
    # the lr job needs all three of its pointers
    rcs.append(lib.tnt_span_sqnorm_lrmul_f32(_p(S["th"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["partial"]), sp.nspan, None, None,
                                             _p(S["lr_t"]), B1, B2, None, T, s))
    assert all(rc <= -1000 for rc in rcs), rcs
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):                      # nothing was launched
        assert torch.equal(S[k], dev(h)), k
    assert torch.equal(S["partial"], part0) and float(good) == 4.0
    assert int(S["adam_t"]) == 6 and int(S["arrive"].abs().sum()) == 0
    assert lib.tnt_version() >= 130
