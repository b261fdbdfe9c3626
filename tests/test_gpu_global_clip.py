"""Global-norm gradient clipping on a real MI355X: the reduction launch tnt_global_sqnorm_f32 in both input forms and the
GC instantiations of the update kernels (tnt_adam_fin_gclip_f32, tnt_adam_gclip_f32, tnt_sgd_gclip_f32,
tnt_dense_dw_adam_gclip_f32 / _fin_gclip_f32) against the float64 restatement of the header's definition
(tests/global_clip_oracle.py).

Tolerances: the update entries take test_gpu_optim_tail's (theta 1e-6, m / v 1e-5 relative per variable, the padding
bit-identical); the reduction takes the per-variable norm tolerance of that file (1e-5) plus the float32 summation
bound of the header's order, global_clip_oracle.gsq_rel_bound(number of variables).

The update tests balance the arena's norms through their own sq_override / extra_part so that no variable holds more
than a fifth of G, put the threshold at a quarter of the global norm (cs = 0.25) and assert from the float64 norms that
every variable's own-norm scale at that threshold is at least twice cs: a kernel that clipped per variable, or not at
all, scales g -- and with it m, bound 1e-5 -- wrongly by a factor of 2 or more.  Where the definition promises bits
(G <= c^2, a tripped guard, the side workgroup's outputs, two launches on the same inputs) the comparison is
bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ops as O
from global_clip_oracle import clip_scale, global_sqnorm, gsq_rel_bound
from test_gpu_ops import close, dev
from test_gpu_optim_tail import (B1, B2, EPS, EXTRA_SEG, F32, LR, OVR_SEG, check_update, desc, host, lr_t_of, norm_launch,
                                 state)
from test_gpu_weight_decay import ENC_SHAPES, SIDE, arena, be, enc_case, plain_state, start  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MU = F32(0.9)


def true_q(A, s):
    """float64 sum (g + 2 lambda theta)^2 of variable s"""
    o, n = A.offs[s], A.lens[s]
    w = A.theta[o:o + n].astype(np.float64)
    g = A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w
    return float((g * g).sum())


def q_list(A, form, ovr=None, extra_part=None):
    """the definition's q_s per variable: fin form (the Embedding's extra_part, a supplied norm, the gradient's) or table
    form (a supplied norm, else the gradient's)"""
    ovr = A.ovr if ovr is None else ovr
    out = []
    for s in range(A.nseg):
        if form == "fin" and s == EXTRA_SEG and extra_part is not None and len(extra_part) > 0:
            out.append(float(np.asarray(extra_part, np.float64).sum()))
        elif ovr[s] >= 0:
            out.append(float(ovr[s]))
        else:
            out.append(true_q(A, s))
    return out


def gsq_launch(be, S, A, form, gsq, ovr=None, n_extra=None):
    ovr = S["ovr"] if ovr is None else ovr
    if form == "fin":
        n_extra = len(A.extra_part) if n_extra is None else n_extra
        be.global_sqnorm(gsq, A.nseg, sq_override=ovr, partial=S["partial"], seg_first=A.sp.seg_first, extra_part=S["ep"],
                         n_extra=n_extra, extra_seg=EXTRA_SEG)
    else:
        be.global_sqnorm(gsq, A.nseg, sq_override=ovr, sq=S["sq"])


# ------------------------------------------------------------------------------------------ the reduction launch
@pytest.mark.parametrize("form", ["fin", "table"])
def test_global_sqnorm_arena(be, arena, form):
    """the weight-decay arena: a scalar tail, one float4, a ragged second AF_U trip, two spans, a 10-span variable (the
    wave walk), OVR_SEG and the Embedding's EXTRA_SEG"""
    A = arena
    S = state(A)
    if form == "fin":
        norm_launch(be, A, S)                     # skips the gradient pass of the two variables with a supplied norm
    else:
        S = plain_state(be, A)
    g1, g2 = torch.full((1,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda")
    gsq_launch(be, S, A, form, g1)
    gsq_launch(be, S, A, form, g2)
    torch.cuda.synchronize()
    want = global_sqnorm(q_list(A, form, extra_part=A.extra_part))
    print(f"G {form}: kernel {float(g1):.9g} float64 {want:.9g} rel {abs(float(g1) - want) / want:.3g} "
          f"bound {gsq_rel_bound(A.nseg):.3g}")
    assert abs(float(g1) - want) <= gsq_rel_bound(A.nseg) * want
    assert torch.equal(g1, g2)                                           # no atomics: the same bits
    if form == "fin":                                                    # n_extra = 0: the Embedding falls back to its supplied norm
        g0 = torch.full((1,), -7.0, device="cuda")
        gsq_launch(be, S, A, form, g0, n_extra=0)
        none = dev(np.full(A.nseg, -1.0, np.float32))                     # ... and without any supplied norm to its partials
        S2 = state(A)
        norm_launch(be, A, S2, skip=False)
        g3 = torch.full((1,), -7.0, device="cuda")
        gsq_launch(be, S2, A, form, g3, ovr=none, n_extra=0)
        torch.cuda.synchronize()
        w0 = global_sqnorm(q_list(A, "table"))
        w3 = global_sqnorm([true_q(A, s) for s in range(A.nseg)])
        assert abs(float(g0) - w0) <= gsq_rel_bound(A.nseg) * w0 and abs(float(g3) - w3) <= gsq_rel_bound(A.nseg) * w3


@pytest.mark.parametrize("lens", [[5], [9 * 8192 + 3], [3] * 730, [3] * 255 + [11 * 8192] + [3] * 300 + [9 * 8192 + 1]],
                         ids=["one-small", "one-10-spans", "730-one-span", "556-two-large"])
def test_global_sqnorm_shapes(be, lens):
    """one variable only, the region-wise model's 730 one-span variables (the thread-strided loop past 256) and large
    variables in the second and third round of a wave: both forms against float64 from random span partials, bit-equal
    to each other (the same order) and over two launches"""
    from masters_thesis_amd.arena import build_spans
    rng = np.random.default_rng(len(lens))
    offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in lens])])[:-1].tolist()
    sp = build_spans(offs, lens, device="cuda")
    nseg = len(lens)
    part = (rng.random(2 * sp.nspan) * 3).astype(np.float32)
    ovr = np.full(nseg, -1.0, np.float32)
    if nseg > 300:
        ovr[[7, 255, 300]] = [2.5, 11.0, 0.0]                            # a large variable with a supplied norm is not walked
    first = sp.seg_first.cpu().numpy()
    q = [float(ovr[s]) if ovr[s] >= 0 else float(part[2 * first[s]:2 * first[s + 1]:2].astype(np.float64).sum())
         for s in range(nseg)]
    want = global_sqnorm(q)
    pd, od = dev(part), dev(ovr)
    # the table a finalize launch files: the span sums in the canonical order (tnt_step_finalize_f32)
    sq, wsq = torch.zeros(nseg, device="cuda"), torch.zeros(nseg, device="cuda")
    be.step_finalize(pd, sp.seg_first, torch.zeros(nseg, device="cuda"), sq, wsq, None, nseg)
    g = [torch.full((1,), -7.0, device="cuda") for _ in range(4)]
    for out in g[:2]:
        be.global_sqnorm(out, nseg, sq_override=od, partial=pd, seg_first=sp.seg_first)
    for out in g[2:]:
        be.global_sqnorm(out, nseg, sq_override=od, sq=sq)
    torch.cuda.synchronize()
    print(f"G: kernel {float(g[0]):.9g} float64 {want:.9g} rel {abs(float(g[0]) - want) / want:.3g}")
    assert abs(float(g[0]) - want) <= gsq_rel_bound(nseg) * want
    for out in g[1:]:
        assert torch.equal(out, g[0])


# ------------------------------------------------------------------------------------------ the update entries
def balanced(A, form):
    """sq_override / extra_part of the update tests: five variables carry about a fifth of G each.  Returns the device
    table, the extra partials (host), the float64 G and the threshold c = sqrt(G) / 4 -- after asserting that cs is in
    [0.1, 0.5] and every variable's own-norm scale at c is at least twice cs."""
    big = max(range(A.nseg), key=lambda s: A.lens[s])
    Q = true_q(A, big)
    ovr = A.ovr.copy()
    for s in (OVR_SEG, 4, 5):
        ovr[s] = Q
    ovr[EXTRA_SEG] = Q                                                    # the table form reads it, the fin form extra_part
    ep = (A.extra_part.astype(np.float64) * (Q / A.extra_part.astype(np.float64).sum())).astype(np.float32)
    q = q_list(A, form, ovr=ovr, extra_part=ep)
    G = global_sqnorm(q)
    c = F32(0.25 * np.sqrt(G))
    cs = clip_scale(G, c)
    assert 0.1 <= cs <= 0.5
    for s, qs in enumerate(q):
        own = c / max(np.sqrt(qs), c)
        assert own >= 2 * cs, (s, own, cs)
    return ovr, ep, G, c


def ref_update(A, cs, kind, t=7, lr_t=None, wd=None, th_m_v=None):
    """float64 L2 + the ONE scale cs + Adam (oracle.ops.adam_update at step t, or at a given lr_t) or SGD, less the decay of
    the theta the step started from"""
    th, m, v = th_m_v if th_m_v is not None else start(A)
    th1, m1, v1 = th.copy(), m.copy(), v.copy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        w = th[o:o + n]
        g = (A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w) * cs
        if kind == "adam":
            t1, m1[o:o + n], v1[o:o + n] = O.adam_update(w, m[o:o + n], v[o:o + n], g, t, LR, B1, B2, EPS)
            if lr_t is not None:
                t1 = w + (t1 - w) * (float(lr_t) / lr_t_of(t))
        else:
            t1, m1[o:o + n] = O.sgd_momentum_update(w, m[o:o + n], g, LR, MU)
        th1[o:o + n] = t1 - (float(LR) * (float(wd[s]) if wd is not None else 0.0)) * w
    return th1, m1, v1


def fin_state(be, A, ovr=None, ep=None):
    S = state(A)
    if ovr is not None:
        S["ovr"], S["ep"] = dev(ovr), dev(ep)
    norm_launch(be, A, S)
    return S


def fin_gclip(be, A, S, fin, c, gsq, wd=None):
    sp = A.sp
    be.adam_fin_gclip(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["ovr"], sp.nspan, EPS, c, fin,
                      gsq, seg_wd=wd)


@pytest.mark.parametrize("decay", [False, True])
def test_adam_fin_gclip_against_float64(be, arena, decay):
    A = arena
    ovr, ep, G, c = balanced(A, "fin")
    S, P = fin_state(be, A, ovr, ep), fin_state(be, A, ovr, ep)
    wd = dev(A.wd) if decay else None
    gsq = torch.zeros(1, device="cuda")
    gsq_launch(be, S, A, "fin", gsq)
    fin_gclip(be, A, S, desc(be, A, S), c, gsq, wd)
    sp = A.sp
    be.adam_fin(P["th"], P["m"], P["v"], P["gr"], sp.span_seg, sp.span_off, sp.span_len, P["ovr"], sp.nspan, EPS, 0.1,
                desc(be, A, P))
    torch.cuda.synchronize()
    assert abs(float(gsq) - G) <= gsq_rel_bound(A.nseg) * G
    want = ref_update(A, clip_scale(G, c), "adam", wd=A.wd if decay else None)
    check_update(A, host(S, "th", "m", "v"), want, before=[A.theta, A.m0, A.v0])
    for k in SIDE:                                    # the side workgroup files what the plain fin launch files, bit for bit
        assert torch.equal(S[k], P[k]), k
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41 and int(S["arrive"].abs().sum()) == 0
    assert torch.equal(S["gr"], dev(A.grad)) and float(gsq) > 0


def ring_args(A, X, c):
    sp = A.sp
    return (X["th"], X["m"], X["v"], X["gr"], sp.span_seg, sp.span_off, sp.span_len, X["l2"], X["sq"], X["ovr"], sp.nspan, 0.0,
            X["lr_t"], B1, B2, EPS, c)


def sgd_args(A, X):
    sp = A.sp
    return (X["th"], X["m"], X["gr"], sp.span_seg, sp.span_off, sp.span_len, X["l2"], X["sq"], X["ovr"], sp.nspan)


def table_state(be, A, ovr):
    S = plain_state(be, A)
    S["ovr"] = dev(ovr)
    return S


@pytest.mark.parametrize("decay", [False, True])
def test_adam_gclip_against_float64(be, arena, decay):
    A = arena
    ovr, _, G, c = balanced(A, "table")
    S = table_state(be, A, ovr)
    gsq = torch.zeros(1, device="cuda")
    gsq_launch(be, S, A, "table", gsq)
    kw = dict(lr=S["lr"], seg_wd=dev(A.wd)) if decay else {}
    be.adam_gclip(*ring_args(A, S, c), gsq, guard=S["guard"], **kw)
    torch.cuda.synchronize()
    assert abs(float(gsq) - G) <= gsq_rel_bound(A.nseg) * G
    want = ref_update(A, clip_scale(G, c), "adam", lr_t=np.float32(lr_t_of(7)), wd=A.wd if decay else None)
    check_update(A, host(S, "th", "m", "v"), want, before=[A.theta, A.m0, A.v0])


@pytest.mark.parametrize("decay", [False, True])
def test_sgd_gclip_against_float64(be, arena, decay):
    A = arena
    ovr, _, G, c = balanced(A, "table")
    S = table_state(be, A, ovr)
    gsq = torch.zeros(1, device="cuda")
    gsq_launch(be, S, A, "table", gsq)
    be.sgd_gclip(*sgd_args(A, S), 0.0, S["lr"], MU, c, gsq, seg_wd=dev(A.wd) if decay else None, guard=S["guard"])
    torch.cuda.synchronize()
    th1, mom1, _ = ref_update(A, clip_scale(G, c), "sgd", wd=A.wd if decay else None)
    check_update(A, host(S, "th", "m"), (th1, mom1), before=[A.theta, A.m0])


# ------------------------------------------------------------------------------------------ the encoder kernel
def enc_run(be, c, shape, form, clip, gsq=None, decay=None, tripped=False, lam=F32(0.01), lr_t=F32(3e-4), partial=None, span=None, sq=None):
    th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
    guard = torch.full((1,), int(tripped), dtype=torch.int32, device="cuda")
    N, E, Bk, ldx = shape
    head = (c.xd, c.dd, th, m, v, lam) + ((partial, *span) if form == "fin" else (sq,))
    tail = (dev([-1.0]), dev([lr_t]), B1, B2, EPS, clip, N, E, Bk, ldx)
    kw = dict(lr=dev([LR]), wd=decay) if decay is not None else {}
    if gsq is None and form == "fin":
        be.dense_dw_adam_fin(*head, *tail, guard=guard)
    elif gsq is None:
        be.dense_dw_adam(*head, *tail, guard=guard)
    elif form == "fin":
        be.dense_dw_adam_fin_gclip(*head, *tail, gsq, guard=guard, **kw)
    else:
        be.dense_dw_adam_gclip(*head, *tail, gsq, guard=guard, **kw)
    torch.cuda.synchronize()
    return th, m, v


@pytest.mark.parametrize("form", ["fin", "sq"])
@pytest.mark.parametrize("decay", [None, 0.05])
@pytest.mark.parametrize("N,E,Bk,ldx", ENC_SHAPES)
def test_dense_dw_adam_gclip(be, enc_case, N, E, Bk, ldx, decay, form):
    """tnt_dense_dw_adam_fin_gclip_f32 / tnt_dense_dw_adam_gclip_f32 as test_gpu_weight_decay.test_dense_dw_adamw argues: g is
    the kernel's own float32 product, everything behind it float64.  The global word is the variable's own norm times 16
    (other variables hold 15/16 of G), the threshold a quarter of the global norm: cs = 0.25, the own-norm scale 1."""
    from masters_thesis_amd.arena import build_spans
    c = enc_case(N, E, Bk, ldx)
    shape = (N, E, Bk, ldx)
    lam, lr_t = F32(0.01), F32(3e-4)
    nslot, k0 = build_spans([0], [N * E], device="cpu").nspan, 3
    partial = torch.full((2 * (k0 + nslot + 5),), 7.0, device="cuda")
    be.dense_dw_sqnorm(c.xd, c.dd, dev(c.theta), lam, partial[2 * k0:], nslot, N, E, Bk, ldx)
    sq = partial[2 * k0:2 * (k0 + nslot):2].sum().reshape(1)
    th64 = c.theta.astype(np.float64)
    q = float(((c.g64 + 2 * lam * th64) ** 2).sum())
    G = F32(16 * q)
    clip = F32(0.25 * np.sqrt(G))
    cs = clip_scale(G, clip)
    assert 0.1 <= cs <= 0.5 and clip / max(np.sqrt(q), clip) >= 2 * cs
    gsq = dev([G])
    common = dict(partial=partial, span=(k0, k0 + nslot), sq=sq)
    th, m, v = enc_run(be, c, shape, form, clip, gsq, decay, **common)
    ge = (c.gk + 2 * lam * th64) * cs
    _, mw, vw = O.adam_update(th64, c.m0.astype(np.float64), c.v0.astype(np.float64), ge, 1, 1.0, B1, B2, EPS)
    tw = (th64 - lr_t * mw / (np.sqrt(vw) + EPS)) - (float(LR) * (decay or 0.0)) * th64
    close(m, mw, rtol=1e-5); close(v, vw, rtol=1e-5); close(th, tw, rtol=1e-6)
    # inactive (G <= c^2): the bits of the plain entry without clipping, decay apart
    if decay is None:
        small = enc_run(be, c, shape, form, 2.0, dev([4.0]), None, **common)        # G == c^2: the edge
        plain = enc_run(be, c, shape, form, 0.0, None, **common)
        for a, b in zip(small, plain):
            assert torch.equal(a, b)
    held = enc_run(be, c, shape, form, clip, gsq, decay, tripped=True, **common)
    for a, h in zip(held, (c.theta, c.m0, c.v0)):
        assert torch.equal(a, dev(h))
    assert float(partial[:2 * k0].max()) == 7.0 and float(partial[2 * (k0 + nslot):].min()) == 7.0


# ------------------------------------------------------------------------------------------ inactive clipping, the guard
def test_inactive_clipping_gives_the_plain_launch_without_clipping(be, arena):
    """G <= c^2: cs == 1.0f exactly, so each gclip entry writes the bits of its plain sibling at clipnorm = 0"""
    A = arena
    sp = A.sp
    c = 3.0
    gsq = dev([F32(c * c)])                                               # G == c^2: the edge
    S, P = fin_state(be, A), fin_state(be, A)
    fin_gclip(be, A, S, desc(be, A, S), c, gsq)
    be.adam_fin(P["th"], P["m"], P["v"], P["gr"], sp.span_seg, sp.span_off, sp.span_len, P["ovr"], sp.nspan, EPS, 0.0,
                desc(be, A, P))
    torch.cuda.synchronize()
    for k in ("th", "m", "v") + SIDE:
        assert torch.equal(S[k], P[k]), k
    S, P = plain_state(be, A), plain_state(be, A)
    be.adam_gclip(*ring_args(A, S, c), gsq, guard=S["guard"])
    be.adam(*ring_args(A, P, 0.0), guard=P["guard"])
    S2, P2 = plain_state(be, A), plain_state(be, A)
    be.sgd_gclip(*sgd_args(A, S2), 0.0, S2["lr"], MU, c, gsq, guard=S2["guard"])
    be.sgd(*sgd_args(A, P2), 0.0, P2["lr"], MU, 0.0, guard=P2["guard"])
    # ... and with decay, the decaying sibling's
    S3, P3 = plain_state(be, A), plain_state(be, A)
    be.adam_gclip(*ring_args(A, S3, c), gsq, lr=S3["lr"], seg_wd=dev(A.wd), guard=S3["guard"])
    be.adamw(*ring_args(A, P3, 0.0), P3["lr"], dev(A.wd), guard=P3["guard"])
    torch.cuda.synchronize()
    for X, Y in ((S, P), (S2, P2), (S3, P3)):
        for k in ("th", "m", "v"):
            assert torch.equal(X[k], Y[k]), k


def test_tripped_guard_leaves_the_state(be, arena):
    A = arena
    gsq, c = dev([100.0]), 1.0
    S = state(A)
    S["guard"][0] = 1
    norm_launch(be, A, S)
    fin_gclip(be, A, S, desc(be, A, S), c, gsq, dev(A.wd))
    R, G = plain_state(be, A), plain_state(be, A)
    R["guard"][0] = 1; G["guard"][0] = 1
    be.adam_gclip(*ring_args(A, R, c), gsq, lr=R["lr"], seg_wd=dev(A.wd), guard=R["guard"])
    be.sgd_gclip(*sgd_args(A, G), 0.0, G["lr"], MU, c, gsq, guard=G["guard"])
    torch.cuda.synchronize()
    for X in (S, R, G):
        for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
            assert torch.equal(X[k], dev(h)), k
    assert int(S["adam_t"]) == 6 and int(S["drop"]) == 40 and int(S["arrive"].abs().sum()) == 0


# ------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_badarg_without_a_launch(be, arena, enc_case):
    from masters_thesis_amd.ops import _p
    A, lib, s = arena, be.lib, be._s()
    sp = A.sp
    S = plain_state(be, A)
    fin, good = desc(be, A, S), dev([4.0])
    spans = (_p(sp.span_seg), _p(sp.span_off), _p(sp.span_len))
    N, E, Bk, ldx = ENC_SHAPES[1]
    c = enc_case(N, E, Bk, ldx)
    th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
    one, part = dev([1.0]), torch.ones(64, device="cuda")
    ring = lambda g, cl: lib.tnt_adam_gclip_f32(_p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]),
                                                _p(S["ovr"]), sp.nspan, 0.0, _p(S["lr_t"]), B1, B2, EPS, cl, None, None, 0, None, 0,
                                                None, g, None, None, s)
    finl = lambda g, cl: lib.tnt_adam_fin_gclip_f32(_p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["ovr"]), sp.nspan,
                                                    EPS, cl, ctypes.addressof(fin), None, 0, None, 0, None, g, None, s)
    sgd = lambda g, cl: lib.tnt_sgd_gclip_f32(_p(S["th"]), _p(S["m"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]), _p(S["ovr"]),
                                              sp.nspan, 0.0, _p(S["lr"]), 0.9, cl, None, g, None, s)
    enc = lambda g, cl: lib.tnt_dense_dw_adam_gclip_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(one), None, _p(one), B1, B2,
                                                        EPS, cl, None, N, E, Bk, ldx, g, None, 0.0, s)
    encf = lambda g, cl: lib.tnt_dense_dw_adam_fin_gclip_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(part), 0, 14, None,
                                                             _p(one), B1, B2, EPS, cl, None, N, E, Bk, ldx, g, None, 0.0, s)
    bad = [(None, 1.0)] + [(_p(good), x) for x in (0.0, -1.0, float("nan"), float("inf"), -float("inf"))]
    for f in (ring, finl, sgd, enc, encf):
        for g, cl in bad:
            rc = f(g, cl)
            assert rc <= -1000, (rc, cl)
    # a decay without its learning rate; a reduction without an output, with both forms or with neither
    assert lib.tnt_adam_gclip_f32(_p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]), _p(S["ovr"]),
                                  sp.nspan, 0.0, _p(S["lr_t"]), B1, B2, EPS, 1.0, None, None, 0, None, 0, None, _p(good), None,
                                  _p(dev(A.wd)), s) <= -1000
    gs = lambda partial, sq, out: lib.tnt_global_sqnorm_f32(partial, _p(sp.seg_first), sq, _p(S["ovr"]), None, 0, -1, A.nseg, out, s)
    for rc in (gs(_p(S["partial"]), None, None), gs(_p(S["partial"]), _p(S["sq"]), _p(good)), gs(None, None, _p(good))):
        assert rc <= -1000, rc
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):                  # nothing was launched
        assert torch.equal(S[k], dev(h)), k
    assert torch.equal(th, dev(c.theta)) and torch.equal(m, dev(c.m0)) and torch.equal(v, dev(c.v0))
    assert int(S["adam_t"]) == 6 and int(S["arrive"].abs().sum()) == 0 and float(good) == 4.0
    assert lib.tnt_version() >= 125


# ------------------------------------------------------------------------------------------ captured replay
def test_a_captured_launch_reads_the_live_word(be, arena):
    """tnt_adam_gclip_f32 captured once; gsq overwritten between the replays: every replay scales by the word present then"""
    A = arena
    S = plain_state(be, A)
    c = 1.0
    gsq = dev([4.0])
    launch = lambda: be.adam_gclip(*ring_args(A, S, c), gsq, guard=S["guard"])
    launch()                                                                  # warm-up outside the capture
    torch.cuda.synchronize()
    prev = host(S, "th", "m", "v")
    lr_t = np.float32(lr_t_of(7))
    check_update(A, prev, ref_update(A, 0.5, "adam", lr_t=lr_t))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    torch.cuda.synchronize()
    assert torch.equal(S["th"], dev(prev[0]))                                 # capturing runs nothing
    for word, cs in ((16.0, 0.25), (0.25, 1.0), (100.0, 0.1)):
        gsq.fill_(word)
        g.replay()
        torch.cuda.synchronize()
        got = host(S, "th", "m", "v")
        check_update(A, got, ref_update(A, cs, "adam", lr_t=lr_t, th_m_v=prev), before=prev)
        prev = got
