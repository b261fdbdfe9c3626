"""The optimizer step's tail on a real MI355X: the fused clip + Adam launch that ends every default Adam training step
(tnt_adam_fin_f32: span workgroups, the side workgroup, the last-arrival tick), the fused update of the dense encoder
kernel (tnt_dense_dw_adam_fin_f32), the norm launches in front of them, and the remaining optimizer kernels (SGD, SAM,
AGC), each against plain float64 numpy.  Tolerances as in test_gpu_ops.test_optimizer (theta 1e-6, moments 1e-5
relative, per variable); integer outputs, counters, copies and state that must stay untouched are compared bit-exact."""
import types

import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))
B1, B2, EPS, LR = F32(0.9), F32(0.98), 1e-8, F32(1e-3)
OVR_SEG, EXTRA_SEG = 6, 8          # a variable whose clip norm is supplied (sq_override >= 0); the Embedding's sparse norm


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def lr_t_of(t):
    """Adam's bias-corrected step size for step t (float64; beta / lr as the float32 values the kernels get)"""
    return LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)


def make_arena(seed, nvar=300):
    """~300 variables (nseg > 256: both strides of the side workgroup), lengths around the float4 / AF_U / SPAN edges and
    two variables of more than 8 spans (one behind variable 256), laid out like ParamArena (64-float slots)."""
    from masters_thesis_amd.arena import build_spans
    rng = np.random.default_rng(seed)
    lens = [1, 3, 4, 5, 4095, 4097, 8191, 8192, 8193, 9 * 8192 + 3]
    lens += [int(n) for n in rng.integers(1, 300, nvar - len(lens))]
    if nvar >= 300:
        lens[270] = 8 * 8192 + 1                                  # 9 spans, in the side workgroup's second round of waves
        lens[299] = 3 * 4096 + 2
    l2 = [0.0 if s % 3 == 0 else float(rng.choice([0.01, 3e-5, 1e-3])) for s in range(nvar)]
    offs, total = [], 0
    for n in lens:
        offs.append(total)
        total += (n + 63) // 64 * 64
    theta, grad, m0, v0 = (np.zeros(total, np.float32) for _ in range(4))
    for o, n in zip(offs, lens):
        theta[o:o + n] = rng.standard_normal(n); grad[o:o + n] = rng.standard_normal(n) * 0.01
        m0[o:o + n] = rng.standard_normal(n) * 0.01; v0[o:o + n] = rng.random(n) * 1e-4
    ovr = np.full(nvar, -1.0, np.float32)
    ovr[OVR_SEG] = 2.5
    ovr[EXTRA_SEG] = 123.0                   # never read: the Embedding's norm comes from extra_part
    A = types.SimpleNamespace(lens=lens, offs=offs, l2=np.array(l2, np.float32), total=total, nseg=nvar, theta=theta,
                              grad=grad, m0=m0, v0=v0, ovr=ovr, sp=build_spans(offs, lens, device="cuda"))
    A.mask = np.zeros(total, bool)
    for o, n in zip(offs, lens):
        A.mask[o:o + n] = True
    # the side workgroup's jobs
    A.x0, A.x1, A.x2 = rng.random(960).astype(np.float32), (rng.random(960) < 0.4).astype(np.float32), rng.random(77).astype(np.float32)
    A.extra_part = (rng.random(300) * 1e-3).astype(np.float32)
    A.ids = rng.integers(0, 5000, 1000).astype(np.int32)
    return A


def state(A):
    return dict(th=dev(A.theta), m=dev(A.m0), v=dev(A.v0), gr=dev(A.grad), l2=dev(A.l2), ovr=dev(A.ovr),
                partial=torch.full((2 * A.sp.nspan,), 7.0, device="cuda"),
                sq=torch.full((A.nseg,), -7.0, device="cuda"), wsq=torch.full((A.nseg,), -7.0, device="cuda"),
                l2o=torch.full((1,), -7.0, device="cuda"), o0=torch.full((1,), -7.0, device="cuda"),
                o1=torch.full((1,), -7.0, device="cuda"), o2=torch.full((1,), -7.0, device="cuda"),
                extra=torch.full((1,), -7.0, device="cuda"), x0=dev(A.x0), x1=dev(A.x1), x2=dev(A.x2), ep=dev(A.extra_part),
                ids=dev(A.ids, torch.int32), ids_dst=torch.full((len(A.ids) + 8,), -1, dtype=torch.int32, device="cuda"),
                adam_t=torch.full((1,), 6, dtype=torch.int64, device="cuda"),
                drop=torch.full((1,), 40, dtype=torch.int32, device="cuda"), lr=dev([LR]),
                lr_t=torch.zeros(1, device="cuda"), guard=torch.zeros(1, dtype=torch.int32, device="cuda"),
                arrive=torch.zeros(16, dtype=torch.int32, device="cuda"))


def desc(be, A, S, extra=True):
    """finalize_desc with every optional job on"""
    kw = dict(extra_part=S["ep"], extra=S["extra"], n_extra=len(A.extra_part), extra_seg=EXTRA_SEG) if extra else {}
    return be.finalize_desc(S["partial"], A.sp.seg_first, S["l2"], S["sq"], S["wsq"], S["l2o"], A.nseg, S["arrive"],
                            x0=S["x0"], out0=S["o0"], x1=S["x1"], out1=S["o1"], n=960, scale=1 / 960, ids_src=S["ids"],
                            ids_dst=S["ids_dst"], n_ids=len(A.ids), adam_t=S["adam_t"], drop_step=S["drop"], lr=S["lr"],
                            lr_t=S["lr_t"], beta1=B1, beta2=B2, guard=S["guard"], x2=S["x2"], out2=S["o2"], n2=77, scale2=0.5,
                            **kw)


def norm_launch(be, A, S, skip=True):
    sp = A.sp
    be.span_sqnorm_lr(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], S["partial"], sp.nspan, S["adam_t"],
                      S["lr"], S["lr_t"], B1, B2, skip=S["ovr"] if skip else None)


def fin_launch(be, A, S, fin, clip, nspan=None, **ring):
    sp = A.sp
    be.adam_fin(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["ovr"],
                sp.nspan if nspan is None else nspan, EPS, clip, fin, **ring)


def host(S, *keys):
    return [S[k].cpu().numpy().astype(np.float64) for k in keys]


def ref_adam(A, th, m, v, t, clip, extra=True):
    """float64 clip + L2 + Adam of every variable from the float32 state (th, m, v); returns the new (th, m, v)"""
    th1, m1, v1 = th.copy(), m.copy(), v.copy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        w = th[o:o + n]
        g = A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w
        if clip > 0:
            if s == EXTRA_SEG and extra:
                q = A.extra_part.astype(np.float64).sum()
            elif A.ovr[s] >= 0:
                q = float(A.ovr[s])
            else:
                q = (g * g).sum()
            g = g * clip / max(np.sqrt(q), clip)
        th1[o:o + n], m1[o:o + n], v1[o:o + n] = O.adam_update(w, m[o:o + n], v[o:o + n], g, t, LR, B1, B2, EPS)
    return th1, m1, v1


def check_update(A, got, want, before=None):
    """per variable: theta 1e-6, m / v 1e-5 relative; the padding between the variables untouched (bit-exact)"""
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        for k, (g_, w_) in enumerate(zip(got, want)):
            try:
                close(g_[o:o + n], w_[o:o + n], rtol=1e-6 if k == 0 else 1e-5)
            except AssertionError as e:
                raise AssertionError(f"variable {s} (length {n}), {'theta m v'.split()[k]}: {e}") from None
    if before is not None:
        for g_, b_ in zip(got, before):
            assert np.array_equal(g_[~A.mask], b_[~A.mask])


def check_side(A, S, th, skip=True, extra=True):
    """the side workgroup's outputs against float64 (th: the theta the norm launch read)"""
    sq, wsq, l2o, o0, o1, o2, ex = host(S, "sq", "wsq", "l2o", "o0", "o1", "o2", "extra")
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        w = th[o:o + n]
        g = A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w
        want_q = 0.0 if skip and A.ovr[s] >= 0 else (g * g).sum()          # a supplied norm: no gradient pass, slot 0
        want_w = 0.0 if skip and A.l2[s] == 0 else (w * w).sum()           # no regulariser: no theta pass, slot 0
        assert abs(sq[s] - want_q) <= 1e-5 * want_q, (s, sq[s], want_q)
        assert abs(wsq[s] - want_w) <= 1e-5 * want_w, (s, wsq[s], want_w)
    want_l2 = sum(float(A.l2[s]) * (th[o:o + n] ** 2).sum() for s, (o, n) in enumerate(zip(A.offs, A.lens)))
    assert abs(l2o[0] - want_l2) <= 1e-5 * want_l2
    for got, want in ((o0, A.x0.astype(np.float64).sum() / 960), (o1, A.x1.astype(np.float64).sum() / 960),
                      (o2, 0.5 * A.x2.astype(np.float64).sum())):
        assert abs(got[0] - want) <= 1e-5 * want, (got, want)
    if extra:
        want = A.extra_part.astype(np.float64).sum()
        assert abs(ex[0] - want) <= 1e-5 * want
    ids = S["ids_dst"].cpu().numpy()
    assert np.array_equal(ids[:len(A.ids)], A.ids) and (ids[len(A.ids):] == -1).all()


# ------------------------------------------------------------------------------------------ (a) norm launch + adam_fin
@pytest.mark.parametrize("clip", [0.1, 0.0])
def test_adam_fin_against_float64(be, clip):
    A = make_arena(21)
    S = state(A)
    fin = desc(be, A, S)
    norm_launch(be, A, S)
    fin_launch(be, A, S, fin, clip)
    torch.cuda.synchronize()
    t = 7                                                              # adam_t was 6: this is step 7
    want = ref_adam(A, A.theta.astype(np.float64), A.m0.astype(np.float64), A.v0.astype(np.float64), t, clip)
    check_update(A, host(S, "th", "m", "v"), want, before=[A.theta, A.m0, A.v0])
    check_side(A, S, A.theta.astype(np.float64))
    assert abs(float(S["lr_t"]) - lr_t_of(t)) <= 1e-6 * lr_t_of(t)
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41
    assert int(S["arrive"].abs().sum()) == 0
    assert torch.equal(S["gr"], dev(A.grad)) and torch.equal(S["ovr"], dev(A.ovr))


# ------------------------------------------------------------------------------------------ (b) fused == unfused
@pytest.mark.parametrize("clip", [0.1, 0.0])
def test_adam_fin_equals_finalize_then_adam(be, clip):
    """span_sqnorm_lr + adam_fin against span_sqnorm + step_finalize + adam: both sum each variable's clip norm from the
    same span partials in the tnt_seg_sums order and take the same lr_t, so theta / m / v (and the filed norms sq / wsq)
    are bit-identical.  The Embedding's norm (extra_part) is handed to the unfused update through sq_override, as the
    fused launch's own total of it."""
    A = make_arena(22)
    S = state(A)
    norm_launch(be, A, S, skip=False)
    fin_launch(be, A, S, desc(be, A, S), clip)
    U = state(A)
    sp = A.sp
    be.span_sqnorm(U["th"], U["gr"], sp.span_seg, sp.span_off, sp.span_len, U["l2"], U["partial"], sp.nspan)
    be.step_finalize(U["partial"], sp.seg_first, U["l2"], U["sq"], U["wsq"], U["l2o"], A.nseg, x0=U["x0"], out0=U["o0"],
                     x1=U["x1"], out1=U["o1"], n=960, scale=1 / 960, extra_part=U["ep"], extra=U["extra"],
                     n_extra=len(A.extra_part), ids_src=U["ids"], ids_dst=U["ids_dst"], n_ids=len(A.ids), adam_t=U["adam_t"],
                     drop_step=U["drop"], lr=U["lr"], lr_t=U["lr_t"], beta1=B1, beta2=B2, guard=U["guard"], x2=U["x2"],
                     out2=U["o2"], n2=77, scale2=0.5)
    ovr_u = U["ovr"].clone()
    ovr_u[EXTRA_SEG] = S["extra"][0]
    be.adam(U["th"], U["m"], U["v"], U["gr"], sp.span_seg, sp.span_off, sp.span_len, U["l2"], U["sq"], ovr_u, sp.nspan, 0.0,
            U["lr_t"], B1, B2, EPS, clip, guard=U["guard"])
    torch.cuda.synchronize()
    assert torch.equal(S["partial"], U["partial"])
    assert torch.equal(S["lr_t"], U["lr_t"])
    for k in ("th", "m", "v", "sq", "wsq", "ids_dst", "adam_t", "drop"):
        assert torch.equal(S[k], U[k]), k


# ------------------------------------------------------------------------------------------ (c) repeated launches
def test_adam_fin_repeated_launches_and_graph_replays(be):
    """3 eager launches of the norm + adam_fin pair, then a captured graph of the pair replayed twice: every step against
    float64 (from the state the step started from), the ticket back at 0 and the counters one further after each."""
    A = make_arena(23)
    S = state(A)
    fin = desc(be, A, S)
    clip = 0.1
    pair = lambda: (norm_launch(be, A, S), fin_launch(be, A, S, fin, clip))

    def check(step, prev):
        got = host(S, "th", "m", "v")
        t = 6 + step
        check_update(A, got, ref_adam(A, *prev, t, clip), before=prev)
        check_side(A, S, prev[0])
        assert int(S["adam_t"]) == t and int(S["drop"]) == 40 + step, (step, int(S["adam_t"]), int(S["drop"]))
        assert int(S["arrive"].abs().sum()) == 0, S["arrive"]
        assert abs(float(S["lr_t"]) - lr_t_of(t)) <= 1e-6 * lr_t_of(t)
        return got

    prev = host(S, "th", "m", "v")
    for step in (1, 2, 3):
        pair()
        torch.cuda.synchronize()
        prev = check(step, prev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    torch.cuda.synchronize()
    assert torch.equal(S["th"], dev(prev[0])) and int(S["adam_t"]) == 9      # capturing runs nothing
    for step in (4, 5):
        g.replay()
        torch.cuda.synchronize()
        prev = check(step, prev)


# ------------------------------------------------------------------------------------------ (d) guard
def test_adam_fin_guard(be):
    """A tripped guard leaves theta / m / v bit-identical and the counters where they are, re-arms the ticket, and still
    files the side workgroup's outputs and the metrics-ring row (what mock_backend models); cleared, the next launch
    ticks once and matches float64."""
    A = make_arena(24)
    S = state(A)
    met = dev(np.arange(1, 6, dtype=np.float32))
    ring, ring_t = torch.full((3, 6), -7.0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    fin = desc(be, A, S)
    S["guard"][0] = 1
    norm_launch(be, A, S)
    fin_launch(be, A, S, fin, 0.1, met=met, ring=ring, ring_t=ring_t)
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
        assert torch.equal(S[k], dev(h)), k
    assert int(S["adam_t"]) == 6 and int(S["drop"]) == 40
    assert int(S["arrive"].abs().sum()) == 0
    check_side(A, S, A.theta.astype(np.float64))
    assert int(ring_t) == 1 and torch.equal(ring[0], dev([1, 2, 3, 4, 5, 0])) and float(ring[1:].max()) == -7.0
    S["guard"][0] = 0
    for k in ("sq", "wsq", "l2o", "o0", "o1", "o2", "extra"):
        S[k].fill_(-7.0)
    norm_launch(be, A, S)
    fin_launch(be, A, S, fin, 0.1, met=met, ring=ring, ring_t=ring_t)
    torch.cuda.synchronize()
    want = ref_adam(A, A.theta.astype(np.float64), A.m0.astype(np.float64), A.v0.astype(np.float64), 7, 0.1)
    check_update(A, host(S, "th", "m", "v"), want, before=[A.theta, A.m0, A.v0])
    check_side(A, S, A.theta.astype(np.float64))
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41 and int(S["arrive"].abs().sum()) == 0
    assert int(ring_t) == 2 and torch.equal(ring[1], dev([1, 2, 3, 4, 5, 1]))


# ------------------------------------------------------------------------------------------ (e) metrics ring
@pytest.mark.parametrize("kind", ["adam_fin", "adam"])
@pytest.mark.parametrize("t0", [0, 0xFFFFFE])
def test_metrics_ring(be, kind, t0):
    """ring_rows = 3 over 5 launches: row rt % 3 holds the launch's metrics vector and rt & 0xFFFFFF, ring_t advances once
    per launch (from 0, and across the 24-bit wrap of the tag column)."""
    A = make_arena(25, nvar=40)
    S = state(A)
    sp = A.sp
    nmet = 5
    met = torch.zeros(nmet, device="cuda")
    ring = torch.full((3, nmet + 1), -7.0, device="cuda")
    ring_t = torch.full((1,), t0, dtype=torch.int32, device="cuda")
    fin = desc(be, A, S)
    mets = {}
    for k in range(5):
        mets[t0 + k] = np.float32([k + 0.5, -k, 1e3 * k, 7, 0.25 * k])
        met.copy_(dev(mets[t0 + k]))
        if kind == "adam_fin":
            norm_launch(be, A, S)
            fin_launch(be, A, S, fin, 0.1, met=met, ring=ring, ring_t=ring_t)
        else:
            be.adam(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], S["sq"], S["ovr"],
                    sp.nspan, 1e-4, None, B1, B2, EPS, 0.0, met=met, ring=ring, ring_t=ring_t)
        torch.cuda.synchronize()
        rt = t0 + k
        assert int(ring_t) == rt + 1
        assert torch.equal(ring[rt % 3], dev(np.append(mets[rt], np.float32(rt & 0xFFFFFF)))), (k, ring)
    assert int(ring_t) == t0 + 5
    for rt in range(t0 + 2, t0 + 5):                                 # the last three launches, each in its row
        assert torch.equal(ring[rt % 3], dev(np.append(mets[rt], np.float32(rt & 0xFFFFFF))))
    if kind == "adam_fin":
        assert int(S["adam_t"]) == 11 and int(S["arrive"].abs().sum()) == 0


# ------------------------------------------------------------------------------------------ (f) nspan == 0
def test_adam_fin_without_spans(be):
    """nspan == 0: the launch is the side workgroup alone; its outputs are right, the counters tick, nothing else moves"""
    A = make_arena(26)
    S = state(A)
    sp = A.sp
    be.span_sqnorm(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], S["partial"], sp.nspan)
    fin_launch(be, A, S, desc(be, A, S), 0.1, nspan=0)
    torch.cuda.synchronize()
    check_side(A, S, A.theta.astype(np.float64), skip=False)
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
        assert torch.equal(S[k], dev(h)), k
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41 and int(S["arrive"].abs().sum()) == 0


# ------------------------------------------------------------------------------------------ (g) dense_dw_adam_fin
@pytest.mark.parametrize("N,E,Bk,ldx,mode", [(20000, 512, 64, 20000, "clip"), (999, 512, 33, 1000, "clip"),
                                             (999, 512, 33, 1000, "override"), (999, 512, 33, 1000, "noclip"),
                                             (112, 1024, 7, 112, "override"), (112, 1024, 7, 112, "clip")])
def test_dense_dw_adam_fin(be, N, E, Bk, ldx, mode):
    """The encoder kernel's fused update: X^T D in the MFMAs, clip from the variable's span partials partial[k0:k1] (summed
    in the canonical order), L2 + Adam, against float64; sq_override >= 0 replaces the partials, clipnorm = 0 ignores
    them, a tripped guard leaves the state bit-identical."""
    from masters_thesis_amd.arena import build_spans
    rng = np.random.default_rng(N + E + len(mode))
    lam, clip = F32(0.01), (0.0 if mode == "noclip" else 0.1)
    x = np.zeros((Bk, ldx), np.float32); x[:, :N] = rng.standard_normal((Bk, N))
    dpre = (rng.standard_normal((Bk, E)) * 0.01).astype(np.float32)
    theta = (rng.standard_normal((N, E)) * 0.05).astype(np.float32)
    m0, v0 = (rng.standard_normal((N, E)) * 1e-3).astype(np.float32), (rng.random((N, E)) * 1e-6).astype(np.float32)
    nslot, k0 = build_spans([0], [N * E], device="cpu").nspan, 3         # the variable's slots behind 3 other spans
    partial = torch.full((2 * (k0 + nslot + 5),), 7.0, device="cuda")
    th, m, v, xd, dd = dev(theta), dev(m0), dev(v0), dev(x), dev(dpre)
    be.dense_dw_sqnorm(xd, dd, th, lam, partial[2 * k0:], nslot, N, E, Bk, ldx)
    ovr = dev([4.0 if mode == "override" else -1.0])
    lr_t = dev([3e-4])
    guard = torch.ones(1, dtype=torch.int32, device="cuda")
    args = (xd, dd, th, m, v, lam, partial, k0, k0 + nslot, ovr, lr_t, B1, B2, EPS, clip, N, E, Bk, ldx)
    be.dense_dw_adam_fin(*args, guard=guard)
    torch.cuda.synchronize()
    assert torch.equal(th, dev(theta)) and torch.equal(m, dev(m0)) and torch.equal(v, dev(v0))
    guard[0] = 0
    be.dense_dw_adam_fin(*args, guard=guard)
    torch.cuda.synchronize()
    # The update is taken from the kernel's own float32 product X^T D (the same MFMA accumulation, written out by
    # dense_dw_skinny; against float64 in test_gpu_ops.test_dense_dw_skinny): with m0 ~ 1e-3 and v0 down to ~1e-10,
    # m / sqrt(v) reaches ~50 and the float32 rounding of the product alone (6.6e-9 on g = -8.6e-5, the accumulation of
    # Bk float32 products) moves theta by 3.1e-7 where the 1e-6 bound is 2.6e-7.  Everything behind the product
    # (L2, clip, Adam) is float64 here.
    gk = torch.zeros(N, E, device="cuda")
    be.dense_dw_skinny(xd, dd, gk, N, E, Bk, ldx)
    g64 = x[:, :N].astype(np.float64).T @ dpre.astype(np.float64)
    close(gk, g64)
    ge = gk.cpu().numpy().astype(np.float64) + 2 * lam * theta.astype(np.float64)
    q = 4.0 if mode == "override" else ((g64 + 2 * lam * theta) ** 2).sum()
    if clip > 0:
        ge = ge * clip / max(np.sqrt(q), clip)
    tw, mw, vw = O.adam_update(theta.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), ge, 1, 1.0, B1, B2, EPS)
    tw = theta - F32(3e-4) * mw / (np.sqrt(vw) + EPS)                     # lr_t is given (3e-4), not derived from t
    close(m, mw, rtol=1e-5); close(v, vw, rtol=1e-5); close(th, tw, rtol=1e-6)
    assert float(partial[:2 * k0].max()) == 7.0 and float(partial[2 * (k0 + nslot):].min()) == 7.0


# ------------------------------------------------------------------------------------------ (h) Gram norm with span jobs
@pytest.mark.parametrize("B,K,E", [(5, 64, 512), (33, 1600, 1024)])
def test_dense_gram_norm_with_span_jobs(be, B, K, E):
    """dense_gram_norm(spans=...) and (spans=..., lr_job=...): the encoder's slots equal the plain Gram-norm launch's, the
    other variables' span partials equal span_sqnorm's / span_sqnorm_lr's (bit-exact: same tnt_span_norm), lr_t is step
    t + 1's and the counter is not touched."""
    rng = np.random.default_rng(B + K)
    lam, ns = F32(0.01), 16
    x, dpre = rng.standard_normal((B, K)), rng.standard_normal((B, E)) * 0.01
    w, bias = rng.standard_normal((K, E)) / np.sqrt(K), 0.1 * rng.standard_normal(E)
    part = torch.zeros(ns * B * E, device="cuda")
    gx, w2 = torch.zeros(ns * 64 * 64, device="cuda"), torch.zeros(ns * (E // 32), device="cuda")
    be.dense_fwd_stream_gram(dev(x), dev(w), part, gx, w2, B, E, K, K, E, ns)
    pre = (part.view(ns, B, E).sum(0) + dev(bias)).contiguous()
    nslot, nw2 = 4 * B + ns * (E // 32) + 3, ns * (E // 32)
    A = make_arena(27, nvar=60)
    S = state(A)
    sp = A.sp
    gargs = (dev(dpre), pre, dev(bias), gx, ns, w2, nw2, lam)
    ref = torch.full((2 * nslot,), 7.0, device="cuda")
    be.dense_gram_norm(*gargs, ref, nslot, B, E)
    span_ref = torch.full((2 * sp.nspan,), 7.0, device="cuda")
    be.span_sqnorm(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], span_ref, sp.nspan)
    span_skip = torch.full((2 * sp.nspan,), 7.0, device="cuda")
    be.span_sqnorm_lr(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], span_skip, sp.nspan, S["adam_t"], S["lr"],
                      S["lr_t"], B1, B2, skip=S["ovr"])
    spans = lambda out: (S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], out, sp.nspan)
    for lr_job, skip, want in ((False, None, span_ref), (True, None, span_ref), (True, S["ovr"], span_skip)):
        got, got_sp = torch.full((2 * nslot,), 7.0, device="cuda"), torch.full((2 * sp.nspan,), 7.0, device="cuda")
        lr_t = torch.zeros(1, device="cuda")
        kw = dict(lr_job=(S["adam_t"], S["lr"], lr_t, B1, B2)) if lr_job else {}
        if skip is not None:
            kw["skip"] = skip
        be.dense_gram_norm(*gargs, got, nslot, B, E, spans=spans(got_sp), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), (lr_job, skip is not None)
        assert torch.equal(got_sp, want), (lr_job, skip is not None)
        if lr_job:
            assert abs(float(lr_t) - lr_t_of(7)) <= 1e-6 * lr_t_of(7)
        else:
            assert float(lr_t) == 0.0
    assert int(S["adam_t"]) == 6


# ------------------------------------------------------------------------------------------ (i) span_sqnorm, l2_total
def test_span_sqnorm_and_l2_total(be):
    A = make_arena(28)
    S = state(A)
    sp = A.sp
    be.span_sqnorm(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], S["partial"], sp.nspan)
    p = S["partial"].cpu().numpy().astype(np.float64).reshape(-1, 2)
    seg, off, ln = (t.cpu().numpy() for t in (sp.span_seg, sp.span_off, sp.span_len))
    for k in range(sp.nspan):
        w = A.theta[off[k]:off[k] + ln[k]].astype(np.float64)
        g = A.grad[off[k]:off[k] + ln[k]] + 2 * float(A.l2[seg[k]]) * w
        for got, want in ((p[k, 0], (g * g).sum()), (p[k, 1], (w * w).sum())):
            assert abs(got - want) <= 1e-5 * want, (k, ln[k], got, want)
    rng = np.random.default_rng(29)
    for nseg in (1, 255, 256, 257, 700):
        wsq, lam = rng.random(nseg).astype(np.float32), (rng.random(nseg) * 0.01).astype(np.float32)
        out = torch.full((2,), -7.0, device="cuda")
        be.l2_total(dev(wsq), dev(lam), nseg, out)
        want = (wsq.astype(np.float64) * lam).sum()
        assert abs(float(out[0]) - want) <= 1e-5 * want and float(out[1]) == -7.0, nseg


# ------------------------------------------------------------------------------------------ SGD
def test_sgd_clip_override_lr_dev_guard(be):
    """clip-by-norm from sq (one variable from sq_override), the step size from lr_dev (the host lr is ignored), momentum;
    a tripped guard leaves theta and the momentum bit-identical"""
    A = make_arena(30)
    S = state(A)
    sp = A.sp
    sq = np.array([((A.grad[o:o + n] + 2 * A.l2[s] * A.theta[o:o + n].astype(np.float64)) ** 2).sum()
                   for s, (o, n) in enumerate(zip(A.offs, A.lens))], np.float32)
    sqd, lr_dev = dev(sq), dev([2e-2])
    S["guard"][0] = 1
    call = lambda: be.sgd(S["th"], S["m"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["l2"], sqd, S["ovr"], sp.nspan,
                          999.0, lr_dev, 0.9, 0.1, guard=S["guard"])
    call()
    torch.cuda.synchronize()
    assert torch.equal(S["th"], dev(A.theta)) and torch.equal(S["m"], dev(A.m0))
    S["guard"][0] = 0
    call()
    torch.cuda.synchronize()
    th, mom = host(S, "th", "m")
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        w = A.theta[o:o + n].astype(np.float64)
        g = A.grad[o:o + n] + 2 * float(A.l2[s]) * w
        q = float(A.ovr[s]) if A.ovr[s] >= 0 else float(sq[s])
        g = g * 0.1 / max(np.sqrt(q), 0.1)
        tw, mw = O.sgd_momentum_update(w, A.m0[o:o + n].astype(np.float64), g, F32(2e-2), F32(0.9))
        close(th[o:o + n], tw, rtol=1e-6); close(mom[o:o + n], mw, rtol=1e-5)
    assert np.array_equal(th[~A.mask], A.theta[~A.mask])


# ------------------------------------------------------------------------------------------ SAM
def test_sam_perturb_and_restore(be):
    """mode 0: ew = rho (g + 2 lambda theta) / ||.|| (sq_override replacing sq where >= 0), theta = float32(w + ew);
    mode 1: theta = float32((w + ew) - ew), and the data gradient takes 2 lambda ew where lambda != 0"""
    A = make_arena(32)
    S = state(A)
    sp = A.sp
    rng = np.random.default_rng(33)
    sq = (rng.random(A.nseg) * 0.1).astype(np.float32)
    rho = F32(0.05)
    ew = torch.full((A.total,), 7.0, device="cuda")
    be.sam(S["th"], S["gr"], ew, sp.span_seg, sp.span_off, sp.span_len, S["l2"], dev(sq), A.nseg, sp.nspan, rho, 0,
           sq_override=S["ovr"])
    torch.cuda.synchronize()
    tot = sum(float(A.ovr[s]) if A.ovr[s] >= 0 else float(sq[s]) for s in range(A.nseg))
    e = ew.cpu().numpy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        g = A.grad[o:o + n] + 2 * float(A.l2[s]) * A.theta[o:o + n].astype(np.float64)
        close(e[o:o + n], rho * g / (np.sqrt(tot) + 1e-12), rtol=1e-5)
    th1 = S["th"].cpu().numpy()
    assert np.array_equal(th1[A.mask], A.theta[A.mask] + e[A.mask])                   # float32 w + ew, bit-exact
    assert np.array_equal(th1[~A.mask], A.theta[~A.mask]) and (e[~A.mask] == 7.0).all()
    assert torch.equal(S["gr"], dev(A.grad))
    be.sam(S["th"], S["gr"], ew, sp.span_seg, sp.span_off, sp.span_len, S["l2"], dev(sq), A.nseg, sp.nspan, rho, 1)
    torch.cuda.synchronize()
    th2, gr2 = S["th"].cpu().numpy(), S["gr"].cpu().numpy()
    assert np.array_equal(th2[A.mask], th1[A.mask] - e[A.mask])                       # float32 (w + ew) - ew, bit-exact
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        if A.l2[s] == 0:
            assert np.array_equal(gr2[o:o + n], A.grad[o:o + n]), s
        else:
            close(gr2[o:o + n], A.grad[o:o + n] + 2 * float(A.l2[s]) * e[o:o + n].astype(np.float64), rtol=1e-6)
    assert np.array_equal(gr2[~A.mask], A.grad[~A.mask])


# ------------------------------------------------------------------------------------------ AGC, colsq
def test_agc_against_adaptive_clip_grad(be):
    """unit-wise adaptive gradient clipping over an arena.AgcTable: rank-1 and rank-2 variables, more rows than
    AgcTable.ROWS (several items per column block), padded storage (the padding never clips), and the Embedding path
    (unit norms of the un-deduplicated rows from colsq, their clipped squared norm in sq_out)"""
    from masters_thesis_amd.arena import AgcTable, ParamArena
    rng = np.random.default_rng(34)
    V, Ee, rows_e = 50, 32, 300
    spec = [("k", (600, 70), (600, 70), 0.01), ("b", (70,), (70,), 0.0), ("b2", (1000,), (1000,), 0.01),
            ("p", (37, 24), (37, 20), 1e-3), ("emb", (V, Ee), (V, Ee), 0.0), ("s", (1,), (1,), 0.0),
            ("k2", (300, 130), (300, 130), 0.0)]
    ar = ParamArena("cuda")
    for name, st, _, lam in spec:
        ar.add(name, st, l2=lam)
    ar.finalize()
    ids = rng.integers(0, V, rows_e)
    drows = rng.standard_normal((rows_e, Ee)) * 10 ** rng.uniform(-4, -1, Ee)
    host_p, host_g = {}, {}
    for name, st, ks, lam in spec:
        w = rng.standard_normal(st) * 0.05
        g = rng.standard_normal(st) * (10 ** rng.uniform(-5, -1, st[-1]) if len(st) == 2 else 10 ** rng.uniform(-5, -1))
        if name == "p":
            w[:, 20:] = 0; g[:, 20:] = 0
        if name == "emb":
            g = np.zeros(st); np.add.at(g, ids, drows)
        host_p[name], host_g[name] = w.astype(np.float32), g.astype(np.float32)
        ar.p(name).copy_(dev(host_p[name])); ar.g(name).copy_(dev(host_g[name]))
    grad0, theta0 = ar.grad.clone(), ar.theta.clone()
    shapes = {name: ks for name, _, ks, _ in spec}
    shapes["p"] = (37, 20)
    for emb in (True, False):
        ar.grad.copy_(grad0)
        tab = AgcTable(ar, shapes, emb_name="emb" if emb else None)
        assert tab.nitem > len(spec) + 4
        gsq, sq_out = None, None
        if emb:
            gsq, sq_out = torch.full((Ee + 3,), -7.0, device="cuda"), torch.full((2,), -7.0, device="cuda")
            be.colsq(dev(drows), gsq, rows_e, Ee, Ee)
        be.agc(ar.theta, ar.grad, tab, gsq, sq_out, 0.01, 1e-3)
        torch.cuda.synchronize()
        for name, st, ks, lam in spec:
            w, g = host_p[name].astype(np.float64), host_g[name].astype(np.float64)
            G = g + 2 * float(np.float32(lam)) * w
            got = ar.g(name).cpu().numpy()
            if name == "emb" and emb:
                rowsc = O.adaptive_clip_grad(w, drows.astype(np.float32).astype(np.float64))
                want = np.zeros(st); np.add.at(want, ids, rowsc)
                assert abs(float(sq_out[0]) - (rowsc ** 2).sum()) <= 1e-5 * (rowsc ** 2).sum()
                assert float(sq_out[1]) == -7.0
            elif name == "p":
                want = np.zeros(st); want[:, :20] = O.adaptive_clip_grad(w[:, :20], G[:, :20]) - 2 * float(np.float32(lam)) * w[:, :20]
                assert (got[:, 20:] == 0).all()
            else:
                want = O.adaptive_clip_grad(w, G) - 2 * float(np.float32(lam)) * w
            # per unit (column of a rank-2 kernel, the whole of a vector): the units' gradients span four decades
            scale = np.abs(want).max(axis=0, keepdims=True) if want.ndim == 2 else np.abs(want).max()
            err = np.abs(got - want)
            assert (err <= 1e-5 * scale + 1e-30).all(), (name, emb, err.max())
        assert torch.equal(ar.theta, theta0)


def test_colsq(be):
    rng = np.random.default_rng(35)
    for rows in (1, 7, 5001):
        for cols in (1, 63, 64, 65, 512):
            ld = cols + 3
            x = rng.standard_normal((rows, ld)).astype(np.float32)
            out = torch.full((cols + 5,), -7.0, device="cuda")
            be.colsq(dev(x), out, rows, cols, ld)
            want = (x[:, :cols].astype(np.float64) ** 2).sum(0)
            got = out.cpu().numpy().astype(np.float64)
            assert (np.abs(got[:cols] - want) <= 1e-5 * want).all(), (rows, cols)
            assert (got[cols:] == -7.0).all(), (rows, cols)
