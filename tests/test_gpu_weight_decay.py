"""Decoupled weight decay inside the update kernels on a real MI355X: the WD instantiations of adam_fin_kernel
(tnt_adamw_fin_f32), adam_kernel (tnt_adamw_ring_f32), sgd_kernel (tnt_sgdw_f32) and of the encoder's fused update
(tnt_dense_dw_adamw_fin_f32, tnt_dense_dw_adamw_f32) against the float64 restatement of the header's definition -- the
plain float64 update (oracle.ops.adam_update) less (lr * wd) * theta of the theta the step started from.

Tolerances are test_gpu_optim_tail's: theta 1e-6 and m / v 1e-5 relative to float64 per variable, the padding between the
variables bit-identical.  With lr = 1e-3 and decays in {0, 0.05, 0.5} the decay moves theta by 5e-5 to 5e-4 relative, so a
kernel that ignored seg_wd would miss the bound by a factor of 50 to 500.  Where the definition promises bits (wd = 0, a
tripped guard, the side workgroup's outputs) the comparison is bit-exact."""
import types

import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_ops import close, dev
from test_gpu_optim_tail import (B1, B2, EPS, EXTRA_SEG, F32, LR, OVR_SEG, check_update, desc, host, lr_t_of, norm_launch,
                                 ref_adam, state)

pytestmark = pytest.mark.gpu

# a scalar tail only (1, 3), one float4 (4), one partial round (1027), the second trip of the AF_U loop with a ragged end
# (4096 + 5), two spans (2 * 4096 + 1028), the variable with a supplied norm (OVR_SEG), 10 spans -- its clip norm takes
# the lane-strided path of tnt_seg_sums --, the Embedding (EXTRA_SEG) and a last one
LENS = [1, 3, 4, 1027, 4096 + 5, 2 * 4096 + 1028, 37, 9 * 8192 + 3, 515, 64]
WDS = [0.5, 0.05, 0.0, 0.05, 0.5, 0.05, 0.5, 0.05, 0.5, 0.0]
SIDE = ("partial", "sq", "wsq", "l2o", "o0", "o1", "o2", "extra", "ids_dst", "adam_t", "drop", "arrive", "lr_t")


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


@pytest.fixture(scope="module")
def arena():
    """laid out like test_gpu_optim_tail.make_arena (64-float slots), with the lengths above"""
    from masters_thesis_amd.arena import build_spans
    rng = np.random.default_rng(31)
    nvar = len(LENS)
    assert OVR_SEG < nvar and EXTRA_SEG < nvar and LENS[7] > 8 * 8192
    l2 = [0.0 if s % 3 == 0 else float(rng.choice([0.01, 3e-5, 1e-3])) for s in range(nvar)]
    offs, total = [], 0
    for n in LENS:
        offs.append(total)
        total += (n + 63) // 64 * 64
    theta, grad, m0, v0 = (np.zeros(total, np.float32) for _ in range(4))
    for o, n in zip(offs, LENS):
        theta[o:o + n] = rng.standard_normal(n); grad[o:o + n] = rng.standard_normal(n) * 0.01
        m0[o:o + n] = rng.standard_normal(n) * 0.01; v0[o:o + n] = rng.random(n) * 1e-4
    ovr = np.full(nvar, -1.0, np.float32)
    ovr[OVR_SEG] = 2.5
    ovr[EXTRA_SEG] = 123.0                   # the fin form never reads it: the Embedding's norm comes from extra_part
    A = types.SimpleNamespace(lens=LENS, offs=offs, l2=np.array(l2, np.float32), total=total, nseg=nvar, theta=theta,
                              grad=grad, m0=m0, v0=v0, ovr=ovr, sp=build_spans(offs, LENS, device="cuda"),
                              wd=np.array(WDS, np.float32))
    A.mask = np.zeros(total, bool)
    for o, n in zip(offs, LENS):
        A.mask[o:o + n] = True
    A.x0, A.x1, A.x2 = rng.random(960).astype(np.float32), (rng.random(960) < 0.4).astype(np.float32), rng.random(77).astype(np.float32)
    A.extra_part = (rng.random(300) * 1e-3).astype(np.float32)
    A.ids = rng.integers(0, 5000, 1000).astype(np.int32)
    return A


def ref_adamw(A, th, m, v, t, clip, lr=LR, wd=None, extra=True):
    """test_gpu_optim_tail.ref_adam (float64, on oracle.ops.adam_update) at learning rate lr -- the Adam step is linear
    in it -- less the decay of the theta the step started from"""
    wd = A.wd if wd is None else wd
    th1, m1, v1 = ref_adam(A, th, m, v, t, clip, extra=extra)
    th1 = th + (th1 - th) * (float(lr) / float(LR))
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        th1[o:o + n] -= (float(lr) * float(wd[s])) * th[o:o + n]
    return th1, m1, v1


def start(A):
    return [A.theta.astype(np.float64), A.m0.astype(np.float64), A.v0.astype(np.float64)]


def fin_launch(be, A, S, fin, clip, wd):
    sp = A.sp
    if wd is None:
        be.adam_fin(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["ovr"], sp.nspan, EPS, clip, fin)
    else:
        be.adamw_fin(S["th"], S["m"], S["v"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, S["ovr"], sp.nspan, EPS, clip, fin, wd)


# ------------------------------------------------------------------------------------------ the span kernel, fin form
@pytest.mark.parametrize("clip", [0.1, 0.0])
def test_adamw_fin_against_float64(be, arena, clip):
    A = arena
    S, P = state(A), state(A)
    wd = dev(A.wd)
    norm_launch(be, A, S)
    fin_launch(be, A, S, desc(be, A, S), clip, wd)
    norm_launch(be, A, P)
    fin_launch(be, A, P, desc(be, A, P), clip, None)
    torch.cuda.synchronize()
    got = host(S, "th", "m", "v")
    check_update(A, got, ref_adamw(A, *start(A), 7, clip), before=[A.theta, A.m0, A.v0])
    # the decay enters neither the moments nor anything the side workgroup files: bit for bit the plain launch's
    assert torch.equal(S["m"], P["m"]) and torch.equal(S["v"], P["v"])
    for k in SIDE:
        assert torch.equal(S[k], P[k]), k
    assert int(S["adam_t"]) == 7 and int(S["drop"]) == 41 and int(S["arrive"].abs().sum()) == 0
    assert abs(float(S["lr_t"]) - lr_t_of(7)) <= 1e-6 * lr_t_of(7)
    # a variable without decay is updated exactly as the plain launch updates it; a decayed one is not
    th, tp = S["th"].cpu().numpy(), P["th"].cpu().numpy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        assert bool(np.array_equal(th[o:o + n], tp[o:o + n])) == (A.wd[s] == 0), s
    assert torch.equal(S["gr"], dev(A.grad)) and torch.equal(wd, dev(A.wd))


def test_adamw_fin_zero_table_is_adam_fin(be, arena):
    A = arena
    S, P = state(A), state(A)
    for X, wd in ((S, torch.zeros(A.nseg, device="cuda")), (P, None)):
        norm_launch(be, A, X)
        fin_launch(be, A, X, desc(be, A, X), 0.1, wd)
    torch.cuda.synchronize()
    for k in ("th", "m", "v") + SIDE:
        assert torch.equal(S[k], P[k]), k


def test_adamw_fin_guard(be, arena):
    A = arena
    S = state(A)
    S["guard"][0] = 1
    norm_launch(be, A, S)
    fin_launch(be, A, S, desc(be, A, S), 0.1, dev(A.wd))
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
        assert torch.equal(S[k], dev(h)), k
    assert int(S["adam_t"]) == 6 and int(S["drop"]) == 40 and int(S["arrive"].abs().sum()) == 0


def test_adamw_fin_captured_launch_decays_with_the_live_rate(be, arena):
    """the norm launch + tnt_adamw_fin_f32 captured once and replayed three times, lr_dev rewritten between the replays:
    every replay's Adam step and decay use the rate present at replay time"""
    A = arena
    S = state(A)
    fin, wd, clip = desc(be, A, S), dev(A.wd), 0.1
    pair = lambda: (norm_launch(be, A, S), fin_launch(be, A, S, fin, clip, wd))
    pair()                                                   # warm-up outside the capture; it is step 7
    torch.cuda.synchronize()
    prev = host(S, "th", "m", "v")
    check_update(A, prev, ref_adamw(A, *start(A), 7, clip))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    torch.cuda.synchronize()
    assert torch.equal(S["th"], dev(prev[0])) and int(S["adam_t"]) == 7          # capturing runs nothing
    for k, lr in enumerate((F32(2e-3), F32(5e-4), F32(1e-3))):
        S["lr"].fill_(lr)
        g.replay()
        torch.cuda.synchronize()
        got = host(S, "th", "m", "v")
        check_update(A, got, ref_adamw(A, *prev, 8 + k, clip, lr=lr), before=prev)
        assert int(S["adam_t"]) == 8 + k and int(S["arrive"].abs().sum()) == 0
        prev = got


# ------------------------------------------------------------------------------------------ the plain form
def plain_state(be, A):
    S = state(A)
    sp = A.sp
    be.seg_sqnorm(S["th"], S["gr"], sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, S["l2"], S["partial"], S["sq"],
                  S["wsq"], None, sp.nspan, A.nseg)
    S["lr_t"].fill_(float(np.float32(lr_t_of(7))))
    return S


@pytest.mark.parametrize("clip", [0.1, 0.0])
def test_adamw_ring_against_float64(be, arena, clip):
    A = arena
    sp = A.sp
    S, P, Z = plain_state(be, A), plain_state(be, A), plain_state(be, A)
    args = lambda X: (X["th"], X["m"], X["v"], X["gr"], sp.span_seg, sp.span_off, sp.span_len, X["l2"], X["sq"], X["ovr"],
                      sp.nspan, 0.0, X["lr_t"], B1, B2, EPS, clip)
    be.adamw(*args(S), S["lr"], dev(A.wd), guard=S["guard"])
    be.adam(*args(P), guard=P["guard"])
    be.adamw(*args(Z), Z["lr"], torch.zeros(A.nseg, device="cuda"), guard=Z["guard"])
    torch.cuda.synchronize()
    th0 = start(A)[0]
    th1, m1, v1 = ref_adam(A, *start(A), 7, clip, extra=False)
    th1 = th0 + (th1 - th0) * (float(np.float32(lr_t_of(7))) / lr_t_of(7))       # lr_t is handed over as a float32
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        th1[o:o + n] -= (float(LR) * float(A.wd[s])) * th0[o:o + n]
    check_update(A, host(S, "th", "m", "v"), (th1, m1, v1), before=[A.theta, A.m0, A.v0])
    assert torch.equal(S["m"], P["m"]) and torch.equal(S["v"], P["v"])
    for k in ("th", "m", "v"):
        assert torch.equal(Z[k], P[k]), k                               # wd = 0: the plain launch's bits
    G = plain_state(be, A)
    G["guard"][0] = 1
    be.adamw(*args(G), G["lr"], dev(A.wd), guard=G["guard"])
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):
        assert torch.equal(G[k], dev(h)), k


@pytest.mark.parametrize("clip", [0.1, 0.0])
def test_sgdw_against_float64(be, arena, clip):
    A = arena
    sp = A.sp
    MU = F32(0.9)
    S, P, Z, G = (plain_state(be, A) for _ in range(4))
    args = lambda X: (X["th"], X["m"], X["gr"], sp.span_seg, sp.span_off, sp.span_len, X["l2"], X["sq"], X["ovr"], sp.nspan)
    be.sgdw(*args(S), S["lr"], MU, clip, dev(A.wd), guard=S["guard"])
    be.sgd(*args(P), 0.0, P["lr"], MU, clip, guard=P["guard"])
    be.sgdw(*args(Z), Z["lr"], MU, clip, torch.zeros(A.nseg, device="cuda"), guard=Z["guard"])
    G["guard"][0] = 1
    be.sgdw(*args(G), G["lr"], MU, clip, dev(A.wd), guard=G["guard"])
    torch.cuda.synchronize()
    th, mom = start(A)[:2]
    th1, mom1 = th.copy(), mom.copy()
    for s, (o, n) in enumerate(zip(A.offs, A.lens)):
        w = th[o:o + n]
        g = A.grad[o:o + n].astype(np.float64) + 2 * float(A.l2[s]) * w
        if clip > 0:
            q = float(A.ovr[s]) if A.ovr[s] >= 0 else (g * g).sum()
            g = g * clip / max(np.sqrt(q), clip)
        t1, mom1[o:o + n] = O.sgd_momentum_update(w, mom[o:o + n], g, LR, MU)
        th1[o:o + n] = t1 - (float(LR) * float(A.wd[s])) * w
    check_update(A, host(S, "th", "m"), (th1, mom1), before=[A.theta, A.m0])
    assert torch.equal(S["m"], P["m"])
    assert torch.equal(Z["th"], P["th"]) and torch.equal(Z["m"], P["m"])
    assert torch.equal(G["th"], dev(A.theta)) and torch.equal(G["m"], dev(A.m0))


# ------------------------------------------------------------------------------------------ the encoder kernel
ENC_SHAPES = [(999, 512, 33, 1000), (112, 1024, 7, 112)]


@pytest.fixture(scope="module")
def enc_case(be):
    """per shape: the operands and the kernel's own float32 product X^T D (dense_dw_skinny), shared by the cases"""
    cache = {}

    def get(N, E, Bk, ldx):
        key = (N, E, Bk, ldx)
        if key not in cache:
            rng = np.random.default_rng(N + E)
            x = np.zeros((Bk, ldx), np.float32); x[:, :N] = rng.standard_normal((Bk, N))
            dpre = (rng.standard_normal((Bk, E)) * 0.01).astype(np.float32)
            theta = (rng.standard_normal((N, E)) * 0.05).astype(np.float32)
            m0, v0 = (rng.standard_normal((N, E)) * 1e-3).astype(np.float32), (rng.random((N, E)) * 1e-6).astype(np.float32)
            xd, dd = dev(x), dev(dpre)
            gk = torch.zeros(N, E, device="cuda")
            be.dense_dw_skinny(xd, dd, gk, N, E, Bk, ldx)
            torch.cuda.synchronize()
            g64 = x[:, :N].astype(np.float64).T @ dpre.astype(np.float64)
            close(gk, g64)
            cache[key] = types.SimpleNamespace(x=x, dpre=dpre, theta=theta, m0=m0, v0=v0, xd=xd, dd=dd,
                                               gk=gk.cpu().numpy().astype(np.float64), g64=g64)
        return cache[key]
    return get


@pytest.mark.parametrize("form", ["fin", "sq"])
@pytest.mark.parametrize("mode", ["clip", "override", "noclip"])
@pytest.mark.parametrize("N,E,Bk,ldx", ENC_SHAPES)
def test_dense_dw_adamw(be, enc_case, N, E, Bk, ldx, mode, form):
    """tnt_dense_dw_adamw_fin_f32 (form "fin": the clip norm from the span partials) and tnt_dense_dw_adamw_f32 ("sq": from
    sq[0]) as test_gpu_optim_tail.test_dense_dw_adam_fin argues: g is the kernel's own float32 product, everything behind
    it (L2, clip, Adam, the decay) float64.  wd = 0 gives the plain entry's bits, a tripped guard leaves the state."""
    from masters_thesis_amd.arena import build_spans
    c = enc_case(N, E, Bk, ldx)
    lam, clip, wd, lr_t = F32(0.01), (0.0 if mode == "noclip" else 0.1), (0.5 if mode == "override" else 0.05), F32(3e-4)
    nslot, k0 = build_spans([0], [N * E], device="cpu").nspan, 3
    partial = torch.full((2 * (k0 + nslot + 5),), 7.0, device="cuda")
    be.dense_dw_sqnorm(c.xd, c.dd, dev(c.theta), lam, partial[2 * k0:], nslot, N, E, Bk, ldx)
    sq = partial[2 * k0:2 * (k0 + nslot):2].sum().reshape(1)
    ovr, lrt, lr = dev([4.0 if mode == "override" else -1.0]), dev([lr_t]), dev([LR])
    guard = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(decay, tripped=False):
        th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
        guard[0] = int(tripped)
        head = (c.xd, c.dd, th, m, v, lam) + ((partial, k0, k0 + nslot) if form == "fin" else (sq,))
        tail = (ovr, lrt, B1, B2, EPS, clip, N, E, Bk, ldx)
        if decay is None and form == "fin":
            be.dense_dw_adam_fin(*head, *tail, guard=guard)
        elif decay is None:
            be.dense_dw_adam(*head, *tail, guard=guard)
        elif form == "fin":
            be.dense_dw_adamw_fin(*head, *tail, lr, decay, guard=guard)
        else:
            be.dense_dw_adamw(*head, *tail, lr, decay, guard=guard)
        torch.cuda.synchronize()
        return th, m, v

    th, m, v = run(wd)
    th64 = c.theta.astype(np.float64)
    ge = c.gk + 2 * lam * th64
    q = 4.0 if mode == "override" else ((c.g64 + 2 * lam * th64) ** 2).sum()
    if clip > 0:
        ge = ge * clip / max(np.sqrt(q), clip)
    _, mw, vw = O.adam_update(th64, c.m0.astype(np.float64), c.v0.astype(np.float64), ge, 1, 1.0, B1, B2, EPS)
    tw = (th64 - lr_t * mw / (np.sqrt(vw) + EPS)) - (float(LR) * wd) * th64       # lr_t is given, not derived from t
    close(m, mw, rtol=1e-5); close(v, vw, rtol=1e-5); close(th, tw, rtol=1e-6)
    plain, zero, held = run(None), run(0.0), run(wd, tripped=True)
    for a, b in zip(zero, plain):
        assert torch.equal(a, b)
    assert torch.equal(m, plain[1]) and torch.equal(v, plain[2]) and not torch.equal(th, plain[0])
    for a, h in zip(held, (c.theta, c.m0, c.v0)):
        assert torch.equal(a, dev(h))
    assert float(partial[:2 * k0].max()) == 7.0 and float(partial[2 * (k0 + nslot):].min()) == 7.0


# ------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_badarg_without_a_launch(be, arena, enc_case):
    from masters_thesis_amd.ops import _p
    A, lib, s = arena, be.lib, be._s()
    sp = A.sp
    S = plain_state(be, A)
    wd, fin = dev(A.wd), desc(be, A, S)
    import ctypes
    spans = (_p(sp.span_seg), _p(sp.span_off), _p(sp.span_len))
    ring = lambda lr, tab: lib.tnt_adamw_ring_f32(_p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]),
                                                  _p(S["ovr"]), sp.nspan, 0.0, _p(S["lr_t"]), B1, B2, EPS, 0.1, None, None, 0, None,
                                                  0, None, lr, tab, s)
    finl = lambda tab: lib.tnt_adamw_fin_f32(_p(S["th"]), _p(S["m"]), _p(S["v"]), _p(S["gr"]), *spans, _p(S["ovr"]), sp.nspan, EPS,
                                             0.1, ctypes.addressof(fin), None, 0, None, 0, None, tab, s)
    sgd = lambda lr, tab: lib.tnt_sgdw_f32(_p(S["th"]), _p(S["m"]), _p(S["gr"]), *spans, _p(S["l2"]), _p(S["sq"]), _p(S["ovr"]),
                                           sp.nspan, lr, 0.9, 0.1, None, tab, s)
    for rc in (ring(None, _p(wd)), ring(_p(S["lr"]), None), finl(None), sgd(None, _p(wd)), sgd(_p(S["lr"]), None)):
        assert rc <= -1000, rc
    N, E, Bk, ldx = ENC_SHAPES[1]
    c = enc_case(N, E, Bk, ldx)
    th, m, v = dev(c.theta), dev(c.m0), dev(c.v0)
    one, part = dev([1.0]), torch.ones(64, device="cuda")
    for lr, w in ((None, 0.05), (_p(S["lr"]), -0.05), (_p(S["lr"]), float("nan")), (_p(S["lr"]), float("inf"))):
        rc = lib.tnt_dense_dw_adamw_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(one), None, _p(one), B1, B2, EPS, 0.1, None,
                                        N, E, Bk, ldx, lr, w, s)
        assert rc <= -1000, (rc, w)
        rc = lib.tnt_dense_dw_adamw_fin_f32(_p(c.xd), _p(c.dd), _p(th), _p(m), _p(v), 0.01, _p(part), 0, 14, None, _p(one), B1, B2, EPS,
                                            0.1, None, N, E, Bk, ldx, lr, w, s)
        assert rc <= -1000, (rc, w)
    torch.cuda.synchronize()
    for k, h in (("th", A.theta), ("m", A.m0), ("v", A.v0)):                  # nothing was launched
        assert torch.equal(S[k], dev(h)), k
    assert torch.equal(th, dev(c.theta)) and torch.equal(m, dev(c.m0)) and torch.equal(v, dev(c.v0))
    assert int(S["adam_t"]) == 6 and int(S["arrive"].abs().sum()) == 0
    assert lib.tnt_version() >= 124
