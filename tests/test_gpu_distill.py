"""The distillation head (tnt_softmax_cce_distill_f32, csrc/distill.hip) on a real MI355X against float64
(tests/distill_oracle.py).

The entry point has the ladder of tnt_softmax_cce_f32 (test_gpu_head.SMX_LADDER), over BOTH rows: the register kernel
softmax_cce_distill_kernel<NV4> needs the student's and the teacher's rows float4-addressable (ld % 4 == 0,
ld_teacher % 4 == 0, 16-byte aligned pointers), softmax_cce_distill_kernel<0> (re-reading) runs everything else:

    ceil(V / 1024)    1    2    3-4    5    6-8    > 8, or either row unaligned
    NV4               1    2    4      5    8      0
    (NV4 = 8 holds 64 VGPRs of row data and does not spill: the ladder is not capped for this entry)

V_LIST has both sides of every bound, and every V runs in the four layouts of test_gpu_head.layouts for the student times
the same four for the teacher, so ld_teacher != ld and a misaligned teacher alone forcing NV4 = 0 are among them.  Every
output is checked element by element against the bounds derived below; the pad columns of both inputs hold NaN / +1e30
and every output buffer a sentinel, and the pad contract is asserted exactly.

Test data stay out of the clip bands of ce (test_gpu_head.near_clip) in the target class only: the kl term has no clip."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_ops import dev
from test_gpu_head import U, FLT_MIN, SENT, fill_pad, check_pad, layouts, near_clip, reg_nv4, reference as head_reference
from test_gpu_head import check_loss as head_check_loss, check_grad as head_check_grad
from distill_oracle import reference

pytestmark = pytest.mark.gpu

V_LIST = [1, 2, 5, 257, 1024, 1025, 2048, 2049, 4096, 4097, 5001, 5120, 5121, 8192, 8193]
AT_LIST = [(0.0, 1.0), (0.5, 1.0), (0.5, 2.0), (1.0, 4.0), (0.3, 0.5)]
GS = 0.25                       # a float32 value: the reference sees the gscale the kernel sees

# ------------------------------------------------------------------------------------------------ tolerances
# The first-order error model at the top of tests/test_gpu_head.py (u = 2^-24), extended to the four reductions and to kl;
# a final factor 2 covers the second-order terms and the rounding of the float64 reference, as there.  alpha, t and gscale
# reach the kernel as float32 values and the reference uses those values.  dx_v = x_v - max x, du_v = u_v - max u.
#   * the exponentials: the kernel forms every one as v_exp_f32 (2^x) of a product, exp(d s) = exp2(fl(d c)) with
#     c = fl(s log2 e) (csrc/distill.hip).  dx_v = fl(x_v - m) carries u relative.  s = 1: c is the float32 log2 e
#     (u / 2) and the product rounds once (u): 2.5u relative in the exponent = 2.5u |dx_v| absolute.  s = 1 / t:
#     c = fl(fl(1 / t) log2 e) carries the reciprocal, the constant and the product (2.5u), so the exponent carries
#     4.5u |dx_v| / t (t == 1 takes c = log2 e; the bound stays).  v_exp_f32 is a 1 ulp instruction; 2 ulp = 4u are
#     allowed.  So exp(dx_v) carries u (2.5 |dx_v| + 4) relative, et_v = exp(dx_v / t) carries u (4.5 |dx_v| / t + 4) and
#     eu_v = exp(du_v / t) carries u (4.5 |du_v| / t + 4).
#   * a sum of V positive terms adds the terms' own errors and u times the longest chain of additions a term passes
#     through: per thread ceil(V / 256) serial adds on the re-reading row and 4 NV4 <= 2 ceil(V / 256) + 4 on the register
#     row (the ladder's widest step is nv4 = 3 -> NV4 = 4), then 6 levels of the wave tree and 3 across the waves:
#     CH = 2 ceil(V / 256) + 13.  With w1 = sum p_v |dx_v|, wt = sum pt_v |dx_v| / t, wu = sum qt_v |du_v| / t:
#       Z1 carries u B1, B1 = 2.5 w1 + 4 + CH;   Zt carries u Bt, Bt = 4.5 wt + 4 + CH;   Zu carries u Bu,
#       Bu = 4.5 wu + 4 + CH.
#   * logf is within 2 ulp: log Zt carries u Bt + 4u |log Zt|, log Zu likewise.
#   * D = sum_v eu_v (du_v - dx_v), terms of either sign.  delta_v = fl(du_v - dx_v) carries the errors of its inputs
#     u (|du_v| + |dx_v|) and its own rounding u |delta_v|; the product with eu_v adds eu_v's relative error and one
#     rounding: err(term_v) <= u eu_v (|du_v| + |dx_v| + |delta_v| (4.5 |du_v| / t + 6)).  The summation adds u CH Dabs,
#     Dabs = sum_v eu_v |delta_v|.  A class whose eu_v is below FLT_MIN (a subnormal or a flushed zero; the kernel adds
#     exactly 0 for eu_v == 0) moves D by at most FLT_MIN |delta_v|.
#   * K = fl(fl(D it) / Zu): it, the product, the division and Zu: err(D) / (t Zu) + u (3 + Bu) |D / (t Zu)|.  Divided
#     through by t Zu the sums over eu_v become sums over qt_v:
#       err(K) <= u [ sum_v qt_v (|du_v| + |dx_v| + |delta_v| (4.5 |du_v| / t + 6)) / t + (CH + 3 + Bu) sum_v qt_v |delta_v| / t ]
#                 + V FLT_MIN max_v |delta_v| / t
#     (|D / (t Zu)| <= sum_v qt_v |delta_v| / t).
#   * kl = fl(fl(K - log Zu) + log Zt): err(K) + err(log Zu) + err(log Zt) + u |K - log Zu| + u |kl|.
#     kl bound = 2 [ all of the above ].  It is absolute: kl may cancel to zero (teacher == student gives exactly 0).
#   * p_v = exp(dx_v) / Z1 carries u (2.5 |dx_v| + B1 + 6) (the reciprocal and the product); ce = -logf(clip(p_y))
#     carries that and 2 ulp of ce; a clipped ce is a float32 constant within u of the float64 one:
#       err(ce) <= u (2.5 |dx_y| + B1 + 6) + 4u |ce| + u.
#   * loss = fl(fl(fl(1 - a) ce) + fl(fl(fl(a t) t) kl)):
#     loss bound = 2 [ (1 - a) (err(ce) + 2u ce) + a t^2 (err(kl) + 3u |kl|) + u |loss| ],  err(kl) the bracket above.
#   * dlogits_v = fl(fl(c1 exp(dx_v) + ct et_v) - cu eu_v), minus gy for v == y, with
#       gy = fl(gscale fl(fl(1 - a) m_y)) (2u), c1 = fl(gy fl(1 / Z1)) (u (B1 + 4)),
#       ct = fl(fl(gscale fl(a t)) / Zt) (u (Bt + 3)), cu likewise with Zu.
#     With H_v = gscale (1 - a) m_y p_v, T_v = gscale a t pt_v, C_v = gscale a t qt_v:
#       grad bound = 2 [ u |H_v| (2.5 |dx_v| + B1 + 9) + u |T_v| (4.5 |dx_v| / t + Bt + 8) + u |C_v| (4.5 |du_v| / t + Bu + 8)
#                        + u |H_v + T_v| + u |H_v + T_v - C_v| + [v == y] (2u |gy| + u |dlogits_y|) ]
#                    + |gscale| (1 + 2 a t) FLT_MIN       (an exponential below FLT_MIN; every Z is >= 1)
#     A row with alpha = 0 whose ce is clipped, and any row under gscale = 0, is exactly zero.
# correct_row, the argmax and the pad handling are exact.
WORST = {"kl": 0.0, "loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\ndistillation head, worst observed error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


def _ratio(key, err, tol, what):
    r = float(np.max(err / tol)) if err.size else 0.0
    WORST[key] = max(WORST[key], r)
    assert r <= 1.0, f"{what}: {key} error {r:.3g} x its bound (worst at {np.unravel_index(np.argmax(err / tol), err.shape)})"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def bounds(ref, alpha, t, gscale):
    """(kl bound (rows), loss bound (rows), grad bound (rows, V)) of the derivation above"""
    rows, V = ref["p"].shape
    idx = np.arange(rows)
    adx, adu = np.abs(ref["dx"]), np.abs(ref["du"])
    delta = np.abs(ref["du"] - ref["dx"])
    p, pt, qt = ref["p"], ref["pt"], ref["qt"]
    CH = 2 * ref["nser"] + 13
    B1 = 2.5 * (p * adx).sum(1) + 4 + CH
    Bt = 4.5 * (pt * adx).sum(1) / t + 4 + CH
    Bu = 4.5 * (qt * adu).sum(1) / t + 4 + CH
    qd = (qt * delta).sum(1) / t
    errK = (U * ((qt * (adu + adx + delta * (4.5 * adu / t + 6))).sum(1) / t + (CH + 3 + Bu) * qd)
            + V * FLT_MIN * delta.max(1) / t)
    K = ref["kl"] + ref["logZu"] - ref["logZt"]
    err_kl = (errK + U * (Bu + 4 * np.abs(ref["logZu"])) + U * (Bt + 4 * np.abs(ref["logZt"]))
              + U * np.abs(K - ref["logZu"]) + U * np.abs(ref["kl"]))
    y = np.where(ref["ok"], ref["y"], 0)
    ady = np.where(ref["ok"], adx[idx, y], 0.0)
    err_ce = U * (2.5 * ady + B1 + 6) + 4 * U * np.abs(ref["ce"]) + U
    loss_b = 2 * ((1 - alpha) * (err_ce + 2 * U * ref["ce"]) + alpha * t * t * (err_kl + 3 * U * np.abs(ref["kl"]))
                  + U * np.abs(ref["loss"]))
    T, C = ref["soft_p"], ref["soft_q"]
    oh = np.zeros((rows, V))
    oh[idx[ref["ok"]], ref["y"][ref["ok"]]] = 1.0
    gy = abs(gscale) * (1 - alpha) * ref["my"]
    Hp = abs(gscale) * ((1 - alpha) * ref["my"])[:, None] * p              # the hard part before the target's patch
    grad_b = (2 * U * (Hp * (2.5 * adx + B1[:, None] + 9) + np.abs(T) * (4.5 * adx / t + Bt[:, None] + 8)
                       + np.abs(C) * (4.5 * adu / t + Bu[:, None] + 8) + np.abs(Hp + T) + np.abs(Hp + T - C)
                       + oh * (2 * gy[:, None] + np.abs(ref["grad"])))
              + abs(gscale) * (1 + 2 * alpha * t) * FLT_MIN)
    return 2 * err_kl, loss_b, grad_b


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def planted_rows(V):
    """(x, u (rows <= 8, V) float32, y, names): unit-scale random rows and the rows that exercise what is distillation's own"""
    rng = np.random.default_rng(3000 + V)
    xs, us, ys, names = [], [], [], []

    def add(x, u, y, name):
        xs.append(x); us.append(u); ys.append(int(y)); names.append(name)
    x = rng.standard_normal(V)
    add(x, rng.standard_normal(V), np.argmax(x), "random (correct)")
    add(rng.standard_normal(V), 2.0 * rng.standard_normal(V), rng.integers(0, V), "random")
    x = rng.standard_normal(V)
    add(x, x.copy(), V - 1, "teacher equal to student")
    add(rng.standard_normal(V), rng.standard_normal(V), V, "target id outside (V)")
    add(rng.standard_normal(V), rng.standard_normal(V), -1, "target id outside (-1)")
    if V >= 2:
        u = rng.standard_normal(V); j = V // 2
        u[j] = u.max() + 60.0
        add(rng.standard_normal(V), u, j, "teacher one-hot-like")
        x = rng.standard_normal(V); a, b = min(3, V - 2), V - 1
        x[a] = x[b] = x.max() + 1.0
        add(x, rng.standard_normal(V), b, "tie")
    if V >= 5:
        # student maximum in lane 0 / wave 0 / float4 element y, teacher maximum in another wave and element where V allows
        x, u = rng.standard_normal(V), rng.standard_normal(V)
        a, b = 1, min(V - 1, 4 * 70 + 2)
        x[a] = x.max() + 2.0
        u[b] = u.max() + 2.0
        add(x, u, b, "maxima apart")
    x, u = np.stack(xs).astype(np.float32), np.stack(us).astype(np.float32)
    assert len(names) <= 8
    return x, u, np.asarray(ys), tuple(names)


def run(be, x32, u32, y, lay_x, lay_u, form, alpha, t, gscale=GS):
    """one launch.  Forms: separate (every output its own buffer), train (dlogits = logits), no_loss / no_kl / no_corr /
    no_dl (that output null)"""
    rows, V = x32.shape
    (_, ld, shift), (_, ldt, shift_t) = lay_x, lay_u

    def stage(a, ld_, sh):
        host = np.full((rows, ld_), SENT, np.float32)
        host[:, :V] = a
        fill_pad(host, V)
        buf = torch.full((sh + rows * ld_,), SENT, device="cuda")
        buf[sh:] = dev(host.ravel())
        return host, buf, buf[sh:]
    host, buf, lg = stage(x32, ld, shift)
    host_t, buf_t, tc = stage(u32, ldt, shift_t)
    vec = lambda: torch.full((rows,), SENT, device="cuda")
    loss, kl, corr = vec(), vec(), vec()
    dl = lg if form == "train" else torch.full((rows * ld,), SENT, device="cuda")
    if form == "no_loss": loss = None
    if form == "no_kl": kl = None
    if form == "no_corr": corr = None
    if form == "no_dl": dl = None
    be.softmax_cce_distill(lg, tc, dev(np.asarray(y), torch.int32), loss, kl, corr, dl, rows, V, ld, ldt, gscale, alpha, t)
    torch.cuda.synchronize()
    aligned = all(s % 4 == 0 for s in (shift, shift_t)) and ldt % 4 == 0 and all(
        a is None or a.data_ptr() % 16 == 0 for a in (lg, tc, dl))
    res = {"nv4": reg_nv4(V, ld, aligned), "host": host, "logits": lg.cpu().numpy().reshape(rows, ld)}
    assert (buf[:shift] == SENT).all().item() and (buf_t[:shift_t] == SENT).all().item(), "wrote in front of a view"
    assert np.array_equal(buf_t[shift_t:].cpu().numpy().reshape(rows, ldt), host_t, equal_nan=True), "teacher modified"
    for k, a in (("loss", loss), ("kl", kl), ("corr", corr)):
        res[k] = None if a is None else a.cpu().numpy()
    res["dl"] = None if dl is None else dl.cpu().numpy().reshape(rows, ld)
    return res


def verify(res, ref, bnd, form, what):
    V = ref["p"].shape[1]
    nv4, host = res["nv4"], res["host"]
    what = f"{what} {form} [{'reg<%d>' % nv4 if nv4 else 'generic'}]"
    if form == "train":                          # aliased: the logits buffer is the output, its own pad the 'before'
        check_pad(res["logits"], host, V, nv4, f"{what} logits buffer")
    else:
        assert np.array_equal(res["logits"], host, equal_nan=True), f"{what}: logits modified"
        check_pad(res["dl"], np.full_like(host, SENT), V, nv4, f"{what} dlogits")
    kl_b, loss_b, grad_b = bnd
    _ratio("kl", np.abs(res["kl"].astype(np.float64) - ref["kl"]), kl_b, what)
    _ratio("loss", np.abs(res["loss"].astype(np.float64) - ref["loss"]), loss_b, what)
    assert np.array_equal(res["corr"], ref["corr"].astype(np.float32)), f"{what} correct_row"
    g = res["dl"][:, :V].astype(np.float64)
    assert np.isfinite(g).all(), what
    zero = (ref["grad"] == 0).all(1) & (ref["soft_q"] == 0).all(1)        # alpha = 0 and ce clipped: exactly zero
    assert (g[zero] == 0).all(), f"{what}: rows {np.nonzero(zero & (g != 0).any(1))[0]} should be all zero"
    _ratio("grad", np.abs(g - ref["grad"]), grad_b, what)


# ------------------------------------------------------------------------------------------------ every path, every form
@pytest.mark.parametrize("alpha,t", AT_LIST)
@pytest.mark.parametrize("V", V_LIST)
def test_every_dispatch_path_and_output_form(be, V, alpha, t):
    x, u, y, names = planted_rows(V)
    a32, t32 = float(np.float32(alpha)), float(np.float32(t))
    ref = reference(x, u, y, a32, t32, GS)
    near = near_clip(ref["py"][ref["ok"]])
    assert not near.any(), "test data: a target's p_y sits on a clip bound"
    # the planted rows really sit where they should
    i = names.index("teacher equal to student")
    assert (ref["kl"][i] == 0) and (ref["pt"][i] == ref["qt"][i]).all()
    for n in ("target id outside (V)", "target id outside (-1)"):
        i = names.index(n)
        assert ref["my"][i] == 0 and ref["corr"][i] == 0 and np.isclose(ref["ce"][i], -np.log(1e-7))
    if V >= 2:
        i = names.index("teacher one-hot-like")
        others = np.delete(ref["qt"][i], V // 2)
        assert (others <= np.exp(-60.0 / t32) * (1 + 1e-4)).all()     # every other class sits 60 / t below the maximum (float32 u)
        if t32 <= 0.5:                           # ... 120 at t = 0.5: qt underflows in every one of them in float32
            assert (others < FLT_MIN).all()
        i = names.index("tie")
        assert ref["amax"][i] == min(3, V - 2) and ref["corr"][i] == 0
    if V > 300:
        i = names.index("maxima apart")
        assert np.argmax(x[i]) == 1 and np.argmax(u[i]) == 282
    bnd = bounds(ref, a32, t32, GS)
    seen = {}
    for lay_x in layouts(V):
        for lay_u in layouts(V):
            what = f"V={V} a={alpha} t={t} student {lay_x[0]} teacher {lay_u[0]}"
            got = {}
            for form in ("separate", "train"):
                got[form] = run(be, x, u, y, lay_x, lay_u, form, a32, t32)
                verify(got[form], ref, bnd, form, what)
            sep = got["separate"]
            # one kernel, one set of values: in place and out of place write the same bits
            assert np.array_equal(got["train"]["logits"][:, :V], sep["dl"][:, :V]), what
            for k in ("loss", "kl", "corr"):
                assert np.array_equal(got["train"][k], sep[k]), (what, k)
            assert sep["kl"][names.index("teacher equal to student")] == 0, f"{what}: kl of identical rows"
            seen[(lay_x[0], lay_u[0])] = sep["nv4"]
            # every output nulled in turn, on every layout pair (the mixed ones run NV4 = 0 through the teacher alone)
            for form, gone in (("no_loss", "loss"), ("no_kl", "kl"), ("no_corr", "corr"), ("no_dl", "dl")):
                res = run(be, x, u, y, lay_x, lay_u, form, a32, t32)
                assert res[gone] is None and np.array_equal(res["logits"], res["host"], equal_nan=True)
                for k in ("loss", "kl", "corr", "dl"):
                    if k != gone:
                        assert np.array_equal(res[k], sep[k], equal_nan=True), (what, form, k)
    for (sx, su), nv4 in seen.items():
        reg = sx in ("r4", "r4+4") and su in ("r4", "r4+4") and V <= 8192
        assert (nv4 > 0) == reg, f"V={V} student {sx} teacher {su}: expected {'a register' if reg else 'the generic'} kernel"


# ------------------------------------------------------------------------------------------------ alpha = 0
@pytest.mark.parametrize("V", [5, 1024, 5001, 8193])
def test_alpha_zero_is_the_plain_head(be, V):
    """alpha = 0: loss / correct / dlogits inside tests/test_gpu_head.py's bounds of tnt_softmax_cce_f32 wherever those are
    the wider ones, inside this file's everywhere, and tnt_softmax_cce_f32 itself on the same rows inside both"""
    x, u, y, names = planted_rows(V)
    inside = (y >= 0) & (y < V)                  # the plain head's reference indexes p with y
    x, u, y = x[inside], u[inside], y[inside]
    rows = len(y)
    gs = 0.25
    ref = reference(x, u, y, 0.0, 1.0, gs)
    href = head_reference(x, y, gs)
    assert np.allclose(ref["loss"], href["loss"], rtol=1e-12, atol=0) and np.allclose(ref["grad"], href["grad"], rtol=1e-12, atol=1e-30)
    bnd = bounds(ref, 0.0, 1.0, gs)
    for lay in layouts(V):
        what = f"V={V} alpha=0 {lay[0]}"
        res = run(be, x, u, y, lay, lay, "separate", 0.0, 1.0, gs)
        verify(res, ref, bnd, "separate", what)
        ld = lay[1]
        lg = dev(res["host"].ravel())
        dl = torch.full((rows * ld,), SENT, device="cuda")
        loss, corr = torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
        be.softmax_cce(lg, dev(y, torch.int32), None, loss, corr, dl, rows, V, ld, gs)
        torch.cuda.synchronize()
        assert np.array_equal(corr.cpu().numpy(), res["corr"])
        plain_l, plain_g = loss.cpu().numpy(), dl.cpu().numpy().reshape(rows, ld)[:, :V]
        head_check_loss(plain_l, href, x, what + " (tnt_softmax_cce_f32)")
        head_check_grad(plain_g, href, gs, what + " (tnt_softmax_cce_f32)")
        # the two kernels against each other: each is within its bound of the same float64 value
        _ratio("loss", np.abs(plain_l.astype(np.float64) - res["loss"]), 2 * bnd[1], what + " against tnt_softmax_cce_f32")
        _ratio("grad", np.abs(plain_g.astype(np.float64) - res["dl"][:, :V]), 2 * bnd[2], what + " against tnt_softmax_cce_f32")


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(be):
    rows, V, ld = 4, 64, 64
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal((rows, ld)).astype(np.float32)
    x, tc = dev(x0), dev(rng.standard_normal((rows, ld)).astype(np.float32))
    tg = torch.zeros(rows, dtype=torch.int32, device="cuda")
    outs = [torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda"),
            torch.full((rows,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")]
    loss, kl, corr, dl = outs

    def untouched():
        torch.cuda.synchronize()
        return all((o == SENT).all().item() for o in outs)

    nan, inf = float("nan"), float("inf")
    ok = dict(lg=x, tc=tc, tg=tg, r=rows, v=V, l=ld, lt=ld, a=0.5, t=2.0)
    bad = [dict(r=-1), dict(v=0), dict(v=-3), dict(l=V - 1), dict(lt=V - 1), dict(lg=None), dict(tc=None), dict(tg=None),
           dict(a=-0.1), dict(a=1.5), dict(a=nan), dict(a=inf), dict(t=0.0), dict(t=-1.0), dict(t=nan), dict(t=inf),
           dict(t=-inf)]
    for change in bad:
        k = dict(ok, **change)
        with pytest.raises(RuntimeError):
            be.softmax_cce_distill(k["lg"], k["tc"], k["tg"], loss, kl, corr, dl, k["r"], k["v"], k["l"], k["lt"], 0.5,
                                   k["a"], k["t"])
    assert untouched(), "a rejected call wrote an output"
    # the teacher aliasing an output: each output in turn
    big = torch.full((rows * ld,), SENT, device="cuda")
    for i in range(4):
        args = [loss, kl, corr, dl]
        args[i] = big
        with pytest.raises(RuntimeError):
            be.softmax_cce_distill(x, big, tg, *args, rows, V, ld, ld, 0.5, 0.5, 2.0)
    assert untouched() and (big == SENT).all().item(), "a rejected call wrote an output"
    be.softmax_cce_distill(x, tc, tg, loss, kl, corr, dl, 0, V, ld, ld, 0.5, 0.5, 2.0)          # rows == 0: a no-op
    be.softmax_cce_distill(x, tc, tg, loss, kl, corr, x, 0, V, ld, ld, 0.5, 0.5, 2.0)
    assert untouched(), "a rows == 0 call wrote an output"
    assert np.array_equal(x.cpu().numpy(), x0)
