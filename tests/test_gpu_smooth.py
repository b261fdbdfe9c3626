"""The label-smoothed head (tnt_softmax_cce_smooth_f32, csrc/smooth.hip) on a real MI355X against float64
(tests/smooth_oracle.py).

The entry point has the dispatch of tnt_softmax_cce_f32: softmax_cce_smooth_kernel<NV4> for 16-byte-aligned rows with
ld % 4 == 0 and ceil(V / 1024) inside a bucket of test_gpu_head.SMX_LADDER, softmax_cce_smooth_kernel<0> (generic) for
everything else.  V_LIST has both sides of every bucket bound, and every V runs in the four layouts of
test_gpu_head.layouts, so on the register kernel (where it exists) and on the generic one.  Every output is checked
element by element against the bounds derived below; pad columns hold NaN / +1e30 and every output buffer a sentinel,
and the pad contract of each kernel is asserted exactly.

Test data stay out of the clip bands (test_gpu_head.near_clip) in EVERY class: a float32 kernel and a float64 reference
cannot agree on m_v for a p_v that sits on a clip bound.  Unit-scale normal logits keep every p_v above 5e-7 up to
V = 16384; the planted classes sit 30 or more below the row maximum (p_v < 1e-12)."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_ops import dev
from test_gpu_head import (U, FLT_MIN, SENT, fill_pad, check_pad, check_probs, check_loss, check_grad, layouts, near_clip,
                           reg_nv4, r4, reference as head_reference)
from smooth_oracle import reference

pytestmark = pytest.mark.gpu

# 1024 / 2048 / 4096 / 5120 / 8192 are the bucket bounds of the ladder (nv4 = 1, 2, 4, 5, 8); 8193 and 16384 run the generic
# kernel in every layout
V_LIST = [1, 2, 5, 64, 257, 1024, 1025, 2048, 2049, 4096, 4097, 5001, 5120, 5121, 8192, 8193, 16384]
EPS_LIST = [0.1, 0.5]
LOG_LO = -np.log(O.CCE_EPS)      # |log(1e-7)|

# ------------------------------------------------------------------------------------------------ tolerances
# The error model at the top of tests/test_gpu_head.py, extended (u = 2^-24, first order, then the same factor 2 for the
# second-order terms and the rounding of the float64 reference).  From there: d_j = fl(x_j - m) carries u |d_j|; p_j and
# log p_j carry REL_j = 2u (|d_j| + BASE), BASE = w + ceil(V / 256) + 25; Z alone carries less than u BASE relative.
# New in this kernel:
#   * log Z = logf(Z): Z's error plus 2 ulp:  E_Z = u BASE + 4u |log Z|.
#   * L_v = d_v - log Z for an unclipped class: u |d_v| + E_Z + u |L_v| (the subtraction).  A clipped class takes the
#     constant logf(1e-7f) or logf(1 - 1e-7f): within 2u * 16.2 resp. 2e-8 < u of the float64 value.
#   * S = sum of d_v over the n_u unclipped classes, all of one sign, so every partial sum is below Sabs = sum |d_v|:
#     the terms' own errors u Sabs, and the summation u Sabs * (the longest chain: ceil(V / 256) serial adds per thread in
#     the generic kernel -- the register kernel's NV4 + 2 is never longer -- 6 levels of the wave tree, 3 across the
#     waves) = u Sabs (ceil(V / 256) + 12).
#   * sumL = (S - n_u log Z) + (n_lo log_lo + n_hi log_hi): n_u is exact (an integer below 2^24); the products, the
#     subtraction and the two additions one rounding each on a magnitude below sumLabs = Sabs + n_u |log Z| +
#     16.2 n_lo + 1.2e-7 n_hi; the constants' own error as above.  Collected:
#     err(sumL) <= u (ceil(V / 256) + 18) sumLabs + n_u E_Z.
#   * eps / V: one rounding for the division, one for its product with sumL (eps itself is passed as a float32 and the
#     reference uses that value): 2u (eps / V) sumLabs.  (1 - eps) L_y: fl(1 - eps) and the product, 2u (1 - eps) |L_y|.
#   * the final addition: u |loss|.
#   loss bound = 2 [ (1 - eps) (u |d_y| + E_Z + 3u |L_y| + u) + (eps / V) (u (ceil(V / 256) + 20) sumLabs + n_u E_Z)
#                    + u |loss| ]
#   * c = fl((1 - eps) m_y + fl(eps / V) n_u): fl(1 - eps), the division, the product and the addition: 4u c.
#   * dlogits_v = fl(fl(c p_v - m_v ys_v) gscale): c p_v carries REL_v + 4u + u (the product); m_v ys_v carries 3u (the
#     division, and for the target's class fl(1 - eps) and the addition); the subtraction, the product with gscale
#     and gscale's own rounding to float32 are u each on the result:
#     grad bound = |gscale| (c p_v (REL_v + 10u) + 6u m_v ys_v + 6u |c p_v - m_v ys_v| + FLT_MIN)
#     (REL_v already holds the factor 2).  A row with c = 0 (nothing unclipped) is exactly zero.
# probs, correct_row, argmax and the pad handling are those of tnt_softmax_cce_f32: test_gpu_head's bounds, exact.
WORST = {"loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nsmooth head, worst observed error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


def _ratio(key, err, tol, what):
    r = float(np.max(err / tol)) if err.size else 0.0
    WORST[key] = max(WORST[key], r)
    assert r <= 1.0, f"{what}: {key} error {r:.3g} x its bound (worst at {np.unravel_index(np.argmax(err / tol), err.shape)})"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def loss_bound(ref, eps):
    rows, V = ref["p"].shape
    idx = np.arange(rows)
    y, d, mask = ref["y"], ref["d"], ref["mask"]
    base = ref["w"] + ref["nser"] + 25
    alogZ = np.abs(ref["logZ"])
    E_Z = U * base + 4 * U * alogZ
    dy = np.abs(d[idx, y])
    Ly = np.abs(np.log(np.clip(ref["p"][idx, y], O.CCE_EPS, 1 - O.CCE_EPS)))
    n_u = ref["n_u"]
    n_hi = (ref["p"] > 1 - O.CCE_EPS).sum(1)
    n_lo = V - n_u - n_hi
    sumLabs = ref["Sabs"] + n_u * alogZ + 16.2 * n_lo + 1.2e-7 * n_hi
    return 2 * ((1 - eps) * (U * dy + E_Z + 3 * U * Ly + U)
                + eps / V * (U * (ref["nser"] + 20) * sumLabs + n_u * E_Z) + U * np.abs(ref["loss"]))


def grad_bound(ref, gscale):
    p, d = ref["p"], ref["d"]
    rel = 2 * U * (np.abs(d) + (ref["w"] + ref["nser"] + 25)[:, None])
    cp = ref["c"][:, None] * p
    mys = ref["mask"] * ref["ys"]
    return abs(gscale) * (cp * (rel + 10 * U) + 6 * U * mys + 6 * U * np.abs(cp - mys) + FLT_MIN)


def check_smooth_loss(loss, ref, eps, what):
    _ratio("loss", np.abs(loss.astype(np.float64) - ref["loss"]), loss_bound(ref, eps), what)


def check_smooth_grad(g, ref, gscale, what):
    g = g.astype(np.float64)
    zero = (ref["c"] == 0) | (gscale == 0)
    assert (g[zero] == 0).all(), f"{what}: rows {np.nonzero(zero & (g != 0).any(1))[0]} should be all zero"
    tol = grad_bound(ref, gscale)
    _ratio("grad", np.where(zero[:, None], 0.0, np.abs(g - ref["grad"])), np.where(zero[:, None], 1.0, tol), what)


# ------------------------------------------------------------------------------------------------ data
def planted_rows(V, rng):
    """(x (rows <= 8, V) float32, y, names): unit-scale random rows, and where V allows them the rows that exercise the
    per-class clip -- one class 30 below the maximum, the target itself clipped low, a saturated row, an exact tie"""
    xs = [rng.standard_normal(V) for _ in range(3)]
    ys = [int(np.argmax(xs[0])), int(rng.integers(0, V)), V - 1]
    names = ["random (correct)", "random", "random (last class)"]
    if V >= 5:
        x = rng.standard_normal(V); j = V // 2
        x[j] = x.max() - 30.0
        xs.append(x); ys.append((j + 1) % V); names.append("one class clipped low")
        x = rng.standard_normal(V); j = 1
        x[j] = x.max() - 30.0
        xs.append(x); ys.append(j); names.append("target clipped low")
        x = rng.standard_normal(V); j = V - 2
        x[j] = 40.0
        xs.append(x); ys.append(j); names.append("saturated")
        x = rng.standard_normal(V); a, b = min(3, V - 2), V - 1
        x[a] = x[b] = x.max() + 1.0
        xs.append(x); ys.append(b); names.append("tie")
    if V == 2:
        xs.append(np.array([0.25, 0.25])); ys.append(1); names.append("tie")
    x = np.stack(xs).astype(np.float32)
    p = O.softmax(x.astype(np.float64))
    near = near_clip(p)
    assert not near.any(), f"test data: classes {np.argwhere(near)[:4]} sit on a clip bound"
    return x, np.asarray(ys), names


def run(be, x32, y, ld, shift, form, gscale, eps):
    """one launch in one output form: separate (everything), loss (loss_row / correct_row only), train (dlogits =
    logits), eval (probs = logits, gscale 0), infer (no target: probs = logits)"""
    rows, V = x32.shape
    host = np.full((rows, ld), SENT, np.float32)
    host[:, :V] = x32
    fill_pad(host, V)
    buf = torch.full((shift + rows * ld,), SENT, device="cuda")
    buf[shift:] = dev(host.ravel())
    lg = buf[shift:]
    out = lambda: torch.full((rows * ld,), SENT, device="cuda")
    vec = lambda: torch.full((rows,), SENT, device="cuda")
    tg = None if y is None else dev(np.asarray(y), torch.int32)
    probs = dl = loss = corr = None
    if form == "separate":
        probs, dl, loss, corr = out(), out(), vec(), vec()
    elif form == "loss":
        loss, corr = vec(), vec()
    elif form == "train":
        dl, loss, corr = lg, vec(), vec()
    elif form == "eval":
        probs, loss, corr, gscale = lg, vec(), vec(), 0.0
    elif form == "infer":
        probs, tg = lg, None
    else:
        raise ValueError(form)
    be.softmax_cce_smooth(lg, tg, probs, loss, corr, dl, rows, V, ld, gscale, eps)
    torch.cuda.synchronize()
    aligned = shift % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (lg, probs, dl))
    res = {"nv4": reg_nv4(V, ld, aligned), "gscale": gscale, "host": host, "logits": lg.cpu().numpy().reshape(rows, ld),
           "shift_head": buf[:shift].cpu().numpy()}
    for k, t in (("probs", probs), ("dl", dl), ("loss", loss), ("corr", corr)):
        res[k] = None if t is None else t.cpu().numpy()
    for k in ("probs", "dl"):
        if res[k] is not None:
            res[k] = res[k].reshape(rows, ld)
    return res


def verify(res, ref, x32, eps, what, form):
    rows, V = x32.shape
    nv4, host = res["nv4"], res["host"]
    what = f"{what} {form} [{'reg<%d>' % nv4 if nv4 else 'generic'}]"
    assert (res["shift_head"] == SENT).all(), f"{what}: wrote in front of the logits view"
    if form == "separate":
        for k in ("probs", "dl"):                # separate outputs: pad zero in the window, else the sentinel
            check_pad(res[k], np.full_like(host, SENT), V, nv4, f"{what} {k}")
    if form in ("separate", "loss"):
        assert np.array_equal(res["logits"], host, equal_nan=True), f"{what}: logits modified"
    else:                                        # aliased: the logits buffer is an output, its own pad the 'before'
        check_pad(res["logits"], host, V, nv4, f"{what} logits buffer")
    if res["probs"] is not None:
        check_probs(res["probs"][:, :V], ref, f"{what} probs")
    if form == "infer":
        return
    check_smooth_loss(res["loss"], ref, eps, f"{what} loss")
    assert np.array_equal(res["corr"], (ref["amax"] == ref["y"]).astype(np.float32)), f"{what} correct_row"
    if res["dl"] is not None:
        check_smooth_grad(res["dl"][:, :V], ref, res["gscale"], f"{what} dlogits")


# ------------------------------------------------------------------------------------------------ every path, every form
@pytest.mark.parametrize("V", V_LIST)
def test_every_dispatch_path_and_output_form(be, V):
    rng = np.random.default_rng(1000 + V)
    x, y, names = planted_rows(V, rng)
    rows = len(names)
    assert rows <= 8
    gs = 0.25                                    # a float32 value: the reference sees the gscale the kernel sees
    for eps in EPS_LIST:
        e32 = float(np.float32(eps))
        ref = reference(x, y, gs, e32)
        if V >= 5:                               # the planted rows really sit where they should
            i = names.index("one class clipped low")
            assert (~ref["mask"][i]).sum() == 1 and ref["mask"][i, y[i]]
            i = names.index("target clipped low")
            assert not ref["mask"][i, y[i]] and ref["n_u"][i] == V - 1
            i = names.index("saturated")
            assert ref["n_u"][i] == 0 and ref["c"][i] == 0 and ref["p"][i, y[i]] > 1 - 1e-7
            i = names.index("tie")
            assert ref["amax"][i] == min(3, V - 2) != y[i]
        seen = {}
        for name, ld, shift in layouts(V):
            got = {}
            for form in ("separate", "loss", "train", "eval", "infer"):
                res = run(be, x, y, ld, shift, form, gs, e32)
                verify(res, ref, x, e32, f"V={V} eps={eps} {name} ld={ld}", form)
                got[form] = res
            if V >= 5:
                assert (got["separate"]["dl"][names.index("saturated"), :V] == 0).all()
            # one kernel, one set of values: every form writes the same bits
            p = got["separate"]["probs"][:, :V]
            assert np.array_equal(got["eval"]["logits"][:, :V], p) and np.array_equal(got["infer"]["logits"][:, :V], p)
            assert np.array_equal(got["train"]["logits"][:, :V], got["separate"]["dl"][:, :V])
            for k in ("loss", "corr"):
                for form in ("loss", "train", "eval"):
                    assert np.array_equal(got[form][k], got["separate"][k]), (name, form, k)
            seen[name] = got["separate"]["nv4"]
        assert seen["odd"] == 0 and seen["shift"] == 0
        assert (seen["r4"] > 0) == (V <= 8192), f"V={V}: aligned rows ran {'the generic' if not seen['r4'] else 'a register'} kernel"


def test_no_target_with_a_gradient_buffer_writes_zero_rows(be):
    rng = np.random.default_rng(5)
    V, rows = 257, 3
    x = rng.standard_normal((rows, V)).astype(np.float32)
    for ld, shift in ((260, 0), (259, 0)):
        host = np.full((rows, ld), SENT, np.float32)
        host[:, :V] = x
        lg = dev(host.ravel())
        dl = torch.full((rows * ld,), SENT, device="cuda")
        loss = torch.full((rows,), SENT, device="cuda")
        be.softmax_cce_smooth(lg, None, None, loss, loss, dl, rows, V, ld, 0.5, 0.1)
        torch.cuda.synchronize()
        assert (dl.cpu().numpy().reshape(rows, ld)[:, :V] == 0).all() and (loss == SENT).all().item()


# ------------------------------------------------------------------------------------------------ eps = 0
@pytest.mark.parametrize("V", [5, 1024, 5001, 8193])
def test_eps_zero_is_the_unsmoothed_head(be, V):
    """label_smoothing = 0: loss / correct / probs / dlogits inside tests/test_gpu_head.py's bounds of tnt_softmax_cce_f32
    (its float64 reference, its check functions), and tnt_softmax_cce_f32 itself on the same data beside it"""
    rng = np.random.default_rng(2000 + V)
    x, y, names = planted_rows(V, rng)
    rows = len(names)
    gs = 1.0 / rows
    ref = head_reference(x, y, gs)
    for name, ld, shift in layouts(V):
        res = run(be, x, y, ld, shift, "separate", gs, 0.0)
        what = f"V={V} eps=0 {name}"
        check_pad(res["probs"], np.full_like(res["host"], SENT), V, res["nv4"], what)
        check_pad(res["dl"], np.full_like(res["host"], SENT), V, res["nv4"], what)
        check_probs(res["probs"][:, :V], ref, what)
        check_loss(res["loss"], ref, x, what)
        check_grad(res["dl"][:, :V], ref, gs, what)
        assert np.array_equal(res["corr"], (ref["amax"] == y).astype(np.float32))
        # the existing entry point on the same buffers' contents
        lg = dev(res["host"].ravel())
        probs, dl = torch.full((rows * ld,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")
        loss, corr = torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
        be.softmax_cce(lg, dev(y, torch.int32), probs, loss, corr, dl, rows, V, ld, gs)
        torch.cuda.synchronize()
        assert np.array_equal(corr.cpu().numpy(), res["corr"])
        check_loss(loss.cpu().numpy(), ref, x, what + " (tnt_softmax_cce_f32)")
        check_grad(dl.cpu().numpy().reshape(rows, ld)[:, :V], ref, gs, what + " (tnt_softmax_cce_f32)")


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(be):
    rows, V, ld = 4, 64, 64
    x0 = np.random.default_rng(1).standard_normal((rows, ld)).astype(np.float32)
    x = dev(x0)
    tg = torch.zeros(rows, dtype=torch.int32, device="cuda")
    outs = [torch.full((rows * ld,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda"),
            torch.full((rows,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")]
    probs, loss, corr, dl = outs

    def untouched():
        torch.cuda.synchronize()
        return all((o == SENT).all().item() for o in outs)

    for r, v, l, lg, eps in ((rows, 0, ld, x, 0.1), (rows, -3, ld, x, 0.1), (rows, V, V - 1, x, 0.1), (rows, V, ld, None, 0.1),
                             (-1, V, ld, x, 0.1), (rows, V, ld, x, -0.1), (rows, V, ld, x, 1.0), (rows, V, ld, x, 1.5),
                             (rows, V, ld, x, float("nan")), (rows, V, ld, x, float("inf")), (rows, V, ld, x, float("-inf"))):
        with pytest.raises(RuntimeError):
            be.softmax_cce_smooth(lg, tg, probs, loss, corr, dl, r, v, l, 0.5, eps)
    assert untouched(), "a rejected call wrote an output"
    be.softmax_cce_smooth(x, tg, probs, loss, corr, dl, 0, V, ld, 0.5, 0.1)              # rows == 0: a no-op
    be.softmax_cce_smooth(x, tg, None, loss, corr, x, 0, V, ld, 0.5, 0.1)
    assert untouched(), "a rows == 0 call wrote an output"
    assert np.array_equal(x.cpu().numpy(), x0)
