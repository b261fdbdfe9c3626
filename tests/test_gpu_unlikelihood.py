"""The unlikelihood head (tnt_softmax_cce_unlikely_f32, csrc/unlikely.hip) on a real MI355X against float64
(tests/unlikelihood_oracle.py).

The entry point has the dispatch of tnt_softmax_cce_f32: softmax_cce_unlikely_kernel<NV4> for 16-byte-aligned rows
with ld % 4 == 0 and ceil(V / 1024) inside a bucket of test_gpu_head.SMX_LADDER, softmax_cce_unlikely_kernel<0> (generic) for
everything else.  Every V runs in the four layouts of test_gpu_head.layouts, so on the register kernel (where it exists)
and on the generic one, with (B, T) = (1, 1), (3, 5) and (2, 64): no prefix, a short one, the full wave.  The separate
outputs of every layout are checked element by element against the bounds derived below; the four other output forms
must write the same bits.  Pad columns hold NaN / +1e30 and every output buffer a sentinel, and the pad contract of each
kernel is asserted exactly.

Test data stay out of the clip bands (test_gpu_head.near_clip) in EVERY class, and every candidate stays out of
1e-8 < 1 - p_c < 1e-5, the band around the bound 1 - p_c = 1e-7 of m_c: a float32 kernel and a float64 reference cannot
agree on a mask whose argument sits on its bound.  Both are asserted on the float64 reference before any launch."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_ops import dev
from test_gpu_head import (U, FLT_MIN, SENT, fill_pad, check_pad, check_probs, check_loss, check_grad, layouts, near_clip,
                           reg_nv4, reference as head_reference)
from unlikelihood_oracle import reference

pytestmark = pytest.mark.gpu

V_LIST = [1, 2, 5, 64, 257, 1024, 1025, 4096, 4097, 5001, 8192, 8193]
BT_LIST = [(1, 1), (3, 5), (2, 64)]
ALPHA_LIST = [0.5, 2.0]
FORMS = ("separate", "loss", "train", "eval", "infer")
LOG_LO = -np.log(O.CCE_EPS)      # |log(1e-7)|

# ------------------------------------------------------------------------------------------------ tolerances
# The error model at the top of tests/test_gpu_head.py, extended as tests/test_gpu_smooth.py extends it (u = 2^-24, first
# order, then a factor 2 on every new term for the second-order terms and the rounding of the float64 reference).  From
# there: p_v carries the relative error REL_v = 2u (|d_v| + BASE), BASE = w + ceil(V / 256) + 25, which holds the factor 2
# already; the ce part of the loss is inside 2u (BASE + |d_y| + 12 M), M = max(1, |m|, |x_y|, |log Z|) (for a target id
# outside [0, V) the kernel writes the constant -logf(1e-7f): d_y and x_y count as 0).
# New in this kernel, per candidate c (p_c computed by the same operations as the element's own p_c: REL_c):
#   * omp_c = fl(1 - p_c): p_c REL_c + u omp_c absolute, so REL_c p_c / omp_c + u relative to omp_c;
#   * q_c = fl(p_c / omp_c): REL_c (1 + p_c / omp_c) = REL_c / omp_c from its operands, u from omp's rounding, 2.5 ulp = 5u
#     for the division:  RQ_c = REL_c / omp_c + 12u  (6u doubled).  A saturated candidate (m_c = 0) has q_c = 0 exactly.
#   * Q = sum of at most 63 non-negative terms over the 6 levels of the wave tree: EQ = sum_c q_c RQ_c + 12u Q absolute;
#   * l_c = -log1pf(-p_c): the argument's error p_c REL_c moves log1p by p_c REL_c / omp_c = REL_c q_c, log1pf itself is
#     within 2 ulp = 4u l_c:  REL_c q_c + 8u l_c.  A saturated candidate takes the constant -logf(1e-7f): 8u * 16.2.
#     ul = their wave-tree sum, 6u ul; alpha ul one product, the addition to ce one rounding of the loss:
#     loss bound = ce bound + alpha (sum_c (REL_c q_c + 8u l_c  or  8u 16.2) + 14u ul) + 2u |loss|.
#   * coef = fl(m_y - fl(alpha Q)) (alpha is passed as a float32 and the reference uses that value): alpha EQ from Q, u for
#     the product, u |coef| for the subtraction:  E_coef = alpha EQ + 2u alpha Q + 2u |coef|.
#   * an element: fl(fl(coef p_v) gscale); column y: fl(fl(coef p_y - m_y) gscale); a candidate's column:
#     fl(fl(coef p_c + fl(alpha q_c)) gscale).  With G_v = m_y (p_v - [v == y]) + alpha ([v in C] q_v - p_v Q), the exact
#     unscaled value: p_v E_coef from coef, |coef| p_v (REL_v + 2u) from p_v and the product, alpha q_v (RQ_v + 2u) in a
#     candidate's column, and u each on the result for the addition / subtraction, the product with gscale and gscale's
#     own rounding to float32:
#     grad bound = |gscale| (p_v E_coef + |coef| p_v (REL_v + 4u) + [v in C] alpha q_v (RQ_v + 4u) + 6u |G_v|) + FLT_MIN.
#   A row with m_y = 0 and Q = 0 (the clip of ce active and no unsaturated candidate), or gscale = 0, is exactly zero.
# probs, correct_row, argmax and the pad handling are those of tnt_softmax_cce_f32: test_gpu_head's bounds, exact.
WORST = {"loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nunlikelihood head, worst observed error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


def _ratio(key, err, tol, what):
    r = float(np.max(err / tol)) if err.size else 0.0
    WORST[key] = max(WORST[key], r)
    assert r <= 1.0, f"{what}: {key} error {r:.3g} x its bound (worst at {np.unravel_index(np.argmax(err / tol), err.shape)})"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def _rel(ref):
    return 2 * U * (np.abs(ref["d"]) + (ref["w"] + ref["nser"] + 25)[:, None])


def _rq(ref):
    """RQ_c where c is an unsaturated candidate, 0 elsewhere"""
    live = ref["q"] > 0
    omp = np.where(live, 1.0 - ref["p"], 1.0)
    return np.where(live, _rel(ref) / omp + 12 * U, 0.0)


def loss_bound(ref, x32, alpha):
    rows, V = ref["p"].shape
    idx = np.arange(rows)
    y = ref["y"]
    ok = (y >= 0) & (y < V)
    yy = np.where(ok, y, 0)
    dy = np.where(ok, np.abs(ref["d"][idx, yy]), 0.0)
    xy = np.where(ok, np.abs(x32[idx, yy].astype(np.float64)), 0.0)
    M = np.maximum.reduce([np.ones(rows), np.abs(ref["m"]), xy, np.abs(ref["logZ"])])
    ce_tol = 2 * U * (ref["w"] + ref["nser"] + 25 + dy + 12 * M)
    sat = ref["cmask"] & (ref["q"] == 0)
    l = -np.log1p(-np.where(ref["q"] > 0, ref["p"], 0.0))
    per = np.where(ref["q"] > 0, _rel(ref) * ref["q"] + 8 * U * l, 0.0) + sat * (8 * U * 16.2)
    return ce_tol + alpha * (per.sum(1) + 14 * U * ref["ul"]) + 2 * U * np.abs(ref["loss"])


def grad_bound(ref, gscale, alpha):
    p, q, Q = ref["p"], ref["q"], ref["Q"]
    rq = _rq(ref)
    EQ = (q * rq).sum(1) + 12 * U * Q
    coef = ref["my"] - alpha * Q
    E_coef = alpha * EQ + 2 * U * alpha * Q + 2 * U * np.abs(coef)
    G = ref["grad"] / gscale if gscale else np.zeros_like(p)
    return abs(gscale) * (p * E_coef[:, None] + np.abs(coef)[:, None] * p * (_rel(ref) + 4 * U) + alpha * q * (rq + 4 * U)
                          + 6 * U * np.abs(G)) + FLT_MIN


def check_ul_loss(loss, ref, x32, alpha, what):
    _ratio("loss", np.abs(loss.astype(np.float64) - ref["loss"]), loss_bound(ref, x32, alpha), what)


def check_ul_grad(g, ref, gscale, alpha, what):
    g = g.astype(np.float64)
    zero = ((ref["my"] == 0) & (ref["Q"] == 0)) | (gscale == 0)
    assert (g[zero] == 0).all(), f"{what}: rows {np.nonzero(zero & (g != 0).any(1))[0]} should be all zero"
    tol = grad_bound(ref, gscale, alpha)
    _ratio("grad", np.where(zero[:, None], 0.0, np.abs(g - ref["grad"])), np.where(zero[:, None], 1.0, tol), what)


# ------------------------------------------------------------------------------------------------ data
def planted(V, B, T, rng, invalid=True):
    """(x (T * B, V) float32, target (T * B,) t-major, {name: row}): unit-scale random logits, captions over a few words
    so that prefixes repeat, and where V and T allow them (V >= 64, T >= 5) the planted rows of caption 0:
      t = 0  y = 7                       an exact tie at the maximum (columns 3 and V - 1)
      t = 1  y = 7   C = {}              the target among the prefix; the target saturated (x_y = max + 40)
      t = 2  y = 0   C = {7}             a saturated candidate (x_7 = max + 40: 1 - p_7 < 1e-7)
      t = 3  y >= V  C = {7}             (``invalid``; else y = 7) a 0 in the prefix
      t = 4  y = 9   C = {7}             a word twice, a 0 and an id >= V in the prefix; the candidate is the row maximum
      t = 10 (T = 64)                    a saturated target in a row that has candidates
    With T = 64 caption 1 holds 1 .. 63 in random order and 0 last (V >= 64): 63 candidates in its last row."""
    rows = T * B
    x = rng.standard_normal((rows, V))
    words = max(1, min(V - 1, 12))
    tg = rng.integers(1, words + 1, (T, B)) if V > 1 else np.zeros((T, B), np.int64)
    if V > 1 and T > 2:
        tg[T - 1, :] = 0                                     # a padding position at the end of every caption
    names = {}
    if V >= 64 and T >= 5:
        tg[:5, 0] = [7, 7, 0, V + 3 if invalid else 7, 9]
        r = lambda t: t * B
        a, b = 3, V - 1
        x[r(0), a] = x[r(0), b] = x[r(0)].max() + 1.0
        names["tie"] = r(0)
        x[r(1), 7] = x[r(1)].max() + 40.0
        names["target among the prefix, saturated"] = r(1)
        x[r(2), 7] = x[r(2)].max() + 40.0
        names["saturated candidate"] = r(2)
        names["invalid target"] = r(3)
        x[r(4), 7] = x[r(4)].max() + 1.0
        names["candidate is the maximum"] = r(4)
        if T == 64:
            tg[10, 0] = 5
            x[r(10), 5] = x[r(10)].max() + 40.0
            names["saturated target with candidates"] = r(10)
            if B > 1:
                tg[:63, 1] = rng.permutation(np.arange(1, 64))
                tg[63, 1] = 0
                names["63 candidates"] = 63 * B + 1
    return x.astype(np.float32), tg.reshape(-1), names


def assert_out_of_bands(ref):
    near = near_clip(ref["p"])
    assert not near.any(), f"test data: classes {np.argwhere(near)[:4]} sit on a clip bound"
    omp = 1.0 - ref["p"][ref["cmask"]]
    assert not ((omp > 1e-8) & (omp < 1e-5)).any(), "test data: a candidate sits on the bound 1 - p_c = 1e-7"


def run(be, x32, tgt, B, T, ld, shift, form, gscale, alpha):
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
    tg = None if tgt is None else dev(np.asarray(tgt), torch.int32)
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
    be.softmax_cce_unlikely(lg, tg, probs, loss, corr, dl, B, T, V, ld, gscale, alpha)
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


def verify_layout(be, x, tgt, B, T, ld, shift, gs, alpha, ref, what):
    """the five forms of one layout: the separate outputs against the reference and its bounds; the pad contract, the
    logits and the space in front of the view exactly, in every form; every other form bit for bit against the separate
    one.  Returns the separate form's result."""
    rows, V = x.shape
    got = {form: run(be, x, tgt, B, T, ld, shift, form, gs, alpha) for form in FORMS}
    nv4, host = got["separate"]["nv4"], got["separate"]["host"]
    what = f"{what} [{'reg<%d>' % nv4 if nv4 else 'generic'}]"
    for form, res in got.items():
        assert (res["shift_head"] == SENT).all(), f"{what} {form}: wrote in front of the logits view"
        if form in ("separate", "loss"):
            assert np.array_equal(res["logits"], host, equal_nan=True), f"{what} {form}: logits modified"
        else:                                    # aliased: the logits buffer is an output, its own pad the 'before'
            check_pad(res["logits"], host, V, nv4, f"{what} {form} logits buffer")
    sep = got["separate"]
    for k in ("probs", "dl"):                    # separate outputs: pad zero in the window, else the sentinel
        check_pad(sep[k], np.full_like(host, SENT), V, nv4, f"{what} {k}")
    check_probs(sep["probs"][:, :V], ref, f"{what} probs")
    check_ul_loss(sep["loss"], ref, x, alpha, f"{what} loss")
    assert np.array_equal(sep["corr"], (ref["amax"] == ref["y"]).astype(np.float32)), f"{what} correct_row"
    check_ul_grad(sep["dl"][:, :V], ref, gs, alpha, f"{what} dlogits")
    # one kernel, one set of values: every form writes the same bits
    p = sep["probs"][:, :V]
    assert np.array_equal(got["eval"]["logits"][:, :V], p) and np.array_equal(got["infer"]["logits"][:, :V], p), what
    assert np.array_equal(got["train"]["logits"][:, :V], sep["dl"][:, :V]), what
    for k in ("loss", "corr"):
        for form in ("loss", "train", "eval"):
            assert np.array_equal(got[form][k], sep[k]), (what, form, k)
    return sep


# ------------------------------------------------------------------------------------------------ every path, every form
@pytest.mark.parametrize("V", V_LIST)
def test_every_dispatch_path_and_output_form(be, V):
    gs = 0.25                                    # a float32 value: the reference sees the gscale the kernel sees
    for B, T in BT_LIST:
        rng = np.random.default_rng(1000 * T + V)
        x, tgt, names = planted(V, B, T, rng)
        for alpha in ALPHA_LIST:
            ref = reference(x, tgt, B, T, gs, alpha)
            assert_out_of_bands(ref)
            ncand = ref["cmask"].sum(1)
            assert (ncand[:B] == 0).all()
            if names:                            # the planted rows really sit where they should
                i = names["tie"]
                assert ref["amax"][i] == 3 and tgt[i] == 7
                i = names["target among the prefix, saturated"]
                assert ncand[i] == 0 and ref["my"][i] == 0 and ref["py"][i] > 1 - 1e-7 and (ref["grad"][i] == 0).all()
                i = names["saturated candidate"]
                assert ref["cmask"][i].nonzero()[0].tolist() == [7] and ref["Q"][i] == 0 and ref["my"][i] == 0
                assert abs(ref["ul"][i] - LOG_LO) < 1e-12 and abs(ref["loss"][i] - (1 + alpha) * LOG_LO) < 1e-9
                i = names["invalid target"]
                assert tgt[i] >= V and ref["cmask"][i].nonzero()[0].tolist() == [7] and ref["my"][i] == 0
                i = names["candidate is the maximum"]
                assert ref["cmask"][i].nonzero()[0].tolist() == [7] and ref["amax"][i] == 7 and ref["my"][i] == 1
                if T == 64:
                    i = names["saturated target with candidates"]
                    assert ref["my"][i] == 0 and ncand[i] >= 3 and ref["Q"][i] > 0
                    assert ncand[names["63 candidates"]] == 63
            seen = {}
            for name, ld, shift in layouts(V):
                sep = verify_layout(be, x, tgt, B, T, ld, shift, gs, alpha, ref, f"V={V} B={B} T={T} alpha={alpha} {name} ld={ld}")
                seen[name] = sep["nv4"]
            assert seen["odd"] == 0 and seen["shift"] == 0
            assert (seen["r4"] > 0) == (V <= 8192), f"V={V}: aligned rows ran {'the generic' if not seen['r4'] else 'a register'} kernel"


def test_no_target_with_a_gradient_buffer_writes_zero_rows(be):
    rng = np.random.default_rng(5)
    V, B, T = 257, 1, 3
    rows = B * T
    x = rng.standard_normal((rows, V)).astype(np.float32)
    for ld, shift in ((260, 0), (259, 0)):
        host = np.full((rows, ld), SENT, np.float32)
        host[:, :V] = x
        lg = dev(host.ravel())
        dl = torch.full((rows * ld,), SENT, device="cuda")
        loss = torch.full((rows,), SENT, device="cuda")
        be.softmax_cce_unlikely(lg, None, None, loss, loss, dl, B, T, V, ld, 0.5, 1.0)
        torch.cuda.synchronize()
        assert (dl.cpu().numpy().reshape(rows, ld)[:, :V] == 0).all() and (loss == SENT).all().item()


# ------------------------------------------------------------------------------------------------ alpha = 0, no candidates
@pytest.mark.parametrize("V", [5, 1024, 5001, 8193])
def test_without_candidates_it_is_the_plain_head(be, V):
    """alpha = 0, and the rows without candidates at alpha = 2: loss / correct / probs / dlogits inside
    tests/test_gpu_head.py's bounds of tnt_softmax_cce_f32 (its float64 reference, its check functions), and
    tnt_softmax_cce_f32 itself on the same data beside it"""
    rng = np.random.default_rng(2000 + V)
    B, T = 3, 5
    x, tgt, names = planted(V, B, T, rng, invalid=False)
    rows = B * T
    gs = 1.0 / rows
    for alpha in (0.0, 2.0):
        full = reference(x, tgt, B, T, gs, alpha)
        assert_out_of_bands(full)
        sel = np.arange(rows) if alpha == 0 else np.nonzero(full["cmask"].sum(1) == 0)[0]
        assert len(sel) >= B and (alpha == 0 or len(sel) < rows or V < 3)
        ref = head_reference(x[sel], tgt[sel], gs)
        for name, ld, shift in layouts(V):
            res = run(be, x, tgt, B, T, ld, shift, "separate", gs, alpha)
            what = f"V={V} alpha={alpha} {name}"
            check_pad(res["probs"], np.full_like(res["host"], SENT), V, res["nv4"], what)
            check_pad(res["dl"], np.full_like(res["host"], SENT), V, res["nv4"], what)
            check_probs(res["probs"][sel, :V], ref, what)
            check_loss(res["loss"][sel], ref, x[sel], what)
            check_grad(res["dl"][sel, :V], ref, gs, what)
            assert np.array_equal(res["corr"], (full["amax"] == tgt).astype(np.float32))
            if alpha:
                continue
            # the existing entry point on the same buffers' contents
            lg = dev(res["host"].ravel())
            probs, dl = torch.full((rows * ld,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")
            loss, corr = torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
            be.softmax_cce(lg, dev(tgt, torch.int32), probs, loss, corr, dl, rows, V, ld, gs)
            torch.cuda.synchronize()
            assert np.array_equal(corr.cpu().numpy(), res["corr"])
            check_loss(loss.cpu().numpy(), ref, x, what + " (tnt_softmax_cce_f32)")
            check_grad(dl.cpu().numpy().reshape(rows, ld)[:, :V], ref, gs, what + " (tnt_softmax_cce_f32)")


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(be):
    B, T, V, ld = 2, 2, 64, 64
    rows = B * T
    x0 = np.random.default_rng(1).standard_normal((rows, ld)).astype(np.float32)
    x = dev(x0)
    tg = torch.ones(rows, dtype=torch.int32, device="cuda")
    outs = [torch.full((rows * ld,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda"),
            torch.full((rows,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")]
    probs, loss, corr, dl = outs

    def untouched():
        torch.cuda.synchronize()
        return all((o == SENT).all().item() for o in outs)

    ok = dict(b=B, t=T, v=V, l=ld, lg=x, a=0.5)
    for bad in (dict(b=-1), dict(t=0), dict(t=-2), dict(t=65), dict(v=0), dict(v=-3), dict(l=V - 1), dict(lg=None),
                dict(a=-0.1), dict(a=float("nan")), dict(a=float("inf")), dict(a=float("-inf"))):
        c = {**ok, **bad}
        with pytest.raises(RuntimeError):
            be.softmax_cce_unlikely(c["lg"], tg, probs, loss, corr, dl, c["b"], c["t"], c["v"], c["l"], 0.5, c["a"])
    assert untouched(), "a rejected call wrote an output"
    be.softmax_cce_unlikely(x, tg, probs, loss, corr, dl, 0, T, V, ld, 0.5, 0.5)          # B == 0: a no-op
    be.softmax_cce_unlikely(x, tg, None, loss, corr, x, 0, T, V, ld, 0.5, 0.5)
    assert untouched(), "a B == 0 call wrote an output"
    assert np.array_equal(x.cpu().numpy(), x0)
