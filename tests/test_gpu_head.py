"""The softmax + cross-entropy head (tnt_softmax_cce_f32) and the two argmax entry points on a real MI355X, against
float64 numpy (oracle/ops.py).

tnt_softmax_cce_f32 picks one of six kernels from V and alignment: softmax_cce_reg_kernel<NV4> for 16-byte-aligned rows
with ld % 4 == 0 and ceil(V / 1024) inside one of the buckets of SMX_LADDER, softmax_cce_kernel (generic) for everything
else.  V_LIST hits every bucket on both sides of each bound (tests/test_host_softmax_dispatch.py keeps it complete
against the source), and every V also runs on the generic kernel (odd ld, or a logits view one float into its buffer)
with the same values.  Outputs are checked element by element with tolerances derived below, not scaled by a row
maximum; pad columns are filled with NaN / +1e30 and the pad contract of each kernel is asserted exactly."""
import math

import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # float32 unit roundoff
FLT_MIN = 2.0 ** -126           # below this a result may be a flushed / rounded subnormal: absolute floor
SENT = 1234.5                   # sentinel in every output buffer: no output of the kernel can take this value
CLIP = O.CCE_EPS

# the dispatch ladder of every softmax head, tnt_row_ladder (csrc/tnt_rowhead.h), restated: (largest nv4 = ceil(V / 1024)
# of the bucket, NV4 of the register kernel it launches); anything past the last bucket, and any unaligned call, runs the
# generic kernel.  tests/test_host_softmax_dispatch.py checks this table and V_LIST against the source.
SMX_LADDER = ((1, 1), (2, 2), (4, 4), (5, 5), (8, 8))
V_LIST = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 5001, 5120, 5121,
          8192, 8193, 16384, 40000]
MAX_ELEMS = 64 * 40004          # rows * ld of one launch stays at or below this

# Tie placements (first index, second index) for the register kernel's equality pass: inside one float4, across lanes
# (j, j+4), across lanes and waves (lane 63 of wave 0 -> lane 0 of wave 1), across waves (j, j+256 floats = +64 float4),
# across registers (j, j+1024); (j, V-1) is added per V.  The first index must win on both kernels.
TIES = ((9, 10), (12, 15), (20, 24), (252, 256), (100, 356), (100, 1124), (1500, 2524))


def r4(v):
    return (v + 3) // 4 * 4


def reg_nv4(V, ld, aligned):
    """NV4 of the register kernel tnt_softmax_cce_f32 launches for this call, 0 for the generic kernel"""
    if not aligned or ld % 4:
        return 0
    nv4 = (V + 1023) // 1024
    for bound, n in SMX_LADDER:
        if nv4 <= bound:
            return n
    return 0


# Layouts of one launch: (name, ld, float offset of the logits view).  "odd" and "shift" force the generic kernel at
# every V; "r4+4" makes a padded row longer than a register-kernel window at the bucket bounds (V = 1024, ld = 1028).
def layouts(V):
    return (("r4", r4(V), 0), ("r4+4", r4(V) + 4, 0), ("odd", V + 1 + V % 2, 0), ("shift", r4(V), 1))


# ------------------------------------------------------------------------------------------------ tolerances
# Error model of both kernels for one row (u = 2^-24, first order; m = max_j x_j, d_j = x_j - m <= 0):
#   * d_j = fl(x_j - m): one rounding, |error| <= u |d_j| in the exponent -> relative u |d_j| on exp(d_j);
#   * expf: <= 2 ulp = 4u relative;  so t_j = expf(d_j) carries u (|d_j| + 4);
#   * Z = sum_j t_j, all terms positive: the terms' own errors add up to u (4 + w), w = sum_j p_j |d_j| (computed here in
#     float64), and the summation to u * (the longest chain of additions any term passes through): ceil(V / 256) serial
#     adds per thread in the generic kernel (the register kernel's per-thread chain, NV4 + 2, is never longer plus the
#     2 below), 6 levels of the wave tree, 3 across the 4 waves, 2 for the register kernel's pair adds;
#   * p_j = t_j * fl(1 / Z): reciprocal and product, 2 roundings = 2u (4u allowed);
#   (below 1e-30 an absolute FLT_MIN is added: expf may return a subnormal or flush it to zero)
#   so |p_j - p64_j| / p64_j <= u (|d_j| + w + ceil(V / 256) + 4 + 4 + 11 + 4) = u (|d_j| + w + ceil(V / 256) + 23).
# A factor 2 covers the second-order terms and the rounding of the float64 reference: REL_j = 2u (|d_j| + BASE), with
# BASE = w + ceil(V / 256) + 25.  |log p - log p64| is bounded by the same REL_j (/(1 - REL_j)).
# Loss: from_logits=False, l = -log(p_y): |dl| <= REL_y + 2 ulp of l; from_logits=True, l = (log Z + m) - x_y: Z's error
# plus 2 ulp of log Z and one rounding per add, each <= 4u max(|m|, |x_y|, |log Z|).  Both are inside
# 2u (BASE + |d_y| + 12 M), M = max(1, |m|, |x_y|, |log Z|) (the 1 covers the clipped case, -log(1 - 1e-7) in float32).
# Gradient (p_j - [j == y]) * gscale: the p error, the subtraction (exact for p_y >= 1/2) and the product:
# |gscale| (REL_j p64_j + 4u |p64_j - [j == y]| + FLT_MIN).
# Pad handling, argmax, correct and every zero row are exact.
WORST = {"p": 0.0, "log p": 0.0, "loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nworst observed error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


def _ratio(key, err, tol, what):
    r = float(np.max(err / tol)) if err.size else 0.0
    WORST[key] = max(WORST[key], r)
    assert r <= 1.0, f"{what}: {key} error {r:.3g} x its bound (worst at {np.unravel_index(np.argmax(err / tol), err.shape)})"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def near_clip(py):
    """p_y (float64) too close to a clip bound for a float32 kernel and a float64 reference to agree on the clip: the
    kernels compare fl(p_y) with 1e-7f and with fl(1 - 1e-7) = 1 - 2^-23, and near 1 fl(p_y) moves in steps of 2^-24
    (fl(Z) in steps of 2^-23): from 1 - 1e-7 up to 1 - 2^-24 the two may differ.  Test data stay out of these bands."""
    return (np.abs(py / CLIP - 1) < 1e-4) | ((py > 1 - 1.2e-7) & (py < 1 - 4e-8))


def reference(x32, y, gscale, from_logits=False, mask_zero=False):
    """float64 softmax / loss / gradient of float32 logits x32 (rows, V), as mock_backend.softmax_cce defines them"""
    x = x32.astype(np.float64)
    rows, V = x.shape
    m = x.max(1)
    d = x - m[:, None]
    p = O.softmax(x)
    ref = {"p": p, "d": d, "m": m, "logZ": np.log(np.exp(d).sum(1)), "w": (p * -d).sum(1),
           "nser": math.ceil(V / 256), "amax": np.argmax(x32, 1)}
    if y is None:
        return ref
    y = np.asarray(y, np.int64)
    live = (y != 0) if mask_zero else np.ones(rows, bool)
    py = p[np.arange(rows), y]
    if from_logits:
        loss = O.sparse_cce_from_logits(x, y)[0]
        oh = np.zeros_like(p)
        oh[np.arange(rows), y] = 1.0
        grad = (p - oh) * gscale
    else:
        near = near_clip(py)
        assert not near.any(), f"test data: p_y of rows {np.nonzero(near)[0]} sits on a clip bound"
        loss = O.cce_from_probs(p, y)
        grad = O.cce_softmax_bwd(p, y, np.full(rows, gscale))
    ref.update(y=y, loss=np.where(live, loss, 0.0), grad=np.where(live[:, None], grad, 0.0), live=live)
    return ref


def check_probs(p, ref, what, rng=None):
    p = p.astype(np.float64)
    p64, d = ref["p"], ref["d"]
    rel = 2 * U * (np.abs(d) + (ref["w"] + ref["nser"] + 25)[:, None])
    assert np.isfinite(p).all() and (p >= 0).all(), what
    big = p64 >= 1e-30
    _ratio("p", np.where(big, np.abs(p - p64), 0.0), np.where(big, rel * p64, 1.0), what)
    assert (np.abs(p - p64) <= rel * p64 + FLT_MIN)[~big].all(), what     # may be subnormal or flushed to zero
    # log p at sampled positions (what beam scores, sampling and SCST read): the argmax, the last column, 32 random
    rows, V = p.shape
    rng = rng or np.random.default_rng(0)
    cols = np.concatenate([ref["amax"][:, None], np.full((rows, 1), V - 1), rng.integers(0, V, (rows, 32))], 1)
    r = np.repeat(np.arange(rows)[:, None], cols.shape[1], 1)
    ok = big[r, cols]
    assert (p[r, cols][ok] > 0).all(), what
    lp = np.log(np.where(ok, p[r, cols], 1.0)) - np.log(np.where(ok, p64[r, cols], 1.0))
    tl = rel[r, cols]
    _ratio("log p", np.abs(lp), tl / (1 - tl), what)


def check_loss(loss, ref, x32, what):
    rows = x32.shape[0]
    y = ref["y"]
    dy = np.abs(ref["d"][np.arange(rows), y])
    M = np.maximum.reduce([np.ones(rows), np.abs(ref["m"]), np.abs(x32[np.arange(rows), y].astype(np.float64)),
                           np.abs(ref["logZ"])])
    tol = 2 * U * (ref["w"] + ref["nser"] + 25 + dy + 12 * M)
    loss = loss.astype(np.float64)
    assert (loss[~ref["live"]] == 0).all(), what
    _ratio("loss", np.abs(loss - ref["loss"]), tol, what)


def check_grad(g, ref, gscale, what):
    g = g.astype(np.float64)
    rows, V = g.shape
    p64 = ref["p"]
    oh = np.zeros_like(p64)
    oh[np.arange(rows), ref["y"]] = 1.0
    rel = 2 * U * (np.abs(ref["d"]) + (ref["w"] + ref["nser"] + 25)[:, None])
    tol = abs(gscale) * (rel * p64 + 4 * U * np.abs(p64 - oh) + FLT_MIN)
    zero = (ref["grad"] == 0).all(1)                 # clip active, mask_zero row, or gscale 0: exactly zero
    assert (g[zero] == 0).all(), f"{what}: rows {np.nonzero(zero & (g != 0).any(1))[0]} should be all zero"
    _ratio("grad", np.abs(g - ref["grad"]), np.where(zero[:, None], 1.0, tol) if gscale else np.ones_like(tol), what)


def fill_pad(host, V):
    host[:, V::2] = np.nan
    host[:, V + 1::2] = 1e30


def check_pad(after, before, V, nv4, what):
    """pad columns [V, ld) of an output: zero inside the register kernel's window [0, 1024 NV4), untouched elsewhere"""
    ld = after.shape[1]
    zeroed = (np.arange(V, ld) < 1024 * nv4)[None, :]
    want = np.where(zeroed, np.float32(0), before[:, V:])
    assert np.array_equal(after[:, V:], want, equal_nan=True), f"{what}: pad columns (register window {1024 * nv4})"


def run(be, x32, y, ld, shift=0, form="separate", gscale=None, r0=0):
    """one tnt_softmax_cce_f32 launch in one of the library's output forms; returns host copies of everything it may
    have written plus the dispatch it took.  Forms:
      separate  probs, dlogits, loss, correct all separate (the bench / test form);
      train     probs = None, dlogits = logits (nic.py, lc_nic.py training step);
      eval      probs = logits, dlogits = None, gscale = 0 (evaluation step);
      infer     target = None, probs = logits, no loss / correct / gradient pointer (decoders);
      tt        from_logits, mask_zero, correct = None, probs = None, dlogits a separate buffer at row offset r0
                (think_and_tell.py)"""
    rows, V = x32.shape
    gscale = 1.0 / rows if gscale is None else gscale
    host = np.full((rows, ld), SENT, np.float32)
    host[:, :V] = x32
    fill_pad(host, V)
    buf = torch.full((shift + rows * ld,), SENT, device="cuda")
    buf[shift:] = dev(host.ravel())
    lg = buf[shift:]
    out = lambda n=rows: torch.full((n * ld,), SENT, device="cuda")
    vec = lambda: torch.full((rows,), SENT, device="cuda")
    tg = None if y is None else dev(np.asarray(y), torch.int32)
    probs = dl = loss = corr = dlb = None
    fl = mz = False
    if form == "separate":
        probs, dl, loss, corr = out(), out(), vec(), vec()
    elif form == "train":
        dl, loss, corr = lg, vec(), vec()
    elif form == "eval":
        probs, loss, corr, gscale = lg, vec(), vec(), 0.0
    elif form == "infer":
        probs, tg = lg, None
    elif form == "tt":
        dlb = out(r0 + rows)
        dl, loss, fl, mz = dlb[r0 * ld:], vec(), True, True
    else:
        raise ValueError(form)
    be.softmax_cce(lg, tg, probs, loss, corr, dl, rows, V, ld, gscale, from_logits=fl, mask_zero=mz)
    torch.cuda.synchronize()
    aligned = shift % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (lg, probs, dl))
    res = {"nv4": reg_nv4(V, ld, aligned), "gscale": gscale, "host": host, "fl": fl, "mz": mz,
           "logits": lg.cpu().numpy().reshape(rows, ld), "shift_head": buf[:shift].cpu().numpy()}
    for k, t in (("probs", probs), ("dl", dl), ("loss", loss), ("corr", corr)):
        res[k] = None if t is None else t.cpu().numpy()
    for k in ("probs", "dl"):
        if res[k] is not None:
            res[k] = res[k].reshape(rows, ld)
    if dlb is not None:
        res["dl_head"] = dlb[:r0 * ld].cpu().numpy()
    return res


def verify(res, ref, x32, what, form="separate"):
    """every output the form writes against the float64 reference, the pad contract, and nothing else written"""
    rows, V = x32.shape
    nv4, host = res["nv4"], res["host"]
    what = f"{what} [{'reg<%d>' % nv4 if nv4 else 'generic'}]"
    assert (res["shift_head"] == SENT).all(), f"{what}: wrote in front of the logits view"
    sep = {"separate": ("probs", "dl"), "tt": ("dl",)}.get(form, ())
    for k in sep:                            # separate outputs: pad zero in the window, else the sentinel
        check_pad(res[k], np.full_like(host, SENT), V, nv4, f"{what} {k}")
    if form in ("separate",):                # logits untouched
        assert np.array_equal(res["logits"], host, equal_nan=True), f"{what}: logits modified"
    else:                                    # aliased: the logits buffer is an output, its own pad the 'before'
        check_pad(res["logits"], host, V, nv4 if form != "tt" else 0, f"{what} logits buffer")
        if form == "tt":
            assert np.array_equal(res["logits"], host, equal_nan=True), f"{what}: logits modified"
    if res["probs"] is not None:
        check_probs(res["probs"][:, :V], ref, f"{what} probs")
    if "loss" in ref:
        if res["loss"] is not None:
            check_loss(res["loss"], ref, x32, f"{what} loss")
        if res["corr"] is not None:
            assert np.array_equal(res["corr"], (ref["amax"] == ref["y"]).astype(np.float32)), f"{what} correct_row"
        if res["dl"] is not None:
            check_grad(res["dl"][:, :V], ref, res["gscale"], f"{what} dlogits")
    if "dl_head" in res:
        assert (res["dl_head"] == SENT).all(), f"{what}: wrote rows in front of the dlogits view"


def random_logits(rng, rows, V, scale=3.0):
    x = (rng.standard_normal((rows, V)) * scale).astype(np.float32)
    if rows > 1 and V > 1:
        x[-1, V - 1] = x[-1].max() + 1           # unique maximum in the last column
    y = rng.integers(0, V, rows)
    y[0] = int(np.argmax(x[0]))                  # at least one correct row
    for i in range(rows):                        # keep random rows clear of the clip bounds (see near_clip)
        while near_clip(O.softmax(x[i].astype(np.float64))[y[i]]):
            x[i] *= np.float32(0.5)
    return x, y


# ------------------------------------------------------------------------------------------------ (a) every dispatch path
@pytest.mark.parametrize("V", V_LIST)
def test_every_dispatch_path(be, V):
    rng = np.random.default_rng(V)
    for rows in (1, 7, 96):
        rows = min(rows, MAX_ELEMS // (r4(V) + 4))
        x, y = random_logits(rng, rows, V)
        ref = reference(x, y, 1.0 / rows)
        seen = {}
        for name, ld, shift in layouts(V):
            res = run(be, x, y, ld, shift)
            verify(res, ref, x, f"V={V} rows={rows} {name} ld={ld}")
            seen[name] = (res["nv4"], res["corr"])
            am = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
            be.argmax_rows(torch.tensor(res["logits"].ravel(), device="cuda"), am, rows, V, ld)
            assert np.array_equal(am.cpu().numpy(), ref["amax"]), f"V={V} {name}: argmax_rows"
        assert seen["odd"][0] == 0 and seen["shift"][0] == 0
        for name, (nv4, corr) in seen.items():
            assert np.array_equal(corr, seen["odd"][1]), f"V={V}: correct_row of {name} differs from the generic kernel's"


# ------------------------------------------------------------------------------------------------ (b) output forms
FORM_CASES = [(1000, 1000, 0), (1000, 1000, 1), (5001, 5004, 0), (5001, 5004, 1), (4096, 4100, 0), (9000, 9000, 0)]


def _spiky(rng, rows, V):
    x, y = random_logits(rng, rows, V)
    x[1, y[1]] = 60.0                            # p_y = 1 in float32 and > 1 - 1e-7 in float64: clip active, zero row
    y[2] = 5 % V
    x[2, y[2]] = -60.0                           # p_y < 1e-7: clip active
    return x, y


@pytest.mark.parametrize("V,ld,shift", FORM_CASES)
def test_output_forms(be, V, ld, shift):
    rng = np.random.default_rng(V + shift)
    rows = 48
    x, y = _spiky(rng, rows, V)
    gs = 1.0 / rows
    ref = reference(x, y, gs)
    got = {}
    for form in ("separate", "train", "eval", "infer"):
        res = run(be, x, y if form != "infer" else None, ld, shift, form, gscale=gs)
        verify(res, ref if form != "infer" else {k: v for k, v in ref.items() if k not in ("loss", "y")}, x,
               f"V={V} ld={ld} shift={shift} {form}", form)
        got[form] = res
    assert (got["separate"]["dl"][1:3, :V] == 0).all()
    # one kernel, one set of values: every form writes the same bits
    p = got["separate"]["probs"][:, :V]
    assert np.array_equal(got["eval"]["logits"][:, :V], p) and np.array_equal(got["infer"]["logits"][:, :V], p)
    assert np.array_equal(got["train"]["logits"][:, :V], got["separate"]["dl"][:, :V])
    for k in ("loss", "corr"):
        assert np.array_equal(got["train"][k], got["separate"][k]) and np.array_equal(got["eval"][k], got["separate"][k])


@pytest.mark.parametrize("V,ld,shift", FORM_CASES)
def test_think_and_tell_form(be, V, ld, shift):
    rng = np.random.default_rng(7 * V + shift)
    rows, r0 = 45, 3
    x, y = random_logits(rng, rows, V)
    y[::5] = 0                                   # padding targets: loss 0, gradient row all zero
    x[1, y[1]] = 60.0                            # from_logits: no clip, a live gradient row and a loss near 0
    for gs in (1.0 / rows, 0.37):
        ref = reference(x, y, gs, from_logits=True, mask_zero=True)
        res = run(be, x, y, ld, shift, "tt", gscale=gs, r0=r0)
        verify(res, ref, x, f"V={V} ld={ld} shift={shift} tt gscale={gs}", "tt")
        assert (res["loss"][::5] == 0).all() and (res["dl"][::5, :V] == 0).all()
        assert (res["dl"][1, :V] != 0).any()


# ------------------------------------------------------------------------------------------------ (c) value edges
def edge_rows(V, rng):
    """rows of value edges + their targets: equal logits, planted ties, 80-100 spreads, p_y on either side of both clip
    bounds.  Returns (x (rows, V) float32, y, description per row)."""
    xs, ys, names = [], [], []

    def add(x, y, name):
        xs.append(np.asarray(x, np.float32)); ys.append(int(y)); names.append(name)

    add(np.full(V, 0.5), V // 2, "equal logits")
    pairs = [(a, b) for a, b in TIES if b < V] + [(min(3, V - 2), V - 1)]
    for k, (a, b) in enumerate(pairs):
        x = rng.standard_normal(V) * 3
        x[a] = x[b] = x.max() + 2
        add(x, a if k % 2 == 0 else b, f"tie {a},{b}")
    for k in range(3):
        x = rng.uniform(-100, -80, V) if k else rng.uniform(-100, 0, V)
        x[rng.integers(0, V, 3)] = 0.0
        add(x + 7.0 * k, rng.integers(0, V), f"spread {k}")
    bg = lambda: rng.uniform(-120, -100, V)
    for q, name in ((CLIP * (1 + 1e-3), "p_y just above 1e-7"), (CLIP * (1 - 1e-3), "p_y just below 1e-7")):
        x = bg(); x[0] = 0.0; x[V - 1] = math.log(q / (1 - q))
        add(x, V - 1, name)
    for s, name in ((3e-7, "p_y = 1 - 3e-7 (inside)"), (3e-8, "p_y = 1 - 3e-8 (outside)")):
        x = bg(); x[V // 3] = 0.0; x[V - 1] = math.log(s)
        add(x, V // 3, name)
    return np.stack(xs), np.asarray(ys), names


@pytest.mark.parametrize("V", [1100, 2600, 5001, 8192, 9000])
def test_value_edges(be, V):
    rng = np.random.default_rng(V + 1)
    x, y, names = edge_rows(V, rng)
    rows = len(names)
    for gs in (1.0 / rows, 0.37, 2.5):
        ref = reference(x, y, gs)
        # the designed clip rows really sit where they should (reference decision = keras's)
        act = ~(ref["grad"] == 0).all(1)
        for i, n in enumerate(names):
            if "above" in n or "inside" in n:
                assert act[i], n
            if "below" in n or "outside" in n:
                assert not act[i], n
        corr = {}
        for name, ld, shift in (("r4", r4(V), 0), ("shift", r4(V), 1)):
            res = run(be, x, y, ld, shift, gscale=gs)
            verify(res, ref, x, f"V={V} {name} gscale={gs}")
            p = res["probs"][:, :V]
            assert (p[0] == p[0, 0]).all() and abs(p[0, 0] * V - 1) < 1e-5, "equal logits: uniform p"
            corr[name] = res["corr"]
            am = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
            be.argmax_rows(torch.tensor(res["logits"].ravel(), device="cuda"), am, rows, V, ld)
            am = am.cpu().numpy()
            assert np.array_equal(am, ref["amax"]), f"V={V} {name}: argmax_rows {am} != {ref['amax']}"
            assert am[0] == 0
            for i, n in enumerate(names):
                if n.startswith("tie"):
                    assert am[i] == int(n.split()[1].split(",")[0]), n
        assert np.array_equal(corr["r4"], corr["shift"]), "correct_row: register and generic kernels disagree"
        assert np.array_equal(corr["r4"], (ref["amax"] == y).astype(np.float32))


# ------------------------------------------------------------------------------------------------ (e) argmax entry points
def first_max(x):
    """np.argmax with NaN ignored; 0 for a row with nothing above -inf"""
    xx = np.where(np.isnan(x), -np.inf, x)
    return np.where((xx == -np.inf).all(-1), 0, np.argmax(xx, -1))


def argmax_rows_data(V, rng):
    rows = [rng.standard_normal(V) * 3 for _ in range(5)]
    for a, b in [(a, b) for a, b in TIES if b < V] + [(0, V - 1)] * (V > 1):
        x = rng.standard_normal(V) * 3
        x[a] = x[b] = x.max() + 2
        rows.append(x)
    rows.append(np.full(V, -np.inf))                         # all -inf -> 0
    x = np.full(V, np.nan)
    rows.append(x)                                           # all NaN -> 0
    x = rng.standard_normal(V)
    x[rng.integers(0, V, max(1, V // 7))] = np.nan           # NaNs ignored
    x[0] = np.nan
    rows.append(x)
    x = np.full(V, -np.inf); x[V - 1] = -1e30; x[0] = np.nan
    rows.append(x)                                           # the one finite entry is last
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("V", V_LIST)
def test_argmax_rows(be, V):
    rng = np.random.default_rng(3 * V)
    x = argmax_rows_data(V, rng)
    want = first_max(x)
    rows = x.shape[0]
    for ld in sorted({V, V + 3, r4(V) + 4}):
        host = np.full((rows, ld), 0, np.float32)
        host[:, :V] = x
        fill_pad(host, V)                                    # NaN / +1e30 in the pad must not win
        out = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
        be.argmax_rows(dev(host), out, rows, V, ld)
        got = out.cpu().numpy()
        assert np.array_equal(got[:rows], want), f"V={V} ld={ld}: {got[:rows]} != {want}"
        assert got[rows] == -7


@pytest.mark.parametrize("B,T,V", [(1, 1, 1), (2, 3, 4), (3, 2, 257), (4, 5, 1025), (2, 2, 8193), (64, 15, 5001)])
def test_onehot_argmax(be, B, T, V):
    rng = np.random.default_rng(B * T * V)
    ids = rng.integers(0, V, (B, T))
    oh = np.zeros((B, T, V), np.float32)
    np.put_along_axis(oh, ids[..., None], 1.0, -1)
    if V > 1:                                                # two ones: the first wins
        for k, (b, t) in enumerate(zip(rng.integers(0, B, 8), rng.integers(0, T, 8))):
            a, c = sorted(rng.choice(V, 2, replace=False)) if k % 2 else (ids[b, t], V - 1)
            if a == c:
                continue
            oh[b, t] = 0; oh[b, t, a] = oh[b, t, c] = 1.0
            ids[b, t] = min(a, c)
    for a, c in [(a, c) for a, c in TIES if c < V]:          # tie placements of the register kernel's argmax
        b, t = rng.integers(0, B), rng.integers(0, T)
        oh[b, t] = 0; oh[b, t, a] = oh[b, t, c] = 1.0
        ids[b, t] = a
    out = torch.full((B * T + 1,), -7, dtype=torch.int32, device="cuda")
    be.onehot_argmax(dev(oh), out, B, T, V)
    got = out.cpu().numpy()
    assert np.array_equal(got[:B * T].reshape(T, B).T, ids)
    assert got[B * T] == -7


# ------------------------------------------------------------------------------------------------ (f) bad arguments
def test_bad_arguments_launch_nothing(be):
    rows, V, ld = 4, 64, 64
    x = dev(np.random.default_rng(1).standard_normal((rows, ld)))
    tg = torch.zeros(rows, dtype=torch.int32, device="cuda")
    outs = [torch.full((rows * ld,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda"),
            torch.full((rows,), SENT, device="cuda"), torch.full((rows * ld,), SENT, device="cuda")]
    ids = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return all((o == SENT).all().item() for o in outs) and (ids == -7).all().item()

    probs, loss, corr, dl = outs
    for r, v, l, lg in ((rows, 0, ld, x), (rows, -3, ld, x), (rows, V, V - 1, x), (rows, V, ld, None), (-1, V, ld, x)):
        with pytest.raises(RuntimeError):
            be.softmax_cce(lg, tg, probs, loss, corr, dl, r, v, l, 0.5)
    for r, v, l, lg in ((rows, 0, ld, x), (rows, V, V - 1, x), (rows, V, ld, None), (-1, V, ld, x)):
        with pytest.raises(RuntimeError):
            be.argmax_rows(lg, ids, r, v, l)
    for b, t, v, lg in ((2, 2, 0, x), (2, 2, -1, x), (2, 2, V, None), (-1, 2, V, x)):
        with pytest.raises(RuntimeError):
            be.onehot_argmax(lg, ids, b, t, v)
    assert untouched(), "a rejected call wrote an output"
    # rows == 0 (an empty batch tail) is a no-op that writes nothing
    be.softmax_cce(x, tg, probs, loss, corr, dl, 0, V, ld, 0.5)
    be.softmax_cce(x, tg, None, loss, corr, x, 0, V, ld, 0.5)
    be.argmax_rows(x, ids, 0, V, ld)
    be.onehot_argmax(x, ids, 0, 2, V)
    be.onehot_argmax(x, ids, 2, 0, V)
    assert untouched(), "a rows == 0 call wrote an output"
    assert np.array_equal(x.cpu().numpy(), np.random.default_rng(1).standard_normal((rows, ld)).astype(np.float32))
