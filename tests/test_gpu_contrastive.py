"""tnt_contrastive_loss_f32 on a real MI355X against tests/contrastive_oracle.py (float64; checked against central differences
and torch autograd in tests/test_host_contrastive.py).

Shapes (B, G): (1, 1); (2, 3); (3, 5) scalar tail only; (5, 63), (7, 65), (16, 64) around one 64-column chunk and one
16-row tile; (17, 20) one more than a tile in B; (64, 512) the workload's; (65, 516); (130, 32) more rows than any one
workgroup's waves; (3, 2048) the widest.  Each hard + symmetric; the four option combinations at (7, 65) and (64, 512); row
strides above G with NaN in the pads, dz absent, dz in place of z, pointers off 16-byte alignment; a zero target row, all
target rows zero, two identical targets, a z row below the epsilon; temperatures 0.07 and 0.5.  Every output and the
workspace lie in front of guard sentinels (tests/test_gpu_attention_paths.guarded).

Bounds, derived: inputs lie in [-1, 1], u = 2^-24, t = inv_temperature, Bv the number of valid rows.
  cosine   three G-term sums, two roots, two divisions: |cos - ref| <= 4 (G + 8) u   (tests/test_gpu_semantic.py)
  logit    one more multiplication of a value <= t:     eL = 4 (G + 9) u t;  the target Gram likewise, eS = 4 (G + 9) u ts
  lse      moving every input by <= eL moves a log-sum-exp by <= eL; then exp of a rounded difference |l - max| <= 2 t, a
           Bv-term sum of terms <= 1 whose total is >= 1, log, and the addition of the maximum (|lse| <= t + ln Bv):
           eLSE = eL + (Bv + 16 + 3 t + ln Bv) u
  P        Pr_ij = exp(L_ij - lse_i) and Pc_ij: RELATIVE error eP = 1.01 (eL + eLSE + 4 u) (e^x - 1 <= 1.01 x below 0.02), so a
           row's or a column's absolute errors add up to eP times its sum, not to Bv eP; soft Q_ij likewise with
           eQ = 1.01 (2 eS + (Bv + 16 + 3 ts) u), hard eQ = 0
  loss_row hard: lse - L_ii:  eLSE + eL + 4 (2 t + ln Bv) u   (roundings of values <= 2 t + ln Bv)
           soft: lse - sum_j Q_ij L_ij, |L| <= t:  eLSE + eL + t eQ + (Bv + 8) t u + 4 (2 t + ln Bv) u
  dz       with a_ij = (1 - b)(Pr - Q)_ij + b (Pc_ij - Q_ji), |P - Q| <= 1, s = weight t / Bv and gmax = max |gn|:
           sum_j |a_ij - ref| <= dA_i = (1 - b)(eP sum_j Pr_ij + eQ sum_j Q_ij) + b (eP sum_j Pc_ij + eQ sum_j Q_ji)
           |dzn_ic - ref| <= E_i = s gmax (dA_i + (sum_j |a_ij|) (G + Bv + 24) u)        (ig, the products, the Bv-term sum)
           |dz_ic - ref| <= iz_i (E_i (1 + |zn_ic| sum_c |zn_ic|) + |zn_ic| (4 G + 24) u sum_c |zn_ic dzn_ic|) + (G + 12) u |dz_ic|
           and iz_i E_i + (G + 12) u |dz_ic| for a z row below the epsilon (no projection there)
  hit_row  exact wherever the reference's two largest logits of the row differ by more than 2 eL; the share of rows this
           leaves out is asserted to be at most 2 % for every case (the seeds are chosen for it, on the reference alone)
  out      exactly the ascending float32 sums of loss_row / hit_row over max(Bv, 1); run to run: the same bits
A worst-case bound is loose; test_bound_discriminates (CPU) shows that at every shape with B >= 5 it still rejects the float64
reference evaluated with inv_temperature * 1.01 and the reference without the caption -> scan term."""
import functools

import numpy as np
import pytest
import torch

import contrastive_oracle as CO

gpu = pytest.mark.gpu
UNIT = 2.0 ** -24
SENT_I = -7
SHAPES = [(1, 1), (2, 3), (3, 5), (5, 63), (7, 65), (16, 64), (17, 20), (64, 512), (65, 516), (130, 32), (3, 2048)]
OPTIONS = [(None, True), (None, False), (0.5, True), (0.5, False)]         # (soft_temperature, symmetric)
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
f32 = lambda x: float(np.float32(x))
WEIGHT = 0.75
SEEDS = {(65, 516): 3, (3, 2048): 1}          # for the 2 % clause of the hit check; test_bound_discriminates and check() assert it


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


@functools.lru_cache(maxsize=None)
def case(B, G, temperature=0.07, soft_temperature=None, symmetric=True, kind="plain", seed=0):
    """(z, g float32 on the host, the float64 reference as CO.evaluate's dict, (inv_t, soft_inv_t)); computed once per case"""
    rng = np.random.default_rng(1000 * B + G + seed + SEEDS.get((B, G), 0))
    z = rng.uniform(-1, 1, (B, G)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, G)).astype(np.float32)
    if kind == "zero_row":
        g[B // 2] = 0
    if kind == "all_zero":
        g[:] = 0
    if kind == "twins":
        g[B - 1] = g[0]
    if kind == "tiny_z":
        z[1] = (1e-9 * z[1]).astype(np.float32)
    inv_t, soft = f32(1.0 / temperature), 0.0 if soft_temperature is None else f32(1.0 / soft_temperature)
    z.setflags(write=False); g.setflags(write=False)
    return z, g, CO.evaluate(z, g, inv_t, soft, symmetric, WEIGHT), (inv_t, soft)


def bounds(d, G, inv_t, soft, twins=False):
    """(loss_row bound [Bv], dz bound [Bv][G], rows whose hit is decided) from the reference's own quantities; ``twins``: the
    last target row repeats the first, so the last column repeats the first bit for bit and is no rival of its own"""
    v, Bv = d["v"], d["Bv"]
    ln = np.log(max(Bv, 1))
    eL, eS = 4 * (G + 9) * UNIT * inv_t, 4 * (G + 9) * UNIT * soft
    eLSE = eL + (Bv + 16 + 3 * inv_t + ln) * UNIT
    eP = 1.01 * (eL + eLSE + 4 * UNIT)
    eQ = 1.01 * (2 * eS + (Bv + 16 + 3 * soft) * UNIT) if soft > 0 else 0.0
    assert eP <= 0.02 and eQ <= 0.02
    row = eLSE + eL + 4 * (2 * inv_t + ln) * UNIT + (inv_t * eQ + (Bv + 8) * inv_t * UNIT if soft > 0 else 0.0)
    b, Pr, Pc, Q, QT = d["b"], d["Pr"], d["Pc"], d["Q"], d["QT"]
    A = np.abs((1 - b) * (Pr - Q) + b * (Pc - QT)).sum(1)
    dA = (1 - b) * (eP * Pr.sum(1) + eQ * Q.sum(1)) + b * (eP * Pc.sum(1) + eQ * QT.sum(1))
    E = (WEIGHT * inv_t / Bv) * np.abs(d["gn"][v]).max() * (dA + A * (G + Bv + 24) * UNIT)
    zn, iz, dz = np.abs(d["zn"][v]), d["iz"][v], np.abs(d["dz"][v])
    W = (zn * np.abs(d["dzn"])).sum(1)
    proj = (d["szz"][v] > CO.EPS)[:, None]
    bd = iz[:, None] * (E[:, None] * (1 + proj * zn * zn.sum(1)[:, None]) + proj * zn * (4 * G + 24) * UNIT * W[:, None]) \
        + (G + 12) * UNIT * dz
    top = -np.sort(-(d["Lv"][:, :-1] if twins else d["Lv"]), axis=1)[:, :2]
    decided = (top[:, 0] - top[:, 1] > 2 * eL) if Bv > 1 else np.ones(Bv, bool)
    return np.full(Bv, row), bd, decided


def ratios(got_loss, got_dz, d, G, inv_t, soft):
    """the largest error / bound of the rows' losses and of the gradient (0 where there is nothing to compare)"""
    if d["Bv"] == 0:
        return 0.0, 0.0
    v = d["v"]
    row, bd, _ = bounds(d, G, inv_t, soft)
    rl = (np.abs(np.asarray(got_loss, np.float64)[v] - d["loss_row"][v]) / row).max()
    rd = 0.0 if got_dz is None else (np.abs(np.asarray(got_dz, np.float64)[v] - d["dz"][v]) / bd).max()
    return rl, rd


# ---------------------------------------------------------------------------------------------------- CPU: the bound
@pytest.mark.parametrize("temperature", [0.07, 0.5])
@pytest.mark.parametrize("B,G", [s for s in SHAPES if s[0] >= 5], ids=ids([s for s in SHAPES if s[0] >= 5]))
def test_bound_discriminates(B, G, temperature):
    """the derived bound accepts the reference, rejects the reference at inv_temperature * 1.01 and the reference with the
    caption -> scan term dropped; and the hit rule leaves out at most 2 % of the rows"""
    z, g, d, (inv_t, soft) = case(B, G, temperature)
    assert ratios(d["loss_row"], d["dz"], d, G, inv_t, soft) == (0.0, 0.0)
    hot = CO.evaluate(z, g, inv_t * 1.01, soft, True, WEIGHT)
    rl, rd = ratios(hot["loss_row"], hot["dz"], d, G, inv_t, soft)
    print(f"  ({B}, {G}) T {temperature}: inv_temperature * 1.01: loss error / bound {rl:.2f}, dz {rd:.2f}", end="")
    assert rl > 1 and rd > 1, (rl, rd)
    one = CO.evaluate(z, g, inv_t, soft, True, WEIGHT, column_term=False)
    rl, rd = ratios(one["loss_row"], one["dz"], d, G, inv_t, soft)
    print(f"; no column term: loss {rl:.1f}, dz {rd:.1f}")
    assert rl > 1 and rd > 1, (rl, rd)
    assert (~bounds(d, G, inv_t, soft)[2]).mean() <= 0.02


def gpu_cases():
    """every case() the GPU tests below run, as (arguments, twins)"""
    for B, G in SHAPES:
        yield (B, G), False
    for B, G in ((7, 65), (64, 512)):
        for soft_temperature, symmetric in OPTIONS:
            yield (B, G, 0.07, soft_temperature, symmetric), False
    for B, G in ((17, 20), (64, 512)):
        for soft_temperature in (None, 0.5):
            yield (B, G, 0.5, soft_temperature, True), False
    for soft_temperature, symmetric in OPTIONS:
        for kind in ("zero_row", "all_zero", "twins", "tiny_z"):
            yield (9, 24, 0.07, soft_temperature, symmetric, kind), kind == "twins"


def test_seeds_keep_the_hit_check():
    """on the reference alone: in no case that runs on the GPU does the hit rule leave out more than 2 % of the rows"""
    for args, twins in gpu_cases():
        _, _, d, (inv_t, soft) = case(*args)
        if d["Bv"]:
            assert (~bounds(d, args[1], inv_t, soft, twins)[2]).mean() <= 0.02, args


# ---------------------------------------------------------------------------------------------------- GPU
def device_rows(h, ld, off=0):
    """[B][ld] on the device with NaN in the pad columns, the first element ``off`` floats into a 16-byte aligned buffer"""
    B, G = h.shape
    flat = torch.full((B * ld + off,), float("nan"), device="cuda")
    d = flat[off:].view(B, ld)
    d[:, :G] = torch.tensor(h, device="cuda")
    return d


def run(be, z, g, inv_t, soft, symmetric, ldz=None, ldg=None, mode="dz", off=0, with_out=True):
    """mode: "dz" (its own buffer), "none", "alias" (in place of z).  Returns dict(loss, hit, out, dz) as host arrays, the
    guards checked"""
    from masters_thesis_amd.ops import contrastive_work_floats
    from test_gpu_attention_paths import guarded, SENT
    B, G = z.shape
    ldz, ldg = ldz or (G + 3) // 4 * 4, ldg or (G + 3) // 4 * 4
    zd, gd = device_rows(z, ldz, off), device_rows(g, ldg, off)
    z0 = zd.clone()
    loss, t1 = guarded(B)
    out, t2 = guarded(2)
    nw = contrastive_work_floats(B, soft > 0)
    wflat = torch.full((nw + 64 + off,), SENT, device="cuda")
    work, t3 = wflat[off:off + nw], wflat[off + nw:]
    dzf = torch.full((B * ldz + 64 + off,), SENT, device="cuda")
    dz, t4 = dzf[off:off + B * ldz].view(B, ldz), dzf[off + B * ldz:]
    dz.fill_(7.0)
    hflat = torch.full((B + 64,), SENT_I, dtype=torch.int32, device="cuda")
    hit, t5 = hflat[:B], hflat[B:]
    arg = dict(dz=dz, none=None, alias=zd)[mode]
    be.contrastive_loss(zd, ldz, gd, ldg, arg, work, loss, hit, out if with_out else None, B, G, inv_t, soft, symmetric, WEIGHT)
    torch.cuda.synchronize()
    for t in (t1, t2, t3, t4):
        assert (t == SENT).all()
    assert (t5 == SENT_I).all()
    assert torch.equal(gd[:, :G], torch.tensor(g, device="cuda")) and torch.isnan(gd[:, G:]).all()
    if mode != "alias":
        assert torch.equal(zd[:, :G], z0[:, :G])
    assert torch.isnan(zd[:, G:]).all()                   # the pad columns are not written, in place or not
    if mode == "dz":
        assert (dz[:, G:] == 7.0).all()
    if not with_out:
        assert torch.isnan(out).all()
    if mode != "dz":
        assert (dz == 7.0).all()
    d = None if mode == "none" else (dz if mode == "dz" else zd)[:, :G].cpu().numpy()
    return dict(loss=loss.cpu().numpy(), hit=hit.cpu().numpy(), out=out.cpu().numpy(), dz=d)


def check(got, d, G, inv_t, soft, what="", twins=False):
    B = len(d["valid"])
    rl, rd = ratios(got["loss"], got["dz"], d, G, inv_t, soft)
    print(f"  ({B}, {G}) {what}: loss error / bound {rl:.3f}, dz {rd:.3f}", end="")
    assert np.isfinite(got["loss"]).all() and rl <= 1, rl
    if got["dz"] is not None:
        assert np.isfinite(got["dz"]).all() and rd <= 1, rd
    inv = ~d["valid"]
    assert not got["loss"][inv].any() and not got["hit"][inv].any()
    if got["dz"] is not None:
        assert not got["dz"][inv].any()
    assert set(np.unique(got["hit"])) <= {0, 1}
    if d["Bv"]:
        decided = bounds(d, G, inv_t, soft, twins)[2]
        print(f", rows left out of the hit check {(~decided).sum()} of {d['Bv']}")
        assert (~decided).mean() <= 0.02
        v, want = d["v"][decided], d["hit"]
        if twins:                                         # the first of the two equal columns wins: the last row cannot hit
            want = (np.argmax(d["Lv"][:, :-1], 1) == np.arange(B)).astype(np.int64)
            want[B - 1] = 0
        assert np.array_equal(got["hit"][v], want[v])
    # the two means: the ascending float32 sums over max(Bv, 1)
    s, h = np.float32(0), np.float32(0)
    for a, b_ in zip(got["loss"], got["hit"]):
        s, h = np.float32(s + a), np.float32(h + np.float32(b_))
    den = np.float32(max(d["Bv"], 1))
    assert got["out"][0] == np.float32(s / den) and got["out"][1] == np.float32(h / den)


def same_bits(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@gpu
@pytest.mark.parametrize("B,G", SHAPES, ids=ids(SHAPES))
def test_against_float64(be, B, G):
    z, g, d, (inv_t, soft) = case(B, G)
    got = run(be, z, g, inv_t, soft, True)
    check(got, d, G, inv_t, soft, "hard, symmetric")
    same_bits(got, run(be, z, g, inv_t, soft, True))        # two runs: the same bits
    if B == 1:
        assert got["loss"][0] == 0 and got["hit"][0] == 1 and not got["dz"].any() and got["out"].tolist() == [0.0, 1.0]


@gpu
@pytest.mark.parametrize("soft_temperature,symmetric", OPTIONS)
@pytest.mark.parametrize("B,G", [(7, 65), (64, 512)], ids=ids([(7, 65), (64, 512)]))
def test_option_combinations(be, B, G, soft_temperature, symmetric):
    z, g, d, (inv_t, soft) = case(B, G, 0.07, soft_temperature, symmetric)
    got = run(be, z, g, inv_t, soft, symmetric)
    check(got, d, G, inv_t, soft, f"soft {soft_temperature}, symmetric {symmetric}")
    same_bits(got, run(be, z, g, inv_t, soft, symmetric))


@gpu
@pytest.mark.parametrize("B,G", [(17, 20), (64, 512)], ids=ids([(17, 20), (64, 512)]))
def test_temperature_one_half(be, B, G):
    for soft_temperature in (None, 0.5):
        z, g, d, (inv_t, soft) = case(B, G, 0.5, soft_temperature, True)
        check(run(be, z, g, inv_t, soft, True), d, G, inv_t, soft, f"T 0.5, soft {soft_temperature}")


@gpu
@pytest.mark.parametrize("soft_temperature", [None, 0.5])
@pytest.mark.parametrize("mode", ["strides", "none", "alias", "unaligned", "no_out"])
def test_argument_forms(be, mode, soft_temperature):
    B, G = 7, 65
    z, g, d, (inv_t, soft) = case(B, G, 0.07, soft_temperature, True)
    ldz, ldg, off = (72, 80, 0) if mode == "strides" else (65, 67, 1) if mode == "unaligned" else (68, 68, 0)
    got = run(be, z, g, inv_t, soft, True, ldz, ldg, mode if mode in ("none", "alias") else "dz", off, with_out=mode != "no_out")
    if mode == "no_out":
        got["out"] = run(be, z, g, inv_t, soft, True)["out"]
    check(got, d, G, inv_t, soft, mode)
    base = run(be, z, g, inv_t, soft, True)
    if mode == "none":
        base["dz"] = None
    same_bits(got, base)                                  # strides, alignment, aliasing and absent outputs change no bit


@gpu
@pytest.mark.parametrize("soft_temperature,symmetric", OPTIONS)
@pytest.mark.parametrize("kind", ["zero_row", "all_zero", "twins", "tiny_z"])
def test_special_rows(be, kind, soft_temperature, symmetric):
    B, G = 9, 24
    z, g, d, (inv_t, soft) = case(B, G, 0.07, soft_temperature, symmetric, kind)
    got = run(be, z, g, inv_t, soft, symmetric)
    check(got, d, G, inv_t, soft, kind, twins=kind == "twins")
    if kind == "zero_row":
        assert d["Bv"] == B - 1 and got["loss"][B // 2] == 0 and got["hit"][B // 2] == 0 and not got["dz"][B // 2].any()
    if kind == "all_zero":
        assert not got["loss"].any() and not got["hit"].any() and not got["dz"].any() and got["out"].tolist() == [0.0, 0.0]
    if kind == "twins":                                   # columns 0 and B - 1 hold the same bits: the first wins
        assert got["hit"][B - 1] == 0
    if kind == "tiny_z":                                  # below the epsilon: the constant normaliser, a finite gradient
        assert (d["szz"][1] <= CO.EPS) and np.isfinite(got["dz"][1]).all() and np.abs(got["dz"][1]).max() > 1.0


@gpu
def test_twins_rank_first_in_their_row(be):
    """hard targets, two identical target rows: the logits of the two columns are the same bits, the first argmax takes the
    smaller column -- with z_0 = z_{B-1} = that target, both rows' largest logit is the pair's"""
    B, G = 6, 40
    z, g, _, (inv_t, soft) = case(B, G, 0.07, None, True, "twins")
    z = z.copy()
    z[0] = z[B - 1] = g[0]
    got = run(be, z, g, inv_t, soft, True)
    check(got, CO.evaluate(z, g, inv_t, soft, True, WEIGHT), G, inv_t, soft, "twins on the diagonal", twins=True)
    assert got["hit"][0] == 1 and got["hit"][B - 1] == 0


@gpu
def test_bad_arguments(be):
    from masters_thesis_amd._lib import KernelLibraryError
    from masters_thesis_amd.ops import contrastive_work_floats
    from test_gpu_attention_paths import guarded, SENT
    B, G = 2, 8
    zd = torch.zeros(B, G, device="cuda")
    loss, t = guarded(B, fill=3.0)
    hit = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    work = torch.full((contrastive_work_floats(B, True),), 3.0, device="cuda")
    ok = dict(z=zd, ldz=G, g=zd, ldg=G, dz=None, work=work, loss_row=loss, hit_row=hit, out=None, B=B, G=G,
              inv_temperature=2.0, soft_inv_temperature=0.0, symmetric=1, weight=1.0)
    nan, inf = float("nan"), float("inf")
    for change, code in ((dict(z=None), 1), (dict(g=None), 1), (dict(work=None), 1), (dict(loss_row=None), 1),
                         (dict(hit_row=None), 1), (dict(ldz=G - 1), 2), (dict(ldg=G - 1), 4), (dict(B=0), 10),
                         (dict(B=1025), 10), (dict(G=0), 11), (dict(G=2049, ldz=4096, ldg=4096), 11),
                         (dict(inv_temperature=0.0), 12), (dict(inv_temperature=-1.0), 12), (dict(inv_temperature=nan), 12),
                         (dict(inv_temperature=inf), 12), (dict(soft_inv_temperature=-1.0), 13),
                         (dict(soft_inv_temperature=nan), 13), (dict(soft_inv_temperature=inf), 13), (dict(weight=-1.0), 15),
                         (dict(weight=nan), 15), (dict(weight=inf), 15)):
        with pytest.raises(KernelLibraryError, match=f"tnt_contrastive_loss_f32 failed with code {-1000 - code}"):
            be.contrastive_loss(**{**ok, **change})
    p = lambda x: x.data_ptr()
    assert be.lib.tnt_contrastive_loss_f32(p(zd), G, p(zd), G, None, p(work), p(loss), p(hit), None, B, G, 2.0, 0.0, 2, 1.0,
                                           None) == -1014
    torch.cuda.synchronize()
    assert (loss == 3.0).all() and (t == SENT).all() and (hit == SENT_I).all() and (work == 3.0).all()     # nothing was launched
    assert be.lib.tnt_version() >= 136
