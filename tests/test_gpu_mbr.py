"""Minimum Bayes risk selection on the GPU, the kernel: tnt_mbr_select_f32 against the exact-integer / float64 restatement
(tests/mbr_oracle.py) over scan counts, candidate and reference counts, caption lengths, orders and both utilities, on a
vocabulary of four ids so that repeated n-grams make the clipping matter: empty captions, captions without a terminator,
captions shorter than the order, duplicates, garbage behind the terminator, end_id = -1, sentinel columns, every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import mbr_oracle as MO

pytestmark = pytest.mark.gpu

END = 2
EPS = 2.0 ** -24                # the relative rounding error of one float32 operation
# kind 0 (ngram-f).  c_k and the tot_k are integers below 2^24, exact in float32.  F_k is one division of two of them
# (<= EPS); the order - 1 <= 3 additions of the non-negative F_k add at most EPS of the running sum each; the division by
# the order one more: u is within (1 + 3 + 1) EPS = 3.0e-7 of the float64 value, relatively.  E accumulates the float32
# utilities in float64 and rounds once: + EPS = 3.6e-7.  Both are inside the bound the definition's order of operations
# was chosen for:
REL0 = 1e-6


def rel1(L):
    """kind 1 (bleu) at captions of up to L tokens, relative.  A = log(L / 0.1) bounds |log(n_k / den_k)|: 0.1 <= n_k <=
    den_k <= L.  q = n_k / den_k carries 2 EPS (the float32 0.1 and the division), which log turns into 2 EPS absolute; logf
    is good to one ulp, <= 2 EPS A; the weight 1 / order and its product add 2 EPS A; over the terms, whose weights sum
    to 1, that is EPS (2 + 4 A), and the <= 3 additions of partial sums of magnitude <= A add 3 EPS A:  |ds| <= EPS (2 + 7 A).
    exp turns ds into a relative error and adds one ulp (2 EPS).  The brevity penalty's argument 1 - len_r / len_h has two
    roundings at a magnitude <= L, 2 EPS L absolute, so bp carries 2 EPS L + 2 EPS; the product bp * exp(s) one more EPS.
    Sum: EPS (7 + 7 A + 2 L); E adds the EPS of its one rounding.  The smallest non-zero value, exp(1 - L) * 0.1 / L > 1e-31
    at L = 64, is a normal float32: no absolute term."""
    return EPS * (8.0 + 7.0 * np.log(L / 0.1) + 2.0 * L)


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def make_ids(seed, B, Nc, L, ld, end_id, garbage=True):
    """ids (Nc, L, ld) int32 over the vocabulary {3, 4, 5, 6} (with end_id = -1 also -1 and 2, ordinary tokens then).  Per
    scan: candidate 1 starts with 0 and candidate 2 with end_id (or 0): empty captions; candidate 3 has no terminator;
    candidate 5 is shorter than four tokens; the others end after a random length at end_id or 0, followed by random
    garbage (``garbage`` False: by zeros).  Candidate 4 is a verbatim copy of candidate 0 (with Nc = 2: candidate 1, on scan
    0), candidate Nc - 1 of candidate 6.  Columns [B, ld) hold a sentinel pattern."""
    rng = np.random.default_rng(seed)
    vocab = np.array([3, 4, 5, 6] + ([-1, 2] if end_id < 0 else []))
    ends = [0] if end_id < 0 else [0, end_id]
    ids = np.empty((Nc, L, ld), np.int32)
    ids[:, :, B:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (Nc, L, ld - B))
    for b in range(B):
        for c in range(Nc):
            row = rng.choice(vocab, L)
            n = {1: 0, 2: 0, 3: L, 5: int(rng.integers(1, 4))}.get(c % 7, int(rng.integers(0, L + 1)))
            if n < L:
                row[n] = ends[-1] if c % 7 == 2 else ends[int(rng.integers(len(ends)))]
                tail = rng.choice(np.concatenate([vocab, ends]), L - n - 1)
                row[n + 1:] = tail if garbage else 0
            ids[c, :, b] = row
    if Nc == 2:
        ids[1, :, 0] = ids[0, :, 0]
    if Nc > 4:
        ids[4, :, :B] = ids[0, :, :B]
    if Nc > 7:
        ids[Nc - 1, :, :B] = ids[6, :, :B]
    return ids


def run(be, ids, B, Nr, end_id, order, kind, outs=True):
    """-> dict(expected (B, Nc), best (B,), and with ``outs`` out_ids (L, B + 2), match (B, Nc, Nr, order), util (B, Nc, Nr))"""
    Nc, L, ld = ids.shape
    d = torch.from_numpy(ids).to("cuda")
    i32, dev = torch.int32, "cuda"
    expected = torch.full((B, Nc), -7.0, device=dev)
    best = torch.full((B,), -9, dtype=i32, device=dev)
    ldo = B + 2
    out = torch.full((L, ldo), -9, dtype=i32, device=dev) if outs else None
    match = torch.full((B, Nc, Nr, order), -9, dtype=i32, device=dev) if outs else None
    util = torch.full((B, Nc, Nr), -7.0, device=dev) if outs else None
    be.mbr_select(d, ld, B, Nc, Nr, L, end_id, order, kind, expected, best, out, ldo, match, util)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), ids)                                       # ids is read only
    res = dict(expected=expected.cpu().numpy(), best=best.cpu().numpy())
    if outs:
        res.update(out_ids=out.cpu().numpy(), match=match.cpu().numpy(), util=util.cpu().numpy())
    return res


def check(got, want, ids, B, Nc, Nr, L, order, kind, tag):
    """one launch's outputs against the restatement; returns worst error / bound"""
    rel = REL0 if kind == 0 else rel1(L)
    assert np.array_equal(got["match"], want["match"]), tag                           # the integer core, exactly
    worst = 0.0
    for name in ("util", "expected"):
        err, bound = np.abs(got[name] - want[name]), rel * np.abs(want[name])
        assert np.all(err <= bound), (tag, name, float(err.max()))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    # best: the first maximum of the kernel's own expected; and its float64 utility is the float64 maximum, up to rounding
    assert np.array_equal(got["best"], MO.first_max(got["expected"])), tag
    e64 = want["expected"]
    assert np.all(e64[np.arange(B), got["best"]] >= e64.max(axis=1) * (1 - 2 * rel)), tag
    # the chosen candidate's L tokens verbatim; the sentinel columns untouched
    assert np.array_equal(got["out_ids"][:, :B], np.stack([ids[got["best"][b], :, b] for b in range(B)], axis=1)), tag
    assert np.all(got["out_ids"][:, B:] == -9), tag
    # duplicates: bit-identical expected utility
    e = got["expected"].view(np.int32)
    if Nc == 2:
        assert e[0, 0] == e[0, 1], tag
    if Nc > 4:
        assert np.array_equal(e[:, 4], e[:, 0]), tag
    if Nc > 7:
        assert np.array_equal(e[:, Nc - 1], e[:, 6]), tag
    if kind == 0:                                                                     # bit-symmetric on the Nr x Nr block
        u = got["util"][:, :Nr, :].view(np.int32)
        assert np.array_equal(u, u.transpose(0, 2, 1)), tag
    return worst


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("order", [1, 4])
@pytest.mark.parametrize("L", [1, 4, 15, 64])
@pytest.mark.parametrize("Nc,Nr", [(1, 1), (2, 1), (5, 5), (17, 16), (64, 64)])
def test_select_matches_the_restatement(be, Nc, Nr, L, order, kind):
    worst = 0.0
    for B in (1, 3):
        if B == 3 and Nc == 64 and L == 64:                 # the restatement's 3 * 4096 pairs of 64 tokens take too long
            continue
        seed = 1000 * Nc + 10 * L + B
        ids = make_ids(seed, B, Nc, L, B + 3, END)
        want = MO.select(ids, B, Nr, END, order, kind)
        got = run(be, ids, B, Nr, END, order, kind)
        worst = max(worst, check(got, want, ids, B, Nc, Nr, L, order, kind, (B, Nc, Nr, L, order, kind)))
    print(f"Nc={Nc} Nr={Nr} L={L} order={order} kind={kind}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", [0, 1])
def test_negative_end_id_only_zero_terminates(be, kind):
    B, Nc, Nr, L, order = 3, 9, 7, 15, 4
    ids = make_ids(77, B, Nc, L, B + 3, -1)
    assert (ids[:, :, :B] == -1).any() and (ids[:, :, :B] == 2).any()
    want = MO.select(ids, B, Nr, -1, order, kind)
    got = run(be, ids, B, Nr, -1, order, kind)
    assert check(got, want, ids, B, Nc, Nr, L, order, kind, ("end_id=-1", kind)) <= 1.0
    # the same tokens cut at 2 as well give other captions: the terminator rule matters on this input
    assert not np.array_equal(MO.select(ids, B, Nr, 2, order, kind)["match"], want["match"])


@pytest.mark.parametrize("Nc,Nr,L", [(5, 5, 4), (17, 16, 15), (64, 64, 64)])
def test_garbage_behind_the_terminator_is_ignored(be, Nc, Nr, L):
    B = 3 if L < 64 else 1
    a = make_ids(5, B, Nc, L, B + 3, END, garbage=True)
    z = make_ids(5, B, Nc, L, B + 3, END, garbage=False)
    assert not np.array_equal(a, z)
    for order, kind in ((4, 0), (4, 1), (1, 1)):
        ga, gz = run(be, a, B, Nr, END, order, kind), run(be, z, B, Nr, END, order, kind)
        for name in ("match", "best"):
            assert np.array_equal(ga[name], gz[name]), (name, order, kind)
        for name in ("util", "expected"):
            assert np.array_equal(ga[name].view(np.int32), gz[name].view(np.int32)), (name, order, kind)
        assert np.array_equal(gz["out_ids"][:, :B], np.stack([z[gz["best"][b], :, b] for b in range(B)], axis=1))


def test_optional_outputs_change_nothing(be):
    B, Nc, Nr, L = 3, 17, 16, 15
    ids = make_ids(9, B, Nc, L, B + 3, END)
    for kind in (0, 1):
        a, b = run(be, ids, B, Nr, END, 4, kind), run(be, ids, B, Nr, END, 4, kind, outs=False)
        assert np.array_equal(a["expected"].view(np.int32), b["expected"].view(np.int32)) and np.array_equal(a["best"], b["best"])


def test_an_exact_tie_goes_to_the_smaller_index(be):
    B, Nc, L = 2, 64, 6
    ids = np.zeros((Nc, L, B), np.int32)
    ids[:, :3, :] = np.array([3, 4, 5])[None, :, None]             # 64 identical captions: every E is equal
    ids[0, :, 1] = [6, 6, 6, 0, 0, 0]                              # scan 1: candidate 0 matches nobody but itself
    got = run(be, ids, B, Nc, END, 4, 0)
    assert got["best"].tolist() == [0, 1]
    assert np.all(got["expected"][0] == got["expected"][0, 0])


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    B, Nc, Nr, L, order, ld, ldo = 3, 5, 4, 6, 4, 5, 4
    i32 = dict(dtype=torch.int32, device="cuda")
    n_ids = Nc * L * ld
    buf = torch.zeros(n_ids + 1024, **i32)                         # ids, and behind them room an output may use
    buf[:n_ids] = torch.from_numpy(make_ids(3, B, Nc, L, ld, END).reshape(-1)).to("cuda")
    ids, tail = buf[:n_ids], buf[n_ids:]
    expected = torch.full((B, Nc), -7.0, device="cuda")
    best = torch.full((B,), -9, **i32)
    out = torch.full((L, ldo), -9, **i32)
    match = torch.full((B, Nc, Nc, order), -9, **i32)              # room for Nr = Nc
    util = torch.full((B, Nc, Nc), -7.0, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    last_read = ((Nc * L - 1) * ld + B - 1)                        # the last element of ids the launch may read

    def call(ids=ids, ld=ld, B=B, Nc=Nc, Nr=Nr, L=L, end_id=END, order=order, kind=0, expected=expected, best=best,
             out_ids=out, ldo=ldo, match=match, util=util):
        return lib.tnt_mbr_select_f32(p(ids), ld, B, Nc, Nr, L, end_id, order, kind, p(expected), p(best), p(out_ids), ldo,
                                      p(match), p(util), None)
    bads = [dict(B=0), dict(B=-1), dict(ld=2), dict(Nc=0), dict(Nc=65), dict(Nc=-1), dict(Nr=0), dict(Nr=6), dict(Nr=-1),
            dict(L=0), dict(L=65), dict(L=-1), dict(order=0), dict(order=5), dict(order=-1), dict(kind=2), dict(kind=-1),
            dict(ids=None), dict(expected=None), dict(best=None), dict(ldo=2),
            dict(expected=buf), dict(best=buf[7:]), dict(out_ids=buf[last_read:]), dict(match=buf[100:]),
            dict(util=buf[last_read:]), dict(expected=buf[last_read:])]
    before = buf.clone()
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                       # TNT_BADARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((expected == -7.0).all()) and bool((best == -9).all())
    assert bool((out == -9).all()) and bool((match == -9).all()) and bool((util == -7.0).all())        # nothing was launched
    # the smallest and the largest accepted values; nullable outputs; outputs right behind the last element read
    assert call() == 0 and call(out_ids=None, match=None, util=None, ldo=0) == 0 and call(Nr=Nc, order=1, kind=1) == 0
    assert call(expected=buf[last_read + 1:], out_ids=tail[512:]) == 0 and call(end_id=-1, Nr=1) == 0
    torch.cuda.synchronize()
    assert bool((best >= 0).all()) and bool((best < Nc).all()) and bool((out[:, :B] != -9).all()) and bool((out[:, B:] == -9).all())
