"""tnt_input_corrupt_f32 (scan dropout and word dropout of a staged batch; definition in include/tnt_hip.h) on the GPU,
bit for bit against the restatement of tests/corrupt_oracle.py, which is built on oracle.philox.uniform24.

Kernel paths and what reaches them:
    input_corrupt_kernel<true>    float4 row stores: N % 4 == ldx % 4 == 0, x and null_scan 16-byte aligned
    input_corrupt_kernel<false>   scalar row stores: odd N or ldx, a misaligned x, a misaligned null_scan
    the xT column stores          with xT, at ldt = B and B + 3
    the second piece of a row     N = 1028 (a workgroup takes 1024 columns of a row: the second piece holds 4)
    the word workgroups           B * T up to 67 * 33 = 2211 positions: three workgroups, the last one partly filled
The pad columns [N, ldx) of x and the columns >= B of xT hold NaN canaries that must come back bit-identical.  Where
0 < rate < 1 and B >= 2 the step word is chosen so that a row fires and one does not and an eligible token fires and one
does not; the test asserts that on the restatement's masks, otherwise a pass would show nothing."""
import numpy as np
import pytest
import torch

from corrupt_oracle import S_SCAN_DROP, S_WORD_DROP, corrupt, pick_step

pytestmark = pytest.mark.gpu

V, UNK, SEED = 50, 7, 0x1234567899


@pytest.fixture(scope="module")
def be():
    from masters_thesis_amd import ops
    return ops.HipBackend()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


class Case:
    """the buffers of one call: x [B][ldx] (pad columns NaN), xT [N][ldt] or None (columns >= B NaN), cap [B][T], null"""

    def __init__(self, B, N, pad, xt, T, with_null, misaligned=False, null_misaligned=False, seed=0):
        rng = np.random.default_rng(1000 * B + N + 7 * T + seed)
        self.B, self.N, self.T = B, N, T
        self.ldx = N if not pad else (N + 3) // 4 * 4 + 4
        self.ldt = 0 if xt is None else B + xt
        self.x0 = np.full((B, self.ldx), np.nan, np.float32)
        self.x0[:, :N] = rng.standard_normal((B, N)).astype(np.float32)
        self.xT0 = None
        if xt is not None:
            self.xT0 = np.full((N, self.ldt), np.nan, np.float32)
            self.xT0[:, :B] = self.x0[:, :N].T
        cap = rng.integers(1, V, size=(B, T)).astype(np.int32)
        for b in range(B):                                   # padded tails (id 0) of ragged length, a 0 inside a caption too
            cap[b, int(rng.integers(1, T + 1)):] = 0
        if T > 3:
            cap[0, 2] = 0
        cap[:, 0] = 1
        self.cap0 = cap
        self.null0 = rng.standard_normal(N).astype(np.float32) if with_null else None
        dev = lambda a, off=0: None if a is None else self._place(a, off)
        self.x = dev(self.x0, 1 if misaligned else 0)
        self.xT, self.cap = dev(self.xT0), dev(self.cap0)
        self.null = dev(self.null0, 1 if null_misaligned else 0)

    @staticmethod
    def _place(a, off):
        """a on the device, ``off`` elements behind a 16-byte boundary"""
        buf = torch.zeros(a.size + off, dtype=torch.from_numpy(a).dtype, device="cuda")
        buf[off:].copy_(torch.from_numpy(a.reshape(-1)))
        return buf[off:].view(a.shape)

    def run(self, be, scan_rate, word_rate, step_dev, unk=UNK, null_ptrs=False):
        x = self.x if (scan_rate > 0 or not null_ptrs) else None
        xT = self.xT if x is not None else None
        cap = self.cap if (word_rate > 0 or not null_ptrs) else None
        be.input_corrupt(x, self.ldx, xT, self.ldt, cap, self.B, self.T, self.N, V, scan_rate,
                         self.null if x is not None else None, word_rate, unk, SEED, S_SCAN_DROP, S_WORD_DROP, step_dev)
        torch.cuda.synchronize()

    def expected(self, scan_rate, word_rate, step, unk=UNK):
        x2, cap2, rows, words = corrupt(self.x0[:, :self.N], self.cap0, scan_rate, word_rate, self.null0, unk, SEED, step)
        x = self.x0.copy()
        x[:, :self.N] = x2
        xT = None
        if self.xT0 is not None:
            xT = self.xT0.copy()
            xT[:, :self.B] = x2.T
        return x, xT, cap2, rows, words

    def check(self, want_x, want_xT, want_cap):
        assert np.array_equal(bits(self.x), want_x.view(np.int32)), "x"
        if self.xT is not None:
            assert np.array_equal(bits(self.xT), want_xT.view(np.int32)), "xT"
        assert np.array_equal(self.cap.cpu().numpy(), want_cap), "cap"

    def untouched(self):
        self.check(self.x0, self.xT0, self.cap0)


# B, N, pad, xT (None / extra columns of ldt), T, scan_rate, word_rate, null given, x misaligned, null misaligned
CASES = [
    (1, 1, False, None, 1, 0.3, 0.3, False, False, False),
    (1, 4, False, 0, 2, 1.0, 1.0, True, False, False),
    (1, 1028, True, 3, 15, 0.3, 0.3, True, False, False),
    (3, 1, True, 0, 2, 0.3, 0.3, True, False, False),
    (3, 3, False, 3, 15, 0.3, 0.3, False, False, False),
    (3, 4, False, None, 33, 0.3, 0.3, True, False, False),
    (3, 4, True, 0, 15, 0.3, 0.0, True, False, False),
    (3, 63, False, None, 15, 0.3, 0.3, True, False, False),
    (3, 63, True, 3, 2, 1.0, 0.3, False, False, False),
    (3, 64, False, 0, 15, 0.3, 1.0, True, False, False),
    (3, 1028, False, 3, 33, 0.3, 0.3, True, False, False),
    (64, 1, False, None, 15, 0.3, 0.3, True, False, False),
    (64, 3, True, 0, 1, 0.3, 0.3, True, False, False),
    (64, 4, False, 3, 15, 0.3, 0.3, False, False, False),
    (64, 63, True, 0, 33, 0.3, 0.3, True, False, False),
    (64, 64, False, 0, 15, 0.3, 0.3, True, False, False),
    (64, 64, True, None, 15, 0.3, 0.3, False, False, False),
    (64, 64, False, 3, 2, 0.0, 0.3, True, False, False),
    (64, 1028, True, 0, 15, 0.3, 0.3, True, False, False),
    (64, 1028, False, None, 33, 1.0, 1.0, False, False, False),
    (67, 1, True, 3, 33, 0.3, 0.3, False, False, False),
    (67, 3, False, None, 15, 0.3, 0.3, True, False, False),
    (67, 4, True, 0, 15, 0.3, 0.3, True, False, False),
    (67, 63, False, 3, 15, 0.3, 0.3, True, False, False),
    (67, 64, False, 3, 33, 0.3, 0.3, False, False, False),
    (67, 1028, False, 0, 2, 0.3, 0.3, True, False, False),
    (67, 1028, True, 3, 33, 0.3, 0.3, True, False, False),
    # the scalar path by alignment alone: N and ldx are multiples of 4
    (3, 64, False, 0, 15, 0.3, 0.3, True, True, False),
    (64, 1028, False, 3, 15, 0.3, 0.3, True, True, False),
    (67, 64, True, None, 15, 0.3, 0.3, True, False, True),
    (64, 4, False, 0, 15, 1.0, 0.3, False, True, False),
]


def ids(c):
    B, N, pad, xt, T, sr, wr, nul, mis, nmis = c
    return (f"B{B}-N{N}{'p' if pad else ''}-xT{'no' if xt is None else xt}-T{T}-s{sr}-w{wr}-{'null' if nul else 'zeros'}"
            f"{'-xmis' if mis else ''}{'-nmis' if nmis else ''}")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_bit_for_bit_against_the_restatement(be, case):
    B, N, pad, xt, T, sr, wr, nul, mis, nmis = case
    c = Case(B, N, pad, xt, T, nul, mis, nmis)
    step = pick_step(B, T, c.cap0, sr, wr, SEED)
    want_x, want_xT, want_cap, rows, words = c.expected(sr, wr, step)
    elig = c.cap0 != 0
    elig[:, 0] = False
    if 0 < sr < 1 and B >= 2:
        assert rows.any() and not rows.all()                    # a row fired and a row did not
    if 0 < wr < 1 and elig.sum() >= 2:
        assert words.any() and (elig & ~words).any()            # an eligible token fired and one did not
    if sr == 1:
        assert rows.all()
    if wr == 1:
        assert np.array_equal(words, elig)
    if sr == 0:
        assert not rows.any()
    if wr == 0:
        assert not words.any()
    assert not words[:, 0].any() and not words[c.cap0 == 0].any()
    step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
    c.run(be, sr, wr, step_dev)
    c.check(want_x, want_xT, want_cap)
    got_cap = c.cap.cpu().numpy()
    assert np.array_equal(got_cap[:, 0], c.cap0[:, 0]) and np.array_equal(got_cap == 0, c.cap0 == 0)


def test_rate_one_fires_everywhere_it_may(be):
    c = Case(67, 63, True, 3, 15, True)
    step_dev = torch.tensor([5], dtype=torch.int32, device="cuda")
    c.run(be, 1.0, 1.0, step_dev)
    x, cap = c.x.cpu().numpy(), c.cap.cpu().numpy()
    assert np.array_equal(x[:, :63], np.broadcast_to(c.null0, (67, 63)))
    assert np.array_equal(c.xT.cpu().numpy()[:, :67], np.broadcast_to(c.null0[:, None], (63, 67)))
    elig = c.cap0 != 0
    elig[:, 0] = False
    assert elig.sum() > 100 and (cap[elig] == UNK).all() and np.array_equal(cap[~elig], c.cap0[~elig])
    assert np.array_equal(bits(c.x)[:, 63:], c.x0.view(np.int32)[:, 63:])
    assert np.array_equal(bits(c.xT)[:, 67:], c.xT0.view(np.int32)[:, 67:])


@pytest.mark.parametrize("off", ["scan", "word", "both"])
def test_rate_zero_takes_null_pointers_and_writes_nothing_for_its_part(be, off):
    c = Case(64, 64, True, 3, 15, True)
    step = pick_step(64, 15, c.cap0, 0.3, 0.3, SEED)
    step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
    sr, wr = (0.0 if off in ("scan", "both") else 0.3), (0.0 if off in ("word", "both") else 0.3)
    c.run(be, sr, wr, step_dev, null_ptrs=True)
    want_x, want_xT, want_cap, rows, words = c.expected(sr, wr, step)
    if off == "both":
        c.untouched()
    else:
        assert (rows.any() if off == "word" else words.any())
        c.check(want_x, want_xT, want_cap)
        if off == "scan":
            assert np.array_equal(bits(c.x), c.x0.view(np.int32)) and np.array_equal(bits(c.xT), c.xT0.view(np.int32))
        else:
            assert np.array_equal(c.cap.cpu().numpy(), c.cap0)


def test_the_step_word_is_read_on_the_device_and_decides_the_masks(be):
    """the same word twice: the same output; another word: other masks; a launch captured once replays with the live word"""
    make = lambda: Case(64, 64, False, 0, 15, True)
    a, b, c = make(), make(), make()
    step_dev = torch.tensor([3], dtype=torch.int32, device="cuda")
    a.run(be, 0.3, 0.3, step_dev)
    b.run(be, 0.3, 0.3, step_dev)
    assert np.array_equal(bits(a.x), bits(b.x)) and np.array_equal(bits(a.xT), bits(b.xT)) and torch.equal(a.cap, b.cap)
    a.check(*a.expected(0.3, 0.3, 3)[:3])
    step_dev.fill_(4)
    c.run(be, 0.3, 0.3, step_dev)
    c.check(*c.expected(0.3, 0.3, 4)[:3])
    r3, w3 = a.expected(0.3, 0.3, 3)[3:]
    r4, w4 = c.expected(0.3, 0.3, 4)[3:]
    assert not np.array_equal(r3, r4) and not np.array_equal(w3, w4)
    assert not torch.equal(a.cap, c.cap) and not np.array_equal(bits(a.x), bits(c.x))
    # captured once, replayed under two step words
    d = make()
    d.run(be, 0.3, 0.3, step_dev)                                       # warm-up outside the capture (step 4)
    d.check(*d.expected(0.3, 0.3, 4)[:3])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        be.input_corrupt(d.x, d.ldx, d.xT, d.ldt, d.cap, d.B, d.T, d.N, V, 0.3, d.null, 0.3, UNK, SEED, S_SCAN_DROP, S_WORD_DROP,
                         step_dev)
    for step in (9, 3):
        e = make()
        d.x.copy_(e.x), d.xT.copy_(e.xT), d.cap.copy_(e.cap)
        step_dev.fill_(step)
        g.replay()
        torch.cuda.synchronize()
        d.check(*e.expected(0.3, 0.3, step)[:3])


def test_bad_arguments_return_badarg_and_write_nothing(be):
    from masters_thesis_amd.ops import _p
    c = Case(64, 64, True, 3, 15, True)
    step_dev = torch.tensor([1], dtype=torch.int32, device="cuda")
    lib, s = be.lib, be._s()
    good = dict(x=_p(c.x), ldx=c.ldx, xT=_p(c.xT), ldt=c.ldt, cap=_p(c.cap), B=c.B, T=c.T, N=c.N, V=V, sr=1.0, null=_p(c.null),
                wr=1.0, unk=UNK, step=_p(step_dev))

    def call(**kw):
        a = dict(good, **kw)
        return lib.tnt_input_corrupt_f32(a["x"], a["ldx"], a["xT"], a["ldt"], a["cap"], a["B"], a["T"], a["N"], a["V"], a["sr"],
                                         a["null"], a["wr"], a["unk"], SEED, S_SCAN_DROP, S_WORD_DROP, a["step"], s)
    nan, inf = float("nan"), float("inf")
    bad = [dict(sr=-0.1), dict(sr=1.5), dict(sr=nan), dict(sr=inf), dict(wr=-0.1), dict(wr=1.0001), dict(wr=nan),
           dict(unk=0), dict(unk=-1), dict(unk=V), dict(unk=V + 3), dict(B=-1), dict(T=-1), dict(N=-1), dict(ldx=c.N - 1),
           dict(ldt=c.B - 1), dict(step=None), dict(x=None), dict(cap=None),
           dict(sr=0.0, step=None), dict(sr=0.0, wr=0.0, step=None), dict(wr=0.0, sr=nan), dict(sr=0.0, wr=0.5, unk=V)]
    for kw in bad:
        rc = call(**kw)
        assert rc <= -1000, (kw, rc)
    # what is not refused: unk_id is not looked at without word dropout, ldt not without xT; both rates 0 launch nothing
    assert call(sr=0.0, wr=0.0) == 0 and call(sr=0.0, wr=0.0, x=None, xT=None, cap=None, null=None) == 0
    torch.cuda.synchronize()
    c.untouched()
    assert call(wr=0.0, unk=0, xT=None, ldt=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.x.cpu().numpy()[:, :c.N], np.broadcast_to(c.null0, (c.B, c.N)))
    assert np.array_equal(bits(c.xT), c.xT0.view(np.int32)) and np.array_equal(c.cap.cpu().numpy(), c.cap0)
    assert lib.tnt_version() >= 126
