"""The accumulation launch (tnt_grad_accumulate_f32, csrc/accumulate.hip) on a real MI355X, bit for bit against the numpy
float32 restatement of its header definition (tests/accum_oracle.py ``reference``): plain float32 adds in a fixed operand
order, one thread per address, leave no error to bound.

Sizes, from the kernel's own constants (read from the source): the empty arena (scalar work only), the n % 4 tail alone
(1, 3), one float4 (4, 5), one workgroup trip of AC_THREADS * AC_U float4s minus one / exactly / plus one float, three
trips plus 2, and AC_MAX_GRID * trip + trip + 7: every workgroup of the capped grid takes a second, grid-strided trip, the
last of them partly filled, with a tail.  Every phase runs at every size; the buffers sit between sentinel words that
must survive."""
import os
import re

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import _lib
from accum_oracle import ADD, CLOSE, OPEN, reference

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "accumulate.hip")).read()
_const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1))
AC_THREADS, AC_U, AC_MAX_GRID = _const("AC_THREADS"), _const("AC_U"), _const("AC_MAX_GRID")
TRIP = 4 * AC_THREADS * AC_U                 # floats per workgroup and trip
BIG = AC_MAX_GRID * TRIP + TRIP + 7
SIZES = [0, 1, 3, 4, 5, TRIP - 1, TRIP, TRIP + 1, 3 * TRIP + 2, BIG]
PAD = 64                 # sentinel floats on both sides of a buffer (keeps the 16-byte alignment)
SENT = -7.25
PHASES = {"open": OPEN, "add": ADD, "close": CLOSE}
_INPUTS = {}


def inputs(n):
    """(acc, grad) float32 of mixed magnitudes (1e-6 .. 1e3, both signs) with zeros, cancelling pairs, pairs whose sum
    rounds, subnormals and an infinity; computed once per size and never modified"""
    if n not in _INPUTS:
        rng = np.random.default_rng(2000 + n % 100003)
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        k = np.arange(n)
        g[k % 7 == 0] = -a[k % 7 == 0]                                 # cancel to +0
        a[k % 11 == 0] = 0.0
        g[k % 13 == 0] = -0.0
        a[k % 19 == 0] = np.float32(3e-42)                             # subnormal
        g[(k % 19 == 0) & (k % 2 == 0)] = np.float32(-1e-41)
        a[k % 1009 == 5] = np.float32(np.inf)
        a.setflags(write=False)
        g.setflags(write=False)
        _INPUTS[n] = (a, g)
    return _INPUTS[n]


def padded(x):
    """x on the device between PAD sentinel floats; returns (whole buffer, the view of x that is passed to the launch).  An
    empty x still passes a valid address: the view then runs into the sentinels, which the launch must leave"""
    buf = torch.full((x.size + 2 * PAD,), SENT, dtype=torch.float32, device="cuda")
    buf[PAD:PAD + x.size].copy_(torch.from_numpy(x.copy()))
    view = buf[PAD:PAD + max(x.size, 1)]
    assert view.data_ptr() % 16 == 0
    return buf, view


def read(buf, n):
    return buf[PAD:PAD + n].cpu().numpy()


def pads_intact(buf, n):
    h = buf.cpu().numpy()
    return (h[:PAD] == SENT).all() and (h[PAD + n:] == SENT).all()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scalars(sq_acc=5.5, sq_slot=0.1, drop_step=41):
    f = lambda v: torch.full((1,), v, dtype=torch.float32, device="cuda")
    return f(sq_acc), f(sq_slot), torch.full((1,), drop_step, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("phase", sorted(PHASES))
def test_one_launch(phase, n):
    ph = PHASES[phase]
    be = ops.backend()
    a, g = inputs(n)
    if ph == OPEN:                      # acc is not read: poison it
        a = np.full(n, np.nan, np.float32)
    abuf, acc = padded(a)
    gbuf, grad = padded(g)
    qa, qs, ds = scalars()
    be.grad_accumulate(acc, grad, n, ph, qa, qs, ds)
    want = reference(a, g, ph, np.float32(5.5), np.float32(0.1), 41)
    got_a, got_g = read(abuf, n), read(gbuf, n)
    assert np.array_equal(bits(got_a), bits(want[0])), f"acc differs at {np.flatnonzero(bits(got_a) != bits(want[0]))[:5]}"
    assert np.array_equal(bits(got_g), bits(want[1])), f"grad differs at {np.flatnonzero(bits(got_g) != bits(want[1]))[:5]}"
    if ph == CLOSE:
        assert np.array_equal(bits(got_a), bits(a)), "CLOSE wrote acc"
    else:
        assert np.array_equal(bits(got_g), bits(g)), "OPEN / ADD wrote grad"
    if ph == OPEN:
        assert not np.isnan(got_a).any(), "OPEN read acc"
    assert bits(qa.cpu().numpy())[0] == bits(want[2])[0] and bits(qs.cpu().numpy())[0] == bits(want[3])[0]
    assert int(ds.item()) == want[4] == (41 if ph == CLOSE else 42)
    assert pads_intact(abuf, n) and pads_intact(gbuf, n), "a word outside the buffers was written"


@pytest.mark.parametrize("n", [0, 5, TRIP + 1, BIG])
@pytest.mark.parametrize("phase", sorted(PHASES))
def test_a_set_guard_leaves_everything(phase, n):
    be = ops.backend()
    a, g = inputs(n)
    abuf, acc = padded(a)
    gbuf, grad = padded(g)
    qa, qs, ds = scalars()
    guard = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    be.grad_accumulate(acc, grad, n, PHASES[phase], qa, qs, ds, guard=guard)
    assert np.array_equal(bits(read(abuf, n)), bits(a)) and np.array_equal(bits(read(gbuf, n)), bits(g))
    assert float(qa.item()) == 5.5 and float(qs.item()) == np.float32(0.1) and int(ds.item()) == 41 and int(guard.item()) == 2
    assert pads_intact(abuf, n) and pads_intact(gbuf, n)
    guard.zero_()                       # a clear guard word: the launch runs
    be.grad_accumulate(acc, grad, n, PHASES[phase], qa, qs, ds, guard=guard)
    want = reference(a, g, PHASES[phase], np.float32(5.5), np.float32(0.1), 41)
    assert np.array_equal(bits(read(abuf, n)), bits(want[0])) and np.array_equal(bits(read(gbuf, n)), bits(want[1]))
    assert int(ds.item()) == want[4]


@pytest.mark.parametrize("n", [0, 3, TRIP + 1])
@pytest.mark.parametrize("phase", sorted(PHASES))
def test_nullable_arguments(phase, n):
    be = ops.backend()
    ph = PHASES[phase]
    a, g = inputs(n)
    want = reference(a, g, ph)
    for with_sq, with_ds in ((False, True), (True, False), (False, False)):
        abuf, acc = padded(a)
        gbuf, grad = padded(g)
        qa, qs, ds = scalars()
        be.grad_accumulate(acc, grad, n, ph, qa if with_sq else None, qs if with_sq else None, ds if with_ds else None)
        assert np.array_equal(bits(read(abuf, n)), bits(want[0])) and np.array_equal(bits(read(gbuf, n)), bits(want[1]))
        sq = reference(a, g, ph, np.float32(5.5), np.float32(0.1))[2:4] if with_sq else (np.float32(5.5), np.float32(0.1))
        assert bits(qa.cpu().numpy())[0] == bits(sq[0])[0] and bits(qs.cpu().numpy())[0] == bits(sq[1])[0]
        assert int(ds.item()) == (42 if with_ds and ph != CLOSE else 41)
        assert pads_intact(abuf, n) and pads_intact(gbuf, n)


def test_a_window_of_four_is_the_float32_sum_in_order():
    """OPEN, ADD, ADD, CLOSE over one accumulator: ((g0 + g1) + g2) + g3 in float32, the norm beside it, three ticks"""
    be = ops.backend()
    n = 3 * TRIP + 2
    rng = np.random.default_rng(9)
    gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 2, n)).astype(np.float32) for _ in range(4)]
    sqs = [np.float32(v) for v in (0.3, 1e-8, 7.25, 0.1)]
    abuf, acc = padded(np.full(n, np.nan, np.float32))
    gbuf, grad = padded(gs[0])
    qa, qs, ds = scalars(np.nan, 0.0, 0)
    for j, ph in enumerate((OPEN, ADD, ADD, CLOSE)):
        grad.copy_(torch.from_numpy(gs[j]))
        qs.fill_(float(sqs[j]))
        be.grad_accumulate(acc, grad, n, ph, qa, qs, ds)
    want = ((gs[0] + gs[1]) + gs[2]) + gs[3]
    assert np.array_equal(bits(read(gbuf, n)), bits(want))
    assert bits(qs.cpu().numpy())[0] == bits(np.float32(np.float32(np.float32(sqs[0] + sqs[1]) + sqs[2]) + sqs[3]))[0]
    assert int(ds.item()) == 3 and pads_intact(abuf, n) and pads_intact(gbuf, n)


def test_refusals_launch_nothing():
    lib = _lib.load()
    n = 1024
    a, g = inputs(TRIP + 1)
    abuf, acc = padded(a)
    gbuf, grad = padded(g)
    qa, qs, ds = scalars()
    stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    ap, gp, qap, qsp, dsp = acc.data_ptr(), grad.data_ptr(), qa.data_ptr(), qs.data_ptr(), ds.data_ptr()

    def call(acc=ap, grad=gp, n=n, phase=1, sq_acc=qap, sq_slot=qsp, drop_step=dsp):
        return lib.tnt_grad_accumulate_f32(acc, grad, n, phase, sq_acc, sq_slot, drop_step, None, stream)
    # misaligned and overlapping views of one allocation: never an invalid device address
    bad = {
        "n < 0": dict(n=-1), "null acc": dict(acc=None), "null grad": dict(grad=None),
        "misaligned acc": dict(acc=ap + 4), "misaligned grad": dict(grad=gp + 8),
        "overlapping": dict(grad=ap + 16 * 4, n=100), "the same buffer": dict(grad=ap), "overlapping, grad first": dict(acc=gp + 32 * 4),
        "phase -1": dict(phase=-1), "phase 3": dict(phase=3), "null sq_acc only": dict(sq_acc=None), "null sq_slot only": dict(sq_slot=None),
        "sq_acc == sq_slot": dict(sq_slot=qap),
    }
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc <= -1000, (what, rc)
    torch.cuda.synchronize()
    assert np.array_equal(bits(read(abuf, TRIP + 1)), bits(a)) and pads_intact(abuf, TRIP + 1)
    assert np.array_equal(bits(read(gbuf, TRIP + 1)), bits(g)) and pads_intact(gbuf, TRIP + 1)
    assert float(qa.item()) == 5.5 and float(qs.item()) == np.float32(0.1) and int(ds.item()) == 41
    # adjacent buffers do not overlap
    both = torch.zeros(2048, dtype=torch.float32, device="cuda")
    assert call(acc=both.data_ptr(), grad=both.data_ptr() + 4096, n=1024) == 0
    assert lib.tnt_version() >= 127
