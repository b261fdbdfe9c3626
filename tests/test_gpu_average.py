"""The weight-averaging launch and the swap (tnt_weight_average_f32, tnt_swap_f32, csrc/average.hip) on a real MI355X
against float64 (tests/average_oracle.py).

Sizes: the n % 4 tail alone (1, 3), one float4 (4, 5), one workgroup's round of 256 float4s (1023 .. 1025), the boundary
of the AV_U = 4 rounds a lane keeps in flight (4 * 256 * 4 = 4096 +- 1) and the grid-stride loop with a ragged last trip
(1 000 003).  Every mode runs at every size.  The step counter lives on the device and is set there between launches.

Bound (derived in tests/average_oracle.py): with the float32 inputs and the float32 constant c the exact result is
e* = e + c (w - e); the kernel rounds the difference and then the fma, so |out - e*| <= 2^-24 (c |w - e| + |e*|) + 2^-149
for every element.  Copies, skips and guarded launches are bitwise; theta is bitwise unchanged always; the buffers sit
between sentinel words that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import _lib
from average_oracle import EMA, SWA, Recursion, plan, reference

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 1_000_003]
PAD = 64                 # sentinel floats on both sides of a buffer (keeps the 16-byte alignment)
SENT = -7.25

# name: (t, kind, momentum, dynamic, start_step, every, guard, what must happen)
MODES = {
    "copy, t < s": (2, EMA, 0.9, 0, 5, 1, None, "copy"),
    "copy, t == s": (5, EMA, 0.9, 0, 5, 1, None, "copy"),
    "copy, start_step 0 at t = 1": (1, EMA, 0.9, 0, 0, 1, None, "copy"),
    "copy, swa": (3, SWA, 0.0, 0, 3, 2, None, "copy"),
    "skip, r % every != 0": (4, EMA, 0.5, 0, 2, 3, None, "skip"),
    "skip, swa": (6, SWA, 0.0, 0, 1, 2, None, "skip"),
    "ema 0.5": (3, EMA, 0.5, 0, 0, 1, None, "blend"),
    "ema 0.999": (7, EMA, 0.999, 0, 0, 1, None, "blend"),
    "ema 0": (2, EMA, 0.0, 0, 0, 1, None, "blend"),
    "ema 0.5, every 3": (8, EMA, 0.5, 0, 2, 3, None, "blend"),
    "dynamic, (1 + n) / (10 + n) wins": (2, EMA, 0.999, 1, 0, 1, None, "blend"),
    "dynamic, momentum wins": (1001, EMA, 0.9, 1, 0, 1, None, "blend"),
    "swa, n = 1": (2, SWA, 0.0, 0, 0, 1, None, "blend"),
    "swa, n = 7": (17, SWA, 0.0, 0, 3, 2, None, "blend"),
    "guard word set": (3, EMA, 0.5, 0, 0, 1, 3, "guard"),
    "guard word clear": (3, EMA, 0.5, 0, 0, 1, 0, "blend"),
    "step counter past 2^32": ((1 << 33) + 1, EMA, 0.5, 0, 1, 2, None, "blend"),
}

WORST = {"blend": 0.0}
_INPUTS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"\nweight average, worst observed error / bound: {WORST['blend']:.6g}")


def inputs(n):
    """(theta, avg) float32 of mixed magnitudes (1e-6 .. 1e3, both signs), with zeros, theta == avg elements, elements
    that differ in the last bit, and a few subnormals; computed once per size and never modified"""
    if n not in _INPUTS:
        rng = np.random.default_rng(1000 + n)
        w = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        e = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        k = np.arange(n)
        e[k % 7 == 0] = w[k % 7 == 0]                                  # theta == avg
        w[k % 11 == 0] = 0.0                                           # zeros, in one buffer or in both
        e[k % 13 == 0] = 0.0
        near = k % 17 == 0
        e[near] = np.nextafter(w[near], np.float32(np.inf))           # one ulp apart
        sub = k % 19 == 0
        w[sub] = np.float32(3e-42)                                     # subnormal
        e[sub & (k % 2 == 0)] = np.float32(-1e-41)
        w.setflags(write=False)
        e.setflags(write=False)
        _INPUTS[n] = (w, e)
    return _INPUTS[n]


def padded(x):
    """x on the device between PAD sentinel floats; returns (whole buffer, the view of x)"""
    buf = torch.full((x.size + 2 * PAD,), SENT, dtype=torch.float32, device="cuda")
    view = buf[PAD:PAD + x.size]
    view.copy_(torch.from_numpy(x.copy()))
    assert view.data_ptr() % 16 == 0
    return buf, view


def pads_intact(buf, n):
    h = buf.cpu().numpy()
    return (h[:PAD] == SENT).all() and (h[PAD + n:] == SENT).all()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_blend(out, want, bound, what):
    err = np.abs(out.astype(np.float64) - want)
    r = float(np.max(err / bound))
    WORST["blend"] = max(WORST["blend"], r)
    assert r <= 1.0, f"{what}: error {r:.3g} x its bound at element {int(np.argmax(err / bound))}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_launch(mode, n):
    t, kind, mom, dyn, start, every, guard, expect = MODES[mode]
    be = ops.backend()
    w, e = inputs(n)
    tbuf, theta = padded(w)
    abuf, avg = padded(e)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    step.fill_(t)                                                      # set on the device, never passed by value
    gd = None if guard is None else torch.full((1,), guard, dtype=torch.int32, device="cuda")
    be.weight_average(theta, avg, n, step, kind, mom, dyn, start, every, guard=gd)
    out = avg.cpu().numpy()
    got_mode, want, bound = reference(w, e, t, kind, mom, dyn, start, every, guard=guard or 0)
    assert got_mode == expect
    assert np.array_equal(bits(theta.cpu().numpy()), bits(w)), "theta was written"
    assert pads_intact(tbuf, n) and pads_intact(abuf, n), "a word outside the buffers was written"
    assert int(step.item()) == t
    if expect == "copy":
        assert np.array_equal(bits(out), bits(w))
    elif expect in ("skip", "guard"):
        assert np.array_equal(bits(out), bits(e))
    else:
        check_blend(out, want, bound, f"{mode}, n = {n}")
        same = bits(w) == bits(e)
        assert np.array_equal(bits(out)[same], bits(e)[same])          # theta == avg stays, whatever c


@pytest.mark.parametrize("n", [5, 4097, 1_000_003])
@pytest.mark.parametrize("kind", [EMA, SWA])
def test_a_run_with_the_counter_advancing_on_the_device(kind, n):
    """eight launches with the same arguments; only the device counter and theta change between them"""
    be = ops.backend()
    mom, dyn, start, every = 0.75, 1, 2, 2
    rng = np.random.default_rng(n + kind)
    w0, e0 = inputs(n)
    tbuf, theta = padded(w0)
    abuf, avg = padded(e0)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    rec = Recursion(e0, kind, mom, dyn, start, every)
    for t in range(1, 9):
        w = (np.asarray(w0) + rng.standard_normal(n).astype(np.float32) * np.float32(0.1 * t)).astype(np.float32)
        theta.copy_(torch.from_numpy(w))
        step.add_(1)
        be.weight_average(theta, avg, n, step, kind, mom, dyn, start, every)
        want, tol = rec.step(w)
        out = avg.cpu().numpy()
        if rec.modes[-1] == "copy":
            assert np.array_equal(bits(out), bits(w)), t
        else:
            assert (np.abs(out.astype(np.float64) - want) <= tol).all(), (t, rec.modes[-1])
    assert rec.modes == ["copy", "copy", "skip", "blend", "skip", "blend", "skip", "blend"]
    assert plan(8, kind, mom, dyn, start, every)[0] == "blend" and pads_intact(tbuf, n) and pads_intact(abuf, n)


@pytest.mark.parametrize("n", SIZES)
def test_swap(n):
    be = ops.backend()
    w, e = inputs(n)
    abuf, a = padded(w)
    bbuf, b = padded(e)
    be.swap(a, b, n)
    assert np.array_equal(bits(a.cpu().numpy()), bits(e)) and np.array_equal(bits(b.cpu().numpy()), bits(w))
    assert pads_intact(abuf, n) and pads_intact(bbuf, n)
    be.swap(a, b, n)
    assert np.array_equal(bits(a.cpu().numpy()), bits(w)) and np.array_equal(bits(b.cpu().numpy()), bits(e))
    assert pads_intact(abuf, n) and pads_intact(bbuf, n)


def test_refusals_launch_nothing():
    lib = _lib.load()
    n = 1024
    w, e = inputs(1025)
    tbuf, theta = padded(w)
    abuf, avg = padded(e)
    step = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    tp, ap, sp = theta.data_ptr(), avg.data_ptr(), step.data_ptr()

    def average(theta=tp, avg=ap, n=n, step=sp, kind=0, momentum=0.5, dynamic=0, start_step=0, every=1):
        mom = ctypes.c_double(momentum) if momentum is not None else None
        return lib.tnt_weight_average_f32(theta, avg, n, step, kind, ctypes.addressof(mom) if mom is not None else None,
                                          dynamic, start_step, every, None, stream)
    bad = {
        "every = 0": dict(every=0), "every < 0": dict(every=-2), "momentum 1.0": dict(momentum=1.0),
        "momentum < 0": dict(momentum=-0.25), "momentum NaN": dict(momentum=float("nan")), "null momentum": dict(momentum=None),
        "misaligned theta": dict(theta=tp + 4), "misaligned avg": dict(avg=ap + 8),
        "overlapping": dict(avg=tp + 16 * 4, n=100), "the same buffer": dict(avg=tp), "overlapping, avg first": dict(theta=ap + 32 * 4),
        "n < 0": dict(n=-1), "start_step < 0": dict(start_step=-1), "kind 2": dict(kind=2), "null step": dict(step=None),
        "null theta": dict(theta=None), "null avg": dict(avg=None),
    }
    for what, kw in bad.items():
        assert average(**kw) != 0, what
    for what, rc in {"swap misaligned": lib.tnt_swap_f32(tp + 4, ap, n, stream), "swap overlapping": lib.tnt_swap_f32(tp, tp + 64, n, stream),
                     "swap n < 0": lib.tnt_swap_f32(tp, ap, -1, stream), "swap null": lib.tnt_swap_f32(tp, None, n, stream)}.items():
        assert rc != 0, what
    torch.cuda.synchronize()
    assert np.array_equal(bits(tbuf.cpu().numpy()[PAD:PAD + 1025]), bits(w)) and pads_intact(tbuf, 1025)
    assert np.array_equal(bits(abuf.cpu().numpy()[PAD:PAD + 1025]), bits(e)) and pads_intact(abuf, 1025)
    # adjacent buffers do not overlap; n = 0 is a no-op
    both = torch.zeros(2048, dtype=torch.float32, device="cuda")
    assert average(theta=both.data_ptr(), avg=both.data_ptr() + 4096, n=1024) == 0
    assert average(n=0) == 0 and lib.tnt_swap_f32(tp, ap, 0, stream) == 0
    assert lib.tnt_version() >= 119
