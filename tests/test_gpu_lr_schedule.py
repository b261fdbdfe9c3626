"""The learning-rate schedule launch (tnt_lr_schedule_f32, csrc/schedule.hip) on a real MI355X against the float64
restatement of tests/lr_schedule_oracle.py: every kind, and Warmup around a float and three of the kinds.

Steps 0 .. 40 and 2^31 + 5.  With decay_steps D = 5, warm-up w = 3 / 4 / 7, restart periods 5, 10, 20 (t_mul 2) and 5
(t_mul 1), boundaries 3, 5, 9 and 2, 4 .. 14 that holds 0 and 1; w - 1, w, w + 1; D - 1, D, D + 1 and 3 D + 1 with and
without the warm-up's shift (the staircase, the cycle and the restart boundaries 5, 15, 35); every piecewise boundary with
its neighbours; and a counter that a 32-bit read would truncate to 5.

Tolerances, derived: a kind whose float64 evaluation uses only + - * / and comparisons (constant under a warm-up,
InverseTimeDecay, PiecewiseConstantDecay) is the same sequence of correctly rounded IEEE operations on both sides and
must give np.float32(oracle) bit for bit.  A kind that calls pow or cos differs from the host's libm by a few float64
ulps, 2^-29 of a float32 ulp each, so the two float32 roundings are equal or adjacent:
|dev - float32(o)| <= spacing(float32(o)).

The output word sits between NaN guard words that must survive, every launch runs twice into separate words and must
repeat its bits, and the counter and the parameters are read from device memory."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import _lib
import lr_schedule_oracle as O
from lr_schedule_cases import CASES

pytestmark = pytest.mark.gpu

STEPS = list(range(0, 41)) + [2 ** 31 + 5]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nlr schedule, worst |dev - float32(oracle)| in float32 spacings:", {k: v for k, v in sorted(WORST.items())})


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(params, steps):
    """one launch per step and repeat: out[r, i] for repeat r, step i; the words on both sides of each stay NaN"""
    be = ops.backend()
    p = torch.tensor(params, dtype=torch.float64, device="cuda")
    counters = torch.tensor(steps, dtype=torch.int64, device="cuda")
    out = torch.full((2, len(steps), 3), float("nan"), dtype=torch.float32, device="cuda")
    for r in range(2):
        for i in range(len(steps)):
            be.lr_schedule(counters[i:i + 1], p, out[r, i, 1:2])
    h = out.cpu().numpy()
    assert np.isnan(h[:, :, 0]).all() and np.isnan(h[:, :, 2]).all(), "a word beside the output was written"
    assert counters.cpu().tolist() == list(steps) and p.cpu().tolist()[1:] == list(params)[1:]
    assert np.array_equal(bits(h[0, :, 1]), bits(h[1, :, 1])), "the launch does not repeat its bits"
    return h[0, :, 1]


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_kind_follows_the_oracle(case):
    make, params = CASES[case]
    assert make().params() == params
    got = run(params, STEPS)
    want = np.array([O.lr32(params, s) for s in STEPS], np.float32)
    assert np.isfinite(want).all()
    if O.is_exact(params):
        assert np.array_equal(bits(got), bits(want)), (case, [(s, g, w) for s, g, w in zip(STEPS, got, want) if g != w])
        return
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    WORST[case] = float(err.max())
    assert (err <= 1.0).all(), (case, [(s, g, w) for s, g, w, e in zip(STEPS, got, want, err) if e > 1.0])
    # and not a constant: the schedule moves over these steps
    assert len(set(bits(got).tolist())) > 3


def test_the_counter_is_read_as_64_bits():
    _, params = CASES["warmup float"]              # ramp over 7 steps, then 0.3: a counter cut to 32 bits would read 5
    got = run(params, [5, 2 ** 31 + 5, 2 ** 32 + 5, 2 ** 40])
    assert got[0] == O.lr32(params, 5) != np.float32(0.3) and (bits(got[1:]) == bits(np.float32(0.3))).all()
    assert run(params, [-3])[0] == O.lr32(params, 0) == np.float32(0.01)          # a negative counter counts as 0


def test_an_unknown_kind_gives_nan():
    for params in ([8.0] + [0.0] * 15, [-1.0] + [0.0] * 15, [0.5] + [0.0] * 15, [float("nan")] + [0.0] * 15,
                   [float("inf")] + [0.0] * 15, O.pack(O.COSINE, [1e-2, 0, 0.1]), O.pack(O.CONSTANT, [0.1], w=1.5),
                   O.pack(O.RESTARTS, [0.1, 1, 1.0 + 2.0 ** -30, 1.0, 0.0])):
        got = run(params, [0, 3, 10 ** 6])
        assert np.isnan(O.lr64(params, 10 ** 6))
        assert np.isnan(got[2]) and all(np.isnan(g) == np.isnan(O.lr64(params, s)) for g, s in zip(got, [0, 3, 10 ** 6])), params


def test_null_pointers_are_refused_and_nothing_is_launched():
    lib = _lib.load()
    stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = torch.tensor(O.pack(O.CONSTANT, [0.25]), dtype=torch.float64, device="cuda")
    out = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    sp, pp, op = step.data_ptr(), p.data_ptr(), out.data_ptr() + 4
    for args in ((None, pp, op), (sp, None, op), (sp, pp, None)):
        assert lib.tnt_lr_schedule_f32(*args, stream) <= -1000, args
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()
    assert lib.tnt_lr_schedule_f32(sp, pp, op, stream) == 0
    assert out.cpu().numpy().tolist()[1] == 0.25 and lib.tnt_version() >= 121
