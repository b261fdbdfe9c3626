"""Restatement of the weight-averaging launch (tnt_weight_average_f32, definition in include/tnt_hip.h) in float64: the
launch's decision (``plan``), one launch on float32 inputs with the error bound of the kernel's two roundings
(``reference``), the recursion over a training run's parameter snapshots with the accumulated bound (``Recursion``), and a
MockBackend with the two ops (``weight_average``, ``swap``).

Error model.  From the float32 inputs w = theta[i], e = avg[i] and the float32 constant c, the exact result is
e* = e + c (w - e).  The kernel rounds the difference, fl(w - e) = (w - e)(1 + d1), and then the fma,
out = (c fl(w - e) + e)(1 + d2), with |d1|, |d2| <= u / (1 + u), u = 2^-24 (round to nearest).  So
  out - e* = c (w - e) d1 + (e* + c (w - e) d1) d2,   |out - e*| <= u (c |w - e| + |e*|)
(the second-order term is covered: u (1 + 2u) / (1 + u)^2 <= u), plus 2^-149 where the fma's result is subnormal (a
subnormal difference is exact)."""
import numpy as np

from mock_backend import MockBackend, flat

U = 2.0 ** -24
TINY = 2.0 ** -149        # the smallest float32 subnormal
EMA, SWA = 0, 1


def plan(t, kind, momentum, dynamic, start_step, every):
    """what the launch does at step counter t: ("copy", None), ("skip", None) or ("blend", c), c = float32(1 - decay) as a
    Python float, the decay in float64"""
    s = max(int(start_step), 1)
    t = int(t)
    if t <= s:
        return "copy", None
    r = t - s
    if r % int(every):
        return "skip", None
    k = float(r // int(every))
    if kind == SWA:
        d = k / (k + 1.0)
    else:
        d = float(momentum)
        if dynamic:
            d = min(d, (1.0 + k) / (10.0 + k))
    return "blend", float(np.float32(1.0 - d))


def reference(theta32, avg32, t, kind, momentum, dynamic, start_step, every, guard=0):
    """one launch on float32 arrays: (mode, out float64, bound float64); mode "copy" / "skip" / "guard" have bound 0 (the
    result is bitwise theta or the old avg)"""
    w, e = np.asarray(theta32, np.float32).astype(np.float64), np.asarray(avg32, np.float32).astype(np.float64)
    if guard:
        return "guard", e, np.zeros_like(e)
    mode, c = plan(t, kind, momentum, dynamic, start_step, every)
    if mode == "copy":
        return mode, w, np.zeros_like(w)
    if mode == "skip":
        return mode, e, np.zeros_like(e)
    out = e + c * (w - e)
    return mode, out, U * (c * np.abs(w - e) + np.abs(out)) + TINY


class Recursion:
    """The average over a run, in float64, from the parameter snapshots after every update: ``step(theta32)`` is the launch
    behind update number ``t`` (1, 2, ...).  ``tol`` accumulates the per-launch bounds; each is taken at the float64 state
    widened by the tolerance so far, so that it covers the launch the device ran on its own (float32) state.  A copy
    resets it: the slot then holds the snapshot's bits."""

    def __init__(self, theta32, kind, momentum, dynamic, start_step, every):
        self.cfg = (kind, momentum, dynamic, start_step, every)
        self.avg = np.asarray(theta32, np.float32).astype(np.float64).copy()       # opt_avg starts as a copy of theta
        self.tol = np.zeros_like(self.avg)
        self.t = 0
        self.modes = []

    def step(self, theta32, guard=0):
        if guard:                               # the counters do not advance and nothing is touched
            self.modes.append("guard")
            return self.avg, self.tol
        self.t += 1
        w = np.asarray(theta32, np.float32).astype(np.float64)
        mode, c = plan(self.t, *self.cfg)
        self.modes.append(mode)
        if mode == "copy":
            self.avg, self.tol = w.copy(), np.zeros_like(w)
        elif mode == "blend":
            out = self.avg + c * (w - self.avg)
            self.tol = self.tol + U * (c * (np.abs(w - self.avg) + self.tol) + np.abs(out) + self.tol) + TINY
            self.avg = out
        return self.avg, self.tol


class AverageMockBackend(MockBackend):
    """MockBackend plus tnt_weight_average_f32 and tnt_swap_f32 from the header text; ``avg_calls`` logs each averaging
    call's scalar arguments, the counter it saw and what it did"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.avg_calls = []

    def weight_average(self, theta, avg, n, step, kind, momentum, dynamic, start_step, every, guard=None):
        assert n >= 0 and every >= 1 and start_step >= 0 and 0.0 <= momentum < 1.0 and kind in (EMA, SWA)
        assert theta.data_ptr() % 16 == 0 and avg.data_ptr() % 16 == 0
        assert theta.data_ptr() + 4 * n <= avg.data_ptr() or avg.data_ptr() + 4 * n <= theta.data_ptr()
        g = int(guard[0]) if guard is not None else 0
        t = int(flat(step)[0])
        mode, out, _ = reference(flat(theta)[:n], flat(avg)[:n], t, kind, momentum, dynamic, start_step, every, guard=g)
        self.avg_calls.append(dict(n=n, t=t, kind=kind, momentum=momentum, dynamic=bool(dynamic), start_step=start_step,
                                   every=every, guard=g, mode=mode))
        if mode in ("copy", "blend"):
            flat(avg)[:n] = out

    def swap(self, a, b, n):
        assert n >= 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        assert a.data_ptr() + 4 * n <= b.data_ptr() or b.data_ptr() + 4 * n <= a.data_ptr()
        x = flat(a)[:n].copy()
        flat(a)[:n] = flat(b)[:n]
        flat(b)[:n] = x
