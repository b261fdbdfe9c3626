"""Keras-style learning-rate schedules (tf.keras.optimizers.schedules), also reachable as ``optimizers.schedules``.

``Adam(learning_rate=CosineDecay(...))`` as in AttemptFour/main.py:81-84.  A schedule carries hyper-parameters only.  A
model compiled with one evaluates it on the device, once per training step, from its own update counter: one
tnt_lr_schedule_f32 launch in front of the update (ModelBase._lr_schedule_launch; the definition and the layout of
``params()`` are in include/tnt_hip.h), so the rule is Keras's ``lr = schedule(optimizer.iterations)`` inside the
recorded launch plan or hipGraph of the step.  ``schedule(step)`` is the same value on the host, for plotting.

``step`` counts the updates applied so far: the first update uses step 0.  All arithmetic is float64, each product and
sum rounded on its own, and the result is rounded once to float32.  Every ``decay_steps`` and boundary is an integer
>= 1, so staircases and cycles are integer divisions.  ``Warmup`` is this library's own (it replaces the reference's
Callbacks/WarmupScheduler.py, which never ran)."""
import math
import numbers

import numpy as np

N_PARAMS = 16
MAX_COUNT = 2 ** 31          # decay_steps, boundaries and warm-up steps stay below this
F32_MAX = float(np.finfo(np.float32).max)
# CosineDecayRestarts finds the period by a subtraction loop, on the device too: 1 < t_mul < T_MUL_MIN would make it long
# (t_mul = 1 has a closed form).  With t_mul >= 1.05 a counter below 2^63 leaves it in under 900 trips
T_MUL_MIN = 1.05


def _num(name, v, lo=None, hi=None, lo_open=False):
    """the value as a float; ValueError unless it is a finite number inside [lo, hi] (``lo_open``: (lo, hi])"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    if not math.isfinite(f):
        raise ValueError(f"{name} must be finite, got {v!r}")
    if (lo is not None and (f <= lo if lo_open else f < lo)) or (hi is not None and f > hi):
        raise ValueError(f"{name} is out of range, got {v!r}")
    return f


def _rate(name, v):
    """a learning rate: finite, >= 0 and a finite float32"""
    return _num(name, v, 0.0, F32_MAX)


def _count(name, v, lo=1):
    """the value as an int; ValueError unless it is an integer in [lo, 2^31) (bool excluded)"""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or v >= MAX_COUNT:
        raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    return int(v)


def _step(step):
    if isinstance(step, bool) or not isinstance(step, numbers.Integral) or step < 0:
        raise ValueError(f"step must be an int >= 0, got {step!r}")
    return int(step)


class LearningRateSchedule:
    """Base class: ``KIND`` is the kind id of tnt_lr_schedule_f32, ``fields()`` the kind's float64 fields, ``value(s)``
    the float64 schedule at ``s`` updates."""

    KIND = None

    def fields(self):
        raise NotImplementedError

    def value(self, s):
        raise NotImplementedError

    def params(self):
        """the 16 float64 parameters of tnt_lr_schedule_f32: kind id, warm-up steps (0: none), warm-up start, fields"""
        f = [float(x) for x in self.fields()]
        assert len(f) <= N_PARAMS - 3
        return [float(self.KIND), 0.0, 0.0] + f + [0.0] * (N_PARAMS - 3 - len(f))

    def __call__(self, step):
        """the learning rate the update behind ``step`` applied updates uses: float64 arithmetic, rounded to float32"""
        return float(np.float32(self.value(_step(step))))

    def key(self):
        return (type(self).__name__,) + tuple(self.params())

    def __eq__(self, other):
        return isinstance(other, LearningRateSchedule) and self.key() == other.key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.key())

    def get_config(self):
        return {k: v for k, v in vars(self).items() if not k.startswith("_")}

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


class _Constant(LearningRateSchedule):
    """a float learning rate under a Warmup"""

    KIND = 0

    def __init__(self, learning_rate):
        self.learning_rate = _rate("learning_rate", learning_rate)

    def fields(self):
        return [self.learning_rate]

    def value(self, s):
        return self.learning_rate


class _Decay(LearningRateSchedule):
    """initial_learning_rate, decay_steps, decay_rate, staircase: p = s / decay_steps, or s // decay_steps"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self.initial_learning_rate = _rate("initial_learning_rate", initial_learning_rate)
        self.decay_steps = _count("decay_steps", decay_steps)
        self.decay_rate = self._check_rate(decay_rate)
        self.staircase = bool(staircase)

    def fields(self):
        return [self.initial_learning_rate, self.decay_steps, self.decay_rate, float(self.staircase)]

    def _p(self, s):
        return float(s // self.decay_steps) if self.staircase else float(s) / float(self.decay_steps)


class ExponentialDecay(_Decay):
    """tf.keras.optimizers.schedules.ExponentialDecay: lr0 * decay_rate ** p (decay_rate > 0)"""

    KIND = 1

    @staticmethod
    def _check_rate(v):
        return _num("decay_rate", v, 0.0, lo_open=True)

    def value(self, s):
        return self.initial_learning_rate * math.pow(self.decay_rate, self._p(s))


class InverseTimeDecay(_Decay):
    """tf.keras.optimizers.schedules.InverseTimeDecay: lr0 / (1 + decay_rate * p) (decay_rate >= 0)"""

    KIND = 2

    @staticmethod
    def _check_rate(v):
        return _num("decay_rate", v, 0.0)

    def value(self, s):
        return self.initial_learning_rate / (1.0 + self.decay_rate * self._p(s))


class CosineDecay(LearningRateSchedule):
    """tf.keras.optimizers.schedules.CosineDecay: c = min(s, D) / D; lr0 * ((1 - alpha) * 0.5 * (1 + cos(pi c)) + alpha),
    0 <= alpha <= 1"""

    KIND = 3

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0):
        self.initial_learning_rate = _rate("initial_learning_rate", initial_learning_rate)
        self.decay_steps = _count("decay_steps", decay_steps)
        self.alpha = _num("alpha", alpha, 0.0, 1.0)

    def fields(self):
        return [self.initial_learning_rate, self.decay_steps, self.alpha]

    def value(self, s):
        c = float(min(s, self.decay_steps)) / float(self.decay_steps)
        return self.initial_learning_rate * ((1.0 - self.alpha) * 0.5 * (1.0 + math.cos(math.pi * c)) + self.alpha)


class CosineDecayRestarts(LearningRateSchedule):
    """tf.keras.optimizers.schedules.CosineDecayRestarts (SGDR): cosine cycles of first_decay_steps, each ``t_mul`` times
    as long and starting ``m_mul`` times as high as the one before.  The cycle is found by subtraction, not by Keras's
    logarithm, so host and device agree at every restart boundary; ``t_mul`` is 1 or >= 1.05 (T_MUL_MIN: the loop's
    length on the device), 0 < m_mul, 0 <= alpha <= 1."""

    KIND = 4

    def __init__(self, initial_learning_rate, first_decay_steps, t_mul=2.0, m_mul=1.0, alpha=0.0):
        self.initial_learning_rate = _rate("initial_learning_rate", initial_learning_rate)
        self.first_decay_steps = _count("first_decay_steps", first_decay_steps)
        self.t_mul = _num("t_mul", t_mul, 1.0)
        if 1.0 < self.t_mul < T_MUL_MIN:
            raise ValueError(f"t_mul must be 1 or at least {T_MUL_MIN} (the period is found by a subtraction loop), got {t_mul!r}")
        self.m_mul = _num("m_mul", m_mul, 0.0, lo_open=True)
        self.alpha = _num("alpha", alpha, 0.0, 1.0)

    def fields(self):
        return [self.initial_learning_rate, self.first_decay_steps, self.t_mul, self.m_mul, self.alpha]

    def value(self, s):
        first = self.first_decay_steps
        period = float(first)
        if self.t_mul == 1.0:
            r, m = float(s % first), math.pow(self.m_mul, float(s // first))
        else:
            r, m = float(s), 1.0
            while r >= period:
                r -= period
                period *= self.t_mul
                m *= self.m_mul
        return self.initial_learning_rate * ((1.0 - self.alpha) * m * 0.5 * (1.0 + math.cos(math.pi * r / period)) + self.alpha)


class PolynomialDecay(LearningRateSchedule):
    """tf.keras.optimizers.schedules.PolynomialDecay: (lr0 - end) * (1 - s' / D') ** power + end with s' = min(s, D),
    D' = D; with ``cycle`` s' = s and D' = D * max(1, ceil(s / D)).  power > 0."""

    KIND = 5

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0, cycle=False):
        self.initial_learning_rate = _rate("initial_learning_rate", initial_learning_rate)
        self.decay_steps = _count("decay_steps", decay_steps)
        self.end_learning_rate = _rate("end_learning_rate", end_learning_rate)
        self.power = _num("power", power, 0.0, lo_open=True)
        self.cycle = bool(cycle)

    def fields(self):
        return [self.initial_learning_rate, self.decay_steps, self.end_learning_rate, self.power, float(self.cycle)]

    def value(self, s):
        d = self.decay_steps
        if self.cycle:
            d *= max(1, -(-s // d))
        else:
            s = min(s, d)
        p = float(s) / float(d)
        return (self.initial_learning_rate - self.end_learning_rate) * math.pow(1.0 - p, self.power) + self.end_learning_rate


class PiecewiseConstantDecay(LearningRateSchedule):
    """tf.keras.optimizers.schedules.PiecewiseConstantDecay: values[i] for the first i with s <= boundaries[i], else the
    last value.  1 to 7 strictly increasing integer boundaries and one more value than boundaries."""

    KIND = 6
    MAX_BOUNDARIES = 7

    def __init__(self, boundaries, values):
        try:
            boundaries, values = list(boundaries), list(values)
        except TypeError:
            raise ValueError("boundaries and values must be sequences") from None
        if not 1 <= len(boundaries) <= self.MAX_BOUNDARIES:
            raise ValueError(f"PiecewiseConstantDecay takes 1 to {self.MAX_BOUNDARIES} boundaries, got {len(boundaries)}")
        if len(values) != len(boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay takes one more value than boundaries")
        self.boundaries = [_count(f"boundaries[{i}]", b) for i, b in enumerate(boundaries)]
        if any(b <= a for a, b in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError(f"boundaries must increase strictly, got {boundaries!r}")
        self.values = [_rate(f"values[{i}]", v) for i, v in enumerate(values)]

    def _padded(self, nb):
        pad = nb - len(self.boundaries)
        return [float(b) for b in self.boundaries] + [math.inf] * pad + self.values + [self.values[-1]] * pad

    def params(self):
        return [float(self.KIND)] + self._padded(self.MAX_BOUNDARIES)

    def value(self, s):
        for b, v in zip(self.boundaries, self.values):
            if s <= b:
                return v
        return self.values[-1]


class Warmup(LearningRateSchedule):
    """Linear warm-up in front of ``after``, a float or one of the schedules above: for s < warmup_steps
    warmup_start + (after(0) - warmup_start) * s / warmup_steps, from warmup_steps on after(s - warmup_steps).  Continuous
    at warmup_steps.  Per update, evaluated on the device like every schedule.  Around a PiecewiseConstantDecay: at most 6
    boundaries (the warm-up's two fields take their place in the 16 parameters)."""

    PIECEWISE_KIND = 7

    def __init__(self, after, warmup_steps, warmup_start=0.0):
        if isinstance(after, Warmup):
            raise ValueError("Warmup wraps a float or a decay schedule, not another Warmup")
        if not isinstance(after, LearningRateSchedule):
            after = _Constant(after)
        if isinstance(after, PiecewiseConstantDecay) and len(after.boundaries) > after.MAX_BOUNDARIES - 1:
            raise ValueError(f"Warmup around a PiecewiseConstantDecay takes at most {after.MAX_BOUNDARIES - 1} boundaries")
        self.after = after
        self.warmup_steps = _count("warmup_steps", warmup_steps)
        self.warmup_start = _rate("warmup_start", warmup_start)

    @property
    def KIND(self):
        return self.PIECEWISE_KIND if isinstance(self.after, PiecewiseConstantDecay) else self.after.KIND

    def params(self):
        if isinstance(self.after, PiecewiseConstantDecay):
            f = self.after._padded(self.after.MAX_BOUNDARIES - 1)
        else:
            f = self.after.params()[3:]
        return [float(self.KIND), float(self.warmup_steps), self.warmup_start] + f

    def value(self, s):
        w = self.warmup_steps
        if s < w:
            return self.warmup_start + (self.after.value(0) - self.warmup_start) * float(s) / float(w)
        return self.after.value(s - w)


KINDS = {"ExponentialDecay": ExponentialDecay, "InverseTimeDecay": InverseTimeDecay, "CosineDecay": CosineDecay,
         "CosineDecayRestarts": CosineDecayRestarts, "PolynomialDecay": PolynomialDecay,
         "PiecewiseConstantDecay": PiecewiseConstantDecay}


def from_config(cfg):
    """A schedule from a mapping (config.yaml's ``lr_schedule:``): ``kind`` names the class, the other keys are its
    arguments; ``warmup_steps`` (and ``warmup_start``) wrap it in a Warmup."""
    if not isinstance(cfg, dict) or "kind" not in cfg:
        raise ValueError(f"lr_schedule must be a mapping with a 'kind' key, got {cfg!r}")
    args = dict(cfg)
    kind = args.pop("kind")
    w, start = args.pop("warmup_steps", None), args.pop("warmup_start", 0.0)
    if kind not in KINDS:
        raise ValueError(f"lr_schedule kind must be one of {sorted(KINDS)}, got {kind!r}")
    try:
        inner = KINDS[kind](**args)
    except TypeError as e:
        raise ValueError(f"lr_schedule {kind}: {e}") from None
    return inner if w is None else Warmup(inner, w, start)
