"""Restatement of the learning-rate schedule launch (tnt_lr_schedule_f32, definition and parameter layout in
include/tnt_hip.h) in float64 with ``math`` only, written from the header text and independently of
masters_thesis_amd/schedules.py: ``pack`` lays the 16 parameters out, ``lr64`` evaluates them at a step, ``lr32`` rounds
once to float32, and ``LrScheduleMockBackend`` is a MockBackend with the op.

Python floats are IEEE float64 and every product and sum below is rounded on its own, in the header's order, so for the
kinds without pow / cos the device must reproduce ``lr32`` bit for bit."""
import math

import numpy as np

from mock_backend import MockBackend, flat

CONSTANT, EXPONENTIAL, INVERSE_TIME, COSINE, RESTARTS, POLYNOMIAL, PIECEWISE, PIECEWISE_WARM = range(8)
RESTART_TRIPS = 4096
EXACT_KINDS = (CONSTANT, INVERSE_TIME, PIECEWISE, PIECEWISE_WARM)       # + - * / and comparisons only


def pack(kind, fields, w=0, start=0.0):
    """kinds 0 - 5: [kind, w, start, fields..., 0...]"""
    assert kind in range(6) and len(fields) <= 13
    return [float(kind), float(w), float(start)] + [float(f) for f in fields] + [0.0] * (13 - len(fields))


def pack_piecewise(boundaries, values, w=0, start=0.0):
    """kind 6 (no warm-up: 7 boundaries, 8 values) or kind 7 (warm-up fields, 6 boundaries, 7 values); unused boundaries
    +inf, unused values the last one"""
    nb = 6 if w else 7
    assert 1 <= len(boundaries) <= nb and len(values) == len(boundaries) + 1
    b = [float(x) for x in boundaries] + [math.inf] * (nb - len(boundaries))
    v = [float(x) for x in values] + [float(values[-1])] * (nb - len(boundaries))
    return ([float(PIECEWISE_WARM), float(w), float(start)] if w else [float(PIECEWISE)]) + b + v


def _piecewise(bounds, values, s):
    for i, b in enumerate(bounds):
        if float(s) <= b:
            return values[i]
    return values[len(bounds)]


def _kind(k, f, s):
    """the kind's value at s >= 0 updates"""
    if k == CONSTANT:
        return f[0]
    if k in (EXPONENTIAL, INVERSE_TIME):
        lr0, D, rate, stair = f[0], int(f[1]), f[2], f[3]
        if D < 1:
            return math.nan
        p = float(s // D) if stair != 0.0 else float(s) / float(D)
        if k == EXPONENTIAL:
            return lr0 * math.pow(rate, p)
        t = rate * p
        return lr0 / (1.0 + t)
    if k == COSINE:
        lr0, D, alpha = f[0], int(f[1]), f[2]
        if D < 1:
            return math.nan
        c = float(min(s, D)) / float(D)
        shape = (1.0 - alpha) * 0.5
        shape = shape * (1.0 + math.cos(math.pi * c))
        return lr0 * (shape + alpha)
    if k == RESTARTS:
        lr0, first, t_mul, m_mul, alpha = f[0], int(f[1]), f[2], f[3], f[4]
        if first < 1:
            return math.nan
        P = float(first)
        if t_mul == 1.0:
            r, m = float(s % first), math.pow(m_mul, float(s // first))
        else:
            r, m, trip = float(s), 1.0, 0
            while r >= P:
                if trip == RESTART_TRIPS:
                    return math.nan
                r, P, m, trip = r - P, P * t_mul, m * m_mul, trip + 1
        shape = (1.0 - alpha) * m
        shape = shape * 0.5
        shape = shape * (1.0 + math.cos(math.pi * r / P))
        return lr0 * (shape + alpha)
    if k == POLYNOMIAL:
        lr0, D, end, power, cycle = f[0], int(f[1]), f[2], f[3], f[4]
        if D < 1:
            return math.nan
        if cycle != 0.0:
            D = D * max(1, (s + D - 1) // D)
        else:
            s = min(s, D)
        p = float(s) / float(D)
        t = (lr0 - end) * math.pow(1.0 - p, power)
        return t + end
    return math.nan


def lr64(params, step):
    """the float64 value the launch rounds, from the 16 parameters and the counter"""
    p = [float(x) for x in params]
    assert len(p) == 16
    s = max(int(step), 0)
    k = int(p[0]) if (0.0 <= p[0] <= 7.0 and p[0] == int(p[0])) else -1
    if k == PIECEWISE:
        return _piecewise(p[1:8], p[8:16], s)
    if k < 0 or not p[1] >= 0.0 or p[1] != int(p[1]):
        return math.nan
    w, start, f = int(p[1]), p[2], p[3:]
    at = (lambda x: _piecewise(f[0:6], f[6:13], x)) if k == PIECEWISE_WARM else (lambda x: _kind(k, f, x))
    if s < w:
        t = (at(0) - start) * float(s)
        return start + t / float(w)
    return at(s - w)


def lr32(params, step):
    return np.float32(lr64(params, step))


def is_exact(params):
    """does the definition promise the oracle's bits (no pow, no cos)?  The warm-up ramp reads the kind at 0 updates,
    which is exact for kinds 0 - 2, 5 (pow(x, 0) = 1, pow(1, y) = 1) but goes through cos(0) for 3, 4: counted inexact."""
    return int(params[0]) in EXACT_KINDS


class LrScheduleMockBackend(MockBackend):
    """MockBackend plus tnt_lr_schedule_f32 from the header text; ``lr_calls`` logs the counter each call saw and the
    float32 it stored"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.lr_calls = []

    def lr_schedule(self, step, params, lr):
        assert step.dtype.is_floating_point is False and step.element_size() == 8
        assert params.element_size() == 8 and params.dtype.is_floating_point and params.numel() == 16
        assert lr.element_size() == 4 and lr.dtype.is_floating_point
        s = int(flat(step)[0])
        v = lr32(flat(params)[:16].tolist(), s)
        self.lr_calls.append(dict(s=s, lr=float(v)))
        flat(lr)[0] = v
