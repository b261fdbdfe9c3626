"""The schedules the learning-rate tests share: name -> (the descriptor of masters_thesis_amd.schedules, the 16 parameters
as tests/lr_schedule_oracle.py lays them out from the header text).  decay_steps D = 5, warm-up w = 3 / 4 / 7, restart
periods 5, 10, 20 (t_mul 2) and 5 (t_mul 1), boundaries 3, 5, 9 and 2 .. 14: steps 0 .. 40 cross every one of them."""
import lr_schedule_oracle as O
from masters_thesis_amd.schedules import (CosineDecay, CosineDecayRestarts, ExponentialDecay, InverseTimeDecay,
                                          PiecewiseConstantDecay, PolynomialDecay, Warmup)

# (descriptor, the oracle's parameters): every kind, and Warmup around a float and three of the kinds
CASES = {
    "exponential": (lambda: ExponentialDecay(0.1, 5, 0.5), O.pack(O.EXPONENTIAL, [0.1, 5, 0.5, 0])),
    "exponential staircase": (lambda: ExponentialDecay(0.1, 5, 0.5, staircase=True), O.pack(O.EXPONENTIAL, [0.1, 5, 0.5, 1])),
    "inverse time": (lambda: InverseTimeDecay(0.3, 5, 0.7), O.pack(O.INVERSE_TIME, [0.3, 5, 0.7, 0])),
    "inverse time staircase": (lambda: InverseTimeDecay(0.3, 5, 0.7, True), O.pack(O.INVERSE_TIME, [0.3, 5, 0.7, 1])),
    "cosine": (lambda: CosineDecay(1e-3, 5, alpha=0.05), O.pack(O.COSINE, [1e-3, 5, 0.05])),
    "restarts": (lambda: CosineDecayRestarts(1e-3, 5, t_mul=2.0, m_mul=0.9, alpha=0.01), O.pack(O.RESTARTS, [1e-3, 5, 2.0, 0.9, 0.01])),
    "restarts t_mul 1": (lambda: CosineDecayRestarts(1e-3, 5, t_mul=1.0, m_mul=0.9), O.pack(O.RESTARTS, [1e-3, 5, 1.0, 0.9, 0.0])),
    "polynomial": (lambda: PolynomialDecay(1e-2, 5, 1e-4, power=2.0), O.pack(O.POLYNOMIAL, [1e-2, 5, 1e-4, 2.0, 0])),
    "polynomial cycle": (lambda: PolynomialDecay(1e-2, 5, 1e-4, power=0.5, cycle=True), O.pack(O.POLYNOMIAL, [1e-2, 5, 1e-4, 0.5, 1])),
    "piecewise": (lambda: PiecewiseConstantDecay([3, 5, 9], [1.0, 0.5, 0.25, 0.1]), O.pack_piecewise([3, 5, 9], [1.0, 0.5, 0.25, 0.1])),
    "piecewise 7": (lambda: PiecewiseConstantDecay(list(range(2, 16, 2)), [2.0 ** -i for i in range(8)]),
                    O.pack_piecewise(list(range(2, 16, 2)), [2.0 ** -i for i in range(8)])),
    "warmup float": (lambda: Warmup(0.3, 7, warmup_start=0.01), O.pack(O.CONSTANT, [0.3], w=7, start=0.01)),
    "warmup cosine": (lambda: Warmup(CosineDecay(1e-3, 5, alpha=0.05), 3), O.pack(O.COSINE, [1e-3, 5, 0.05], w=3)),
    "warmup inverse time": (lambda: Warmup(InverseTimeDecay(0.3, 5, 0.7), 3, 0.05), O.pack(O.INVERSE_TIME, [0.3, 5, 0.7, 0], w=3, start=0.05)),
    "warmup piecewise": (lambda: Warmup(PiecewiseConstantDecay([3, 5], [1.0, 0.5, 0.25]), 4, 0.125),
                         O.pack_piecewise([3, 5], [1.0, 0.5, 0.25], w=4, start=0.125)),
}
