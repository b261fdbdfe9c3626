"""Restatement of the training-time input corruption (tnt_input_corrupt_f32, definition in include/tnt_hip.h), written from
the header text on top of oracle.philox.uniform24:

    scan part   row b fires when u(b, S_SCAN_DROP) < rate; a fired row of x becomes the null scan (None: zeros)
    word part   position (b, t), 1 <= t < T, cap[b][t] != 0, fires when u(b * T + t, S_WORD_DROP) < rate; a fired
                position becomes unk_id

with u the 24-bit uniform of the Philox stream (seed, site, step) and the rate compared in float32.  ``corrupt`` returns
the corrupted copies and the two masks; ``CorruptMockBackend`` is a MockBackend with the launch, which also logs it."""
import numpy as np

from mock_backend import MockBackend, flat, mat
from oracle.philox import uniform24

S_SCAN_DROP, S_WORD_DROP = 241, 242


def corrupt(x, cap, scan_rate, word_rate, null, unk_id, seed, step, site_scan=S_SCAN_DROP, site_word=S_WORD_DROP):
    """(x (B, N) float, cap (B, T) int, rates, null (N,) or None, unk_id, seed, step) -> (x', cap', row_mask (B,),
    word_mask (B, T)): copies; the masks hold what was replaced"""
    x, cap = np.array(x, copy=True), np.array(cap, copy=True)
    B, T = cap.shape
    row_mask, word_mask = np.zeros(B, bool), np.zeros((B, T), bool)
    if scan_rate > 0 and B > 0:
        row_mask = uniform24(B, int(seed), int(site_scan), int(step)) < np.float32(scan_rate)
        x[row_mask] = 0 if null is None else np.asarray(null, dtype=x.dtype)[None, :]
    if word_rate > 0 and B * T > 0:
        u = uniform24(B * T, int(seed), int(site_word), int(step)).reshape(B, T)
        word_mask = (u < np.float32(word_rate)) & (cap != 0)
        word_mask[:, 0] = False
        cap[word_mask] = unk_id
    return x, cap, row_mask, word_mask


def corrupt_batch(data, scan_rate, word_rate, null, unk_id, seed, step):
    """the restatement on a ((betas, cap, a0, c0), target) batch's inputs: (corrupted inputs, row_mask, word_mask)"""
    x, cap, a0, c0 = data
    x2, cap2, rows, words = corrupt(x, cap, scan_rate, word_rate, null, unk_id, seed, step)
    return (x2, cap2, a0, c0), rows, words


def pick_step(B, T, cap, scan_rate, word_rate, seed, steps=range(64)):
    """the first step word at which a row fires and one does not, and an eligible token fires and one does not"""
    for step in steps:
        _, _, rows, words = corrupt(np.zeros((B, 1), np.float32), cap, scan_rate, word_rate, None, 1, seed, step)
        elig = (cap != 0)
        elig[:, 0] = False
        ok_r = not (0 < scan_rate < 1 and B >= 2) or (rows.any() and not rows.all())
        ok_w = not (0 < word_rate < 1 and elig.sum() >= 2) or (words.any() and (elig & ~words).any())
        if ok_r and ok_w:
            return step
    raise AssertionError("no step word in range gives a mixed mask")


class CorruptMockBackend(MockBackend):
    """MockBackend plus tnt_input_corrupt_f32 from the header text; ``corrupt_calls`` logs the arguments of every call"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.corrupt_calls = []

    def input_corrupt(self, x, ldx, xT, ldt, cap, B, T, N, V, scan_rate, null_scan, word_rate, unk_id, seed, site_scan, site_word,
                      step_dev):
        assert 0 <= scan_rate <= 1 and 0 <= word_rate <= 1 and step_dev is not None and ldx >= N
        assert word_rate == 0 or (1 <= unk_id < V and cap is not None)
        assert scan_rate == 0 or x is not None
        assert xT is None or ldt >= B
        step = int(step_dev[0]) & 0xFFFFFFFF
        self.corrupt_calls.append(dict(scan_rate=float(scan_rate), word_rate=float(word_rate), unk_id=int(unk_id), step=step,
                                       null=None if null_scan is None else flat(null_scan)[:N].copy(), xT=xT is not None,
                                       sites=(int(site_scan), int(site_word)), seed=int(seed), B=B, T=T, N=N))
        xs = mat(x, B, N, ldx) if x is not None else np.zeros((B, N), np.float32)
        cs = flat(cap)[:B * T].reshape(B, T) if cap is not None else np.zeros((B, T), np.int32)
        null = None if null_scan is None else flat(null_scan)[:N]
        x2, cap2, rows, words = corrupt(xs, cs, scan_rate, word_rate, null, unk_id, seed, step, site_scan, site_word)
        if scan_rate > 0:
            xs[rows] = x2[rows]
            if xT is not None:
                mat(xT, N, B, ldt)[:, rows] = x2[rows].T
        if word_rate > 0:
            cs[words] = cap2[words]
