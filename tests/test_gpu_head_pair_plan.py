"""The vocabulary head's gradient pair planned for the rows that exist (ModelBase ``g3_live_map``): a small nic.NIC whose
input gradient dX = dlogits W^T is a split product over three row tiles (T * B = 144 rows, V = 301: ten 32-deep stages, the
plan forced to the 64 x 128 tile with split 2 -- at this size the cost model would not split) trains on batches whose live row
counts differ:

    short    every caption <start> <end>: 48 rows, one row tile -- the warm-up step, which sets the expected count to 49
    medium   half the captions one token longer ... 84 rows, two row tiles
    full     every caption at full length: 144 rows, all three tiles, well above what the launch was planned for
    short    again, after the recorded step has run the other counts

The switch on against off at the tolerances of tests/test_gpu_compact_head.py (the two differ in the summation order of dX
only); the recorded launch plan against the hipGraph replay bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_compact_head import dev

pytestmark = pytest.mark.gpu

B, T, U, V, NV = 24, 6, 512, 301, 256
DX = (T * B, U, V, False, True, 1)          # the key of the input gradient in g3_force
DW = (U, V, T * B, True, False, 1)


def captions(rng, lengths):
    """<start>, `length` tokens, <end>, zero pad (length <= T - 2)"""
    cap = np.zeros((B, T), np.int32)
    for b, n in enumerate(lengths):
        cap[b, 0] = 1
        cap[b, 1:1 + n] = rng.integers(3, V, size=n)
        cap[b, 1 + n] = 2
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    return cap, tgt


def batches():
    rng = np.random.default_rng(17)
    x, z = dev(rng.standard_normal((B, NV)).astype(np.float32)), dev(np.zeros((B, U), np.float32))
    out = {}
    for name, lengths in (("short", [0] * B), ("medium", [0] * 12 + [3] * 12), ("full", [T - 2] * B)):
        cap, tgt = captions(rng, lengths)
        out[name] = ((x, dev(cap, torch.int32), z, z.clone()), dev(tgt, torch.int32))
    return [out[k] for k in ("short", "short", "medium", "full", "short")], (48, 48, 84, 144, 48)


def make_model(live_map, plan_step=True):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    m = NIC(NV, U, U, V, T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, seed=42)
    m.g3_live_map = live_map
    m.g3_force = {DX: (5, 2), DW: (5, 1)}
    m.plan_step = plan_step
    m.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def run(m, seq, lives):
    hist = []
    for batch, rows in zip(seq, lives):
        hist.append(m.train_step(batch).as_floats())
        assert int(m.head_live.item()) == rows
    m.check_device_errors()
    return hist


def head_pair_modes(m):
    """(splitk, live_mode) of the NT product of every pair descriptor the model built"""
    return sorted((d2.splitk, d2.live_mode) for _, d2 in m._g3_descs.values() if d2.transB and d2.live)


def test_training_with_the_live_map_against_without_and_plan_against_graph():
    from masters_thesis_amd.ops import LIVE_ROWS_M, LIVE_ROWS_M_MAP
    seq, lives = batches()
    a, b = make_model(True), make_model(False)
    ha, hb = run(a, seq, lives), run(b, seq, lives)
    if not a._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    key = ("train", B, T, "compact")
    assert key in a._graphs and key in b._graphs
    assert a._head_plan_rows(T * B) == 49                      # planned for the warm-up count: 144 rows is well above it
    assert set(head_pair_modes(a)) == {(2, LIVE_ROWS_M_MAP)} and set(head_pair_modes(b)) == {(2, LIVE_ROWS_M)}
    for x, y in zip(ha, hb):
        print(x, y)
        assert abs(x["loss"] - y["loss"]) <= 2e-5 * abs(y["loss"]), (x, y)
        assert abs(x["accuracy"] - y["accuracy"]) <= 2.0 / (B * T)
    wa, wb = a.get_weights_dict(), b.get_weights_dict()
    for k in wa:
        d = np.abs(wa[k] - wb[k])
        print(k, d.max(), (d > 3e-5).mean())
        assert (d > 3e-5).mean() <= 5e-3, (k, d.max(), (d > 3e-5).mean())
    # the recorded launch plan (a) against the hipGraph replay: the same bits, whatever the live word held at each replay
    g = make_model(True, plan_step=False)
    hg = run(g, seq, lives)
    assert isinstance(a._graphs[key], tuple) and set(head_pair_modes(g)) == {(2, LIVE_ROWS_M_MAP)}
    assert ha == hg
    wg = g.get_weights_dict()
    assert all(np.array_equal(wa[k], wg[k]) for k in wa)
