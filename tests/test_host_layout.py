"""The shared weight layout (model_base.pack / unpack and ModelBase.set_weight / get_weight / get_gradient /
get_optimizer_slot) on every model class, on CPU through the mock backend: exact round trips in the keras layout, the
zero padding on the device, and the refusal of a shape pair that is none of the four layouts."""
import numpy as np
import pytest

import masters_thesis_amd.ops as ops
from masters_thesis_amd import think_and_tell as TT, show_and_tell as SAT, think_and_tell_att as ATT
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import pack, unpack, interleave_gates, deinterleave_gates
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from helpers import tiny_groups
from mock_backend import MockBackend

N, U, E = 23, 16, 12


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    ops.set_backend(MockBackend())
    yield
    ops.set_backend(old)


def _lc(V, **kw):
    g = (tiny_groups(N, 4, np.random.default_rng(3)), [16] * 4)
    return LcNIC(g, U, 512, E, 6, V, 5, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11, **kw)


def _tt(mod, V):
    m = mod.CaptionGenerator(mod.Encoder(E), mod.Decoder(E, U, V), None, 5, device="cpu", seed=11)
    m._create(N)          # these models lay their arena out at the first batch, when the input width is known
    return m


MODELS = {
    "nic": lambda V: NIC(N, U, E, V, 5, 0.0, 0.0, 0.0, 0.01, 3e-5, 1e-5, device="cpu", seed=11),
    "lc_nic depth 1": lambda V: _lc(V, depth=1),
    "lc_nic layer-norm LSTM, 2 subjects": lambda V: _lc(V, use_layer_norm=True, n_subjects=2),
    "fc_nic": lambda V: NICfc(N, U, E, E, V, 5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.01, 3e-5, 1e-5, device="cpu", seed=11),
    "think_and_tell": lambda V: _tt(TT, V),
    "show_and_tell": lambda V: _tt(SAT, V),
    "think_and_tell_att": lambda V: _tt(ATT, V),
}
CASES = [(k, V) for k in MODELS for V in (12, 13)]


def _filled(kind, V):
    """the model with every variable of keras_shapes set to its own random non-zero values, and those values"""
    model = MODELS[kind](V)
    rng = np.random.default_rng(5)
    w = {n: rng.uniform(1.0, 2.0, s).astype(np.float32) for n, s in model.keras_shapes.items()}
    for n, v in w.items():
        model.set_weight(n, v)
    return model, w


@pytest.mark.parametrize("kind,V", CASES)
def test_set_then_get_is_exact_for_every_variable(kind, V):
    model, w = _filled(kind, V)
    assert any("moving_" in n for n in w) == (len(model.state_tensors()) > 0)
    for n, v in w.items():
        got = model.get_weight(n)
        assert got.shape == tuple(model.keras_shapes[n]) and got.dtype == np.float32, n
        assert np.array_equal(got, v), n
    for n, v in model.get_weights_dict().items():
        assert np.array_equal(v, w[n]), n
    # the moving statistics live outside the arena, in the order dp.py broadcasts them: the means, then the variances
    stats = [n for n in w if n.endswith("/moving_mean")] + [n for n in w if n.endswith("/moving_variance")]
    assert len(stats) == len(model.state_tensors())
    for n, t in zip(stats, model.state_tensors()):
        assert n not in model.arena.entries and np.array_equal(t.numpy(), w[n]), n


@pytest.mark.parametrize("kind,V", CASES)
def test_device_layout_gates_interleaved_padding_zero(kind, V):
    model, w = _filled(kind, V)
    ldV = (V + 3) // 4 * 4
    seen = set()
    for n, e in model.arena.entries.items():
        dev, ks = model.arena.p(n).numpy(), tuple(model.keras_shapes[n])
        if dev.shape == ks:
            assert np.array_equal(dev, w[n]), n
        elif dev.ndim == len(ks) + 1:                         # gate blocks [.., gU] -> [.., U, 4]
            g = 3 if n.startswith("gru/") else 4
            assert dev.shape == ks[:-1] + (U, 4) and ks[-1] == g * U, n
            for k in range(g):
                assert np.array_equal(dev[..., k], w[n][..., k * U:(k + 1) * U]), (n, k)
            if g == 3:
                assert np.all(dev[..., 3] == 0.0), n          # the GRU has no fourth gate: its slot stays zero
            seen.add(f"gates{g}")
        elif dev.ndim == len(ks) and dev.shape[-1] != ks[-1]:  # the vocabulary axis, V -> ldV
            assert ks[-1] == V and dev.shape == ks[:-1] + (ldV,), n
            assert np.array_equal(dev[..., :V], w[n]) and np.all(dev[..., V:] == 0.0), n
            seen.add("pad")
        else:                                                  # same elements, same order
            assert np.array_equal(dev.reshape(ks), w[n]), n
    assert ("pad" in seen) == (V % 4 != 0)
    assert ("gates3" if kind == "think_and_tell_att" else "gates4") in seen


@pytest.mark.parametrize("kind,V", CASES)
def test_gradient_and_optimizer_slots_come_back_in_keras_shape(kind, V):
    model, w = _filled(kind, V)
    model.compile(Adam(1e-3))
    model._init_optimizer_state()
    a = model.arena
    a.grad.copy_(a.theta)
    model.opt_m.copy_(a.theta * 2)
    model.opt_v.copy_(a.theta * 4)
    for n in model.trainable_names():
        for got, want in ((model.get_gradient(n), w[n]), (model.get_optimizer_slot(n, "m"), w[n] * 2),
                          (model.get_optimizer_slot(n, "v"), w[n] * 4)):
            assert got.shape == tuple(model.keras_shapes[n]), n
            assert np.array_equal(got, want), n


def test_pack_unpack_the_four_layouts():
    rng = np.random.default_rng(1)
    for ks, ds in (((5, 7), (5, 7)), ((3, 64), (3, 16, 4)), ((64,), (16, 4)), ((2, 48), (2, 16, 4)), ((5, 13), (5, 16)),
                   ((13,), (16,)), ((6, 1), (6,))):
        w = rng.standard_normal(ks).astype(np.float32)
        dev = pack(w, ds, "w")
        assert dev.shape == ds and dev.dtype == np.float32 and dev.flags["C_CONTIGUOUS"]
        assert dev.sum(dtype=np.float64) == pytest.approx(w.sum(dtype=np.float64), abs=1e-4)     # nothing but zeros added
        back = unpack(dev, ks, "w")
        assert np.array_equal(back, w) and not np.shares_memory(back, dev)
    w = rng.standard_normal((3, 64)).astype(np.float32)
    assert np.array_equal(pack(w, (3, 16, 4)), interleave_gates(w, 16))
    assert np.array_equal(deinterleave_gates(interleave_gates(w, 16)), w)
    w3 = rng.standard_normal((2, 48)).astype(np.float32)
    assert np.array_equal(pack(w3, (2, 16, 4)), ATT.interleave3(w3, 16))
    assert np.array_equal(ATT.deinterleave3(ATT.interleave3(w3, 16)), w3)


@pytest.mark.parametrize("ks,ds", [((3, 5), (4, 4)),            # another element count
                                   ((8, 32), (8, 16, 4)),       # two gate blocks
                                   ((8, 80), (8, 16, 4)),       # five
                                   ((4, 64), (3, 16, 4)),       # gate blocks under other leading axes
                                   ((16,), (13,)),              # a device axis shorter than the keras one
                                   ((4, 13), (5, 16))])         # padding under other leading axes
def test_a_shape_pair_outside_the_four_layouts_raises_and_names_the_variable(ks, ds):
    with pytest.raises(ValueError, match="some/kernel"):
        pack(np.zeros(ks, np.float32), ds, "some/kernel")
    with pytest.raises(ValueError, match="some/kernel"):
        unpack(np.zeros(ds, np.float32), ks, "some/kernel")


def test_set_weight_keeps_its_shape_check():
    model = MODELS["nic"](13)
    with pytest.raises(AssertionError):
        model.set_weight("lstm/bias", np.zeros((U, 4), np.float32))       # the device shape is not the keras shape
