"""The step tail (model_base.StepTail: what a fused training step's launches leave to its update) is not inherited from a
step that failed between its loss and its update.  On the CPU through the mock backend, with every public backend call
logged by name, scalar arguments and tensor shapes."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from helpers import synth_batch, tiny_groups
from mock_backend import MockBackend

B, N, T, V, U, E = 5, 23, 6, 13, 16, 16


class Injected(RuntimeError):
    pass


def describe(v):
    if torch.is_tensor(v):
        return f"T{tuple(v.shape)}@{v.storage_offset()}"
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(describe(x) for x in v) + ")"
    return repr(v)


class RecordingBackend(MockBackend):
    """``calls`` logs every public call when it is made (a ``hasattr`` probe of the model's is no call); the next call of
    ``fail_on`` raises Injected in place of running"""

    def __init__(self):
        super().__init__()
        self.calls, self.fail_on = [], None

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v):
            return v
        me = lambda attr: object.__getattribute__(self, attr)

        def logged(*a, **k):
            if me("fail_on") == name:
                self.fail_on = None
                raise Injected(name)
            me("calls").append(name + "(" + ",".join([describe(x) for x in a] + [f"{n}={describe(x)}" for n, x in sorted(k.items())]) + ")")
            return v(*a, **k)
        return logged


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def make(kind, attn_units=5, dropout_attn=0):
    rng = np.random.default_rng(1)
    if kind == "dense":
        model = NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11)
    else:
        g = (tiny_groups(N, 4, rng), [16] * 4)
        model = LcNIC(g, U, 512, 12, attn_units, V, T, 0, 0, 0, dropout_attn, 0, 0.1, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11)
    for name in model.trainable_names():
        model.set_weight(name, 0.3 * rng.standard_normal(model.keras_shapes[name]))
    model.compile(Adam(1e-2, clipnorm=0.1))
    return model


def batch(seed):
    return synth_batch(B, N, T, V, U, np.random.default_rng(seed))


def trace(be, model, switch):
    """the calls of the next train_step and the next test_step, ``switch`` set on the model in front of them"""
    for k, v in switch.items():
        setattr(model, k, v)
    out = []
    for step, seed in ((model.train_step, 4), (model.test_step, 5)):
        del be.calls[:]
        step(batch(seed)).as_floats()
        out.append(list(be.calls))
    return out


@pytest.mark.parametrize("switch", [{}, {"sparse_emb_bwd": False}], ids=["same step", "sparse_emb_bwd off behind the failure"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_a_failed_fused_step_leaves_nothing_to_the_next_steps(kind, switch, mock_backend):
    """A fused step raises in its BatchNorm backward: behind the loss launch (whose totals are deferred), the attention
    metric's partials and the sparse Embedding backward's hand-off, in front of the update that would have taken them.
    The next train_step and the next test_step issue exactly the calls of a model whose step did not fail -- also where
    the next step runs the dense Embedding backward, which hands nothing over, so that an inherited hand-off would show in
    the finalize launch's arguments."""
    be = mock_backend
    fresh = make(kind)
    fresh.train_step(batch(3)).as_floats()
    want = trace(be, fresh, switch)
    assert any(c.startswith("step_finalize(") for c in want[0]) and any(c.startswith("sum2(") for c in want[1])
    assert any(c.startswith("embedding_bwd_sparse(") for c in want[0]) == (not switch)

    model = make(kind)
    model.train_step(batch(3)).as_floats()
    del be.calls[:]
    be.fail_on = "batchnorm_bwd"
    with pytest.raises(Injected):
        model.train_step(batch(6))
    names = [c.split("(")[0] for c in be.calls]
    # past the loss and the Embedding backward, short of the update
    assert "embedding_bwd_sparse" in names and not any(n in ("span_sqnorm", "step_finalize", "adam", "sum2") for n in names)
    tail = model._tail
    assert tail.deferring is False and tail.x0 is not None and tail.ids_src is not None     # what the failed step handed over
    assert trace(be, model, switch) == want
