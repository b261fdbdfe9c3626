"""Restatement of gradient accumulation: the accumulation launch (tnt_grad_accumulate_f32, definition in include/tnt_hip.h)
in numpy float32 (``reference``), a MockBackend with the op (``AccumMockBackend``), and the accumulating training step of
the float64 oracle models (``AccumStep``), built from their public forward, backward and AdamState.apply.

The launch is plain float32 adds in a fixed operand order, one thread per address, so ``reference`` is exact: a kernel
result is compared bit for bit, there is no error bound."""
import numpy as np

from mock_backend import MockBackend, flat
from oracle import models as M

OPEN, ADD, CLOSE = 0, 1, 2


def reference(acc, grad, phase, sq_acc=None, sq_slot=None, drop_step=None, guard=0):
    """One launch on float32 arrays ``acc`` and ``grad`` (n elements each), the float32 scalars ``sq_acc`` / ``sq_slot`` (None
    together: no scalar sum) and the integer ``drop_step`` (None: no counter).  Returns the new
    (acc, grad, sq_acc, sq_slot, drop_step); what a phase does not write comes back as it went in."""
    assert phase in (OPEN, ADD, CLOSE) and (sq_acc is None) == (sq_slot is None)
    acc, grad = np.array(acc, np.float32), np.array(grad, np.float32)
    f = lambda v: None if v is None else np.float32(v)
    sq_acc, sq_slot = f(sq_acc), f(sq_slot)
    if guard:
        return acc, grad, sq_acc, sq_slot, drop_step
    with np.errstate(invalid="ignore", over="ignore"):
        if phase == OPEN:
            acc = grad.copy()
            sq_acc = sq_slot
        elif phase == ADD:
            acc = acc + grad
            sq_acc = None if sq_acc is None else np.float32(sq_acc + sq_slot)
        else:
            grad = acc + grad
            sq_slot = None if sq_acc is None else np.float32(sq_acc + sq_slot)
    if phase != CLOSE and drop_step is not None:
        drop_step = (int(drop_step) + 1) & 0xFFFFFFFF
    return acc, grad, sq_acc, sq_slot, drop_step


class AccumMockBackend(MockBackend):
    """MockBackend plus tnt_grad_accumulate_f32 from the header text; ``acc_calls`` logs each call's phase, size, guard and
    the scalars it saw"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.acc_calls = []

    def grad_accumulate(self, acc, grad, n, phase, sq_acc=None, sq_slot=None, drop_step=None, guard=None):
        assert n >= 0 and phase in (OPEN, ADD, CLOSE)
        assert acc.data_ptr() % 16 == 0 and grad.data_ptr() % 16 == 0
        assert acc.data_ptr() + 4 * n <= grad.data_ptr() or grad.data_ptr() + 4 * n <= acc.data_ptr()
        assert (sq_acc is None) == (sq_slot is None) and (sq_acc is None or sq_acc.data_ptr() != sq_slot.data_ptr())
        g = int(guard[0]) if guard is not None else 0
        qa, qs = (None, None) if sq_acc is None else (flat(sq_acc)[0], flat(sq_slot)[0])
        ds = None if drop_step is None else int(flat(drop_step)[0])
        self.acc_calls.append(dict(n=n, phase=phase, guard=g, sq_acc=qa, sq_slot=qs, drop_step=ds))
        a, gr, qa, qs, ds = reference(flat(acc)[:n], flat(grad)[:n], phase, qa, qs, ds, guard=g)
        if g:
            return
        if phase == CLOSE:
            flat(grad)[:n] = gr
        else:
            flat(acc)[:n] = a
        if sq_acc is not None:
            flat(sq_acc)[0], flat(sq_slot)[0] = qa, qs
        if drop_step is not None:
            flat(drop_step)[0] = ds


def forward_backward(orc, data, y_ids, drop):
    """One micro-batch through an oracle model (oracle.models.NICDense / LcNIC): its metrics, its gradients (each with its L2
    term), its Embedding IndexedSlices norm; BatchNorm's moving statistics advance."""
    out, cache = orc.forward(data, training=True, drop=drop)
    if isinstance(out, tuple):
        probs, attn = out
        ce, acc, al = orc.metrics(probs, attn, y_ids)
        met = {"loss": ce, "L2": orc.l2_loss(), "accuracy": acc, "attention": al}
    else:
        probs = out
        ce, acc = orc.metrics(probs, y_ids)
        met = {"loss": ce, "L2": orc.l2_loss(), "accuracy": acc}
    grads, sparse = orc.backward(probs, cache, y_ids)
    if "enc" in cache:
        enc = cache["enc"]
        orc.p["input_bn/moving_mean"], orc.p["input_bn/moving_variance"] = enc["new_mm"], enc["new_mv"]
        for i, dc in enumerate(enc.get("deep", [])):
            orc.p[f"input_bn/deep{i}/moving_mean"], orc.p[f"input_bn/deep{i}/moving_variance"] = dc["new_mm"], dc["new_mv"]
    else:
        orc.p["batch_norm/moving_mean"], orc.p["batch_norm/moving_variance"] = cache["new_mm"], cache["new_mv"]
    return met, grads, sparse


class AccumStep:
    """The accumulating training step in float64: ``micro_step(data, y_ids)`` is one train_step of a model compiled with
    gradient_accumulation_steps=k.  The k-th of a window applies ONE update: the gradients are the mean of the k
    micro-batch gradients, the Embedding's sparse norm is sqrt(sum_j norm_j^2) / k (every micro-batch's rows carry 1 / k),
    micro-step i of the run draws its masks from DropCtx(seed, step=i), BatchNorm's moving statistics advance per
    micro-batch.  ``last_grads`` / ``last_sparse``: what the last update consumed."""

    def __init__(self, orc, opt, k, seed):
        self.orc, self.opt, self.k, self.seed = orc, opt, int(k), seed
        self.i = 0              # micro-steps run
        self.window = []        # (grads, sparse) of the open window
        self.last_grads = self.last_sparse = None

    def micro_step(self, data, y_ids):
        met, grads, sparse = forward_backward(self.orc, data, y_ids, M.DropCtx(seed=self.seed, step=self.i, training=True))
        self.i += 1
        self.window.append((grads, sparse))
        if len(self.window) == self.k:
            k = self.k
            mean = {n: (None if g is None else sum(w[0][n] for w in self.window) / k) for n, g in grads.items()}
            norms = {n: np.sqrt(sum(w[1][n] ** 2 for w in self.window)) / k for n in sparse}
            self.opt.apply(self.orc.p, mean, norms)
            self.last_grads, self.last_sparse = mean, norms
            self.window = []
        return met
