"""Keras-style optimizer / loss descriptor objects.

They carry hyper-parameters only; the arithmetic is the multi-tensor HIP kernels in
csrc/optim.hip driven by the model (reference construction: AttemptFour/main.py:97-110).
"""
from . import schedules
from .schedules import LearningRateSchedule


class _LearningRate:
    """``lr`` / ``learning_rate`` of a descriptor: a float, or a schedules.LearningRateSchedule (main.py:81-84), which
    ``learning_rate`` and ``lr`` then return as the object.  A model compiled with a schedule evaluates it on the device
    per update (ModelBase._lr_schedule_launch); assigning a float replaces the schedule."""

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, v):
        self._lr = v if isinstance(v, LearningRateSchedule) else float(v)

    learning_rate = lr


def optimizer_schedule(optimizer):
    """the LearningRateSchedule a descriptor holds as its learning rate, or None for a float"""
    lr = getattr(optimizer, "lr", None)
    return lr if isinstance(lr, LearningRateSchedule) else None


class Adam(_LearningRate):
    """tf.keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon, clipnorm) -- main.py:97.
    ``learning_rate``: a float or an ``optimizers.schedules`` object.
    ``clipnorm`` is per variable; None disables it (the TF<=2.3 behaviour of a
    custom tape.gradient -> apply_gradients step)."""

    kind = "adam"

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, **kw):
        self.lr = kw.pop("lr", learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.iterations = 0


class SGD(_LearningRate):
    """tf.keras.optimizers.SGD(learning_rate, momentum, nesterov=False) -- main.py:100-102.  ``learning_rate``: a float
    or an ``optimizers.schedules`` object."""

    kind = "sgd"

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, **kw):
        if nesterov:
            raise NotImplementedError("nesterov momentum is not used by the reference path")
        self.lr = kw.pop("lr", learning_rate)
        self.momentum = float(momentum)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.iterations = 0


class Average:
    """What an averaging wrapper hands ``ModelBase.compile`` (its ``average`` attribute): the arguments of the averaging
    launch, tnt_weight_average_f32 (definition in include/tnt_hip.h).  kind "ema" / "swa"; momentum: the EMA decay;
    dynamic: tfa's dynamic_decay; start_step: the update that seeds the average (at least the first); every: one sample
    per ``every`` updates behind the seed."""

    KINDS = ("ema", "swa")
    __slots__ = ("kind", "momentum", "dynamic", "start_step", "every")

    def __init__(self, kind, momentum, dynamic, start_step, every):
        if kind not in self.KINDS:
            raise ValueError(f"average kind must be one of {self.KINDS}, got {kind!r}")
        self.kind, self.momentum, self.dynamic = kind, check_average_decay(momentum), bool(dynamic)
        self.start_step = _check_count("start_step", start_step, 0)
        self.every = _check_count("every", every, 1)

    @property
    def kind_id(self):
        return self.KINDS.index(self.kind)

    def key(self):
        return (self.kind, self.momentum, self.dynamic, self.start_step, self.every)

    def __eq__(self, other):
        return isinstance(other, Average) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return (f"Average(kind={self.kind!r}, momentum={self.momentum}, dynamic={self.dynamic}, start_step={self.start_step}, "
                f"every={self.every})")


def _delegate(name):
    def get(self):
        return getattr(self._optimizer, name)

    def put(self, v):
        setattr(self._optimizer, name, v)
    return property(get, put)


class _AveragedOptimizer:
    """An Adam / SGD descriptor with a weight average beside it.  The update is the wrapped optimizer's, unchanged: the
    hyper-parameters are read from and written to the wrapped object (so LearningRateScheduler keeps working), and
    ``average`` tells ``ModelBase.compile`` to keep one more slot, ``opt_avg``, that one tnt_weight_average_f32 launch
    advances behind every update (ModelBase._average_update)."""

    kind = _delegate("kind")
    lr = _delegate("lr")
    learning_rate = _delegate("learning_rate")
    beta_1 = _delegate("beta_1")
    beta_2 = _delegate("beta_2")
    epsilon = _delegate("epsilon")
    clipnorm = _delegate("clipnorm")
    momentum = _delegate("momentum")
    iterations = _delegate("iterations")

    def __init__(self, optimizer, average):
        if getattr(optimizer, "average", None) is not None:
            raise ValueError(f"{type(self).__name__} wraps an Adam or SGD descriptor, not another averaging wrapper")
        if getattr(optimizer, "kind", None) not in ("adam", "sgd"):
            raise ValueError(f"{type(self).__name__} wraps an Adam or SGD descriptor, got {optimizer!r}")
        self._optimizer, self.average = optimizer, average


class MovingAverage(_AveragedOptimizer):
    """tfa.optimizers.MovingAverage(optimizer, average_decay, num_updates, start_step, dynamic_decay): an exponential
    moving average of the trained parameters, avg += (1 - d) (theta - avg) behind every update, d = average_decay; with
    ``dynamic_decay`` d = min(average_decay, (1 + k) / (10 + k)) for the k-th sample.  The average is seeded with the
    parameters after update max(start_step, 1) -- it never holds the initial weights -- and ``every`` (this library's
    own) takes one sample per ``every`` updates.  ``num_updates`` is refused: the dynamic rule counts its own samples.
    Use: model.compile(MovingAverage(Adam(...))), then model.averaged_weights() / swap_weights() /
    assign_average_vars() / save_weights(path, averaged=True) / callbacks.AverageModelCheckpoint."""

    def __init__(self, optimizer, average_decay=0.99, num_updates=None, start_step=0, dynamic_decay=False, every=1):
        if num_updates is not None:
            raise NotImplementedError("num_updates is not implemented: dynamic_decay counts the samples the average has taken")
        super().__init__(optimizer, Average("ema", average_decay, dynamic_decay, start_step, every))


class SWA(_AveragedOptimizer):
    """tfa.optimizers.SWA(optimizer, start_averaging, average_period): stochastic weight averaging (Izmailov et al. 2018),
    the equal-weight mean of the parameters after update max(start_averaging, 1) and after every ``average_period``-th
    update behind it.  Use as MovingAverage."""

    def __init__(self, optimizer, start_averaging=0, average_period=10):
        super().__init__(optimizer, Average("swa", 0.0, False, start_averaging, average_period))


def check_average_decay(d):
    """the value as a float; ValueError unless 0 <= d < 1 (NaN included)"""
    try:
        v = float(d)
    except (TypeError, ValueError):
        raise ValueError(f"average_decay must be a number in [0, 1), got {d!r}") from None
    if isinstance(d, bool) or not 0.0 <= v < 1.0:
        raise ValueError(f"average_decay must be in [0, 1), got {d!r}")
    return v


def _check_count(name, v, lo):
    """the value as an int; ValueError unless it is an integer >= lo (bool excluded)"""
    import numbers
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or v >= 2 ** 31:
        raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    return int(v)


def optimizer_average(optimizer):
    """the Average of a compile() optimizer argument: None for a plain descriptor"""
    avg = getattr(optimizer, "average", None)
    if avg is not None and not isinstance(avg, Average):
        raise ValueError(f"optimizer.average must be an optimizers.Average or None, got {avg!r}")
    return avg


class CategoricalCrossentropy:
    """tf.keras.losses.CategoricalCrossentropy(from_logits=False, reduction='none') -- main.py:107-110.
    Only this configuration is implemented by the fused softmax+CE kernel.  ``label_smoothing`` (keras: the target
    becomes (1 - eps) * onehot + eps / V) is read by ``ModelBase.compile``; with eps > 0 the training and the
    evaluation step launch tnt_softmax_cce_smooth_f32 instead of tnt_softmax_cce_f32.

    ``unlikelihood`` (this library's own; Welleck et al. 2020, token level): with alpha > 0 every position also lowers
    the probability of the words that occurred earlier in its own ground-truth caption,
    loss = ce - alpha * sum_{c in prefix} log(1 - p_c), from one tnt_softmax_cce_unlikely_f32 launch in place of
    tnt_softmax_cce_f32 (definition in include/tnt_hip.h).  The ``loss`` metric of train_step and test_step is then the
    mean of ce + alpha * ul, with no metric key of its own; the plain likelihood of a caption is what
    ``evaluate.caption_perplexity`` reports.  Not together with ``label_smoothing``."""

    def __init__(self, from_logits=False, reduction="none", label_smoothing=0.0, unlikelihood=0.0):
        if from_logits:
            raise NotImplementedError("the reference path uses from_logits=False")
        self.label_smoothing = check_label_smoothing(label_smoothing)
        self.unlikelihood = check_unlikelihood(unlikelihood)
        self.from_logits, self.reduction = from_logits, reduction


def check_label_smoothing(eps):
    """the value as a float; ValueError unless 0 <= eps < 1 (NaN included)"""
    try:
        v = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {eps!r}") from None
    if not 0.0 <= v < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {eps!r}")
    return v


def loss_label_smoothing(loss):
    """label_smoothing of a compile() loss argument: None, or an object without the attribute, means 0"""
    return check_label_smoothing(getattr(loss, "label_smoothing", 0.0) if loss is not None else 0.0)


def check_unlikelihood(alpha):
    """the value as a float; ValueError unless it is finite and >= 0"""
    try:
        v = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"unlikelihood must be a finite number >= 0, got {alpha!r}") from None
    if not 0.0 <= v < float("inf"):
        raise ValueError(f"unlikelihood must be finite and >= 0, got {alpha!r}")
    return v


def loss_unlikelihood(loss):
    """unlikelihood of a compile() loss argument: None, or an object without the attribute, means 0"""
    return check_unlikelihood(getattr(loss, "unlikelihood", 0.0) if loss is not None else 0.0)
