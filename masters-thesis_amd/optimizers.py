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


def check_weight_decay(wd):
    """None, or the value as a float; ValueError unless it is a finite number >= 0 (bool, str and NaN refused)"""
    import numbers
    if wd is None:
        return None
    if isinstance(wd, bool) or not isinstance(wd, numbers.Real):
        raise ValueError(f"weight_decay must be None or a finite number >= 0, got {wd!r}")
    v = float(wd)
    if not 0.0 <= v < float("inf"):
        raise ValueError(f"weight_decay must be finite and >= 0, got {wd!r}")
    return v


class _WeightDecay:
    """``weight_decay`` of a descriptor (keras >= 2.11: the argument of every optimizer, and AdamW): decoupled weight decay,
    every update also shrinks a decayed variable by lr * weight_decay * theta outside the gradient path (definition:
    tnt_adamw_ring_f32 in include/tnt_hip.h), with lr the step's learning rate, a schedule's value included.  None or 0:
    no decay, and the update launches are the plain ones.

    Keras's rule: EVERY variable the optimizer updates is decayed unless it is excluded.  To leave the biases and the
    normalisation parameters alone, as is usual, call
    ``optimizer.exclude_from_weight_decay(var_names=["bias", "gamma", "beta"])`` before the model builds its optimizer
    state (compile of a built model, or the first step).  The model's variable names: ``model.trainable_names()``.

    Single device only, like weight averaging: dp.attach / a model with a grad_sync, train_step_sam and enable_agc()
    refuse a decaying optimizer with NotImplementedError."""
    _wd_built = False       # a model has built its optimizer state from this descriptor (ModelBase._init_optimizer_state)

    @property
    def weight_decay(self):
        return self._weight_decay

    @weight_decay.setter
    def weight_decay(self, v):
        self._weight_decay = check_weight_decay(v)

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        """keras's Optimizer.exclude_from_weight_decay: ``var_list`` holds exact variable names, ``var_names`` substrings
        matched against the variable names; each call replaces the earlier exclusions.  Raises once a model has built its
        optimizer state from this descriptor, as keras does once the optimizer is built."""
        if self._wd_built:
            raise ValueError("exclude_from_weight_decay() must be called before the model builds its optimizer state")
        for what, v in (("var_list", var_list), ("var_names", var_names)):
            if v is not None and (isinstance(v, str) or not all(isinstance(n, str) for n in v)):
                raise ValueError(f"{what} must be a list of variable names, got {v!r}")
        self._wd_exclude_exact = frozenset(var_list or ())
        self._wd_exclude_sub = tuple(var_names or ())


def weight_decay_table(optimizer, names):
    """one decay per variable name, in order: the descriptor's ``weight_decay`` (a wrapper's: the wrapped descriptor's), 0
    for a variable that exclude_from_weight_decay names; None when nothing decays"""
    inner = getattr(optimizer, "_optimizer", optimizer)
    wd = check_weight_decay(getattr(inner, "weight_decay", None))
    if not wd:
        return None
    exact, sub = getattr(inner, "_wd_exclude_exact", frozenset()), getattr(inner, "_wd_exclude_sub", ())
    tab = [0.0 if (n in exact or any(s in n for s in sub)) else wd for n in names]
    return tab if any(tab) else None


def check_global_clipnorm(c):
    """None, or the value as a float; ValueError unless it is a finite number > 0 (bool, str and NaN refused)"""
    import numbers
    if c is None:
        return None
    if isinstance(c, bool) or not isinstance(c, numbers.Real):
        raise ValueError(f"global_clipnorm must be None or a finite number > 0, got {c!r}")
    v = float(c)
    if not 0.0 < v < float("inf"):
        raise ValueError(f"global_clipnorm must be finite and > 0, got {c!r}")
    return v


CLIPVALUE_REFUSAL = ("clipvalue is not implemented: keras clips an IndexedSlices gradient row by row before the rows are summed, "
                     "which the Embedding scatter here does not do.  Use clipnorm or global_clipnorm")


class _GlobalClipnorm:
    """``global_clipnorm`` of a descriptor (keras: the argument of every optimizer; tf.clip_by_global_norm): ONE norm over
    the gradients of all variables, every gradient scaled by c / max(norm, c), which keeps the direction of the whole
    update (definition: tnt_global_sqnorm_f32 in include/tnt_hip.h).  None: off.  Not together with ``clipnorm`` (keras's
    rule); ``clipvalue`` is refused.  ``model.global_grad_norm()`` reads the last step's norm.

    Single device only: dp.attach / a model with a grad_sync, train_step_sam and enable_agc() refuse it with
    NotImplementedError."""

    @property
    def global_clipnorm(self):
        return self._global_clipnorm

    @global_clipnorm.setter
    def global_clipnorm(self, v):
        v = check_global_clipnorm(v)
        if v is not None and getattr(self, "clipnorm", None) is not None:
            raise ValueError("clipnorm and global_clipnorm cannot both be set: at most one of them, as in keras")
        self._global_clipnorm = v

    def _init_clipping(self, clipnorm, global_clipnorm, kw):
        if kw.pop("clipvalue", None) is not None:
            raise NotImplementedError(CLIPVALUE_REFUSAL)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.global_clipnorm = global_clipnorm


def check_gradient_accumulation_steps(k):
    """None, or the value as an int >= 2; 1 is None (no accumulation).  ValueError unless it is None or an integer >= 1
    (bool, float and str refused)"""
    import numbers
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1 or k >= 2 ** 31:
        raise ValueError(f"gradient_accumulation_steps must be None or an int >= 1, got {k!r}")
    return int(k) if k > 1 else None


class _GradientAccumulation:
    """``gradient_accumulation_steps`` of a descriptor (keras 3: the argument of every optimizer): with k >= 2 a
    ``train_step`` is a micro-step, the gradients of k consecutive micro-steps are summed on the device
    (tnt_grad_accumulate_f32, definition in include/tnt_hip.h), each scaled by 1 / k, and the k-th applies ONE update from
    their mean -- an effective batch of k micro-batches at the memory and kernel shapes of one.  None or 1: off.
    ``ModelBase._train_step_accum`` holds the counting rules (what advances per update and what per micro-step).

    nic.NIC and lc_nic.NIC only, on one device; data parallel, enable_agc, train_step_sam, scheduled sampling,
    self-critical training, teacher_forcing=False, attention_coverage, normalise="weights" and n_subjects > 1 refuse it
    with NotImplementedError."""

    @property
    def gradient_accumulation_steps(self):
        return self._gradient_accumulation_steps

    @gradient_accumulation_steps.setter
    def gradient_accumulation_steps(self, v):
        self._gradient_accumulation_steps = check_gradient_accumulation_steps(v)


class Adam(_LearningRate, _WeightDecay, _GlobalClipnorm, _GradientAccumulation):
    """tf.keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon, clipnorm, weight_decay) -- main.py:97.
    ``learning_rate``: a float or an ``optimizers.schedules`` object.
    ``clipnorm`` is per variable; None disables it (the TF<=2.3 behaviour of a
    custom tape.gradient -> apply_gradients step).
    ``weight_decay``: decoupled weight decay, see ``_WeightDecay``; None or 0 is plain Adam.
    ``global_clipnorm``: one norm over all gradients in ``clipnorm``'s place, see ``_GlobalClipnorm``; ``clipvalue`` is
    refused.
    ``gradient_accumulation_steps``: one update per k micro-steps, see ``_GradientAccumulation``; None or 1 is off."""

    kind = "adam"

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, weight_decay=None,
                 global_clipnorm=None, gradient_accumulation_steps=None, **kw):
        self.lr = kw.pop("lr", learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self._init_clipping(clipnorm, global_clipnorm, kw)
        self.weight_decay = weight_decay
        self.gradient_accumulation_steps = gradient_accumulation_steps
        self.iterations = 0


class AdamW(Adam):
    """tf.keras.optimizers.AdamW(learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
    clipnorm): Adam with decoupled weight decay (Loshchilov & Hutter 2019), the rule of torch.optim.AdamW.  Every
    variable is decayed unless ``exclude_from_weight_decay`` names it (see ``_WeightDecay``)."""

    def __init__(self, learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None,
                 global_clipnorm=None, gradient_accumulation_steps=None, **kw):
        if weight_decay is None:
            raise ValueError("AdamW needs a weight_decay; Adam is the optimizer without one")
        super().__init__(learning_rate, beta_1, beta_2, epsilon, clipnorm, weight_decay, global_clipnorm,
                         gradient_accumulation_steps, **kw)


class SGD(_LearningRate, _WeightDecay, _GlobalClipnorm, _GradientAccumulation):
    """tf.keras.optimizers.SGD(learning_rate, momentum, nesterov=False, weight_decay) -- main.py:100-102.
    ``learning_rate``: a float or an ``optimizers.schedules`` object.  ``weight_decay``: decoupled weight decay, see
    ``_WeightDecay``; None or 0 is plain SGD.  ``global_clipnorm``: see ``_GlobalClipnorm``.
    ``gradient_accumulation_steps``: see ``_GradientAccumulation``."""

    kind = "sgd"

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, weight_decay=None,
                 global_clipnorm=None, gradient_accumulation_steps=None, **kw):
        if nesterov:
            raise NotImplementedError("nesterov momentum is not used by the reference path")
        self.lr = kw.pop("lr", learning_rate)
        self.momentum = float(momentum)
        self._init_clipping(clipnorm, global_clipnorm, kw)
        self.weight_decay = weight_decay
        self.gradient_accumulation_steps = gradient_accumulation_steps
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
    weight_decay = _delegate("weight_decay")
    global_clipnorm = _delegate("global_clipnorm")
    gradient_accumulation_steps = _delegate("gradient_accumulation_steps")

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        self._optimizer.exclude_from_weight_decay(var_list=var_list, var_names=var_names)

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
    ``evaluate.caption_perplexity`` reports.  Not together with ``label_smoothing``.

    ``class_weight`` (keras ``fit(class_weight=...)``: an array-like of one weight per class, or an ``{id: weight}`` dict in
    which a missing id weighs 1), ``focal_gamma`` (keras CategoricalFocalCrossentropy's gamma) and ``normalise``: position
    r with target y contributes w_y (1 - p_y)^gamma ce, and the ``loss`` metric is the sum of that over the positions
    divided by their count (``normalise="count"``, keras's rule) or by the sum of their weights (``"weights"``: with
    ``class_weight={0: 0}`` the mean over the non-padding tokens, and ``accuracy`` the accuracy over them).  One
    tnt_softmax_cce_weighted_f32 launch in place of tnt_softmax_cce_f32 (definition in include/tnt_hip.h), in training
    and evaluation.  Not together with ``label_smoothing`` or ``unlikelihood``; ``model.set_class_weight`` replaces the
    weights of a compiled model.

    ``distillation`` (an ``optimizers.Distillation``; Hinton et al. 2015): the training loss of every position becomes
    (1 - alpha) ce + alpha t^2 KL(softmax(teacher / t) || softmax(student / t)) against the logits of the frozen model
    given to ``model.set_teacher``, from one tnt_softmax_cce_distill_f32 launch in place of tnt_softmax_cce_f32
    (definition in include/tnt_hip.h); train_step also reports ``distill_kl``, the mean unscaled KL.  test_step stays
    the plain cross-entropy.  Not together with any of the settings above."""

    def __init__(self, from_logits=False, reduction="none", label_smoothing=0.0, unlikelihood=0.0, class_weight=None,
                 focal_gamma=0.0, normalise="count", distillation=None):
        if from_logits:
            raise NotImplementedError("the reference path uses from_logits=False")
        self.label_smoothing = check_label_smoothing(label_smoothing)
        self.unlikelihood = check_unlikelihood(unlikelihood)
        self.class_weight = class_weight if class_weight is None else check_class_weight(class_weight)
        self.focal_gamma = check_focal_gamma(focal_gamma)
        self.normalise = check_normalise(normalise)
        self.distillation = check_distillation(distillation)
        self.from_logits, self.reduction = from_logits, reduction


class CategoricalFocalCrossentropy(CategoricalCrossentropy):
    """tf.keras.losses.CategoricalFocalCrossentropy(alpha=0.25, gamma=2.0, from_logits=False): every class weighs ``alpha``
    and the focal exponent is ``gamma``, i.e. CategoricalCrossentropy(class_weight=<alpha everywhere>, focal_gamma=gamma).
    The uniform weight is expanded to the model's vocabulary by ``ModelBase.compile``."""

    def __init__(self, alpha=0.25, gamma=2.0, from_logits=False, reduction="none", normalise="count"):
        super().__init__(from_logits=from_logits, reduction=reduction, focal_gamma=gamma, normalise=normalise)
        try:
            a = float(alpha)
        except (TypeError, ValueError):
            raise ValueError(f"alpha must be a finite number >= 0, got {alpha!r}") from None
        if not 0.0 <= a < float("inf"):
            raise ValueError(f"alpha must be finite and >= 0, got {alpha!r}")
        self.alpha, self.gamma = a, self.focal_gamma
        self.class_weight = UniformClassWeight(a)


class UniformClassWeight:
    """the same weight for every class of a vocabulary whose size the loss object does not know"""

    def __init__(self, value):
        self.value = float(value)

    def __eq__(self, other):
        return isinstance(other, UniformClassWeight) and other.value == self.value

    def __hash__(self):
        return hash(("UniformClassWeight", self.value))


class Distillation:
    """Knowledge distillation (Hinton et al. 2015) as a setting of the compile loss:
    ``CategoricalCrossentropy(distillation=Distillation(alpha, temperature))``.  ``alpha`` in [0, 1] weighs the teacher's
    term against the ground truth's, ``temperature`` > 0 softens both distributions; alpha = 0 is the plain loss."""

    def __init__(self, alpha=0.5, temperature=2.0):
        self.alpha = _check_distill_number("alpha", alpha, lambda v: 0.0 <= v <= 1.0, "in [0, 1]")
        self.temperature = _check_distill_number("temperature", temperature, lambda v: 0.0 < v < float("inf"),
                                                 "finite and > 0")

    @property
    def neutral(self):
        return self.alpha == 0.0

    def __eq__(self, other):
        return isinstance(other, Distillation) and (other.alpha, other.temperature) == (self.alpha, self.temperature)

    def __hash__(self):
        return hash(("Distillation", self.alpha, self.temperature))

    def __repr__(self):
        return f"Distillation(alpha={self.alpha!r}, temperature={self.temperature!r})"


def _check_distill_number(name, v, ok, rule):
    """the value as a float; ValueError for a bool, a str, anything float() refuses, NaN, or a value outside the rule"""
    if isinstance(v, (bool, str)):
        raise ValueError(f"distillation {name} must be a number {rule}, got {v!r}")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"distillation {name} must be a number {rule}, got {v!r}") from None
    if not ok(f):                                  # NaN fails every compare
        raise ValueError(f"distillation {name} must be {rule}, got {v!r}")
    return f


def check_distillation(d):
    """None, a Distillation, or an ``{alpha: , temperature: }`` mapping (the config key) -> None or a Distillation"""
    if d is None or isinstance(d, Distillation):
        return d
    if isinstance(d, dict):
        extra = set(d) - {"alpha", "temperature"}
        if extra:
            raise ValueError(f"distillation takes the keys alpha and temperature, got {sorted(map(str, extra))}")
        return Distillation(**d)
    raise ValueError(f"distillation must be an optimizers.Distillation or None, got {d!r}")


def loss_distillation(loss):
    """distillation of a compile() loss argument: None, an object without the attribute, or a neutral descriptor
    (alpha == 0) means None"""
    d = check_distillation(getattr(loss, "distillation", None) if loss is not None else None)
    return None if d is None or d.neutral else d


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


def check_class_weight(w, vocab_size=None):
    """class weights as keras's fit(class_weight=) takes them, checked: an ``{id: weight}`` dict (returned as a dict with int
    keys and float values) or an array-like of one weight per class (returned as a float32 array); with ``vocab_size``
    either form becomes the float32 array of that length, ids a dict does not name weighing 1.  ValueError unless every
    weight is finite and >= 0 (NaN included), every id an integer in [0, vocab_size), and an array's length vocab_size."""
    import numbers
    import numpy as np
    if isinstance(w, UniformClassWeight):
        return w if vocab_size is None else np.full(int(vocab_size), w.value, np.float32)
    if isinstance(w, dict):
        out = {}
        for k, v in w.items():
            if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 0:
                raise ValueError(f"class_weight ids must be integers >= 0, got {k!r}")
            if vocab_size is not None and k >= vocab_size:
                raise ValueError(f"class_weight names id {k!r}, outside the vocabulary of {vocab_size} classes")
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"class_weight[{k!r}] must be a finite number >= 0, got {v!r}") from None
            if not 0.0 <= f < float("inf"):
                raise ValueError(f"class_weight[{k!r}] must be finite and >= 0, got {v!r}")
            out[int(k)] = f
        if vocab_size is None:
            return out
        arr = np.ones(int(vocab_size), np.float32)
        for k, f in out.items():
            arr[k] = f
        return arr
    try:
        arr = np.asarray(w, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"class_weight must be an array-like of weights or an {{id: weight}} dict, got {w!r}") from None
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError(f"class_weight must hold one weight per class, got an array of shape {arr.shape}")
    if not (np.isfinite(arr).all() and (arr >= 0).all()):
        raise ValueError("every class weight must be finite and >= 0")
    if vocab_size is not None and arr.size != vocab_size:
        raise ValueError(f"class_weight holds {arr.size} weights for a vocabulary of {vocab_size} classes")
    return arr.astype(np.float32)


def loss_class_weight(loss, vocab_size=None):
    """class_weight of a compile() loss argument: None, or an object without the attribute, means none"""
    w = getattr(loss, "class_weight", None) if loss is not None else None
    return None if w is None else check_class_weight(w, vocab_size)


def check_focal_gamma(gamma):
    """the value as a float; ValueError unless it is finite and >= 0 (NaN included)"""
    try:
        v = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"focal_gamma must be a finite number >= 0, got {gamma!r}") from None
    if isinstance(gamma, bool) or not 0.0 <= v < float("inf"):
        raise ValueError(f"focal_gamma must be finite and >= 0, got {gamma!r}")
    return v


def loss_focal_gamma(loss):
    """focal_gamma of a compile() loss argument: None, or an object without the attribute, means 0"""
    return check_focal_gamma(getattr(loss, "focal_gamma", 0.0) if loss is not None else 0.0)


NORMALISE_MODES = ("count", "weights")


def check_normalise(mode):
    """``"count"`` or ``"weights"``; ValueError otherwise"""
    if not isinstance(mode, str) or mode not in NORMALISE_MODES:
        raise ValueError(f'normalise must be "count" or "weights", got {mode!r}')
    return mode


def loss_normalise(loss):
    """normalise of a compile() loss argument: None, or an object without the attribute, means ``"count"``"""
    return check_normalise(getattr(loss, "normalise", "count") if loss is not None else "count")
