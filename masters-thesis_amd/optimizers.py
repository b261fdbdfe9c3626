"""Keras-style optimizer / loss descriptor objects.

They carry hyper-parameters only; the arithmetic is the multi-tensor HIP kernels in
csrc/optim.hip driven by the model (reference construction: AttemptFour/main.py:97-110).
"""


class Adam:
    """tf.keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon, clipnorm) -- main.py:97.
    ``clipnorm`` is per variable; None disables it (the TF<=2.3 behaviour of a
    custom tape.gradient -> apply_gradients step)."""

    kind = "adam"

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, **kw):
        self.lr = float(kw.pop("lr", learning_rate))
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.iterations = 0

    @property
    def learning_rate(self):
        return self.lr

    @learning_rate.setter
    def learning_rate(self, v):
        self.lr = float(v)


class SGD:
    """tf.keras.optimizers.SGD(learning_rate, momentum, nesterov=False) -- main.py:100-102."""

    kind = "sgd"

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, **kw):
        if nesterov:
            raise NotImplementedError("nesterov momentum is not used by the reference path")
        self.lr = float(kw.pop("lr", learning_rate))
        self.momentum = float(momentum)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.iterations = 0

    @property
    def learning_rate(self):
        return self.lr

    @learning_rate.setter
    def learning_rate(self, v):
        self.lr = float(v)


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
