"""Keras callback protocol objects used by AttemptFour/main.py:197-232 (SURVEY component 12).

``ModelBase.fit`` calls ``on_train_begin, on_epoch_begin, on_train_batch_begin,
on_train_batch_end(batch, logs), on_test_batch_end(batch, logs), on_epoch_end(epoch, logs),
on_train_end`` and sets ``.model``; any object with these methods works (the reference's
``Callbacks/EpochLoss.py`` LossHistory included, once its keras base class is swapped for
``Callback`` below).
"""
import csv
import os

from .optimizers import optimizer_schedule


class Callback:
    def __init__(self):
        self.model = None

    def set_model(self, model):
        self.model = model


class LossHistory(Callback):
    """Callbacks/EpochLoss.py:12-52: per-batch training/validation logs -> CSV at epoch end."""

    def __init__(self, file_name, out_dir=None):
        super().__init__()
        self.file_name, self.rows, self.epoch = file_name, [], 0

    def on_epoch_begin(self, epoch, logs=None):
        self.epoch = epoch

    def on_train_batch_end(self, batch, logs=None):
        self.rows.append(dict(epoch=self.epoch, batch=batch, phase="train", **(logs or {})))

    def on_test_batch_end(self, batch, logs=None):
        self.rows.append(dict(epoch=self.epoch, batch=batch, phase="val", **{f"val_{k}": v for k, v in (logs or {}).items()}))

    def on_epoch_end(self, epoch, logs=None):
        keys = []
        for r in self.rows:
            for k in r:
                if k not in keys:
                    keys.append(k)
        with open(self.file_name, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=keys)
            w.writeheader()
            w.writerows(self.rows)


class LearningRateScheduler(Callback):
    """tf.keras.callbacks.LearningRateScheduler(schedule) -- main.py:86-92,218-219."""

    def __init__(self, schedule, verbose=0):
        super().__init__()
        self.schedule = schedule

    def set_model(self, model):
        super().set_model(model)
        _refuse_schedule(self)

    def on_train_begin(self, logs=None):
        _refuse_schedule(self)

    def on_epoch_begin(self, epoch, logs=None):
        self.model.optimizer.lr = float(self.schedule(epoch))


def _refuse_schedule(cb):
    """keras: a callback that sets the learning rate refuses an optimizer whose learning rate is a schedule object"""
    opt = getattr(cb.model, "optimizer", None)
    if optimizer_schedule(opt) is not None:
        raise TypeError(f"{type(cb).__name__} sets optimizer.lr, but the optimizer's learning rate is the schedule "
                        f"{opt.lr!r}: use one or the other")


class ReduceLROnPlateau(Callback):
    """tf.keras.callbacks.ReduceLROnPlateau(monitor, factor, patience, min_delta, min_lr, cooldown, mode) -- commented out
    in the reference's main*.py.  Host only, once per epoch, through ``optimizer.lr``: when ``monitor`` has not improved
    by more than ``min_delta`` for ``patience`` epochs, lr = max(lr * factor, min_lr), and ``cooldown`` epochs pass before
    the count starts again.  mode "min" / "max"; "auto" is "max" for a monitor with "acc" in its name."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, verbose=0, mode="auto", min_delta=1e-4, cooldown=0,
                 min_lr=0.0):
        super().__init__()
        if not 0.0 <= factor < 1.0:
            raise ValueError(f"ReduceLROnPlateau does not support a factor outside [0, 1), got {factor!r}")
        if mode not in ("auto", "min", "max"):
            raise ValueError(f"mode must be 'auto', 'min' or 'max', got {mode!r}")
        if patience < 0 or cooldown < 0 or min_lr < 0 or min_delta < 0:
            raise ValueError("patience, cooldown, min_lr and min_delta must be >= 0")
        self.monitor, self.factor, self.patience, self.min_delta = monitor, float(factor), int(patience), float(min_delta)
        self.cooldown, self.min_lr = int(cooldown), float(min_lr)
        self.sign = -1 if (mode == "max" or (mode == "auto" and "acc" in monitor)) else 1
        self._reset()

    def _reset(self):
        self.best, self.wait, self.cooldown_counter = float("inf"), 0, 0

    def set_model(self, model):
        super().set_model(model)
        _refuse_schedule(self)

    def on_train_begin(self, logs=None):
        _refuse_schedule(self)
        self._reset()

    def on_epoch_end(self, epoch, logs=None):
        cur = (logs or {}).get(self.monitor)
        if logs is not None:
            logs["lr"] = self.model.optimizer.lr
        if cur is None:
            return
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if self.sign * cur < self.best - self.min_delta:
            self.best, self.wait = self.sign * cur, 0
        elif self.cooldown_counter == 0:
            self.wait += 1
            if self.wait >= self.patience:
                old = self.model.optimizer.lr
                if old > self.min_lr:
                    self.model.optimizer.lr = max(old * self.factor, self.min_lr)
                    self.cooldown_counter, self.wait = self.cooldown, 0


class ModelCheckpoint(Callback):
    """tf.keras.callbacks.ModelCheckpoint(filepath, monitor, save_weights_only=True, save_best_only, mode)
    -- main.py:168-190.  Weights are written by ``model.save_weights`` (.npz, keras names/layouts)."""

    def __init__(self, filepath, monitor="val_loss", verbose=0, save_weights_only=True, save_best_only=False, mode="min",
                 period=1):
        super().__init__()
        self.filepath, self.monitor, self.best_only, self.sign = filepath, monitor, save_best_only, (1 if mode == "min" else -1)
        self.best = float("inf")

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        cur = logs.get(self.monitor)
        rank0 = True
        if getattr(self.model, "dp_world", 1) > 1:
            # data parallel: every rank averages the per-replica BatchNorm moving statistics (a collective,
            # so it runs before any rank-local decision), then only rank 0 writes the file
            import torch.distributed as dist
            from . import dp
            dp.average_moving_stats(self.model)
            rank0 = dist.get_rank() == 0
        if not rank0:
            return
        if self.best_only:
            if cur is None or self.sign * cur >= self.best:
                return
            self.best = self.sign * cur
        path = self.filepath.format(epoch=epoch + 1, **logs)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self._save(path)

    def _save(self, path):
        self.model.save_weights(path)


class AverageModelCheckpoint(ModelCheckpoint):
    """tfa.callbacks.AverageModelCheckpoint(update_weights, filepath, ...): ModelCheckpoint for a model compiled with
    optimizers.MovingAverage / SWA that writes the averaged weights (``save_weights(path, averaged=True)``).
    ``update_weights=True`` also makes them the model's weights (``assign_average_vars``), as tfa's callback does;
    False leaves the model as it is."""

    def __init__(self, update_weights, filepath, monitor="val_loss", verbose=0, save_weights_only=True, save_best_only=False,
                 mode="min", period=1):
        super().__init__(filepath, monitor, verbose, save_weights_only, save_best_only, mode, period)
        self.update_weights = bool(update_weights)

    def _save(self, path):
        if self.update_weights:
            self.model.assign_average_vars()
        self.model.save_weights(path, averaged=True)


class EarlyStopping(Callback):
    """tf.keras.callbacks.EarlyStopping(monitor, min_delta, patience, mode): training stops once ``monitor`` has not
    improved by more than ``min_delta`` for more than ``patience`` epochs.  mode "min" (the default: a loss) or "max" (a
    caption metric such as ``val_rouge_l`` of fit(validation_captions=...)); ``best`` holds sign * value, as
    ModelCheckpoint's does."""

    def __init__(self, monitor="val_loss", min_delta=0.0, patience=0, mode="min"):
        super().__init__()
        if mode not in ("min", "max"):
            raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
        self.monitor, self.min_delta, self.patience, self.sign = monitor, min_delta, patience, (1 if mode == "min" else -1)
        self.best, self.wait = float("inf"), 0

    def on_epoch_end(self, epoch, logs=None):
        cur = (logs or {}).get(self.monitor)
        if cur is None:
            return
        if self.sign * cur < self.best - self.min_delta:
            self.best, self.wait = self.sign * cur, 0
        else:
            self.wait += 1
            if self.wait > self.patience:
                self.model.stop_training = True
