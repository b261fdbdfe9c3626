"""Which training options refuse to be combined: the features, the table of excluded pairs, and the one check.

A feature is a short key with one predicate ``on(model, pending)``.  ``pending`` overlays the values the current call is
about to store (the optimizer and the loss settings compile was handed, the multipliers set_lr_multipliers resolved, the
ScanDropout being assigned, ...) under the model's attribute names, so a check runs before its caller changes anything.
A row is one unordered pair: ``(a, b, exception class, text[, text when only b arrived])``.  ``check(model, arriving,
**pending)`` raises the first row, in table order, whose two sides are on and one of whose sides is in ``arriving``.

The model is taken duck-typed: nothing here imports a model class."""
from collections import namedtuple

from .optimizers import check_weight_decay

# ---------------------------------------------------------------------------------------------------- the texts
WEIGHTS_DP_REFUSAL = ("normalise=\"weights\" is not implemented under data parallel: the weight sum the loss is divided by is "
                      "formed per rank inside the head launch, so the ranks' gradients would carry different "
                      "denominators.  normalise=\"count\" works")
DISTILL_REFUSAL = ("knowledge distillation (CategoricalCrossentropy(distillation=...) / set_teacher) is built for the plain "
                   "single-device teacher-forced step of nic.NIC and lc_nic.NIC only: {what}")
WEIGHT_DECAY_REFUSAL = ("decoupled weight decay (weight_decay= / AdamW) is built for the single-device update launches only: "
                        "{what} does not apply it.  Train with weight_decay=None there, or on one device without it")
GLOBAL_CLIP_REFUSAL = ("global-norm clipping (global_clipnorm=) is built for the single-device update launches only: "
                       "{what} does not apply it.  Train with clipnorm there, or on one device without it")
FINETUNE_REFUSAL = ("layer freezing and learning-rate multipliers (freeze / set_lr_multipliers / layer.trainable) are built "
                    "for the single-device update launches only: {what} does not apply them.  Unfreeze everything and "
                    "clear the multipliers there, or train on one device without it")
GRAD_ACCUM_REFUSAL = ("gradient accumulation (gradient_accumulation_steps=) is built for the teacher-forced single-device "
                      "train_step of nic.NIC and lc_nic.NIC only: {what}.  Train with gradient_accumulation_steps=None there")
GRAD_ACCUM_WEIGHTS = ("normalise=\"weights\" divides each head launch's gradient by the weight sum of its own micro-batch, so "
                      "the micro-steps would carry different denominators (the reason of WEIGHTS_DP_REFUSAL); "
                      "normalise=\"count\" works")
AVERAGE_DP_REFUSAL = ("weight averaging (optimizers.MovingAverage / SWA) has no data-parallel schedule: the pipelined "
                      "schedules update the arena in slices and the row-sharded encoder finishes its update behind "
                      "_update_fused, so one averaging launch behind the update has no single place there.  Train it on "
                      "one device")
CORRUPT_DP_REFUSAL = ("scan_dropout / word_dropout are built for the single-device step only: the ranks of a data-parallel "
                      "step (dp.attach / grad_sync) would draw the same coins for their slices.  Train them on one device")
SEMANTIC_DP_REFUSAL = ("semantic (the sentence-embedding target) has no data-parallel schedule: its mean runs over one "
                       "rank's rows and the gradient launches of guse_out sit in none of the all-reduce buckets; train it on "
                       "one device")
COVERAGE_DP_REFUSAL = ("attention_coverage has no data-parallel schedule: the sum over the batch axis is not a per-rank "
                       "quantity, and the sum over time would need the ranks' gradient scales.  Train it on one device")
INIT_STATE_DP_REFUSAL = ("init_state (the learned initial LSTM state) has no data-parallel schedule: its gradient launches "
                         "sit in none of the all-reduce buckets.  Train it on one device")
_SCST_LOSS = "its loss is the advantage-weighted tnt_scst_cce_f32, not the compile loss"
_ONE_HEAD = "one head kernel computes one of them"
_WEIGHTS = "class_weight / focal_gamma / normalise=\"weights\""
_CORRUPT = "scan_dropout / word_dropout"
_INIT = "init_state (the learned initial LSTM state)"
_AGC_STEP = "a step with adaptive gradient clipping (enable_agc)"
_NOT_HEAD = "does not compute its loss with the caption head over (position, caption) rows"


# ---------------------------------------------------------------------------------------------------- the features
def _get(m, p, name):
    return p[name] if name in p else getattr(m, name)


def _weight_decay_on(m, p):
    """``weight_decay`` in the overlay (set_weight_decay's value; the optimizer-state build: whether its table decays
    anything), else the overlay's optimizer (compile), else the built table or the stored optimizer's value"""
    if "weight_decay" in p:
        return bool(p["weight_decay"])
    if "optimizer" in p:
        return bool(check_weight_decay(getattr(p["optimizer"], "weight_decay", None)))
    return m.seg_wd is not None or bool(check_weight_decay(getattr(m.optimizer, "weight_decay", None)))


FEATURES = {
    # ---- the compile loss
    "label_smoothing": lambda m, p: (p["label_smoothing"] if "label_smoothing" in p else m.label_smoothing) > 0,
    "unlikelihood": lambda m, p: (p["unlikelihood"] if "unlikelihood" in p else m.unlikelihood) > 0,
    "token_weights": lambda m, p: m._token_weights_on(p),
    "normalise_weights": lambda m, p: _get(m, p, "loss_normalise") == "weights",
    "distill_loss": lambda m, p: m._distill_on(p),                              # the compile loss's descriptor
    "distillation": lambda m, p: m._distill_on(p) or p.get("teacher") is not None,  # ... or a teacher arriving (set_teacher)
    # ---- the optimizer and the update
    "weight_decay": _weight_decay_on,
    "global_clip": lambda m, p: m._gclip(p) is not None,
    "grad_accum": lambda m, p: m._accum_k(p) is not None,
    "finetune": lambda m, p: bool(_get(m, p, "_lr_mul")),
    "average": lambda m, p: _get(m, p, "average") is not None,
    "agc": lambda m, p: bool(p["agc"] if "agc" in p else m.agc),
    # ---- the step
    "scheduled_sampling": lambda m, p: m.scheduled_sampling is not None,
    "self_critical": lambda m, p: m.self_critical is not None,
    "free_running": lambda m, p: not _get(m, p, "teacher_forcing"),     # (call_naive_attention: for that call)
    "attention_coverage": lambda m, p: m.attention_coverage is not None,
    "init_state": lambda m, p: m.init_state is not None,
    "semantic": lambda m, p: m.semantic is not None,
    "corruption": lambda m, p: m._corruption(p) is not None,
    "multi_subject": lambda m, p: int(m.S) > 1,
    "layer_norm_lstm": lambda m, p: bool(getattr(m, "use_layer_norm", False)),
    # ---- data parallel: a hook or a world, or dp.attach arriving (dp=True); ``dp_multi`` where only more than one rank
    # is refused
    "dp": lambda m, p: p["dp"] if "dp" in p else (m.grad_sync is not None or m.dp_world > 1),
    "dp_multi": lambda m, p: _get(m, p, "dp_world") > 1,
    # ---- train_step_sam / train_step_SAM: on for the call that arrives as it (sam=<its name>)
    "sam": lambda m, p: bool(p.get("sam")),
    # ---- the classes' capability flags
    "no_label_smoothing": lambda m, p: not m.SUPPORTS_LABEL_SMOOTHING,
    "no_unlikelihood": lambda m, p: not m.SUPPORTS_UNLIKELIHOOD,
    "no_token_weights": lambda m, p: not m.SUPPORTS_TOKEN_WEIGHTS,
    "no_grad_accum": lambda m, p: not m.SUPPORTS_GRAD_ACCUMULATION,
    "no_distillation": lambda m, p: not m.SUPPORTS_DISTILLATION,
}


def any_on(model, keys, _none={}):
    """whether one of the features ``keys`` is active on ``model`` as it stands"""
    for k in keys:
        if FEATURES[k](model, _none):
            return True
    return False


# ---------------------------------------------------------------------------------------------------- the rows
Row = namedtuple("Row", "a b exc text text_b", defaults=(None,))
NIE, VE = NotImplementedError, ValueError
_wd, _gc, _ft, _ga, _di = (t.format for t in (WEIGHT_DECAY_REFUSAL, GLOBAL_CLIP_REFUSAL, FINETUNE_REFUSAL,
                                              GRAD_ACCUM_REFUSAL, DISTILL_REFUSAL))
_DP_UPDATE = "the data-parallel update (dp.attach / grad_sync, the row-sharded encoder update included)"

# ``{cls}`` is the model's class name, ``{sam}`` the name of the sharpness-aware step that arrived.  The order is the
# order of the refusals where several rows are violated at once: the sharpness-aware step's, then what a constructor
# checks, then compile's order, then what is left of dp.attach's.
ROWS = (
    # a class without an accumulating step says so, whatever else its step would refuse
    Row("grad_accum", "no_grad_accum", NIE, _ga(what="{cls} has no accumulating step")),
    # ---- train_step_sam / train_step_SAM: two passes and an update of their own
    Row("sam", "weight_decay", NIE, _wd(what="{sam}")),                 # its update launches take no decay
    Row("sam", "global_clip", NIE, _gc(what="{sam}")),                  # ... and no global norm
    Row("sam", "finetune", NIE, _ft(what="{sam}")),                     # ... and no multiplier table
    Row("sam", "grad_accum", NIE, _ga(what="train_step_sam applies an update of its own every step")),
    Row("sam", "free_running", NIE, "train_step_sam is a teacher-forced step (lc_NIC.py:713-838): not built for "
                                    "teacher_forcing=False"),
    Row("sam", "multi_subject", NIE, "train_step_sam is a single-subject step (lc_NIC.py)"),
    Row("sam", "scheduled_sampling", NIE, "train_step_sam is a teacher-forced step: not built for scheduled_sampling"),
    Row("sam", "attention_coverage", NIE, "train_step_sam adds its own attention term (MSE(ones, attention_scores), the "
                                          "alpha_mse gradient of its first pass): not built for attention_coverage"),
    Row("sam", "init_state", NIE, f"train_step_sam is not built for {_INIT}"),
    Row("sam", "distillation", NIE, _di(what="train_step_sam's two passes do not run the teacher")),
    # ---- the ways to feed the decoder: one per model, each built for one subject and the plain LSTM cell
    Row("scheduled_sampling", "self_critical", VE, "a model takes scheduled_sampling or self_critical, not both"),
    Row("scheduled_sampling", "free_running", VE, "scheduled_sampling is a teacher-forced curriculum: it cannot be combined "
                                                  "with teacher_forcing=False (the free-running decoder)"),
    Row("scheduled_sampling", "multi_subject", NIE, "scheduled sampling is a single-subject mode: n_subjects > 1 is not "
                                                    "supported"),
    Row("scheduled_sampling", "layer_norm_lstm", NIE, "scheduled sampling is not built for the LayerNormLSTMCell "
                                                      "(use_layer_norm=True)"),
    Row("free_running", "multi_subject", NIE, "the free-running decoder (call_naive_attention) is a single-subject mode: "
                                              "n_subjects > 1 is not supported"),
    Row("free_running", "layer_norm_lstm", NIE, "the free-running decoder (call_naive_attention) is not built for the "
                                                "LayerNormLSTMCell (use_layer_norm=True)"),
    # ---- scan_dropout / word_dropout: the teacher-forced single-subject step
    Row("corruption", "scheduled_sampling", NIE, f"{_CORRUPT} are built for the teacher-forced step: not for scheduled_sampling"),
    Row("corruption", "self_critical", NIE, f"{_CORRUPT} are built for the teacher-forced step: not for self_critical"),
    Row("corruption", "free_running", NIE, f"{_CORRUPT} are built for the teacher-forced step: not for teacher_forcing=False "
                                           "(the free-running decoder)"),
    Row("corruption", "multi_subject", NIE, f"{_CORRUPT} are single-subject options: n_subjects > 1 is not supported"),
    # ---- semantic: the sentence-embedding target of nic.NIC
    Row("semantic", "scheduled_sampling", NIE, "semantic (the sentence-embedding target) has not been checked under "
                                               "scheduled_sampling"),
    Row("semantic", "self_critical", NIE, "semantic (the sentence-embedding target) is not built for the self_critical step, "
                                          "whose rows are copies of the scans"),
    # ---- attention_coverage: a term of the teacher-forced single-subject step
    Row("attention_coverage", "free_running", NIE, "attention_coverage is built for the teacher-forced step: not for "
                                                   "teacher_forcing=False (the free-running decoder)"),
    Row("attention_coverage", "scheduled_sampling", NIE, "attention_coverage is built for the teacher-forced step: not for "
                                                         "scheduled_sampling"),
    Row("attention_coverage", "multi_subject", NIE, "attention_coverage is a single-subject term: n_subjects > 1 is not "
                                                    "supported"),
    Row("attention_coverage", "layer_norm_lstm", NIE, "attention_coverage is not built for the LayerNormLSTMCell "
                                                      "(use_layer_norm=True)"),
    # ---- init_state: the learned initial LSTM state
    Row("init_state", "free_running", NIE, f"{_INIT} has not been checked on the free-running decoder: not with "
                                           "teacher_forcing=False"),
    Row("init_state", "scheduled_sampling", NIE, f"{_INIT} has not been checked under scheduled_sampling"),
    Row("init_state", "multi_subject", NIE, f"{_INIT} is a single-subject layer: n_subjects > 1 is not supported"),
    Row("init_state", "layer_norm_lstm", NIE, f"{_INIT} is not built for the LayerNormLSTMCell (use_layer_norm=True)"),
    Row("init_state", "agc", NIE, f"{_INIT} is not built for adaptive gradient clipping (enable_agc)"),
    # ---- the compile loss: the classes that do not read it, and one head kernel per step
    Row("label_smoothing", "no_label_smoothing", NIE, "{cls} computes its own masked sparse loss and does not read the "
                                                      "compile loss: label_smoothing > 0 is not implemented for it"),
    Row("label_smoothing", "self_critical", VE, f"label_smoothing > 0 does not apply to a self_critical model: {_SCST_LOSS}"),
    Row("unlikelihood", "no_unlikelihood", NIE, f"{{cls}} {_NOT_HEAD}: unlikelihood > 0 is not implemented for it"),
    Row("unlikelihood", "label_smoothing", VE, "unlikelihood > 0 together with label_smoothing > 0 is not implemented: one "
                                               "head kernel computes one of the two"),
    Row("unlikelihood", "self_critical", VE, f"unlikelihood > 0 does not apply to a self_critical model: {_SCST_LOSS}"),
    Row("token_weights", "no_token_weights", NIE, f"{{cls}} {_NOT_HEAD}: {_WEIGHTS} is not implemented for it"),
    Row("token_weights", "label_smoothing", VE, f"{_WEIGHTS} together with label_smoothing > 0 or unlikelihood > 0 is not "
                                                f"implemented: {_ONE_HEAD}"),
    Row("token_weights", "unlikelihood", VE, f"{_WEIGHTS} together with label_smoothing > 0 or unlikelihood > 0 is not "
                                             f"implemented: {_ONE_HEAD}"),
    Row("token_weights", "self_critical", VE, f"{_WEIGHTS} does not apply to a self_critical model: {_SCST_LOSS}"),
    # normalise="weights": the denominator is formed per head launch -- per rank, per micro-step, per subject
    Row("normalise_weights", "dp", NIE, WEIGHTS_DP_REFUSAL),
    Row("normalise_weights", "grad_accum", NIE, _ga(what=GRAD_ACCUM_WEIGHTS)),
    Row("normalise_weights", "multi_subject", NIE, "normalise=\"weights\" with n_subjects > 1 is not implemented: the "
                                                   "per-subject metrics divide each subject's sums by its position count "
                                                   "Bs * T, not by its weight sum.  normalise=\"count\" works"),
    # ---- distillation: one more head kernel (``distill_loss``: the descriptor), and the plain single-device
    # teacher-forced step runs the teacher (``distillation``: the descriptor, or a teacher arriving without one)
    Row("distill_loss", "label_smoothing", VE, "distillation together with label_smoothing > 0, unlikelihood > 0 or class_weight "
                                               f"/ focal_gamma / normalise=\"weights\" is not implemented: {_ONE_HEAD}"),
    Row("distill_loss", "unlikelihood", VE, "distillation together with label_smoothing > 0, unlikelihood > 0 or class_weight "
                                            f"/ focal_gamma / normalise=\"weights\" is not implemented: {_ONE_HEAD}"),
    Row("distill_loss", "token_weights", VE, "distillation together with label_smoothing > 0, unlikelihood > 0 or class_weight "
                                             f"/ focal_gamma / normalise=\"weights\" is not implemented: {_ONE_HEAD}",
        # the weights that arrive behind compile (set_class_weight; fit(class_weight=) comes through there)
        f"class_weight together with distillation is not implemented: {_ONE_HEAD}"),
    Row("distill_loss", "self_critical", VE, f"distillation does not apply to a self_critical model: {_SCST_LOSS}"),
    Row("distillation", "no_distillation", NIE, _di(what="{cls} does not support it")),
    Row("distillation", "dp", NIE, _di(what="there is no data-parallel schedule (dp.attach / grad_sync) that runs the teacher")),
    Row("distillation", "grad_accum", NIE, _di(what="gradient_accumulation_steps has no distilled micro-step")),
    Row("distillation", "scheduled_sampling", NIE, _di(what="scheduled_sampling feeds the student its own words, the teacher "
                                                            "the caption's")),
    Row("distillation", "self_critical", NIE, _di(what=f"a self_critical model's loss is the advantage-weighted "
                                                       "tnt_scst_cce_f32, not the compile loss")),
    Row("distillation", "semantic", NIE, _di(what="semantic (the sentence-embedding target) was not checked beside a "
                                                  "teacher's pass")),
    Row("distillation", "free_running", NIE, _di(what="the free-running decoder (teacher_forcing=False) feeds the student its "
                                                      "own words")),
    Row("distillation", "multi_subject", NIE, _di(what="n_subjects > 1 is not supported on the student")),
    # ---- the optimizer: what the single-device update launches do and the others do not
    # the averaging launch has no place in the data-parallel schedules
    Row("average", "dp", NIE, AVERAGE_DP_REFUSAL),
    # the data-parallel update launches (slices, the row-sharded encoder) do not decay
    Row("weight_decay", "dp", NIE, _wd(what=_DP_UPDATE)),
    Row("weight_decay", "agc", NIE, _wd(what=_AGC_STEP)),
    # the pipelined schedules update in slices before all norms exist
    Row("global_clip", "dp", NIE, _gc(what="the data-parallel update (dp.attach / grad_sync)")),
    Row("global_clip", "agc", NIE, _gc(what=_AGC_STEP)),
    # the sum over micro-steps takes the all-reduce's place; the two are not combined
    Row("grad_accum", "dp", NIE, _ga(what="accumulation under data parallel (dp.attach / grad_sync) is not implemented")),
    Row("grad_accum", "agc", NIE, _ga(what="adaptive gradient clipping (enable_agc) would clip each micro-batch's gradient, "
                                           "not the window's")),
    Row("grad_accum", "finetune", NIE, _ft(what="a step with gradient_accumulation_steps")),
    Row("grad_accum", "scheduled_sampling", NIE, _ga(what="scheduled_sampling has no accumulating step")),
    Row("grad_accum", "self_critical", NIE, _ga(what="self_critical has no accumulating step")),
    Row("grad_accum", "free_running", NIE, _ga(what="the free-running decoder (teacher_forcing=False) has no accumulating step")),
    Row("grad_accum", "attention_coverage", NIE, _ga(what="attention_coverage's gradient scale is not threaded through the "
                                                          "micro-steps")),
    Row("grad_accum", "init_state", NIE, _ga(what=f"{_INIT} has no accumulating step")),
    Row("grad_accum", "semantic", NIE, _ga(what="semantic (the sentence-embedding target) has no accumulating step: its "
                                                "gradient scale is not threaded through the micro-steps")),
    Row("grad_accum", "multi_subject", NIE, _ga(what="n_subjects > 1 has no accumulating step")),
    Row("finetune", "semantic", NIE, _ft(what="a model with semantic= (the sentence-embedding target: its launches do not "
                                              "leave out a frozen variable's share)")),
    # the data-parallel update launches (slices, the row-sharded encoder) take no table
    Row("finetune", "dp", NIE, _ft(what=_DP_UPDATE)),
    Row("finetune", "agc", NIE, _ft(what=_AGC_STEP)),
    # ---- data parallel: what has no schedule there.  Where the wordings differ, the first is that of the model's side (the
    # constructor handed a hook, the step which finds one attached since), the second dp.attach's
    Row("free_running", "dp", NIE, "the free-running step (teacher_forcing=False) has no data-parallel schedule",
        "data parallel training of the free-running decoder (teacher_forcing=False) is not supported: train it on one device"),
    Row("scheduled_sampling", "dp", NIE, "scheduled sampling has no data-parallel schedule: train it on one device",
        "data parallel training with scheduled sampling is not supported: train it on one device"),
    # the self-critical step's host round trip has no data-parallel schedule
    Row("self_critical", "dp", NIE, "self-critical training has no data-parallel schedule: train it on one device",
        "data parallel self-critical training is not supported: train it on one device"),
    Row("attention_coverage", "dp", NIE, COVERAGE_DP_REFUSAL),
    Row("init_state", "dp", NIE, INIT_STATE_DP_REFUSAL),
    Row("semantic", "dp", NIE, SEMANTIC_DP_REFUSAL),
    Row("corruption", "dp", NIE, CORRUPT_DP_REFUSAL),
    # ---- adaptive gradient clipping.  agc.py:25-30 clips the Embedding by the column norms of its UN-merged IndexedSlices
    # rows; across replicas those are per-rank partial sums that would have to be all-reduced before every rank scales the
    # summed gradient, and the pipelined schedules update slice by slice without an AGC pass.  One rank (world = 1) is fine
    Row("agc", "dp_multi", NIE, "adaptive gradient clipping is not supported under data parallel (dp.attach)",
        "adaptive gradient clipping (enable_agc) is not supported under data parallel: call enable_agc(None) before "
        "dp.attach, or train on one device"),
    Row("agc", "semantic", NIE, "semantic (the sentence-embedding target) is not built for adaptive gradient clipping "
                                "(enable_agc)"),
)

# per arriving key: the indices of the rows that mention it, in table order
_BY_KEY = {}
for _i, _r in enumerate(ROWS):
    assert _r.a in FEATURES and _r.b in FEATURES, _r
    _BY_KEY.setdefault(_r.a, []).append(_i)
    _BY_KEY.setdefault(_r.b, []).append(_i)


def check(model, arriving, **pending):
    """Raise the first row of the table whose two features are on and one of which is in ``arriving``; return where none
    of the arriving features is on.  Call it before anything is stored."""
    live = [k for k in arriving if FEATURES[k](model, pending)]
    if not live:
        return
    idx = _BY_KEY.get(live[0], ()) if len(live) == 1 else sorted({i for k in live for i in _BY_KEY.get(k, ())})
    known = dict.fromkeys(live, True)
    for i in idx:
        row = ROWS[i]
        for k in (row.a, row.b):
            if k not in known:
                known[k] = FEATURES[k](model, pending)
        if known[row.a] and known[row.b]:
            text = row.text_b if row.text_b is not None and row.a not in arriving else row.text
            raise row.exc(text.replace("{cls}", type(model).__name__).replace("{sam}", str(pending.get("sam"))))


# ---------------------------------------------------------------------------------------------------- the table as text
def markdown():
    """the matrix as markdown (tools/refusal_matrix.py --markdown): feature x feature with the row's number in the cell, and
    under it the rows by number -- exception class and reason -- in the order they are checked"""
    keys = [k for k in FEATURES if k in _BY_KEY]
    cell = {}
    for i, r in enumerate(ROWS, 1):
        cell[r.a, r.b] = cell[r.b, r.a] = str(i)
    out = ["| | " + " | ".join(f"`{k}`" for k in keys) + " |", "|---|" + "---|" * len(keys)]
    out += [f"| `{a}` | " + " | ".join(cell.get((a, b), "") for b in keys) + " |" for a in keys]
    out += ["", "| row | pair | raises | reason |", "|---|---|---|---|"]
    flat = lambda t: " ".join(t.split()).replace("|", "\\|")
    for i, r in enumerate(ROWS, 1):
        why = flat(r.text) if r.text_b is None else f"{flat(r.text)}<br>where only `{r.b}` arrives: {flat(r.text_b)}"
        out.append(f"| {i} | `{r.a}` x `{r.b}` | `{r.exc.__name__}` | {why} |")
    return "\n".join(out)
