"""``config.yaml`` loader: the reference's YAML (AttemptFour/config.yaml:1-60, loaded with
yaml.safe_load at main.py:36-38) is accepted unchanged; ``build_model`` constructs the model
the way main.py:113-134 does."""
import yaml

from . import schedules
from .model_base import AttentionCoverage, LearnedInitState, ScanDropout, SemanticTarget, WordDropout
from .optimizers import Adam, AdamW, SGD, CategoricalCrossentropy


def load_config(path):
    with open(path, "r") as f:
        return yaml.safe_load(f)


def build_optimizer(config):
    """main.py:96-104 (the Adam learning rate is hard-coded to 1e-4 there; config['alpha'] holds the same value)."""
    # lr_schedule: an optional key of this library's (main.py:81-84 builds its schedule in code): ``kind`` plus that
    # optimizers.schedules class's arguments, optional warmup_steps / warmup_start.  It takes the learning rate's place
    sched = schedules.from_config(config["lr_schedule"]) if config.get("lr_schedule") is not None else None
    # weight_decay / weight_decay_exclude (a list of name substrings): optional keys of this library's, decoupled weight
    # decay (optimizers._WeightDecay); ``optimizer: AdamW`` is Adam as above with keras's default decay 0.004 unless given
    wd, excl = config.get("weight_decay"), config.get("weight_decay_exclude")
    if excl is not None and (isinstance(excl, str) or not isinstance(excl, (list, tuple))):
        raise ValueError(f"weight_decay_exclude must be a list of name substrings, got {excl!r}")
    # global_clipnorm: an optional key of this library's, one norm over all gradients (optimizers._GlobalClipnorm).  With it
    # set, ``clipnorm`` may be absent or null; the two together are refused, as in keras
    gclip = config.get("global_clipnorm")
    if gclip is not None and config.get("clipnorm") is not None:
        raise ValueError("clipnorm and global_clipnorm cannot both be set: at most one of them, as in keras")
    # gradient_accumulation_steps: an optional key of this library's, one update per k training steps
    # (optimizers._GradientAccumulation); absent, null or 1: off
    accum = config.get("gradient_accumulation_steps")
    if config["optimizer"] in ("Adam", "AdamW"):
        kw = dict(learning_rate=0.0001 if sched is None else sched, beta_1=0.9, beta_2=0.98, epsilon=10.0e-9,
                  clipnorm=config["clipnorm"] if gclip is None else None, global_clipnorm=gclip,
                  gradient_accumulation_steps=accum)
        if config["optimizer"] == "AdamW":
            opt = AdamW(weight_decay=0.004 if wd is None else wd, **kw)
        else:
            opt = Adam(weight_decay=wd, **kw)
    elif config["optimizer"] == "SGD":
        opt = SGD(learning_rate=config["alpha"] if sched is None else sched, momentum=0.9, nesterov=False, weight_decay=wd,
                  global_clipnorm=gclip, gradient_accumulation_steps=accum)
    else:
        raise ValueError("No optimizer specified")
    if excl:
        opt.exclude_from_weight_decay(var_names=list(excl))
    return opt


def _corruption_keys(config, kw):
    """scan_dropout: a rate or {rate: } and word_dropout: {rate: , unk_id: }: optional keys of this library's
    (model_base.ScanDropout / WordDropout) -> the constructor keywords, unless the caller passed them"""
    sd, wd = config.get("scan_dropout"), config.get("word_dropout")
    if sd is not None and "scan_dropout" not in kw:
        if isinstance(sd, dict):
            if set(sd) != {"rate"}:
                raise ValueError(f"scan_dropout must be a rate or a mapping with rate, got {sd!r}")
            sd = sd["rate"]
        kw["scan_dropout"] = ScanDropout(sd)
    if wd is not None and "word_dropout" not in kw:
        if not isinstance(wd, dict) or set(wd) != {"rate", "unk_id"}:
            raise ValueError(f"word_dropout must be a mapping with rate and unk_id, got {wd!r}")
        kw["word_dropout"] = WordDropout(wd["rate"], wd["unk_id"])


def build_model(config, groups, mode="attention", input_size=None, **kw):
    """lc_NIC.NIC(...) exactly as main.py:113-132 builds it, compiled as at main.py:134.
    mode="fc" builds the fully-connected variant instead (the call_fc / greedy_predict_fc dispatch the
    reference selects by editing lc_NIC.py:163-167,507-509); it needs ``input_size`` (#voxels).
    mode="dense" builds nic.NIC (Model/NIC.py: the dense encoder in front of the LSTM, embedding_text wide); it needs
    ``input_size`` too, and ``groups`` is not used."""
    vocab_size = config["top_k"] + 1
    # semantic: {dim: , weight: , reg: , loss: , temperature: , symmetric: , soft_temperature: }: an optional key of this library's (model_base.SemanticTarget), the sentence-embedding
    # target of nic.NIC; the other models do not take it
    sem = SemanticTarget.from_config(config.get("semantic")) if "semantic" not in kw else None
    if sem is not None:
        if mode != "dense":
            raise NotImplementedError(f"semantic (the sentence-embedding target) is built for nic.NIC (mode=\"dense\") only, "
                                      f"not for mode={mode!r}")
        kw["semantic"] = sem
    if mode == "fc":
        from .fc_nic import NICfc
        model = NICfc(input_size, config["units"], config["embedding_features"], config["embedding_text"], vocab_size,
                      config["max_length"], config["dropout_input"], config["dropout_features"], config["dropout_text"],
                      config["dropout_lstm"], config["dropout_out"], config["input_reg"], config["lstm_reg"],
                      config["output_reg"], seed=config.get("seed", 42), **kw)
    elif mode == "dense":
        from .nic import NIC as DenseNIC
        _corruption_keys(config, kw)
        model = DenseNIC(input_size, config["units"], config["embedding_text"], vocab_size, config["max_length"],
                         config["dropout_input"], config["dropout_features"], config["dropout_lstm"], config["input_reg"],
                         config["lstm_reg"], config["output_reg"], seed=config.get("seed", 42), **kw)
    elif mode == "attention":
        from .lc_nic import NIC
        _corruption_keys(config, kw)
        # attention_coverage: {weight: , axis: }: an optional key of this library's (model_base.AttentionCoverage)
        cov = config.get("attention_coverage")
        if cov is not None and "attention_coverage" not in kw:
            if not isinstance(cov, dict) or not set(cov) <= {"weight", "axis"} or "weight" not in cov:
                raise ValueError(f"attention_coverage must be a mapping with weight and optionally axis, got {cov!r}")
            kw["attention_coverage"] = AttentionCoverage(cov["weight"], cov.get("axis", "time"))
        # learn_init_state: true or {reg: }: an optional key of this library's (model_base.LearnedInitState)
        if "init_state" not in kw:
            init = LearnedInitState.from_config(config.get("learn_init_state"))
            if init is not None:
                kw["init_state"] = init
        model = NIC(groups, config["units"], config["embedding_features"], config["embedding_text"],
                    config["attn_units"], vocab_size, config["max_length"], config["dropout_input"],
                    config["dropout_features"], config["dropout_text"], config["dropout_attn"], config["dropout_lstm"],
                    config["dropout_out"], config["input_reg"], config["attn_reg"], config["lstm_reg"],
                    config["output_reg"], seed=config.get("seed", 42), **kw)
    else:
        raise ValueError(f"unknown mode {mode!r}")
    # label_smoothing, unlikelihood: optional keys of this library's (the reference's config has none), default 0; so are
    # class_weight (an {id: weight} mapping), focal_gamma and loss_normalise ("count" / "weights"), default neutral; and
    # distillation ({alpha: , temperature: }; the caller gives the model its teacher with set_teacher), default none
    loss = CategoricalCrossentropy(from_logits=False, reduction="none", label_smoothing=config.get("label_smoothing", 0.0),
                                   unlikelihood=config.get("unlikelihood", 0.0), class_weight=config.get("class_weight"),
                                   focal_gamma=config.get("focal_gamma", 0.0),
                                   normalise=config.get("loss_normalise", "count"),
                                   distillation=config.get("distillation"))
    # freeze (a list of layer / variable names) and lr_multipliers ({name: multiplier}): optional keys of this library's,
    # the fine-tuning recipe (ModelBase.freeze / set_lr_multipliers); compile validates the names
    model.compile(build_optimizer(config), loss, run_eagerly=True, freeze=config.get("freeze"),
                  lr_multipliers=config.get("lr_multipliers"))
    return model
