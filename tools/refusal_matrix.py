"""The feature-exclusion matrix of the training options, observed from outside: every ordered pair of features, turned on
one behind the other through the public entry points (constructors, compile, set_*, freeze, the dropout setters,
enable_agc, dp.attach, a grad_sync hook, train_step, train_step_sam), on the CPU over the tests' mock backend.

    python tools/refusal_matrix.py                 # the cases as JSON on stdout
    python tools/refusal_matrix.py --out FILE      # ... into FILE (tests/data/refusal_matrix.json is one such recording)
    python tools/refusal_matrix.py --markdown      # the table of masters_thesis_amd.compat as markdown

A case is ``"<model>|<feature A>:<how>|<feature B>:<how>"`` (or ``"<model>|<feature>:<how>"`` for a feature alone, which is
what a class without the capability refuses) and records ``"ok"`` or ``{"error": [exception class, message], "clean": ...}``;
``clean`` says that the refused call left optimizer, grad_sync, agc, the multipliers and the class weights as they were and
launched nothing (null where the refusing call is the constructor).  Only the last call of a case may refuse: a case
whose earlier calls fail is not a case of this pair and is left out, and so is every set of features that no case
refuses.  tests/test_host_refusals.py runs the same cases against the recording."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, U, E, V, T, G = 23, 16, 16, 13, 6, 8           # the shapes of tests/test_host_grad_accum.py


def _backend():
    from accum_oracle import AccumMockBackend
    from average_oracle import AverageMockBackend
    from corrupt_oracle import CorruptMockBackend
    from coverage_oracle import CoverageMockBackend
    from distill_oracle import DistillMockBackend
    from finetune_oracle import FinetuneMockBackend
    from init_state_oracle import InitMockBackend
    from lr_schedule_oracle import LrScheduleMockBackend
    from scst_oracle import SCSTMockBackend
    from semantic_oracle import SemanticMockBackend
    from smooth_oracle import SmoothMockBackend
    from ss_att_oracle import SSAttMockBackend
    from unlikelihood_oracle import UnlikelihoodMockBackend
    from test_host_naive_attention import NaiveMockBackend
    from weighted_oracle import WeightedMockBackend

    class Backend(AccumMockBackend, FinetuneMockBackend, LrScheduleMockBackend, AverageMockBackend, DistillMockBackend,
                  WeightedMockBackend, UnlikelihoodMockBackend, SmoothMockBackend, CorruptMockBackend, CoverageMockBackend,
                  InitMockBackend, SemanticMockBackend, SCSTMockBackend, SSAttMockBackend, NaiveMockBackend):
        """every mock op of the host tests; ``names`` logs the public calls"""

        def __init__(self):
            super().__init__()
            self.names = []

        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if name.startswith("_") or not callable(v):
                return v
            names = object.__getattribute__(self, "names")

            def logged(*a, **k):
                names.append(name)
                return v(*a, **k)
            return logged
    return Backend()


# ---------------------------------------------------------------------------------------------------- models
def _models():
    from helpers import tiny_groups
    from masters_thesis_amd import think_and_tell as TT
    from masters_thesis_amd import think_and_tell_att as TTA
    from masters_thesis_amd.fc_nic import NICfc
    from masters_thesis_amd.lc_nic import NIC as LcNIC
    from masters_thesis_amd.ms_nic import NIC as MsNIC
    from masters_thesis_amd.nic import NIC

    def attention(cls=LcNIC, **kw):
        g = (tiny_groups(N, 4, np.random.default_rng(1)), [16] * 4)
        return cls(g, U, 512, 12, 5, V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu", seed=11, **kw)

    def generator(mod):
        return lambda **kw: mod.CaptionGenerator(mod.Encoder(E, 0.01, "glorot_uniform", 0.0),
                                                 mod.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0), None, T, device="cpu",
                                                 seed=11, **kw)
    return {"dense": lambda **kw: NIC(N, U, E, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw),
            "attention": attention,
            "ms": lambda **kw: attention(MsNIC, **kw),
            "fc": lambda **kw: NICfc(N, U, E, E, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", seed=11, **kw),
            "think_and_tell": generator(TT),
            "think_and_tell_att": generator(TTA)}


def _hook():
    hook = lambda m: None
    hook.world = 2
    return hook


def _batch(kind, model):
    from helpers import synth_batch
    rng = np.random.default_rng(0)
    if kind.startswith("think_and_tell"):
        x = rng.standard_normal((4, 19)).astype(np.float32)
        tgt = rng.integers(1, V, (4, T)).astype(np.int32)
        return x, None, tgt
    data, tgt = synth_batch(4, N, T, V, U, rng)
    if getattr(model, "semantic", None) is not None:
        data = data + (rng.standard_normal((4, G)).astype(np.float32),)
    return data, tgt


# ---------------------------------------------------------------------------------------------------- how a feature is turned on
# A way is (stage, name, payload).  Stages, in the order a case runs them:
#   0 ctor      payload: constructor keywords
#   1 before    payload: f(model, kind) in front of compile
#   2 compile   payload: dict(opt=..., loss=..., wrap=..., kw=..., after=...) merged into the one compile call
#   3 behind    payload: f(model, kind) behind compile; ``late`` ways are seen by the next train_step only
#   4 built     payload: f(model, kind) behind one training step (the optimizer state exists)
#   5 step      payload: f(model, kind), the step itself
# ``last_only`` ways cannot be followed by anything (dp.attach broadcasts on success; the SAM step is the case's end).
class Way:
    def __init__(self, stage, name, payload, models=("dense", "attention"), late=False, last_only=False):
        self.stage, self.name, self.payload, self.models, self.late, self.last_only = stage, name, payload, models, late, last_only


def _ways():
    from masters_thesis_amd import dp
    from masters_thesis_amd.model_base import (AttentionCoverage, LearnedInitState, ScanDropout, ScheduledSampling,
                                               SelfCritical, SemanticTarget, WordDropout)
    from masters_thesis_amd.optimizers import Distillation

    both, dense, att = ("dense", "attention"), ("dense",), ("attention",)
    every = ("dense", "attention", "ms", "fc", "think_and_tell", "think_and_tell_att")
    arena = every[:4]                               # (the generators build their variables at the first batch)

    def ctor(name, models=both, **kw):
        return Way(0, name, kw, models)

    def act(name, f, models=every, stages=(1, 3), **flags):
        return [Way(s, f"{name}@{s}", f, models, **flags) for s in stages]

    def comp(name, models=every, **parts):
        return Way(2, name, parts, models)

    def assign(attr, value):
        return lambda m, kind: setattr(m.optimizer, attr, value)

    def teacher(m, kind):
        m.set_teacher(_models()["dense"]())

    def attach(world):
        def f(m, kind):
            try:
                dp.attach(m, world=world, rank=0)
            except Exception:
                if m.grad_sync is None:
                    raise                           # a refusal; behind them attach fails at its broadcast (no process group)
        return f

    F = {}
    F["scheduled_sampling"] = [ctor("ctor", scheduled_sampling=ScheduledSampling.linear(0.5, 0.0))]
    F["self_critical"] = [ctor("ctor", dense, self_critical=SelfCritical(2, n_samples=2, baseline="mean", reward="bleu4"))]
    F["free_running"] = [ctor("ctor", att, teacher_forcing=False)]
    F["attention_coverage"] = [ctor("ctor", att, attention_coverage=AttentionCoverage(0.5))]
    F["init_state"] = [ctor("ctor", att, init_state=LearnedInitState())]
    F["semantic"] = [ctor("ctor", dense, semantic=SemanticTarget(G, 0.7, 0.02))]
    F["multi_subject"] = [ctor("ctor", att, n_subjects=2)]
    F["layer_norm_lstm"] = [ctor("ctor", att, use_layer_norm=True)]
    # one way per entry point and per place in the order of a case: more ways of the same call record the same refusals
    F["corruption"] = ([ctor("ctor_scan", every[:3], scan_dropout=ScanDropout(0.5))]
                       + act("set_word", lambda m, kind: setattr(m, "word_dropout", WordDropout(0.5, 2)), stages=(3,)))
    F["dp"] = ([ctor("ctor_hook", every, grad_sync=_hook())]
               + act("hook", lambda m, kind: setattr(m, "grad_sync", _hook()), stages=(3,), late=True)
               + act("attach1", attach(1), stages=(3,), last_only=True))
    F["dp_multi"] = act("attach2", attach(2), stages=(3,), last_only=True)
    F["agc"] = act("enable_agc", lambda m, kind: m.enable_agc(0.02, 1e-3))
    F["finetune"] = (act("freeze", lambda m, kind: m.freeze(_layer(m)), arena)
                     + [comp("compile_freeze", arena, kw=lambda m: dict(freeze=[_layer(m)]))])
    F["label_smoothing"] = [comp("loss", loss=dict(label_smoothing=0.1))]
    F["unlikelihood"] = [comp("loss", loss=dict(unlikelihood=0.5))]
    F["token_weights"] = ([comp("class_weight", loss=dict(class_weight={0: 0.0}))]
                          + act("set_class_weight", lambda m, kind: m.set_class_weight({0: 0.5}), stages=(3,)))
    F["normalise_weights"] = [comp("loss", loss=dict(class_weight={0: 0.0}, normalise="weights"))]
    F["distillation"] = ([comp("loss", loss=dict(distillation=Distillation(0.5, 2.0)), after=teacher)]
                         + act("set_teacher", teacher, stages=(3,)))
    F["weight_decay"] = ([comp("opt", opt=dict(weight_decay=0.01))]
                         + act("assign", assign("weight_decay", 0.01), stages=(3,), late=True)
                         + act("set_weight_decay", lambda m, kind: m.set_weight_decay(0.01), stages=(4,)))
    F["global_clip"] = ([comp("opt", opt=dict(global_clipnorm=1.0))]
                        + act("assign", assign("global_clipnorm", 1.0), stages=(3, 4), late=True))
    F["grad_accum"] = ([comp("opt", opt=dict(gradient_accumulation_steps=2))]
                       + act("assign", assign("gradient_accumulation_steps", 2), stages=(3, 4), late=True))
    F["average"] = [comp("opt", wrap=True)]
    F["sam"] = ([Way(5, "train_step_sam", lambda m, kind: m.train_step_sam(_batch(kind, m)), ("attention", "ms"), last_only=True),
                 Way(5, "train_step_SAM", lambda m, kind: m.train_step_SAM(_batch(kind, m)),
                     ("think_and_tell", "think_and_tell_att"), last_only=True)])
    return F


def _layer(model):
    """a layer without BatchNorm statistics to freeze: the first whose name holds 'lstm', else the last one"""
    names = list(model.layers_spec)
    return next((n for n in names if "lstm" in n), names[-1])


# ---------------------------------------------------------------------------------------------------- one case
class _NotACase(Exception):
    pass


def _state(model, be):
    cw = None if model.class_weight is None else model.class_weight.tolist()
    return (id(model.optimizer), id(model.grad_sync), model.agc, dict(model._lr_mul), cw, len(be.names))


def run_case(kind, ways):
    """``ways``: one or two (feature, Way), in the order they are turned on"""
    import masters_thesis_amd.ops as ops
    from masters_thesis_amd.optimizers import Adam, CategoricalCrossentropy, MovingAverage
    be = _backend()
    old = ops._backend
    ops.set_backend(be)
    try:
        ways = sorted(ways, key=lambda fw: fw[1].stage)         # (stable: equal stages keep the order given)
        last = ways[-1][1]

        def guarded(w, call, model=None):
            """run one call of the case; a failure anywhere but in the case's last call is not this case"""
            before = None if model is None else _state(model, be)
            try:
                return call(), None
            except Exception as e:                               # noqa: BLE001 -- the recording is the point
                if w is not last:
                    raise _NotACase() from e
                clean = None if model is None else _state(model, be) == before
                return None, {"error": [type(e).__name__, str(e)], "clean": clean}

        kw = {}
        for _, w in ways:
            if w.stage == 0:
                kw.update(w.payload)
        ctor_way = last if last.stage == 0 else None
        model, err = guarded(ctor_way, lambda: _models()[kind](**kw))
        if err:
            return err
        for _, w in ways:
            if w.stage == 1:
                _, err = guarded(w, lambda: w.payload(model, kind), model)
                if err:
                    return err
        if last.stage < 2 and not last.late:
            return "ok"
        comp = [w for _, w in ways if w.stage == 2]
        opt, loss, wrap, ckw = {}, {}, False, {}
        for w in comp:
            opt.update(w.payload.get("opt", {}))
            loss.update(w.payload.get("loss", {}))
            wrap = wrap or w.payload.get("wrap", False)
            ckw.update(w.payload["kw"](model) if "kw" in w.payload else {})
        optimizer = Adam(1e-3, **opt)
        optimizer = MovingAverage(optimizer, 0.9) if wrap else optimizer
        loss = CategoricalCrossentropy(from_logits=False, reduction="none", **loss) if loss else None
        _, err = guarded(comp[-1] if comp else None, lambda: model.compile(optimizer, loss, **ckw), model)
        if err:
            return err
        for w in comp:
            if "after" in w.payload:                # (the teacher a distilling compile loss needs before its first step)
                _, err = guarded(w, lambda: w.payload["after"](model, kind), model)
                if err:
                    return err
        for _, w in ways:
            if w.stage == 3:
                _, err = guarded(w, lambda: w.payload(model, kind), model)
                if err:
                    return err
        if last.stage <= 3 and not any(w.late for _, w in ways):
            return "ok"
        step = lambda: model.train_step(_batch(kind, model))
        if any(w.stage <= 3 and w.late for _, w in ways) or last.stage == 4:
            late_last = last if last.stage <= 3 and last.late else None
            _, err = guarded(late_last, step, model)
            if err:
                return err
        for _, w in ways:
            if w.stage in (4, 5):
                _, err = guarded(w, lambda: w.payload(model, kind), model)
                if err:
                    return err
                if w.late:
                    _, err = guarded(w, step, model)
                    if err:
                        return err
        return "ok"
    finally:
        ops.set_backend(old)


def cases():
    """{case id: (model kind, [(feature, Way), ...])}: every feature alone on every class that takes the call, and every
    ordered pair on the two caption models"""
    F = _ways()
    out = {}
    for kind in _models():
        for f, ws in F.items():
            for w in ws:
                if kind in w.models:
                    out[f"{kind}|{f}:{w.name}"] = (kind, [(f, w)])
    for kind in ("dense", "attention"):
        for fa, was in F.items():
            for fb, wbs in F.items():
                if fa == fb or {fa, fb} == {"dp", "dp_multi"}:
                    continue
                for wa in was:
                    for wb in wbs:
                        if kind not in wa.models or kind not in wb.models or wa.last_only or wa.stage > wb.stage:
                            continue
                        if wa.stage == wb.stage and wa.stage in (0, 2) and fa > fb:
                            continue                # one constructor, one compile: the order is not observable
                        out[f"{kind}|{fa}:{wa.name}|{fb}:{wb.name}"] = (kind, [(fa, wa), (fb, wb)])
    return out


def record():
    """the outcome of every case of every (model, set of features) of which some case is refused: a configuration that
    violates nothing in any order and through any entry point is not written down (were it refused later, it would
    turn up here as a case the earlier recording does not have)"""
    out, groups = {}, {}
    for cid, (kind, ways) in cases().items():
        try:
            out[cid] = run_case(kind, ways)
        except _NotACase:
            continue
        groups.setdefault((kind, frozenset(f for f, _ in ways)), []).append(cid)
    return {cid: out[cid] for ids in groups.values() if any(out[i] != "ok" for i in ids) for cid in ids}


def dump(rec):
    """a recording as text: the distinct messages once, then the cases by all but their last call -- the refused ones as
    {last call: [exception class, message number, clean]}, the accepted ones as [last call, ...]"""
    msgs = sorted({v["error"][1] for v in rec.values() if v != "ok"})
    at = {m: i for i, m in enumerate(msgs)}
    js = lambda x: json.dumps(x, separators=(",", ":"))
    refused, ok = {}, {}
    for k, v in sorted(rec.items()):
        head, _, last = k.rpartition("|")
        if v == "ok":
            ok.setdefault(head, []).append(last)
        else:
            refused.setdefault(head, {})[last] = [v["error"][0], at[v["error"][1]], v["clean"]]
    lines = lambda d: ",\n".join(f"{js(head)}:{js(lasts)}" for head, lasts in d.items())
    return ('{"messages":[\n' + ",\n".join(js(m) for m in msgs) + '],\n"refused":{\n' + lines(refused)
            + '},\n"ok":{\n' + lines(ok) + "}}\n")


def load(path):
    """a file written by ``dump``, in the form ``record`` returns"""
    with open(path) as f:
        d = json.load(f)
    out = {f"{head}|{last}": "ok" for head, lasts in d["ok"].items() for last in lasts}
    out.update({f"{head}|{last}": {"error": [cls, d["messages"][i]], "clean": clean}
                for head, lasts in d["refused"].items() for last, (cls, i, clean) in lasts.items()})
    return out


def markdown():
    from masters_thesis_amd import compat
    return compat.markdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the JSON recording here instead of stdout")
    ap.add_argument("--markdown", action="store_true", help="print the table of masters_thesis_amd.compat")
    args = ap.parse_args()
    if args.markdown:
        print(markdown())
    else:
        text = dump(record())
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        else:
            sys.stdout.write(text)
