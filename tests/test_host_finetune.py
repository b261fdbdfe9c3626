"""Layer freezing and per-variable learning-rate multipliers (freeze / unfreeze / set_lr_multipliers / layer.trainable) on
the CPU through a mock backend that follows the header definition (tests/finetune_oracle.py): names and values, the
refusals in both orders, the *_lrmul call in the plain one's place on every update route, three training steps of both
caption models against the float64 oracle with a mixed table, frozen variables bit for bit, what a toggle does to the
recordings, the gradient launches a frozen decoder or encoder leaves out, and the transfer journey (train on one
subject, load into a model with another voxel count, train the encoder under a frozen decoder).

Model-level tolerances are test_host_global_clip's for the same comparison (rtol 2e-4 and its per-variable atol).  The mixed
table carries multipliers 0.1 and 10: an update that ignored the table moves those variables by 10x too much or too
little, far outside the bound; a frozen variable is compared bit for bit."""
import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import dp
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import SGD, Adam, AdamW
from oracle import models as M
from average_oracle import AverageMockBackend
from finetune_oracle import FinetuneMockBackend, FinetuneState
from helpers import synth_batch
from lr_schedule_oracle import LrScheduleMockBackend
from test_host_weight_decay import ADAM as ADAM_CLIP, B, N, T, U, V, WD, attention, batch, dense
from weight_decay_oracle import decay_of

ADAM = {k: v for k, v in ADAM_CLIP.items() if k != "clipnorm"}
LRMUL = {"adam": "adam_lrmul", "sgd": "sgd_lrmul", "adamw": "adam_lrmul", "sgdw": "sgd_lrmul", "adam_gclip": "adam_lrmul",
         "sgd_gclip": "sgd_lrmul", "dense_dw_adam": "dense_dw_adam_lrmul", "dense_dw_adamw": "dense_dw_adam_lrmul",
         "dense_dw_adam_gclip": "dense_dw_adam_lrmul", "span_sqnorm": "span_sqnorm_lrmul", "seg_sqnorm": "seg_sqnorm_lrmul",
         "global_sqnorm": "global_sqnorm_lrmul"}
DECODER = ("emb_text", "lstm", "time_distributed_softmax")
HEAD = ("time_distributed_softmax/kernel", "time_distributed_softmax/bias")
LSTM = ("lstm/kernel", "lstm/recurrent_kernel", "lstm/bias")
C = 0.02          # test_host_global_clip's threshold: it clips these models by a factor of 2 at least


class RecordingBackend(FinetuneMockBackend, LrScheduleMockBackend, AverageMockBackend):
    """the mock with the table forms; ``names`` logs every public call, ``ptrs`` the addresses of its tensor arguments"""

    def __init__(self):
        super().__init__()
        self.names, self.ptrs = [], []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v):
            return v
        names, ptrs = object.__getattribute__(self, "names"), object.__getattribute__(self, "ptrs")

        def logged(*a, **k):
            names.append(name)
            flat_args = list(a) + list(k.values())
            flat_args += [x for d in flat_args if isinstance(d, dict) for x in d.values()]
            ptrs.append((name, {x.data_ptr() for x in flat_args if torch.is_tensor(x)}))
            return v(*a, **k)
        return logged


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def mixed(model):
    """a table with every case: frozen, slower, faster, untouched"""
    names = list(model.arena.entries)
    tab = {"lstm/recurrent_kernel": 0.0, "time_distributed_softmax/bias": 0.0, "lstm/kernel": 0.1, "emb_text/embeddings": 10.0,
           "time_distributed_softmax/kernel": 0.5}
    if "dense_img/kernel" in names:         # the variable whose update may be the encoder's fused one: a scalar multiplier
        tab["dense_img/kernel"] = 2.0
    assert set(tab) <= set(names) and len(tab) < len(names)
    return tab


def atol_of(k, step):
    return 3e-3 * (step + 1) if k == "attention/V/bias" else (2e-5 if k == "dense_img/bias" else 3e-6)


# ---------------------------------------------------------------------------------------------------- names and values
@pytest.mark.parametrize("make", [dense, attention])
def test_names_values_and_surface(make):
    model = make()
    every = list(model.arena.entries)
    assert model.trainable_names() == [n for n in model.keras_shapes if "moving_" not in n]
    assert set(model.non_trainable_names()) == {n for n in model.keras_shapes if "moving_" in n}
    assert list(model.lr_multipliers()) == every and set(model.lr_multipliers().values()) == {1.0}
    for bad in (-1, -0.0001, float("nan"), float("inf"), True, "2", None, [1.0]):
        with pytest.raises(ValueError):
            model.set_lr_multipliers({"lstm": bad})
    for bad in ("no_such_layer", "", 3):
        with pytest.raises(ValueError):
            model.freeze(bad)
        with pytest.raises(ValueError):
            model.set_lr_multipliers({bad: 0.5})
    with pytest.raises(ValueError):
        model.set_lr_multipliers([("lstm", 0.5)])
    assert set(model.lr_multipliers().values()) == {1.0} and model.seg_lrm is None          # a refused call changes nothing
    count = model.count_params()
    model.freeze("lstm")                                                     # a layer name: its variables
    assert [n for n in model.non_trainable_names() if "moving_" not in n] == list(LSTM)
    assert not set(LSTM) & set(model.trainable_names()) and not model.get_layer("lstm").trainable
    assert [n for n, _ in model.trainable_variables] == model.trainable_names()
    model.set_lr_multipliers({"bias": 0.25})                                 # a substring: every bias, the frozen one too
    biases = [n for n in every if "bias" in n]
    assert len(biases) >= 3 and all(model.lr_multipliers()[n] == 0.25 for n in biases)
    assert model.lr_multipliers()["lstm/kernel"] == 0.0 and model.get_layer("lstm").trainable
    model.set_lr_multipliers({"time_distributed_softmax/kernel": 0})         # an exact name; 0 is freeze
    assert "time_distributed_softmax/kernel" in model.non_trainable_names()
    with pytest.raises(ValueError, match="frozen"):
        model.get_gradient("time_distributed_softmax/kernel")
    with pytest.raises(ValueError, match="frozen"):
        model.unfreeze("emb_text")                                           # not frozen
    model.unfreeze("time_distributed_softmax/kernel", multiplier=0.1)
    assert model.lr_multipliers()["time_distributed_softmax/kernel"] == np.float32(0.1)
    layer = model.get_layer("emb_text")
    layer.trainable = False
    assert not layer.trainable and "emb_text/embeddings" in model.non_trainable_names()
    layer.trainable = True
    assert layer.trainable and model.lr_multipliers()["emb_text/embeddings"] == 1.0
    with pytest.raises(ValueError):
        layer.trainable = 0
    assert model.count_params() == count
    lines = []
    model.summary(print_fn=lines.append)
    size = lambda names: int(sum(np.prod(model.keras_shapes[n]) for n in names))
    assert f"Trainable params: {size(model.trainable_names()):,d}" in lines
    assert f"Non-trainable params: {size(model.non_trainable_names()):,d}" in lines
    assert size(model.trainable_names()) + size(model.non_trainable_names()) == count


def test_batchnorm_is_refused_and_layernorm_freezes():
    model = dense()
    for how in (lambda: model.freeze("batch_norm"), lambda: model.freeze("batch_norm/gamma"), lambda: model.freeze("gamma"),
                lambda: model.set_lr_multipliers({"batch_norm/beta": 0}),
                lambda: model.compile(Adam(1e-3, **ADAM_CLIP), freeze=["batch_norm"])):
        with pytest.raises(NotImplementedError, match="BatchNorm"):
            how()
    assert set(model.lr_multipliers().values()) == {1.0}
    model.set_lr_multipliers({"batch_norm": 0.5})                            # a multiplier other than 0 is fine
    ln = NIC(N, U, 10, V, T, 0, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=11, norm="layer")
    ln.freeze("batch_norm")                                                  # the layer-norm variant has no moving statistics
    assert {"batch_norm/gamma", "batch_norm/beta"} <= set(ln.non_trainable_names())


def test_config_keys_through_compile():
    model = dense()
    model.compile(Adam(1e-3, **ADAM_CLIP), freeze=["lstm", "emb_text"], lr_multipliers={"dense_img": 2.0})
    mul = model.lr_multipliers()
    assert all(mul[n] == 0.0 for n in LSTM + ("emb_text/embeddings",)) and mul["dense_img/kernel"] == 2.0
    assert mul["time_distributed_softmax/kernel"] == 1.0
    for kw in (dict(freeze="lstm"), dict(freeze=["nothing_like_it"]), dict(lr_multipliers=[("lstm", 1.0)]),
               dict(lr_multipliers={"lstm": -1})):
        with pytest.raises(ValueError):
            dense().compile(Adam(1e-3, **ADAM_CLIP), **kw)
    # ... and through config.build_model, from a config that carries the two keys
    from masters_thesis_amd import config as cfg
    from helpers import tiny_groups
    from test_host_weight_decay import LC
    rng = np.random.default_rng(1)
    g = (tiny_groups(LC["N"], LC["R"], rng), [LC["D"]] * LC["R"])
    base = dict(units=LC["U"], embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], top_k=LC["V"] - 1,
                max_length=LC["T"], dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0,
                dropout_out=0, input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3,
                clipnorm=0.1, decay=0)
    assert set(cfg.build_model(base, g, device="cpu").lr_multipliers().values()) == {1.0}
    built = cfg.build_model({**base, "freeze": ["lstm", "emb_text"], "lr_multipliers": {"attention": 0.5}}, g, device="cpu")
    mul = built.lr_multipliers()
    assert all(mul[n] == 0.0 for n in LSTM + ("emb_text/embeddings",)) and not built.get_layer("lstm").trainable
    assert mul["attention/W1/kernel"] == 0.5 and mul["time_distributed_softmax/kernel"] == 1.0
    for bad in (dict(freeze="lstm"), dict(freeze=["nothing_like_it"]), dict(lr_multipliers={"lstm": -1}),
                dict(freeze=["input_bn"])):
        with pytest.raises((ValueError, NotImplementedError)):
            cfg.build_model({**base, **bad}, g, device="cpu")


# ---------------------------------------------------------------------------------------------------- refusals
def test_data_parallel_refuses():
    model = dense()
    model.compile(Adam(1e-3, **ADAM_CLIP))
    model.freeze("lstm")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.attach(model, world=1, rank=0)
    assert model.grad_sync is None
    other = dense()
    hook = lambda m: None
    hook.world = 2
    other.grad_sync = hook
    other.compile(Adam(1e-2, clipnorm=0.1))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        other.freeze("lstm")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        other.compile(Adam(1e-2, clipnorm=0.1), lr_multipliers={"lstm": 0.5})
    other.compile(Adam(1e-2, clipnorm=0.1), lr_multipliers={"lstm": 1.0})       # multipliers of 1 make no table: nothing to refuse
    assert set(other.lr_multipliers().values()) == {1.0}


def test_agc_refuses():
    model = dense()
    model.compile(Adam(1e-3, **ADAM_CLIP))
    model.set_lr_multipliers({"lstm": 0.5})
    with pytest.raises(NotImplementedError, match="enable_agc"):
        model.enable_agc(0.02, 1e-3)
    other = dense()
    other.compile(Adam(1e-3, **ADAM_CLIP))
    other.enable_agc(0.02, 1e-3)
    with pytest.raises(NotImplementedError, match="enable_agc"):
        other.freeze("lstm")
    assert set(other.lr_multipliers().values()) == {1.0}


def test_sam_refuses():
    model = attention()
    model.compile(Adam(1e-3, **ADAM_CLIP))
    model.freeze("lstm")
    model.train_step(batch(model))
    with pytest.raises(NotImplementedError, match="train_step_sam"):
        model.train_step_sam(batch(model))
    model.unfreeze("lstm")
    model.train_step_sam(batch(model))


def test_gradient_accumulation_refuses():
    model = dense()
    model.freeze("lstm")
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        model.compile(Adam(1e-3, **ADAM_CLIP, gradient_accumulation_steps=2))
    other = dense()
    other.compile(Adam(1e-3, **ADAM_CLIP, gradient_accumulation_steps=2))
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        other.freeze("lstm")
    third = dense()
    opt = Adam(1e-3, **ADAM_CLIP)
    third.compile(opt)
    third.freeze("lstm")
    third.train_step(batch(third))
    opt.gradient_accumulation_steps = 2                                      # assigned behind a recorded step: found by the next
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        third.train_step(batch(third))


# ---------------------------------------------------------------------------------------------------- routes
ROUTES = {
    "dense fused": (lambda: dense(), lambda: Adam(1e-3, **ADAM_CLIP)),
    "dense fused_update=False": (lambda: dense(fused_update=False), lambda: Adam(1e-3, **ADAM_CLIP)),
    "dense SGD": (lambda: dense(), lambda: SGD(1e-3, momentum=0.9, clipnorm=0.1)),
    "dense SGD decay": (lambda: dense(fused_update=False), lambda: SGD(1e-3, momentum=0.9, clipnorm=0.1, weight_decay=WD)),
    "dense AdamW": (lambda: dense(), lambda: AdamW(1e-3, WD, **ADAM_CLIP)),
    "dense global clip": (lambda: dense(), lambda: Adam(1e-3, **ADAM, global_clipnorm=C)),
    "dense encoder update": (lambda: dense(E=512), lambda: Adam(1e-3, **ADAM_CLIP)),
    "attention fused": (lambda: attention(), lambda: Adam(1e-3, **ADAM_CLIP)),
    "attention fused_update=False": (lambda: attention(fused_update=False), lambda: AdamW(1e-3, WD, **ADAM, global_clipnorm=C)),
    "attention SGD": (lambda: attention(), lambda: SGD(1e-3, momentum=0.9, clipnorm=0.1)),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_issues_the_lrmul_call_where_the_plain_one_was(route, mock_backend):
    make, opt = ROUTES[route]
    runs = {}
    for case in ("plain", "ones", "table"):
        model = make()
        model.compile(opt())
        if case == "ones":
            model.set_lr_multipliers({"lstm": 1.0, "bias": 1})               # multipliers of 1: no table, nothing changes
        if case == "table":
            model.skip_frozen_work = False
            model.set_lr_multipliers({"time_distributed_softmax/bias": 0.5, "lstm/bias": 0.0})
        mock_backend.names.clear()
        for s in (3, 4):
            model.train_step(batch(model, seed=s))
        runs[case] = list(mock_backend.names)
        assert (model.seg_lrm is not None) == (case == "table")
    assert runs["ones"] == runs["plain"] and not any(n.endswith("_lrmul") for n in runs["plain"])
    want = [LRMUL.get(n, n) for n in runs["plain"]]
    if route == "dense encoder update":
        # the fused update stays, at the variable's multiplier as a scalar
        assert "dense_dw_adam" in runs["plain"] and runs["table"].count("dense_dw_adam_lrmul") == 2
    assert runs["table"] == want, (route, runs["table"])
    assert any(n.endswith("_lrmul") for n in runs["table"])


# ---------------------------------------------------------------------------------------------------- against float64
def optimizer_pair(kind, orc):
    """(the library's descriptor, the oracle's arguments)"""
    if kind == "adam":
        return Adam(1e-3, **ADAM_CLIP), dict(kind="adam", clipnorm=0.1)
    if kind == "adamw-gclip":
        opt = AdamW(1e-3, WD, **ADAM, global_clipnorm=C)
        opt.exclude_from_weight_decay(var_names=["bias"])
        return opt, dict(kind="adam", global_clipnorm=C, wd=decay_of(orc.p, WD, substrings=["bias"]))
    return SGD(1e-3, momentum=0.9, clipnorm=0.1), dict(kind="sgd", clipnorm=0.1, momentum=0.9)


@pytest.mark.parametrize("kind", ["adam", "adamw-gclip", "sgd"])
@pytest.mark.parametrize("make", [dense, attention, lambda: dense(E=512), lambda: dense(fused_update=False)],
                         ids=["dense", "attention", "dense-wide-encoder", "dense-unfused"])
def test_three_steps_match_the_float64_oracle_with_a_mixed_table(make, kind, mock_backend):
    model = make()
    orc = model.orc
    opt, okw = optimizer_pair(kind, orc)
    model.compile(opt)
    tab = mixed(model)
    model.set_lr_multipliers(tab)
    state = FinetuneState(orc.p, lr=1e-3, mul=tab, **okw)
    frozen = [n for n, m in tab.items() if m == 0.0]
    start = {n: model.get_weight(n) for n in frozen}
    rng = np.random.default_rng(5)
    for step in range(3):
        data, tgt = synth_batch(*model.dims, rng)
        res, _, _ = orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        got = model.train_step((data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) < 3e-5 * max(1, abs(res["loss"])), (step, got, res)
        if kind == "adamw-gclip":
            assert state.norm >= 2 * C
            assert abs(model.global_grad_norm() - state.norm) <= 2e-4 * state.norm, (step, model.global_grad_norm(), state.norm)
        for k, v in orc.p.items():
            w = model.get_weight(k)
            assert np.allclose(w, v, rtol=2e-4, atol=atol_of(k, step)), (kind, step, k, np.abs(w - v).max())
    for n in frozen:                                                         # bit for bit, with both optimizer slots
        assert np.array_equal(model.get_weight(n), start[n]), n
        assert not model.get_optimizer_slot(n, "m").any(), n
        if kind != "sgd":
            assert not model.get_optimizer_slot(n, "v").any(), n
    assert model.iterations == 3
    assert {c["name"] for c in mock_backend.lrm_calls} >= {"span_sqnorm_lrmul" if model.fused_update else "seg_sqnorm_lrmul"}


def test_gradual_unfreezing_matches_the_oracle_and_keeps_the_moments(mock_backend):
    """two steps, freeze the LSTM for two steps, unfreeze it at 0.1 for two: the global step count runs on, the frozen
    steps leave weights and moments bit for bit, the resumed steps use the old moments"""
    model = dense()
    orc = model.orc
    model.compile(Adam(1e-3, **ADAM_CLIP))
    state = FinetuneState(orc.p, lr=1e-3, kind="adam", clipnorm=0.1)
    rng = np.random.default_rng(9)
    held = None
    for step in range(6):
        if step == 2:
            model.freeze("lstm")
            state.mul = {n: 0.0 for n in LSTM}
            held = {n: (model.get_weight(n), model.get_optimizer_slot(n, "m"), model.get_optimizer_slot(n, "v")) for n in LSTM}
            assert all(h[1].any() and h[2].any() for h in held.values())
        if step == 4:
            for n in LSTM:
                for got, want in zip((model.get_weight(n), model.get_optimizer_slot(n, "m"), model.get_optimizer_slot(n, "v")),
                                     held[n]):
                    assert np.array_equal(got, want), n
            model.unfreeze("lstm", multiplier=0.1)
            state.mul = {n: 0.1 for n in LSTM}
        data, tgt = synth_batch(*model.dims, rng)
        orc.train_step(data, tgt, state, M.DropCtx(seed=11, step=step, training=True))
        model.train_step((data, tgt))
        for k, v in orc.p.items():
            w = model.get_weight(k)
            assert np.allclose(w, v, rtol=2e-4, atol=atol_of(k, step)), (step, k, np.abs(w - v).max())
    assert model.iterations == 6 and state.t == 6


# ---------------------------------------------------------------------------------------------------- recordings
def test_a_toggle_keeps_the_recordings_and_a_first_or_last_multiplier_drops_them(mock_backend):
    model = dense()
    model.skip_frozen_work = False          # (with skipping, a change of the frozen set changes the launches: see below)
    model.compile(Adam(1e-3, **ADAM_CLIP))
    model.train_step(batch(model))
    model._graphs["sentinel"] = 1
    model.set_lr_multipliers({"lstm": 1.0})                                  # still no table
    assert "sentinel" in model._graphs and model.seg_lrm is None
    model.set_lr_multipliers({"lstm": 0.5})                                  # the first multiplier: other launches
    assert "sentinel" not in model._graphs and model.seg_lrm is not None
    model.train_step(batch(model, seed=4))
    model._graphs["sentinel"] = 1
    table = model.seg_lrm
    for change in ({"lstm": 0.0}, {"lstm/kernel": 2.0}, {"emb_text": 0.0, "lstm": 0.25}):
        model.set_lr_multipliers(change)
        assert "sentinel" in model._graphs and model.seg_lrm is table         # written in place
        want = [model.lr_multipliers()[n] for n in model.arena.entries]
        assert model.seg_lrm.tolist() == want and model.seg_lrm_host.tolist() == want
        model.train_step(batch(model, seed=5))
    model.set_lr_multipliers({n: 1.0 for n in model.arena.entries})          # the last one gone: the plain launches again
    assert "sentinel" not in model._graphs and model.seg_lrm is None
    mock_backend.names.clear()
    model.train_step(batch(model, seed=6))
    assert "adam" in mock_backend.names and not any(n.endswith("_lrmul") for n in mock_backend.names)
    # with skipping on, the frozen set decides the launches: a change of it drops the recordings, another multiplier does not
    other = dense()
    other.compile(Adam(1e-3, **ADAM_CLIP))
    other.set_lr_multipliers({"lstm": 0.5})
    other.train_step(batch(other))
    other._graphs["sentinel"] = 1
    other.set_lr_multipliers({"lstm": 0.25})
    assert "sentinel" in other._graphs
    other.freeze("lstm")
    assert "sentinel" not in other._graphs


# ---------------------------------------------------------------------------------------------------- dead work
SKIPS = {
    "head": (HEAD, dense),
    "lstm": (LSTM, dense),
    "embedding": (("emb_text/embeddings",), dense),
    "encoder": (("dense_img/kernel",), dense),
    "encoder wide": (("dense_img/kernel",), lambda **k: dense(E=512, **k)),
    "decoder": (HEAD + LSTM + ("emb_text/embeddings",), dense),
    "attention head": (HEAD, attention),
    "attention lstm": (LSTM, attention),
    "attention embedding": (("emb_text/embeddings",), attention),
}
# the launches that walk the whole arena: they take the gradient buffer's base address, which is also the first variable's
WHOLE_ARENA = {"span_sqnorm_lrmul", "seg_sqnorm_lrmul", "adam_lrmul", "sgd_lrmul", "step_finalize", "global_sqnorm_lrmul"}


@pytest.mark.parametrize("case", sorted(SKIPS))
def test_a_frozen_variable_has_no_gradient_launch_and_the_rest_trains_the_same(case, mock_backend):
    names, make = SKIPS[case]
    runs = {}
    for skip in (True, False):
        model = make(skip_frozen_work=skip)
        model.compile(Adam(1e-3, **ADAM_CLIP))
        model.freeze(*names)
        a = model.arena
        if skip:
            for n in names:
                a.g(n).fill_(float("nan"))          # stale: whatever reads it poisons a norm, a metric or a weight
        mock_backend.ptrs.clear()
        mets = [model.train_step(batch(model, seed=s)).as_floats() for s in (3, 4)]
        grads = {a.g(n).data_ptr() for n in names}
        writers = [nm for nm, ptrs in mock_backend.ptrs if nm not in WHOLE_ARENA and ptrs & grads]
        if case == "attention head":
            # the softmax bias gradient rides in the nonlinear layer's bias / activation launch, which is still needed
            assert set(writers) <= ({"bias_act_drop_bwd", "colsum"} if skip else set(writers))
        elif skip:
            assert not writers, (case, writers)
        else:
            assert writers, case                    # the same run without skipping does form them
        if skip:
            for n in names:
                assert torch.isnan(a.g(n)).all() or case == "attention head", n
        assert all(np.isfinite(list(m.values())).all() for m in mets)
        runs[skip] = (mets, {n: model.get_weight(n) for n in a.entries}, len(mock_backend.ptrs))
    for (ma, mb) in zip(runs[True][0], runs[False][0]):
        assert ma == mb
    for n in runs[True][1]:
        assert np.array_equal(runs[True][1][n], runs[False][1][n]), n
    assert runs[True][2] < runs[False][2] or case in ("attention head",)


# ---------------------------------------------------------------------------------------------------- the transfer journey
def test_transfer_to_another_subject(tmp_path, mock_backend):
    """train A (N voxels), save; B has another voxel count: load what fits, freeze the decoder, train the encoder"""
    A = dense()
    A.compile(Adam(1e-3, **ADAM_CLIP))
    for s in (3, 4, 5):
        A.train_step(batch(A, seed=s))
    path = tmp_path / "subject_a.npz"
    A.save_weights(path)
    N2 = N + 9
    Bm = NIC(N2, U, 10, V, T, 0, 0.2, 0.2, 0.01, 3e-5, 1e-5, device="cpu", seed=12)
    before = {n: Bm.get_weight(n) for n in Bm.keras_shapes}
    with pytest.raises(ValueError, match="shape mismatch"):
        Bm.load_weights(path, by_name=True)
    Bm.load_weights(path, by_name=True, skip_mismatch=True)
    assert np.array_equal(Bm.get_weight("dense_img/kernel"), before["dense_img/kernel"])     # the mismatch was skipped
    Bm.compile(Adam(1e-3, **ADAM_CLIP), freeze=list(DECODER))
    decoder = [n for n in Bm.arena.entries if n.split("/")[0] in DECODER]
    assert len(decoder) == 6 and [n for n in Bm.non_trainable_names() if "moving_" not in n] == decoder
    rng = np.random.default_rng(8)
    for _ in range(3):
        m = Bm.train_step(synth_batch(B, N2, T, V, U, rng)).as_floats()
        assert np.isfinite(m["loss"])
    for n in decoder:
        assert np.array_equal(Bm.get_weight(n), A.get_weight(n)), n           # bit for bit subject A's decoder
    for n in ("dense_img/kernel", "dense_img/bias", "batch_norm/gamma"):
        assert not np.array_equal(Bm.get_weight(n), before[n]), n             # the encoder trained
    Bm.unfreeze(*DECODER, multiplier=0.1)                                    # later: the decoder at a small rate
    Bm.train_step(synth_batch(B, N2, T, V, U, rng))
    assert not np.array_equal(Bm.get_weight("lstm/kernel"), A.get_weight("lstm/kernel"))
