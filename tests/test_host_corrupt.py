"""Scan dropout and word dropout (``scan_dropout=`` / ``word_dropout=`` of nic.NIC and lc_nic.NIC) on the CPU through a mock
backend that follows tnt_input_corrupt_f32's header definition (tests/corrupt_oracle.py): the descriptors and the config
keys, the launch sequence of each staging route (the corrupt call once, directly behind the staging; never in test_step,
__call__, a decode or score_captions; the stage_fwd ride declined only under scan dropout), train_step_sam's one call for
its two passes, every refusal, a neutral or None model against today's calls and keys, an assigned rate against the
recordings, Guidance(null=None) against null_scan, and three training steps of both tiny models against the float64
oracle step fed the restated corrupted batch (the host tests' tolerance, rtol 2e-4)."""
import copy

import numpy as np
import pytest
import torch

import masters_thesis_amd.ops as ops
from masters_thesis_amd import config as cfg
from masters_thesis_amd import dp
from masters_thesis_amd.fc_nic import NICfc
from masters_thesis_amd.lc_nic import NIC as LcNIC
from masters_thesis_amd.model_base import (Guidance, S_SCAN_DROP, S_WORD_DROP, ScanDropout, ScheduledSampling as SS,
                                           SelfCritical, WordDropout)
from masters_thesis_amd.ms_nic import NIC as MsNIC
from masters_thesis_amd.nic import NIC
from masters_thesis_amd.optimizers import Adam
from oracle import models as M
import corrupt_oracle as CO
from helpers import synth_batch, tiny_groups
from score_oracle import ScoreMockBackend
from test_host_guidance import GuidanceMockBackend
from test_host_weight_decay import ADAM, LC, B, N, T, U, V, attention, batch, dense

SEED = 11                   # the seed of the tiny models (test_host_weight_decay.dense / attention)
STAGING = ("stage_batch", "stage_batch_map", "dense_fwd_stream_gram_stage")


class RecordingBackend(CO.CorruptMockBackend, GuidanceMockBackend, ScoreMockBackend):
    """the mock with every public call logged in ``calls`` as (name, args, kwargs)"""

    def __init__(self):
        self.calls = []
        super().__init__()

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(v):
            return v
        calls = object.__getattribute__(self, "calls")

        def logged(*a, **k):
            calls.append((name, a, k))
            return v(*a, **k)
        return logged

    @property
    def names(self):
        """the launches: the size queries of the buffer builds (bn_nchunk, *_work_floats, *_parts, *_supported) left out"""
        query = lambda n: n == "bn_nchunk" or n.endswith(("_work_floats", "_parts", "_supported"))
        return [c[0] for c in self.calls if not query(c[0])]


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    be = RecordingBackend()
    ops.set_backend(be)
    yield be
    ops.set_backend(old)


def null_of(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def on_device(data, tgt):
    """the batch as the one-launch staging route takes it: contiguous tensors in the staged dtypes"""
    x, cap, a0, c0 = data
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    return (t(x, torch.float32), t(cap, torch.int32), t(a0, torch.float32), t(c0, torch.float32)), t(tgt, torch.int32)


def make(kind, **kw):
    return dense(**kw) if kind == "dense" else attention(**kw)


# ---------------------------------------------------------------------------------------------------- descriptors, config
def test_the_sites_are_free():
    from masters_thesis_amd import lc_nic, model_base as mb
    assert (S_SCAN_DROP, S_WORD_DROP) == (241, 242) == (CO.S_SCAN_DROP, CO.S_WORD_DROP)
    taken = set()
    for base, n in ((mb.S_ATTN, 32), (mb.S_LSTM_IN, 32), (mb.S_LSTM_OUT, 32), (mb.S_SAMPLE, 32), (lc_nic.S_NOUT, 32),
                    (mb.S_SS_COIN, 32), (mb.S_SS_DRAW, 32), (mb.S_SCST_LAST, 1), (lc_nic.S_DEEP, 10)):
        taken |= set(range(base, base + n))
    taken |= {mb.S_IN, mb.S_FEAT, mb.S_TEXT, mb.S_OUT, lc_nic.S_FEAT2}
    assert not taken & {S_SCAN_DROP, S_WORD_DROP}


def test_descriptors_validate():
    s = ScanDropout(0.25, [1.0, 2.0, 3.0])
    assert s.rate == 0.25 and s.null.dtype == np.float32 and s.null.tolist() == [1.0, 2.0, 3.0] and not s.neutral
    assert ScanDropout(0).neutral and ScanDropout(0.0, np.ones(4)).neutral and ScanDropout(1).rate == 1.0
    assert ScanDropout(np.float32(0.5)).rate == 0.5 and ScanDropout(0.5).null is None
    assert ScanDropout(0.5, torch.ones(3)).null.tolist() == [1.0] * 3
    assert repr(s) == "ScanDropout(rate=0.25, null=<array (3,)>)" and repr(ScanDropout(0.5)) == "ScanDropout(rate=0.5, null=None)"
    w = WordDropout(0.5, 3)
    assert (w.rate, w.unk_id, w.neutral) == (0.5, 3, False) and WordDropout(0, 1).neutral
    assert WordDropout(1, np.int64(2)).unk_id == 2 and repr(w) == "WordDropout(rate=0.5, unk_id=3)"
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.5", None, True, False, [0.5]):
        with pytest.raises(ValueError, match="rate"):
            ScanDropout(bad)
        with pytest.raises(ValueError, match="rate"):
            WordDropout(bad, 1)
    for bad in (np.zeros((2, 3)), np.zeros(0), [1.0, float("nan")], "zeros", 3.0, [[1.0], [2.0, 3.0]]):
        with pytest.raises(ValueError, match="null"):
            ScanDropout(0.5, bad)
    for bad in (0, -1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="unk_id"):
            WordDropout(0.5, bad)


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_keywords_are_readable_assignable_and_validated(kind, mock_backend):
    model = make(kind)
    assert model.scan_dropout is None and model.word_dropout is None and model.null_scan is None
    n_in = model._input_width()
    null = null_of(n_in)
    sd, wd = ScanDropout(0.5, null), WordDropout(0.25, V - 1)
    model.scan_dropout, model.word_dropout = sd, wd
    assert model.scan_dropout is sd and model.word_dropout is wd and np.array_equal(model.null_scan, null)
    for bad in (0.5, "x", wd):
        with pytest.raises(ValueError, match="ScanDropout"):
            model.scan_dropout = bad
    for bad in (0.5, "x", sd):
        with pytest.raises(ValueError, match="WordDropout"):
            model.word_dropout = bad
    with pytest.raises(ValueError, match="vocab_size"):
        model.word_dropout = WordDropout(0.5, V)
    with pytest.raises(ValueError, match="input width"):
        model.scan_dropout = ScanDropout(0.5, null_of(n_in + 1))
    assert model.scan_dropout is sd and model.word_dropout is wd                # a refused assignment changes nothing
    model.scan_dropout = ScanDropout(0.5)
    assert model.null_scan is None
    model.scan_dropout = model.word_dropout = None
    assert model.scan_dropout is None and model.word_dropout is None
    assert mock_backend.names == []
    # the constructor takes them, and validates the same way
    args = (N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5)
    m = NIC(*args, device="cpu", scan_dropout=ScanDropout(0.5, null_of(N)), word_dropout=WordDropout(0.5, 2))
    assert m.scan_dropout.rate == 0.5 and m.word_dropout.unk_id == 2 and m.null_scan.shape == (N,)
    with pytest.raises(ValueError, match="vocab_size"):
        NIC(*args, device="cpu", word_dropout=WordDropout(0.5, V))
    with pytest.raises(ValueError, match="input width"):
        NIC(*args, device="cpu", scan_dropout=ScanDropout(0.5, null_of(N - 1)))
    with pytest.raises(ValueError, match="ScanDropout"):
        NIC(*args, device="cpu", scan_dropout=0.5)


def test_models_without_the_keywords_refuse_them():
    from masters_thesis_amd.think_and_tell import CaptionGenerator
    with pytest.raises(TypeError):
        NICfc(N, U, 512, 16, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", scan_dropout=ScanDropout(0.5))
    with pytest.raises(TypeError):
        NICfc(N, U, 512, 16, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu", word_dropout=WordDropout(0.5, 1))
    fc = NICfc(N, U, 512, 16, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu")
    with pytest.raises(NotImplementedError, match="scan_dropout"):
        fc.scan_dropout = ScanDropout(0.5)
    with pytest.raises(NotImplementedError, match="word_dropout"):
        fc.word_dropout = WordDropout(0.5, 1)
    assert not CaptionGenerator.SUPPORTS_INPUT_CORRUPTION


def test_config_keys():
    rng = np.random.default_rng(1)
    g = (tiny_groups(N, LC["R"], rng), [LC["D"]] * LC["R"])
    base = dict(units=LC["U"], embedding_features=512, embedding_text=LC["Et"], attn_units=LC["A"], top_k=LC["V"] - 1,
                max_length=LC["T"], dropout_input=0, dropout_features=0, dropout_text=0, dropout_attn=0, dropout_lstm=0,
                dropout_out=0, input_reg=0.01, attn_reg=0.001, lstm_reg=3e-5, output_reg=1e-5, optimizer="Adam", alpha=1e-3,
                clipnorm=0.1, decay=0)
    g = (tiny_groups(LC["N"], LC["R"], rng), [LC["D"]] * LC["R"])
    plain = cfg.build_model(base, g, device="cpu")
    assert plain.scan_dropout is None and plain.word_dropout is None
    m = cfg.build_model({**base, "scan_dropout": 0.1, "word_dropout": {"rate": 0.25, "unk_id": 3}}, g, device="cpu")
    assert (m.scan_dropout.rate, m.scan_dropout.null) == (0.1, None) and (m.word_dropout.rate, m.word_dropout.unk_id) == (0.25, 3)
    assert cfg.build_model({**base, "scan_dropout": {"rate": 0.2}}, g, device="cpu").scan_dropout.rate == 0.2
    own = ScanDropout(0.3)
    assert cfg.build_model({**base, "scan_dropout": 0.1}, g, device="cpu", scan_dropout=own).scan_dropout is own
    for bad in (dict(scan_dropout=1.5), dict(scan_dropout={"p": 0.1}), dict(scan_dropout={"rate": 0.1, "null": 0}),
                dict(scan_dropout="0.1"), dict(word_dropout=0.25), dict(word_dropout={"rate": 0.25}),
                dict(word_dropout={"rate": 0.25, "unk_id": 0}), dict(word_dropout={"rate": 2, "unk_id": 1}),
                dict(word_dropout={"rate": 0.25, "unk_id": LC["V"]}), dict(word_dropout={"rate": 0.1, "unk_id": 1, "x": 1})):
        with pytest.raises(ValueError):
            cfg.build_model({**base, **bad}, g, device="cpu")


# ---------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("route", ["general", "one launch"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_the_call_sits_once_directly_behind_the_staging(kind, route, mock_backend):
    model = make(kind)
    n_in = model._input_width()
    null = null_of(n_in)
    model.scan_dropout, model.word_dropout = ScanDropout(0.5, null), WordDropout(0.25, 2)
    model.compile(Adam(1e-3, **ADAM))
    for step in range(2):
        data, tgt = batch(model, seed=3 + step)
        fed = on_device(data, tgt) if route == "one launch" else (data, tgt)
        mock_backend.calls.clear()
        model.train_step(fed)
        names = mock_backend.names
        assert names.count("input_corrupt") == 1, names
        i = names.index("input_corrupt")
        if route == "one launch":
            assert names[i - 1] == "stage_batch" and i == 1, names[:4]
        else:                   # the per-tensor path: torch copies (and the attention model's mask launch), no staging entry
            assert not set(names[:i]) & set(STAGING) and set(names[:i]) <= {"dropout_mask4", "onehot_argmax"}, names[:i]
        c = mock_backend.corrupt_calls[-1]
        assert (c["scan_rate"], c["word_rate"], c["unk_id"], c["step"], c["seed"]) == (0.5, 0.25, 2, step, SEED)
        assert c["sites"] == (S_SCAN_DROP, S_WORD_DROP) and np.array_equal(c["null"], null) and c["N"] == n_in
        assert c["xT"] == (model.xT is not None)
        # the staged buffers hold the restated corrupted batch
        x2, cap2, rows, words = CO.corrupt(data[0][:, :n_in], data[1], 0.5, 0.25, null, 2, SEED, step)
        assert np.array_equal(model.x.numpy()[:, :n_in], x2) and np.array_equal(model.cap.numpy(), cap2)
        if model.xT is not None:
            assert np.array_equal(model.xT.numpy()[:, :x2.shape[0]], x2.T)


@pytest.mark.parametrize("route", ["general", "one launch"])
def test_the_voxel_major_copy_is_corrupted_with_the_rows(route, mock_backend):
    """an attention model whose encoder reads the voxel-major copy (no input Dropout, n_in % 4 == 0)"""
    rng = np.random.default_rng(8)
    n = 24
    g = (tiny_groups(n, LC["R"], rng, overlap=False), [LC["D"]] * LC["R"])
    model = LcNIC(g, LC["U"], 512, LC["Et"], LC["A"], LC["V"], LC["T"], 0, 0.2, 0, 0.2, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu",
                  seed=SEED, scan_dropout=ScanDropout(0.5, null_of(n)))
    model.compile(Adam(1e-3, **ADAM))
    data, tgt = synth_batch(LC["B"], n, LC["T"], LC["V"], LC["U"], rng)
    model.train_step(on_device(data, tgt) if route == "one launch" else (data, tgt))
    assert model.xT is not None and model._input_width() == n and mock_backend.corrupt_calls[-1]["xT"]
    x2, _, rows, _ = CO.corrupt(data[0], data[1], 0.5, 0.0, null_of(n), 1, SEED, 0)
    assert rows.any() and not rows.all()
    assert np.array_equal(model.x.numpy()[:, :n], x2) and np.array_equal(model.xT.numpy()[:, :LC["B"]], x2.T)
    assert np.array_equal(model.cap.numpy(), data[1])                       # no word dropout: the ids stay


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_evaluation_decodes_and_scoring_never_corrupt(kind, mock_backend):
    model = make(kind)
    model.scan_dropout, model.word_dropout = ScanDropout(1.0, null_of(model._input_width())), WordDropout(1.0, 2)
    model.compile(Adam(1e-3, **ADAM))
    Bm, Nm, Tm, Vm, Um = model.dims
    data, tgt = batch(model)
    z, start = np.zeros((Bm, Um), np.float32), np.ones(Bm, np.int64)
    model.test_step((data, tgt))
    model.test_step(on_device(data, tgt))
    model(data, training=False)
    model(data, training=True)
    model.greedy_predict(data[0], z, z, start, Tm)
    model.sample_predict(data[0], z, z, start, Tm)
    model.beam_search(data[0], z, z, start, Tm, beam_width=2)
    model.greedy_predict(data[0], z, z, start, Tm, guidance=Guidance(1.0))
    caps = np.tile(data[1][:, None, :], (1, 2, 1))
    model.score_captions(data[0], z, z, caps)
    assert "input_corrupt" not in mock_backend.names and mock_backend.corrupt_calls == []
    model.train_step((data, tgt))
    assert mock_backend.names.count("input_corrupt") == 1


class RidingBackend(RecordingBackend):
    """the mock with the two staging riders the dense step asks for by name, as plain staging (their by-products are not
    looked at here)"""

    def stage_batch_map(self, x, x_dst, cap, cap_dst, tgt, tgt_tmajor, a0, h0, c0, c0_dst, B, T, N, ldx, U, *map_bufs):
        self.stage_batch(x, x_dst, cap, cap_dst, tgt, tgt_tmajor, a0, h0, c0, c0_dst, B, T, N, ldx, U)

    def dense_fwd_stream_gram_stage(self, x, w, part, gx_part, w2_part, B, E, N, ldw, nsplit, x_dst, ldx_dst, cap, cap_dst, tgt,
                                    tgt_dst, a0, h0, c0, c0_dst, T, U, *map_bufs):
        self.stage_batch(x, x_dst, cap, cap_dst, tgt, tgt_dst, a0, h0, c0, c0_dst, B, T, N, ldx_dst, U)
        return True


def test_the_stage_fwd_ride_is_declined_only_under_scan_dropout():
    """_stage_batch with both riders on offer (the row map and the encoder forward; the mock step never offers them, so the
    two hooks are stood in for): word dropout alone keeps the ride, scan dropout takes the separate staging launch"""
    be = RidingBackend()
    ops.set_backend(be)
    fake = tuple(torch.zeros(4) for _ in range(6))
    want = {(None, None): "dense_fwd_stream_gram_stage", (None, 0.5): "dense_fwd_stream_gram_stage",
            (0.5, None): "stage_batch_map", (0.5, 0.5): "stage_batch_map", (0.0, 0.5): "dense_fwd_stream_gram_stage"}
    for (sr, wr), staging in want.items():
        model = dense(E=16)
        model.N = model.ldx = 24                                            # (n_cols == ldx is the ride's condition)
        model.scan_dropout = None if sr is None else ScanDropout(sr)
        model.word_dropout = None if wr is None else WordDropout(wr, 2)
        model._head_map_bufs = lambda B, T: fake
        model._stage_fwd_args = lambda B: (fake[0],) * 4 + (16, 16, 16)
        data, tgt = on_device(*synth_batch(B, 24, T, V, U, np.random.default_rng(1)))
        be.calls.clear()
        model._stage_batch(data, tgt, 24, head_map=True, fwd=True, corrupt=True)
        names = [n for n in be.names if n != "stage_batch"]                 # (the stand-ins call the plain staging)
        active = bool(sr) or bool(wr)
        assert names == [staging] + (["input_corrupt"] if active else []), ((sr, wr), names)
        assert model._route.stage_fwd_done == (staging == "dense_fwd_stream_gram_stage")
        assert model._route.head_map_fresh
        # ... and an evaluation's staging (corrupt=False) rides as ever and corrupts nothing
        be.calls.clear()
        model._stage_batch(data, tgt, 24, head_map=True, fwd=True)
        assert [n for n in be.names if n != "stage_batch"] == ["dense_fwd_stream_gram_stage"]


def test_train_step_sam_issues_the_call_once_for_its_two_passes(mock_backend):
    model = attention()
    null = null_of(model._input_width())
    model.scan_dropout, model.word_dropout = ScanDropout(0.5, null), WordDropout(0.5, 2)
    model.compile(Adam(1e-3, **ADAM))
    data, tgt = batch(model)
    model.train_step_sam((data, tgt))
    names = mock_backend.names
    assert names.count("input_corrupt") == 1 and names.count("sam") == 2
    assert names.index("input_corrupt") < min(i for i, n in enumerate(names) if n not in ("dropout_mask4", "input_corrupt"))
    x2, cap2, rows, words = CO.corrupt(data[0], data[1], 0.5, 0.5, null, 2, SEED, 0)
    assert rows.any() and not rows.all() and words.any()
    assert np.array_equal(model.x.numpy()[:, :x2.shape[1]], x2) and np.array_equal(model.cap.numpy(), cap2)


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_refusal(mock_backend):
    rng = np.random.default_rng(2)
    on = (dict(scan_dropout=ScanDropout(0.5)), dict(word_dropout=WordDropout(0.5, 2)))
    g = (tiny_groups(LC["N"], LC["R"], rng), [LC["D"]] * LC["R"])
    lc_args = (g, LC["U"], 512, LC["Et"], LC["A"], LC["V"], LC["T"], 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5)
    nic_args = (N, U, 16, V, T, 0, 0, 0, 0.01, 3e-5, 1e-5)
    hook = lambda m: None
    for kw in on:
        for mode, what in ((dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                           (dict(self_critical=SelfCritical(2)), "self_critical"),
                           (dict(grad_sync=hook), "data-parallel")):
            with pytest.raises(NotImplementedError, match=what):
                NIC(*nic_args, device="cpu", **mode, **kw)
        for mode, what in ((dict(scheduled_sampling=SS.linear(0.5, 0.0)), "scheduled_sampling"),
                           (dict(teacher_forcing=False), "teacher_forcing"),
                           (dict(n_subjects=2), "n_subjects"),
                           (dict(grad_sync=hook), "data-parallel")):
            with pytest.raises(NotImplementedError, match=what):
                LcNIC(*lc_args, device="cpu", **mode, **kw)
        with pytest.raises(NotImplementedError, match="n_subjects"):
            MsNIC(*lc_args, device="cpu", **kw)
    with pytest.raises(ValueError, match="vocab_size"):
        LcNIC(*lc_args, device="cpu", word_dropout=WordDropout(0.5, LC["V"]))
    with pytest.raises(ValueError, match="input width"):
        LcNIC(*lc_args, device="cpu", scan_dropout=ScanDropout(0.5, null_of(LC["N"] + 1)))
    # assigned onto a model of such a mode, and a mode attached behind the constructor's back
    ss = NIC(*nic_args, device="cpu", scheduled_sampling=SS.linear(0.5, 0.0))
    with pytest.raises(NotImplementedError, match="scheduled_sampling"):
        ss.word_dropout = WordDropout(0.5, 2)
    for kind in ("dense", "attention"):
        for kw in on:
            model = make(kind)
            model.compile(Adam(1e-3, **ADAM))
            for k, v in kw.items():
                setattr(model, k, v)
            with pytest.raises(NotImplementedError, match="data-parallel"):
                dp.attach(model, world=1, rank=0)
            assert model.grad_sync is None
            model.grad_sync = hook
            with pytest.raises(NotImplementedError, match="data-parallel"):
                model.train_step(batch(model))
            if kind == "attention":
                with pytest.raises(NotImplementedError, match="data-parallel"):
                    model.train_step_sam(batch(model))
    assert mock_backend.names == []                                         # nothing was launched by any of them
    # neutral settings refuse nothing
    NIC(*nic_args, device="cpu", scheduled_sampling=SS.linear(0.5, 0.0), scan_dropout=ScanDropout(0), word_dropout=WordDropout(0, 1))
    MsNIC(*lc_args, device="cpu", scan_dropout=ScanDropout(0.0), word_dropout=WordDropout(0.0, 1))
    m = make("dense")
    m.scan_dropout, m.word_dropout = ScanDropout(0.0), WordDropout(0.0, 1)
    m.grad_sync = hook
    m._corrupt_check()


# ---------------------------------------------------------------------------------------------------- neutral, assignment
def norm(x):
    """a call argument by value; a tensor by shape and dtype (two models own different buffers)"""
    if isinstance(x, torch.Tensor):
        return ("tensor", tuple(x.shape), str(x.dtype))
    if isinstance(x, (tuple, list)):
        return tuple(norm(y) for y in x)
    if isinstance(x, dict):
        return tuple(sorted((k, norm(v)) for k, v in x.items()))
    return x


def capture_keys(model):
    keys = []
    for name in ("_run_captured", "_run_planned"):
        run = getattr(model, name)
        setattr(model, name, lambda key, fn, run=run: (keys.append(key), run(key, fn))[1])
    return keys


@pytest.mark.parametrize("setting", ["None", "neutral", "set and taken back"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_a_neutral_model_issues_the_calls_keys_and_bits_of_today(kind, setting, mock_backend):
    runs = {}
    for which in ("plain", setting):
        model = make(kind)
        if which == "neutral":
            model.scan_dropout, model.word_dropout = ScanDropout(0.0, null_of(model._input_width())), WordDropout(0, 2)
        elif which == "set and taken back":
            model.scan_dropout, model.word_dropout = ScanDropout(0.5), WordDropout(0.5, 2)
            model.scan_dropout = model.word_dropout = None
        model.compile(Adam(1e-3, **ADAM))
        keys = capture_keys(model)
        mock_backend.calls.clear()
        mets = []
        for s in (3, 4):
            d = batch(model, seed=s)
            mets.append(model.train_step(on_device(*d) if s == 4 else d).as_floats())
        mets.append(model.test_step(batch(model, seed=5)).as_floats())
        runs[which] = ([(n, norm(a), norm(k)) for n, a, k in mock_backend.calls], list(keys), mets, model.arena.theta.clone())
    a, b = runs["plain"], runs[setting]
    assert "input_corrupt" not in [c[0] for c in b[0]]
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3])
    assert a[1], "no step key was seen"


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_assigning_a_rate_keeps_the_recordings(kind, mock_backend):
    model = make(kind)
    model.scan_dropout, model.word_dropout = ScanDropout(0.5), WordDropout(0.5, 2)
    model.compile(Adam(1e-3, **ADAM))
    model.train_step(batch(model))
    model._graphs["sentinel"] = 1
    model.scan_dropout, model.word_dropout = ScanDropout(0.25), WordDropout(0.75, 3)
    model.train_step(batch(model, seed=4))
    c = mock_backend.corrupt_calls[-1]
    assert "sentinel" in model._graphs and (c["scan_rate"], c["word_rate"], c["unk_id"], c["step"]) == (0.25, 0.75, 3, 1)
    model.scan_dropout = model.word_dropout = None
    mock_backend.calls.clear()
    model.train_step(batch(model, seed=5))
    assert "sentinel" in model._graphs and "input_corrupt" not in mock_backend.names


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_guidance_without_a_null_decodes_against_null_scan(kind, mock_backend):
    model = make(kind)
    Bm, Nm, Tm, Vm, Um = model.dims
    n_in = model._input_width()
    x = np.random.default_rng(3).standard_normal((Bm, n_in)).astype(np.float32)
    z = np.zeros((Bm, Um), np.float32)
    null, other = null_of(n_in), null_of(n_in, seed=6)
    slab = lambda g: model._guidance(g, x, z, z, Bm)[1][Bm:]
    assert np.array_equal(slab(Guidance(1.0)), np.zeros_like(x))            # a model without it: the zeros of today
    model.scan_dropout = ScanDropout(0.5)
    assert model.null_scan is None and np.array_equal(slab(Guidance(1.0)), np.zeros_like(x))
    model.scan_dropout = ScanDropout(0.0, null)                             # the rate does not matter to a decode
    assert np.array_equal(slab(Guidance(1.0)), np.tile(null, (Bm, 1)))
    assert np.array_equal(slab(Guidance(1.0, other)), np.tile(other, (Bm, 1)))     # an explicit null wins
    # through a decode: the null slab of the staged scans
    model.greedy_predict(x, z, z, np.ones(Bm, np.int64), Tm, guidance=Guidance(1.0))
    assert np.array_equal(model.x.numpy()[Bm:2 * Bm, :n_in], np.tile(null, (Bm, 1)))
    assert np.array_equal(model.x.numpy()[:Bm, :n_in], x)


# ---------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("route", ["general", "one launch"])
@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_three_steps_match_the_oracle_on_the_restated_batch(kind, route, mock_backend):
    model = make(kind)
    n_in = model._input_width()
    null = null_of(n_in)
    model.scan_dropout, model.word_dropout = ScanDropout(0.5, null), WordDropout(0.5, 1)
    model.compile(Adam(1e-3, **ADAM))
    orc = model.orc
    state = M.AdamState(orc.p, lr=1e-3, clipnorm=0.1)
    twin = copy.deepcopy(orc)
    rng = np.random.default_rng(5)
    caps = []
    for step in range(3):
        data, tgt = synth_batch(*model.dims, rng)
        fed, rows, words = CO.corrupt_batch(data, 0.5, 0.5, null, 1, SEED, step)
        elig = data[1] != 0
        elig[:, 0] = False
        assert rows.any() and not rows.all() and words.any() and (elig & ~words).any(), step
        res, _, _ = orc.train_step(fed, tgt, state, M.DropCtx(seed=SEED, step=step, training=True))
        got = model.train_step(on_device(data, tgt) if route == "one launch" else (data, tgt)).as_floats()
        assert abs(got["loss"] - res["loss"]) < 3e-5 * max(1, abs(res["loss"])), (step, got, res)
        assert abs(got["accuracy"] - res["accuracy"]) < 1e-6
        for k, v in orc.p.items():
            w = model.get_weight(k)
            atol = 3e-3 * (step + 1) if k == "attention/V/bias" else (2e-5 if k == "dense_img/bias" else 3e-6)
            assert np.allclose(w, v, rtol=2e-4, atol=atol), (step, k, np.abs(w - v).max())
        caps.append(model.cap.numpy().copy())
        if step == 0:
            first = {k: model.get_weight(k).copy() for k in orc.p}
    # an oracle step on the clean batch is told apart by the same weight comparison
    data, tgt = synth_batch(*model.dims, np.random.default_rng(5))
    twin.train_step(data, tgt, M.AdamState(twin.p, lr=1e-3, clipnorm=0.1), M.DropCtx(seed=SEED, step=0, training=True))
    assert sum(not np.allclose(first[k], v, rtol=2e-4, atol=3e-6) for k, v in twin.p.items()) >= 3
    assert not np.array_equal(caps[0], caps[1])
