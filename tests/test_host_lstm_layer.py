"""lstm_layer.lstm_layer_fwd / lstm_layer_bwd on a recording backend: the step launches of every form a model uses, argument
for argument, and the one chain launch.  S = 3 steps, B = 2 rows, U = 16 units.

A tensor argument is named by its buffer: "xz[1]" is the slab of step 1 ([B][U][4] of xz, [B][U] of hs / cs / out / dout),
a bare name the whole buffer.  The argument order is that of ops.HipBackend's methods."""
import inspect

import pytest
import torch

from masters_thesis_amd.lstm_layer import lstm_layer_fwd, lstm_layer_bwd, lstm_layer_step_fwd
from masters_thesis_amd.ops import HipBackend

S, B, U = 3, 2, 16


class Recorder:
    """records (method, arguments bound to HipBackend's signature); with ``chain`` it also has the chain entry points"""

    def __init__(self, bufs, chain=False):
        self.calls, self.bufs = [], bufs
        self.methods = ("lstm_step_fwd", "lstm_step_bwd") + (("lstm_seq_fwd", "lstm_seq_bwd") if chain else ())

    def name(self, v):
        if not isinstance(v, torch.Tensor):
            return v
        for name, (buf, slab) in self.bufs.items():
            if buf.untyped_storage().data_ptr() == v.untyped_storage().data_ptr():
                if v.shape == buf.shape and v.storage_offset() == 0:
                    return name
                n = int(torch.Size(slab).numel())
                assert tuple(v.shape) == slab and v.storage_offset() % n == 0, (name, v.shape, v.storage_offset())
                return f"{name}[{v.storage_offset() // n}]"
        raise AssertionError("a tensor that is none of the layer's buffers")

    def __getattr__(self, method):
        if method not in self.methods:
            raise AttributeError(method)
        sig = inspect.signature(getattr(HipBackend, method))

        def call(*args, **kw):
            bound = sig.bind(None, *args, **kw)
            bound.apply_defaults()
            self.calls.append((method,) + tuple(self.name(v) for v in list(bound.arguments.values())[1:]))
        return call


def buffers(flat=False, shared_gates=False, steps_out=S):
    """the layer's buffers, per-step ones as [S][B][..] or (``flat``) as [S*B] rows"""
    z = torch.zeros
    lead = lambda n: (n * B,) if flat else (n, B)
    b = {"xz": (z(*lead(S), U, 4), (B, U, 4)), "hs": (z(S + 1, B, U), (B, U)), "cs": (z(S + 1, B, U), (B, U)),
         "Ur": (z(U, U, 4), ()), "bias": (z(U, 4), ()), "ids": (torch.ones(B, S, dtype=torch.int32), ()),
         "out": (z(*lead(steps_out), U), (B, U)), "dout": (z(*lead(steps_out), U), (B, U)),
         "gates": (z(B, U, 4), ()) if shared_gates else (z(S, B, U, 4), (B, U, 4)),
         "dz": (z(*lead(S), U, 4), (B, U, 4)), "da": (z(B, U), ()), "dc": (z(B, U), ()), "dcarry": (z(B, U), ()),
         "sync": (z(1025, dtype=torch.int32), ()), "guard": (z(1), ()), "work": (z(64), ()),
         "pos": (z(S * B, dtype=torch.int32), ())}
    return b, {k: v[0] for k, v in b.items()}


def fwd(t, rec, bias, ids, mask_T, s0, **kw):
    lstm_layer_fwd(rec, t["xz"], t["hs"], t["cs"], t["Ur"], t[bias] if bias else None, t[ids] if ids else None, mask_T, s0,
                   t["out"], t["gates"], S, B, U, **kw)
    return rec.calls


def bwd(t, rec, ids, mask_T, s0, scratch, **kw):
    lstm_layer_bwd(rec, t["Ur"], t["dout"], t[ids] if ids else None, mask_T, s0, t["gates"], t["cs"], t["dz"],
                   tuple(t[k] if k else None for k in scratch), S, B, U, **kw)
    return rec.calls


# lstm_step_fwd(xz, h_prev, c_prev, Ur, ctx, Wc, D, mask_ids, mask_T, mask_t, out_prev, h, c, out, gates, B, U, xz_bias)
def test_fwd_steps_nic():
    """mask_s0 = 1 with ids: an unmasked feature step without `out`, then the text steps; the carried output from text step 1 on"""
    b, t = buffers(steps_out=S - 1)
    assert fwd(t, Recorder(b), "bias", "ids", 2, 1) == [
        ("lstm_step_fwd", "xz[0]", "hs[0]", "cs[0]", "Ur", None, None, 0, None, 2, 0, None, "hs[1]", "cs[1]", None, "gates[0]",
         2, 16, "bias"),
        ("lstm_step_fwd", "xz[1]", "hs[1]", "cs[1]", "Ur", None, None, 0, "ids", 2, 0, None, "hs[2]", "cs[2]", "out[0]",
         "gates[1]", 2, 16, "bias"),
        ("lstm_step_fwd", "xz[2]", "hs[2]", "cs[2]", "Ur", None, None, 0, "ids", 2, 1, "out[0]", "hs[3]", "cs[3]", "out[1]",
         "gates[2]", 2, 16, "bias")]


def test_fwd_steps_fc():
    """mask_s0 = 0 with ids: every step masked"""
    b, t = buffers()
    assert fwd(t, Recorder(b), "bias", "ids", 3, 0) == [
        ("lstm_step_fwd", "xz[0]", "hs[0]", "cs[0]", "Ur", None, None, 0, "ids", 3, 0, None, "hs[1]", "cs[1]", "out[0]",
         "gates[0]", 2, 16, "bias"),
        ("lstm_step_fwd", "xz[1]", "hs[1]", "cs[1]", "Ur", None, None, 0, "ids", 3, 1, "out[0]", "hs[2]", "cs[2]", "out[1]",
         "gates[1]", 2, 16, "bias"),
        ("lstm_step_fwd", "xz[2]", "hs[2]", "cs[2]", "Ur", None, None, 0, "ids", 3, 2, "out[1]", "hs[3]", "cs[3]", "out[2]",
         "gates[2]", 2, 16, "bias")]


def test_fwd_steps_plain():
    """no ids (ThinkAndTell): nothing masked, nothing carried; the bias went through the projection; buffers as rows"""
    b, t = buffers(flat=True)
    assert fwd(t, Recorder(b), None, None, 0, 0, carry_out=False) == [
        ("lstm_step_fwd", "xz[0]", "hs[0]", "cs[0]", "Ur", None, None, 0, None, 0, 0, None, "hs[1]", "cs[1]", "out[0]",
         "gates[0]", 2, 16, None),
        ("lstm_step_fwd", "xz[1]", "hs[1]", "cs[1]", "Ur", None, None, 0, None, 0, 1, None, "hs[2]", "cs[2]", "out[1]",
         "gates[1]", 2, 16, None),
        ("lstm_step_fwd", "xz[2]", "hs[2]", "cs[2]", "Ur", None, None, 0, None, 0, 2, None, "hs[3]", "cs[3]", "out[2]",
         "gates[2]", 2, 16, None)]


def test_fwd_steps_length_mask():
    """carry_out=False with a length mask (ShowAndTell): masked, out_prev always null"""
    b, t = buffers(flat=True)
    assert fwd(t, Recorder(b), None, "ids", 3, 0, carry_out=False) == [
        ("lstm_step_fwd", "xz[0]", "hs[0]", "cs[0]", "Ur", None, None, 0, "ids", 3, 0, None, "hs[1]", "cs[1]", "out[0]",
         "gates[0]", 2, 16, None),
        ("lstm_step_fwd", "xz[1]", "hs[1]", "cs[1]", "Ur", None, None, 0, "ids", 3, 1, None, "hs[2]", "cs[2]", "out[1]",
         "gates[1]", 2, 16, None),
        ("lstm_step_fwd", "xz[2]", "hs[2]", "cs[2]", "Ur", None, None, 0, "ids", 3, 2, None, "hs[3]", "cs[3]", "out[2]",
         "gates[2]", 2, 16, None)]


def test_fwd_steps_shared_gates_slab():
    """gates without a step axis (NIC._score_pass off the chain): every step writes the one slab"""
    b, t = buffers(flat=True, shared_gates=True)
    assert fwd(t, Recorder(b), "bias", "ids", 4, 0) == [
        ("lstm_step_fwd", "xz[0]", "hs[0]", "cs[0]", "Ur", None, None, 0, "ids", 4, 0, None, "hs[1]", "cs[1]", "out[0]",
         "gates", 2, 16, "bias"),
        ("lstm_step_fwd", "xz[1]", "hs[1]", "cs[1]", "Ur", None, None, 0, "ids", 4, 1, "out[0]", "hs[2]", "cs[2]", "out[1]",
         "gates", 2, 16, "bias"),
        ("lstm_step_fwd", "xz[2]", "hs[2]", "cs[2]", "Ur", None, None, 0, "ids", 4, 2, "out[1]", "hs[3]", "cs[3]", "out[2]",
         "gates", 2, 16, "bias")]


def test_single_step_is_the_loop_body():
    b, t = buffers(steps_out=S - 1)
    whole = fwd(t, Recorder(b), "bias", "ids", 2, 1)
    rec = Recorder(b)
    for s in range(S):
        lstm_layer_step_fwd(rec, s, t["xz"], t["hs"], t["cs"], t["Ur"], t["bias"], t["ids"], 2, 1, t["out"], t["gates"], B, U)
    assert rec.calls == whole


# lstm_step_bwd(dz_next, Ur, da_pass_in, dh_ext, dc_in, dout_in, dout_t, mask_ids, mask_T, mask_t, gates, c, c_prev, dz,
#               da_pass_out, dc_out, dout_out, B, U, Wc, D, dctx_part)
def test_bwd_steps_nic():
    """mask_s0 = 1, pass_out_last=False: the feature step takes no output gradient and hands nothing on"""
    b, t = buffers(steps_out=S - 1)
    assert bwd(t, Recorder(b), "ids", 2, 1, ("da", "dc", "dcarry"), pass_out_last=False) == [
        ("lstm_step_bwd", None, "Ur", None, None, None, None, "dout[1]", "ids", 2, 1, "gates[2]", "cs[3]", "cs[2]", "dz[2]",
         "da", "dc", "dcarry", 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[2]", "Ur", "da", None, "dc", "dcarry", "dout[0]", "ids", 2, 0, "gates[1]", "cs[2]", "cs[1]",
         "dz[1]", "da", "dc", "dcarry", 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[1]", "Ur", "da", None, "dc", None, None, None, 2, 0, "gates[0]", "cs[1]", "cs[0]", "dz[0]",
         None, None, None, 2, 16, None, 0, None)]


def test_bwd_steps_fc():
    """mask_s0 = 0: every step a sequence step, the pass-out pointers on every launch"""
    b, t = buffers()
    assert bwd(t, Recorder(b), "ids", 3, 0, ("da", "dc", "dcarry")) == [
        ("lstm_step_bwd", None, "Ur", None, None, None, None, "dout[2]", "ids", 3, 2, "gates[2]", "cs[3]", "cs[2]", "dz[2]",
         "da", "dc", "dcarry", 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[2]", "Ur", "da", None, "dc", "dcarry", "dout[1]", "ids", 3, 1, "gates[1]", "cs[2]", "cs[1]",
         "dz[1]", "da", "dc", "dcarry", 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[1]", "Ur", "da", None, "dc", "dcarry", "dout[0]", "ids", 3, 0, "gates[0]", "cs[1]", "cs[0]",
         "dz[0]", "da", "dc", "dcarry", 2, 16, None, 0, None)]


def test_bwd_steps_feature_step_passes_on():
    """mask_s0 = 1 with the default pass_out_last: the feature step gets da / dc, never the output carry"""
    b, t = buffers(steps_out=S - 1)
    assert bwd(t, Recorder(b), "ids", 2, 1, ("da", "dc", "dcarry"))[2] == (
        "lstm_step_bwd", "dz[1]", "Ur", "da", None, "dc", None, None, None, 2, 0, "gates[0]", "cs[1]", "cs[0]", "dz[0]",
        "da", "dc", None, 2, 16, None, 0, None)


@pytest.mark.parametrize("ids,mask_T", [("ids", 3), (None, 0)])
def test_bwd_steps_no_carry(ids, mask_T):
    """no out-carry scratch (ThinkAndTell; with ShowAndTell's length mask): dout_in and dout_out null on every launch"""
    b, t = buffers(flat=True)
    assert bwd(t, Recorder(b), ids, mask_T, 0, ("da", "dc", None)) == [
        ("lstm_step_bwd", None, "Ur", None, None, None, None, "dout[2]", ids, mask_T, 2, "gates[2]", "cs[3]", "cs[2]", "dz[2]",
         "da", "dc", None, 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[2]", "Ur", "da", None, "dc", None, "dout[1]", ids, mask_T, 1, "gates[1]", "cs[2]", "cs[1]",
         "dz[1]", "da", "dc", None, 2, 16, None, 0, None),
        ("lstm_step_bwd", "dz[1]", "Ur", "da", None, "dc", None, "dout[0]", ids, mask_T, 0, "gates[0]", "cs[1]", "cs[0]",
         "dz[0]", "da", "dc", None, 2, 16, None, 0, None)]


# lstm_seq_fwd(xz, hs, cs, Ur, xz_bias, mask_ids, mask_T, mask_s0, out, gates, S, B, U, sync, guard_out, out_pos)
# lstm_seq_bwd(Ur, dout_seq, mask_ids, mask_T, mask_s0, gates, cs, dz, work, S, B, U, sync, guard_out, dout_pos)
@pytest.mark.parametrize("pos", [None, "pos"])
def test_chain_is_one_launch(pos):
    b, t = buffers(steps_out=S - 1)
    rec = Recorder(b, chain=True)
    kw = lambda k: {k: t[pos]} if pos else {}
    assert fwd(t, rec, "bias", "ids", 2, 1, chain=(t["sync"], t["guard"]), **kw("out_pos")) == [
        ("lstm_seq_fwd", "xz", "hs", "cs", "Ur", "bias", "ids", 2, 1, "out", "gates", 3, 2, 16, "sync", "guard", pos)]
    rec = Recorder(b, chain=True)
    assert bwd(t, rec, "ids", 2, 1, ("da", "dc", "dcarry"), chain=(t["sync"], t["guard"], t["work"]), pass_out_last=False,
               **kw("dout_pos")) == [
        ("lstm_seq_bwd", "Ur", "dout", "ids", 2, 1, "gates", "cs", "dz", "work", 3, 2, 16, "sync", "guard", pos)]


def test_chain_unmasked_form():
    """ThinkAndTell's chain launch: no bias, no ids, mask_T = mask_s0 = 0, buffers as rows"""
    b, t = buffers(flat=True)
    rec = Recorder(b, chain=True)
    assert fwd(t, rec, None, None, 0, 0, chain=(t["sync"], t["guard"]), carry_out=False) == [
        ("lstm_seq_fwd", "xz", "hs", "cs", "Ur", None, None, 0, 0, "out", "gates", 3, 2, 16, "sync", "guard", None)]
    rec = Recorder(b, chain=True)
    assert bwd(t, rec, None, 0, 0, ("da", "dc", None), chain=(t["sync"], t["guard"], t["work"])) == [
        ("lstm_seq_bwd", "Ur", "dout", None, 0, 0, "gates", "cs", "dz", "work", 3, 2, 16, "sync", "guard", None)]


def test_no_chain_entry_point_no_chain_launch():
    """a backend without the chain entry points is never asked for them on the per-step arm"""
    b, t = buffers()
    rec = Recorder(b)
    fwd(t, rec, "bias", "ids", 3, 0)
    bwd(t, rec, "ids", 3, 0, ("da", "dc", "dcarry"))
    assert [c[0] for c in rec.calls] == ["lstm_step_fwd"] * 3 + ["lstm_step_bwd"] * 3
