"""Every kernel variant of csrc/lstm.hip's recurrent core on a real MI355X against the float64 oracle (oracle/ops.py:
lstm_step_fwd, lstm_step_bwd; mask, carry and `out` semantics written out in numpy in ref_chain_fwd / ref_chain_bwd),
at ragged batch sizes, short sequences and every launch path.

Which test launches which kernel -- read against the dispatch at tnt_lstm_step_{fwd,bwd}_f32 and tnt_lstm_seq_{fwd,bwd}_f32:

    kernel                          test                                   arguments that select it
    lstm_fwd_kernel<16, 8>          test_step_fwd[w16-*]                   U % 32 == 0 and U >= 512: (1, 512) (17, 512) (33, 544) (5, 1024)
    lstm_fwd_kernel<8, 16>          test_step_fwd[w8-*]                    every other U % 16 == 0: (17, 480) (33, 528) (1, 16)
    lstm_bwd_lds_kernel<8>          test_step_bwd[lds-*]                   dz_next given and U % 256 == 0: (5, 256) (17, 512) (33, 768) (20, 1024)
    lstm_bwd_kernel                 test_step_bwd[plain-*]                 dz_next null: (17, 512) (5, 1024); U % 256 != 0: (19, 48) (16, 528)
    lstm_seq_fwd_kernel<true, 8>    test_chain_fwd[B-S], B <= 64           B in 1 5 9 37 63 (9: the last 8-row block holds one row)
                                    test_row_maps[13]
    lstm_seq_fwd_kernel<true, 16>   test_chain_fwd[B-S], B > 64            B in 65 72 100 127 (65: the last 16-row block holds one row)
                                    test_row_maps[70], test_ab_variants (TNT_SEQ_RB16=1, B <= 64)
    lstm_seq_fwd_kernel<false, 16>  test_ab_variants                       TNT_SEQ_FLAGS=1 in a child process
    lstm_seq_bwd_kernel<true, 8>    test_chain_bwd[B-S], B <= 64           as the forward chain
    lstm_seq_bwd_kernel<true, 16>   test_chain_bwd[B-S], B > 64            as the forward chain
    lstm_seq_bwd_kernel<false, 16>  test_ab_variants                       TNT_SEQ_FLAGS=1 in a child process

Chain modes (CHAIN_MODES): nic = one unmasked feature step, then the masked text steps (mask_s0 = 1); fc = every step masked
(mask_s0 = 0); plain = no ids; s0S = ids and `out` supplied but mask_s0 == S, so neither is ever used; wideT = nic with an id
stride of (S - mask_s0) + 3 whose surplus columns hold other ids.  S = 1 has no hand-off, S = 2 one, S = 3 resets the last
sentinel slab / ring buffer, S = 5 is the first wrap of the backward ring of three.

Guard bands: every output is a view into the middle of a larger buffer whose remainder holds POISON; after each launch the
bands in front of and behind the view must be bit-unchanged (Guards.check).  Outputs start as NaN, so an element that the
kernel does not write fails its comparison.

Inputs are rounded to float32 before the reference sees them.  Tolerance against float64: `close` of tests/test_gpu_ops.py
with its RTOL = 1e-4 of the reference tensor's largest magnitude, for every tensor at every shape, U = 768 and U = 1024
included -- no wider bound was needed.  For the record, the same oracle evaluated in float32 numpy against float64 (on the
CPU, the inputs of test_step_fwd / test_step_bwd; max-norm error over the tensor's largest magnitude, worst tensor of the
case): forward 1.1e-6 at U = 544 and 9.9e-7 at U = 1024 (8.2e-7 at U = 512), backward 2.3e-7 at U = 768 and 1.8e-7 at
U = 1024 (1.6e-7 at U = 512), that is a factor of 80 and
more inside RTOL.  Chain against the per-step launches: 2e-6 forward (test_lstm_seq_fwd_equals_step_kernels),
2e-6 max(1, scale) + 1e-6 scale backward (test_lstm_seq_bwd_matches_oracle_and_step_kernels); the same bounds hold between
the A/B variants and the default kernels, which sum in a different order."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from masters_thesis_amd.lstm_layer import lstm_layer_fwd, lstm_layer_bwd
from oracle import ops as O
from test_gpu_ops import close, dev, il, unil

pytestmark = pytest.mark.gpu

NAN = float("nan")
POISON = 1234.5                 # around every guarded output: no kernel may write there
BAND = 256                      # floats in front of and behind a guarded view (a multiple of 4: the view stays 16-byte aligned)
KEEP = -77.25                   # initial value of `out` rows that a launch must leave alone
U_SEQ = 512
SKIP_SEQ = "persistent LSTM kernel not supported on this device (needs 256 CUs, 32 workgroups per XCD)"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def r32(a):
    """round to float32, keep float64: the reference and the device start from the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


class Guards:
    """guarded output buffers of one launch: new() hands out the view, check() asserts every band is bit-unchanged"""
    def __init__(self):
        self.items = []

    def new(self, name, *shape, fill=NAN):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * BAND,), POISON, device="cuda")
        view = flat[BAND:BAND + n].view(*shape)
        view.fill_(fill)
        self.items.append((name, flat, n))
        return view

    def check(self):
        want = torch.full((BAND,), POISON, device="cuda").view(torch.int32)
        for name, flat, n in self.items:
            assert torch.equal(flat[:BAND].view(torch.int32), want), f"{name}: written in front of the buffer"
            assert torch.equal(flat[BAND + n:].view(torch.int32), want), f"{name}: written behind the buffer"


def mask_ids_for(rng, B, T, t):
    """ids [B][T] whose column t masks row B - 1 and keeps row B - 2: a masked and an unmasked row inside the ragged last
    16-row block.  Where that block holds one row only (B = 17, 33) it is the masked one and the kept row closes the block in
    front of it; the unmasked cases of the same shape run that row unmasked.  The other rows and columns are random."""
    ids = rng.integers(0, 3, (B, T)).astype(np.int32)
    ids[B - 1, t] = 0
    if B > 1:
        ids[B - 2, t] = 5
    return ids


# ------------------------------------------------------------------------------------------------ (a) step forward
# (masked, xz_bias, D): every pair of option values appears on each variant
STEP_OPTS = [(True, True, 3), (False, False, 32), (True, False, 64), (False, True, 0),
             (False, True, 64), (True, False, 0), (False, False, 3), (True, True, 32)]
STEP_FWD_SHAPES = {"w16": [(1, 512), (17, 512), (33, 544), (5, 1024)], "w8": [(17, 480), (33, 528), (1, 16)]}
STEP_FWD_CASES = [pytest.param(v, *shapes[i % len(shapes)], *opt,
                               id=f"{v}-{shapes[i % len(shapes)][0]}x{shapes[i % len(shapes)][1]}-"
                                  f"{'m' if opt[0] else 'u'}{'b' if opt[1] else ''}-D{opt[2]}")
                  for v, shapes in STEP_FWD_SHAPES.items() for i, opt in enumerate(STEP_OPTS)]


def step_fwd_inputs(B, U, masked, bias, D, seed):
    rng = np.random.default_rng(seed)
    n = types.SimpleNamespace(T=3, t=1)
    n.xz = r32(rng.standard_normal((B, 4 * U)) * 0.5)
    n.h0, n.c0 = r32(rng.standard_normal((B, U)) * 0.5), r32(rng.standard_normal((B, U)) * 0.5)
    n.Ur = r32(rng.standard_normal((U, 4 * U)) / np.sqrt(U))
    n.bl = r32(rng.standard_normal(4 * U) * 0.3) if bias else None
    n.ctx = r32(rng.standard_normal((B, D))) if D else None
    n.Wc = r32(rng.standard_normal((D, 4 * U)) / np.sqrt(D)) if D else None
    n.ids = mask_ids_for(rng, B, n.T, n.t) if masked else None
    n.outp = r32(rng.standard_normal((B, U)))
    return n


def step_fwd_ref(n, dtype=np.float64):
    """(h, c, out, gates [B][U][4]) of one masked step, evaluated in `dtype`"""
    c = lambda a: None if a is None else a.astype(dtype)
    xz = c(n.xz) + (c(n.bl) if n.bl is not None else 0) + (c(n.ctx) @ c(n.Wc) if n.ctx is not None else 0)
    h2, c2, cache = O.lstm_step_fwd(xz, c(n.h0), c(n.c0), c(n.Ur))
    g = np.stack(cache[:4], axis=-1)
    if n.ids is None:
        return h2, c2, h2, g
    m = (n.ids[:, n.t] != 0)[:, None]
    return np.where(m, h2, n.h0), np.where(m, c2, n.c0), np.where(m, h2, n.outp), g


@pytest.mark.parametrize("variant,B,U,masked,bias,D", STEP_FWD_CASES)
def test_step_fwd(be, variant, B, U, masked, bias, D):
    """tnt_lstm_step_fwd_f32, both variants: h, c, out and gates against float64 at ragged B, with a partial last chunk
    (U = 480), a second chunk on wave 0 (U = 544: 17 chunks of 32) and on every wave (U = 1024), U % 32 == 16 past 512
    (528, the 8-wave kernel), the smallest size, and masked / xz_bias / context D in {0, 3, 32, 64} pairwise."""
    assert (variant == "w16") == (U % 32 == 0 and U // 32 >= 16)
    n = step_fwd_inputs(B, U, masked, bias, D, 1000 + 7 * B + U + D)
    hw, cw, ow, gw = step_fwd_ref(n)
    if masked and B > 1:
        assert n.ids[B - 1, n.t] == 0 and n.ids[B - 2, n.t] != 0
    gs = Guards()
    h, c, out, gates = gs.new("h", B, U), gs.new("c", B, U), gs.new("out", B, U), gs.new("gates", B, U, 4)
    be.lstm_step_fwd(dev(il(n.xz, U)), dev(n.h0), dev(n.c0), dev(il(n.Ur, U)), dev(n.ctx) if D else None,
                     dev(il(n.Wc, U)) if D else None, D, dev(n.ids, torch.int32) if masked else None, n.T, n.t,
                     dev(n.outp) if masked else None, h, c, out, gates, B, U, xz_bias=dev(il(n.bl, U)) if bias else None)
    torch.cuda.synchronize()
    gs.check()
    close(h, hw); close(c, cw); close(out, ow); close(gates, gw)


# ------------------------------------------------------------------------------------------------ (b) step backward
STEP_BWD_SHAPES = [("lds", 5, 256, True), ("lds", 17, 512, True), ("lds", 33, 768, True), ("lds", 20, 1024, True),
                   ("plain", 17, 512, False), ("plain", 5, 1024, False), ("plain", 19, 48, True), ("plain", 16, 528, True)]
CTX_D = (3, 20, 64)
STEP_BWD_CASES = [pytest.param(v, B, U, nxt, masked, full, CTX_D[(i + masked) % 3],
                               id=f"{v}-{B}x{U}-{'next' if nxt else 'first'}-{'m' if masked else 'u'}-{'all' if full else 'null'}")
                  for i, (v, B, U, nxt) in enumerate(STEP_BWD_SHAPES) for masked in (0, 1) for full in (1, 0)]


def step_bwd_inputs(B, U, nxt, masked, full, D, seed):
    rng = np.random.default_rng(seed)
    n = types.SimpleNamespace(T=3, t=1, D=D)
    f = lambda *s: r32(rng.standard_normal(s))
    n.Ur = r32(rng.standard_normal((U, 4 * U)) / np.sqrt(U))
    n.Wc = r32(rng.standard_normal((D, 4 * U)) / np.sqrt(D))
    n.gates = r32(rng.uniform(0.1, 0.9, (B, U, 4)))                  # i, f, g, o of a forward step
    n.gates[..., 2] = r32(rng.uniform(-0.9, 0.9, (B, U)))
    n.c, n.cprev = f(B, U), f(B, U)
    n.dz_next = r32(rng.standard_normal((B, 4 * U)) * 0.3) if nxt else None
    n.da_in, n.dh_ext, n.dc_in, n.dout_in, n.dout_t = (f(B, U) if full else None for _ in range(5))
    n.ids = mask_ids_for(rng, B, n.T, n.t) if masked else None
    return n


def step_bwd_ref(n, dtype=np.float64):
    """(dz [B][4U], da_pass_out, dc_out, dout_out) of one masked backward step, evaluated in `dtype`"""
    c = lambda a: 0.0 if a is None else a.astype(dtype)
    B, U = n.c.shape
    zero = np.zeros((B, U), dtype)
    da = zero + c(n.da_in) + c(n.dh_ext) + (c(n.dz_next) @ c(n.Ur).T if n.dz_next is not None else 0)
    dout = zero + c(n.dout_in) + c(n.dout_t)
    dc_in = zero + c(n.dc_in)
    g = c(n.gates)
    cache = (g[..., 0], g[..., 1], g[..., 2], g[..., 3], c(n.cprev), np.tanh(c(n.c)), None)
    dz, _, dcp = O.lstm_step_bwd(da + dout, dc_in, cache, c(n.Ur))
    if n.ids is None:
        return dz, 0 * da, dcp, 0 * dout
    m = (n.ids[:, n.t] != 0)[:, None]
    return np.where(m, dz, 0), np.where(m, 0, da), np.where(m, dcp, dc_in), np.where(m, 0, dout)


@pytest.mark.parametrize("variant,B,U,nxt,masked,full,D", STEP_BWD_CASES)
def test_step_bwd(be, variant, B, U, nxt, masked, full, D):
    """tnt_lstm_step_bwd_f32, both variants: dz, da_pass_out, dc_out and dout_out against float64; the LDS kernel at 1, 2, 3
    and 4 K-chunks of 1024 with ragged B, the plain kernel without dz_next and at U % 256 != 0.  Masked rows of dz are exactly
    0.0.  `all`: every optional pointer given, and dctx_part asked for at D in {3, 20, 64} -- the entry point's documented
    guard is D <= 64 with a 16-byte aligned Wc, so none of these D is refused; the sum of the partials over the unit blocks
    is compared with the ORACLE's dz @ Wc^T and asking for them leaves dz bit-identical.  `null`: every optional pointer null."""
    assert (variant == "lds") == (nxt and U % 256 == 0)
    n = step_bwd_inputs(B, U, nxt, masked, full, D, 2000 + 7 * B + U + masked)
    dzw, daw, dcw, dow = step_bwd_ref(n)
    o = lambda a, dt=torch.float32: None if a is None else dev(a, dt)
    ins = (o(il(n.dz_next, U)) if nxt else None, dev(il(n.Ur, U)), o(n.da_in), o(n.dh_ext), o(n.dc_in), o(n.dout_in), o(n.dout_t),
           o(n.ids, torch.int32), n.T, n.t, dev(n.gates), dev(n.c), dev(n.cprev))
    Wc = dev(il(n.Wc, U))
    runs = []
    for parts in ((False, True) if full else (False,)):
        gs = Guards()
        dz = gs.new("dz", B, U, 4)
        da_o, dc_o, do_o = (gs.new(k, B, U) if full else None for k in ("da_pass_out", "dc_out", "dout_out"))
        part = gs.new("dctx_part", U // 16, B, D) if parts else None
        be.lstm_step_bwd(*ins, dz, da_o, dc_o, do_o, B, U, Wc=Wc if parts else None, D=D if parts else 0, dctx_part=part)
        torch.cuda.synchronize()
        gs.check()
        runs.append((dz, da_o, dc_o, do_o, part))
    dz, da_o, dc_o, do_o, _ = runs[0]
    close(unil(dz.cpu().numpy()), dzw)
    if masked:
        dead = torch.tensor(n.ids[:, n.t] == 0, device="cuda")
        assert bool(dead.any()) and not bool(dead.all())
        assert torch.equal(dz[dead], torch.zeros_like(dz[dead]))
    if full:
        close(da_o, daw); close(dc_o, dcw); close(do_o, dow)
        for a, b in zip(runs[0][:4], runs[1][:4]):
            assert torch.equal(a, b)                         # asking for the partials changes nothing else
        close(runs[1][4].sum(0), dzw @ n.Wc.T)


# ------------------------------------------------------------------------------------------------ chain references
def ref_chain_fwd(xz, bl, Ur, h0, c0, ids, s0):
    """The masked LSTM over S steps in float64 (keras LSTM with a mask, NIC.py:138-140): step s < s0 is unmasked, step
    s >= s0 advances row b only where ids[b][s - s0] != 0 (all rows without ids); `out` of a step >= s0 is the new h of the
    advancing rows and the carried previous output (zero at first) of the others.
    Returns Hs [S+1], Cs [S+1], G [S][B][U][4], Out [S-s0] and the step caches and masks that ref_chain_bwd takes."""
    S, B = xz.shape[:2]
    Hs, Cs, G, Out, caches, ms = [h0], [c0], [], [], [], []
    out = np.zeros_like(h0)
    for s in range(S):
        h2, c2, cache = O.lstm_step_fwd(xz[s] + (0 if bl is None else bl), Hs[-1], Cs[-1], Ur)
        m = (ids[:, s - s0] != 0)[:, None] if (ids is not None and s >= s0) else np.ones((B, 1), bool)
        G.append(np.stack(cache[:4], axis=-1)); caches.append(cache); ms.append(m)
        Hs.append(np.where(m, h2, Hs[-1])); Cs.append(np.where(m, c2, Cs[-1]))
        if s >= s0:
            out = np.where(m, h2, out)
            Out.append(out)
    U = h0.shape[1]
    return np.stack(Hs), np.stack(Cs), np.stack(G), np.stack(Out) if Out else np.zeros((0, B, U)), caches, ms


def ref_chain_bwd(caches, ms, dOut, Ur, s0):
    """BPTT through ref_chain_fwd in float64: dOut [S-s0][B][U] is the gradient of Out; a masked row passes its pending
    gradients (of h, c and of the carried output) on to the step before.  Returns dz [S][B][4U]."""
    S = len(caches)
    B, U = caches[0][0].shape
    da, dc, dout = np.zeros((B, U)), np.zeros((B, U)), np.zeros((B, U))
    dzw = np.zeros((S, B, 4 * U))
    for s in reversed(range(S)):
        m = ms[s]
        dout = dout + dOut[s - s0] if s >= s0 else np.zeros((B, U))
        dz, dh_prev, dc_prev = O.lstm_step_bwd(np.where(m, da + dout, 0), np.where(m, dc, 0), caches[s], Ur)
        dzw[s] = dz
        da = np.where(m, 0, da) + dh_prev
        dc = np.where(m, 0, dc) + dc_prev
        dout = np.where(m, 0, dout)
    return dzw


CHAIN_MODES = ("nic", "fc", "plain", "s0S", "wideT")


@functools.lru_cache(maxsize=16)
def chain_case(B, S, mode, bias):
    """inputs (float32-rounded) and float64 references of one chain case, never modified; the most recent ones are kept,
    so the launches of one test and the children of the A/B test share one reference"""
    U = U_SEQ
    rng = np.random.default_rng([B, S, CHAIN_MODES.index(mode), int(bias)])
    n = types.SimpleNamespace(B=B, S=S, U=U, mode=mode)
    n.s0 = {"nic": 1, "fc": 0, "plain": 0, "s0S": S, "wideT": 1}[mode]
    n.nseq = S - n.s0
    n.mask_T = max(n.nseq, 1) + (3 if mode == "wideT" else 0)
    n.xz = r32(rng.standard_normal((S, B, 4 * U)) * 0.5)
    n.Ur = r32(rng.standard_normal((U, 4 * U)) / np.sqrt(U))
    n.bl = r32(rng.standard_normal(4 * U) * 0.3) if bias else None
    n.h0, n.c0 = r32(rng.standard_normal((B, U)) * 0.3), r32(rng.standard_normal((B, U)) * 0.3)
    n.ids = None
    if mode != "plain":
        ids = rng.integers(1, 50, (B, n.mask_T)).astype(np.int32)
        for b in range(B):
            cut = int(rng.integers(1, n.nseq + 1)) if n.nseq else 0
            ids[b, cut:n.nseq] = 0                          # padding tail: masked steps
        ids[:, n.nseq:] = rng.integers(0, 2, (B, n.mask_T - n.nseq)) * 7               # never read: other ids on purpose
        if B > 1 or S % 2:
            ids[B - 1, :n.nseq] = 0                         # a row masked from the first text step on, in the ragged block
        n.ids = ids
    n.dOut = r32(rng.standard_normal((n.nseq, B, U)) * 0.1)
    n.Hs, n.Cs, n.G, n.Out, caches, ms = ref_chain_fwd(n.xz, n.bl, n.Ur, n.h0, n.c0, n.ids, n.s0)
    n.caches, n.ms = caches, ms
    n.dz = ref_chain_bwd(caches, ms, n.dOut, n.Ur, n.s0)
    return n


class ChainDev:
    """device copies of a chain case's inputs"""
    def __init__(self, n):
        U = n.U
        self.xz, self.Ur = dev(il(n.xz, U)), dev(il(n.Ur, U))
        self.bl = dev(il(n.bl, U)) if n.bl is not None else None
        self.ids = dev(n.ids, torch.int32) if n.ids is not None else None
        self.h0, self.c0 = dev(n.h0), dev(n.c0)
        self.dOut = dev(n.dOut) if n.nseq else torch.zeros(1, n.B, U, device="cuda")
        self.sync = torch.zeros(1025, dtype=torch.int32, device="cuda")
        self.guard = torch.zeros(1, device="cuda")


def chain_fwd_launch(be, n, d, pos=None):
    """one guarded launch of tnt_lstm_seq_fwd_f32; returns (hs, cs, out, gates) after checking bands and error words"""
    S, B, U = n.S, n.B, n.U
    gs = Guards()
    hs, cs = gs.new("hs", S + 1, B, U), gs.new("cs", S + 1, B, U)
    hs[0], cs[0] = d.h0, d.c0
    out = gs.new("out", max(n.nseq, 1) * B, U, fill=KEEP if (pos is not None or n.nseq == 0) else NAN)
    gates = gs.new("gates", S, B, U, 4)
    be.lstm_seq_fwd(d.xz, hs, cs, d.Ur, d.bl, d.ids, n.mask_T, n.s0, out, gates, S, B, U, d.sync, d.guard, out_pos=pos)
    torch.cuda.synchronize()
    assert int(d.sync[1024]) == 0 and float(d.guard) == 0.0, "error word of the persistent kernel set"
    gs.check()
    return hs, cs, out, gates


def chain_bwd_launch(be, n, d, gates, cs, junk=None, pos=None, dout=None):
    """one guarded launch of tnt_lstm_seq_bwd_f32 (the exchange ring zeroed, or pre-filled with `junk`); returns dz"""
    S, B, U = n.S, n.B, n.U
    gs = Guards()
    dz = gs.new("dz", S, B, U, 4)
    nw = be.lstm_seq_bwd_work_floats(B, U)
    work = gs.new("work", nw, fill=0.0)
    if junk is not None:
        work.copy_(junk[:nw])
    be.lstm_seq_bwd(d.Ur, d.dOut if dout is None else dout, d.ids, n.mask_T, n.s0, gates, cs, dz, work, S, B, U, d.sync, d.guard,
                    dout_pos=pos)
    torch.cuda.synchronize()
    assert int(d.sync[1024]) == 0 and float(d.guard) == 0.0, "error word of the persistent kernel set"
    gs.check()
    return dz


def step_chain_fwd(be, n, d):
    """the same sequence as S launches of the step kernel: the models' own per-step loop (lstm_layer.lstm_layer_fwd)"""
    S, B, U = n.S, n.B, n.U
    Hs, Cs = torch.zeros(S + 1, B, U, device="cuda"), torch.zeros(S + 1, B, U, device="cuda")
    Hs[0], Cs[0] = d.h0, d.c0
    Out, G = torch.zeros(max(n.nseq, 1), B, U, device="cuda"), torch.zeros(S, B, U, 4, device="cuda")
    lstm_layer_fwd(be, d.xz, Hs, Cs, d.Ur, d.bl, d.ids, n.mask_T, n.s0, Out, G, S, B, U, chain=None)
    return Hs, Cs, Out, G


def step_chain_bwd(be, n, d, G, Cs):
    """BPTT as S launches of the step kernel: the models' own per-step loop (lstm_layer.lstm_layer_bwd)"""
    S, B, U = n.S, n.B, n.U
    dZ = torch.zeros(S, B, U, 4, device="cuda")
    z = lambda: torch.zeros(B, U, device="cuda")
    dap, dcp, dop = z(), z(), z()
    lstm_layer_bwd(be, d.Ur, d.dOut, d.ids, n.mask_T, n.s0, G, Cs, dZ, (dap, dcp, dop), S, B, U, chain=None)
    return dZ


CHAIN_BS = [(B, S) for B in (1, 5, 9, 37, 63, 65, 72, 100, 127) for S in (1, 2, 3, 5)] + [(37, 16), (100, 16)]
CHAIN_IDS = [f"{B}-{S}" for B, S in CHAIN_BS]


def chain_variants(B, S):
    """(mode, bias) of one (B, S): every mode, the bias alternating so that each mode meets both at every B"""
    return [(mode, bool((i + S + B) % 2)) for i, mode in enumerate(CHAIN_MODES)] + [("nic", bool((S + B + 1) % 2))]


# ------------------------------------------------------------------------------------------------ (c) forward chain
@pytest.mark.parametrize("B,S", CHAIN_BS, ids=CHAIN_IDS)
def test_chain_fwd(be, B, S):
    """tnt_lstm_seq_fwd_f32 at ragged B (8-row blocks up to 64, 16-row blocks past it) and short S, in every mode, with
    and without xz_bias: every hs, cs, gates and out slab against float64, error word and guard 0, bands intact, a second
    launch bit-identical; at B = 37 and 100 also against S launches of the step kernel within 2e-6."""
    if not be.lstm_seq_supported(B, U_SEQ):
        pytest.skip(SKIP_SEQ)
    for mode, bias in chain_variants(B, S):
        n = chain_case(B, S, mode, bias)
        d = ChainDev(n)
        hs, cs, out, gates = chain_fwd_launch(be, n, d)
        close(hs, n.Hs); close(cs, n.Cs); close(gates, n.G)
        if n.nseq:
            close(out.view(n.nseq, B, n.U), n.Out)
        else:
            assert bool((out == KEEP).all()), "`out` written although no step is a sequence step"
        if n.ids is not None and n.nseq and (B > 1 or S % 2):
            assert torch.equal(hs[S, B - 1], hs[n.s0, B - 1])          # the fully masked row holds its state
        again = chain_fwd_launch(be, n, d)
        for a, b in zip((hs, cs, out, gates), again):
            assert torch.equal(a, b), (mode, bias)
        if B in (37, 100) and mode != "s0S":
            for name, a, b in zip(("hs", "cs", "out", "gates"), (hs, cs, out.view(-1, B, n.U), gates), step_chain_fwd(be, n, d)):
                if name != "out" or n.nseq:
                    assert (a - b).abs().max().item() <= 2e-6, (mode, bias, name)


# ------------------------------------------------------------------------------------------------ (d) backward chain
@pytest.mark.parametrize("B,S", CHAIN_BS, ids=CHAIN_IDS)
def test_chain_bwd(be, B, S):
    """tnt_lstm_seq_bwd_f32 at the same B, S and modes: dz against the float64 chain (masked rows exactly 0.0), error word
    and guard 0, bands intact (dz and the exchange ring), a second launch -- its whole ring pre-filled with plausible
    garbage -- bit-identical; at B = 37 and 100 also against the step-kernel chain."""
    if not be.lstm_seq_supported(B, U_SEQ):
        pytest.skip(SKIP_SEQ)
    rng = np.random.default_rng(B * 100 + S)
    junk = torch.tensor(rng.standard_normal(be.lstm_seq_bwd_work_floats(B, U_SEQ)) * 0.01, dtype=torch.float32, device="cuda")
    for mode, bias in chain_variants(B, S)[:len(CHAIN_MODES)]:
        n = chain_case(B, S, mode, bias)
        d = ChainDev(n)
        hs, cs, out, gates = chain_fwd_launch(be, n, d)
        dz = chain_bwd_launch(be, n, d, gates, cs)
        close(unil(dz.cpu().numpy()), n.dz)
        for s in range(S):
            dead = torch.tensor(~n.ms[s][:, 0], device="cuda")
            assert torch.equal(dz[s][dead], torch.zeros_like(dz[s][dead])), (mode, s)
        dz2 = chain_bwd_launch(be, n, d, gates, cs, junk=junk)
        assert torch.equal(dz, dz2), (mode, bias)
        if B in (37, 100):
            dzs = step_chain_bwd(be, n, d, gates, cs)
            scale = dzs.abs().max().item()
            assert (dz - dzs).abs().max().item() <= 2e-6 * max(1.0, scale) + 1e-6 * scale, (mode, bias)


# ------------------------------------------------------------------------------------------------ (e) row maps
@pytest.mark.parametrize("B", [13, 70])
@pytest.mark.parametrize("mode", ["nic", "fc"])
def test_row_maps(be, B, mode):
    """out_pos on the forward chain and dout_pos on the backward chain at ragged B, S = 5: a random injective map of (t, b)
    to rows with about a quarter of the positions set to -1.  Forward: row pos[t*B + b] of `out` is the oracle's output of
    (t, b), rows that no position maps to keep their initial value, hs / cs / gates are bit-identical to the run without a
    map.  Backward: the oracle chain with dOut gathered through the map, zero where it is -1."""
    S, U = 5, U_SEQ
    if not be.lstm_seq_supported(B, U):
        pytest.skip(SKIP_SEQ)
    n = chain_case(B, S, mode, True)
    d = ChainDev(n)
    rng = np.random.default_rng(B + len(mode))
    rows = n.nseq * B
    pos = rng.permutation(rows).astype(np.int32)
    drop = rng.random(rows) < 0.25
    drop[B - 1], drop[(n.nseq - 1) * B + B - 1] = False, True        # the last row of the ragged block: once with a row, once without
    pos[drop] = -1
    live = pos >= 0
    assert 0.1 < 1 - live.mean() < 0.45 and len(set(pos[live])) == live.sum()
    posd = dev(pos, torch.int32)
    hs, cs, out, gates = chain_fwd_launch(be, n, d)
    hs_m, cs_m, out_m, gates_m = chain_fwd_launch(be, n, d, pos=posd)
    assert torch.equal(hs, hs_m) and torch.equal(cs, cs_m) and torch.equal(gates, gates_m)
    flat = n.Out.reshape(rows, U)
    close(out_m[torch.tensor(pos[live].astype(np.int64), device="cuda")], flat[live])
    free = np.setdiff1d(np.arange(rows), pos[live])
    assert len(free) and bool((out_m[torch.tensor(free, device="cuda")] == KEEP).all()), "a row without a position was written"
    # backward: gradient rows addressed through the same map
    dout_rows = r32(rng.standard_normal((rows, U)) * 0.1)
    dO = np.where(live[:, None], dout_rows[np.maximum(pos, 0)], 0.0).reshape(n.nseq, B, U)
    dzw = ref_chain_bwd(n.caches, n.ms, dO, n.Ur, n.s0)
    dz = chain_bwd_launch(be, n, d, gates, cs, pos=posd, dout=dev(dout_rows).view(n.nseq, B, U))
    close(unil(dz.cpu().numpy()), dzw)
    dz_p = chain_bwd_launch(be, n, d, gates, cs, dout=dev(dO))          # position-ordered, no map: the same arithmetic
    assert torch.equal(dz, dz_p)


# ------------------------------------------------------------------------------------------------ (f) A/B variants
AB_BS = (5, 37, 64, 100)
AB_CODE = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests'); import test_gpu_lstm_paths as P; "
           "P.ab_child(sys.argv[1])")


def ab_child(path):
    """body of one child process of test_ab_variants: both chains at every B of AB_BS, S = 5, nic mode; saves the results
    and prints the error words"""
    import masters_thesis_amd.ops as ops
    be = ops.backend()
    res = {}
    for B in AB_BS:
        n = chain_case(B, 5, "nic", True)
        d = ChainDev(n)
        S, U = n.S, n.U
        hs, cs = torch.zeros(S + 1, B, U, device="cuda"), torch.zeros(S + 1, B, U, device="cuda")
        hs[0], cs[0] = d.h0, d.c0
        out, gates = torch.full((n.nseq, B, U), NAN, device="cuda"), torch.full((S, B, U, 4), NAN, device="cuda")
        dz = torch.full((S, B, U, 4), NAN, device="cuda")
        work = torch.zeros(be.lstm_seq_bwd_work_floats(B, U), device="cuda")
        be.lstm_seq_fwd(d.xz, hs, cs, d.Ur, d.bl, d.ids, n.mask_T, n.s0, out, gates, S, B, U, d.sync, d.guard)
        be.lstm_seq_bwd(d.Ur, d.dOut, d.ids, n.mask_T, n.s0, gates, cs, dz, work, S, B, U, d.sync, d.guard)
        torch.cuda.synchronize()
        print("ERR", B, int(d.sync[1024]), float(d.guard), flush=True)
        for k, v in (("hs", hs), ("gates", gates), ("out", out), ("dz", dz)):
            res[f"{k}{B}"] = v.cpu().numpy()
    np.savez(path, **res)


def test_ab_variants(be, tmp_path):
    """TNT_SEQ_FLAGS=1 (flag-per-step kernels, <false, 16>) and TNT_SEQ_RB16=1 (16-row blocks at B <= 64, <true, 16>) are
    read once per process, so each runs in a fresh child of its own, one after another, next to a child with neither set:
    return code 0, error words 0, hs / gates / out / dz against float64 under `close`, and the variants within the
    chain-against-step-kernel bounds of the default child (not bit-identical: the summation order differs)."""
    if not be.lstm_seq_supported(64, U_SEQ):
        pytest.skip(SKIP_SEQ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("TNT_SEQ_FLAGS", "TNT_SEQ_RB16")}
    got = {}
    for name, extra in (("default", {}), ("flags", {"TNT_SEQ_FLAGS": "1"}), ("rb16", {"TNT_SEQ_RB16": "1"})):
        path = str(tmp_path / f"{name}.npz")
        p = subprocess.run([sys.executable, "-c", AB_CODE, path], cwd=root, env=dict(base, **extra), capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        errs = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ERR ")]
        assert [int(e[1]) for e in errs] == list(AB_BS), (name, p.stdout[-2000:])
        assert all(int(e[2]) == 0 and float(e[3]) == 0.0 for e in errs), (name, errs)
        with np.load(path) as z:
            got[name] = {k: z[k] for k in z.files}
        for B in AB_BS:
            n = chain_case(B, 5, "nic", True)
            r = got[name]
            close(r[f"hs{B}"], n.Hs); close(r[f"gates{B}"], n.G); close(r[f"out{B}"], n.Out)
            close(unil(r[f"dz{B}"]), n.dz)
            if name != "default":
                ref = got["default"]
                for k in ("hs", "gates", "out"):
                    assert np.abs(r[f"{k}{B}"] - ref[f"{k}{B}"]).max() <= 2e-6, (name, k, B)
                scale = float(np.abs(ref[f"dz{B}"]).max())
                assert np.abs(r[f"dz{B}"] - ref[f"dz{B}"]).max() <= 2e-6 * max(1.0, scale) + 1e-6 * scale, (name, B)


# ------------------------------------------------------------------------------------------------ (g) refusals
def seq_max_barriers():
    """TNT_SEQ_MAX_BARRIERS of csrc/tnt_seq_sync.h"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "masters-thesis_amd", "csrc", "tnt_seq_sync.h")) as f:
        return int(re.search(r"constexpr\s+int\s+TNT_SEQ_MAX_BARRIERS\s*=\s*(\d+)\s*;", f.read()).group(1))


def test_chain_refuses_bad_arguments(be):
    """Both chain entry points return an error code before any launch for: S - 1 > TNT_SEQ_MAX_BARRIERS, mask_s0 > S,
    S - mask_s0 > mask_T with ids, a work buffer one float short, a misaligned work pointer; lstm_seq_supported is false
    for B = 129, B = 0 and U = 256.  Nothing is written and the sync state is untouched."""
    from masters_thesis_amd._lib import KernelLibraryError
    assert not be.lstm_seq_supported(129, 512) and not be.lstm_seq_supported(0, 512) and not be.lstm_seq_supported(64, 256)
    B, U = 8, U_SEQ
    if not be.lstm_seq_supported(B, U):
        pytest.skip(SKIP_SEQ)
    Smax = seq_max_barriers() + 2                       # the first S with S - 1 > TNT_SEQ_MAX_BARRIERS
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    xz, Ur = f(Smax, B, U, 4), f(U, U, 4)
    hs, cs, out, gates, dz = f(Smax + 1, B, U), f(Smax + 1, B, U), f(Smax, B, U), f(Smax, B, U, 4), f(Smax, B, U, 4)
    ids = torch.ones(B, Smax, dtype=torch.int32, device="cuda")
    sync = torch.zeros(1025, dtype=torch.int32, device="cuda")
    guard = torch.zeros(1, device="cuda")
    nw = be.lstm_seq_bwd_work_floats(B, U)
    work = f(nw + 4)
    S = 5
    fwd = lambda S_, T_, s0_: be.lstm_seq_fwd(xz, hs, cs, Ur, None, ids, T_, s0_, out, gates, S_, B, U, sync, guard)
    bwd = lambda S_, T_, s0_, w: be.lstm_seq_bwd(Ur, out, ids, T_, s0_, gates, cs, dz, w, S_, B, U, sync, guard)
    for S_, T_, s0_ in ((Smax, Smax, 0), (S, S, S + 1), (S, S - 2, 1)):
        with pytest.raises(KernelLibraryError):
            fwd(S_, T_, s0_)
        with pytest.raises(KernelLibraryError):
            bwd(S_, T_, s0_, work[:nw])
    with pytest.raises(KernelLibraryError):
        bwd(S, S, 0, work[:nw - 1])
    with pytest.raises(KernelLibraryError):
        bwd(S, S, 0, work[1:nw + 1])
    torch.cuda.synchronize()
    assert all(float(t.min()) == 7.0 == float(t.max()) for t in (hs, cs, out, gates, dz, work))
    assert int(sync.abs().max()) == 0 and float(guard) == 0.0


def test_step_refuses_bad_arguments(be):
    """The step entry points return an error code before any launch for U = 24, B = 0, h aliasing h_prev, dz aliasing dz_next
    and dctx_part with D = 65.  Nothing is written."""
    from masters_thesis_amd._lib import KernelLibraryError
    B, U, D = 4, 32, 65
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    xz, h0, c0, Ur = f(B, U, 4), f(B, U), f(B, U), f(U, U, 4)
    h, c, out, gates, dz, dzn, dc_o = f(B, U), f(B, U), f(B, U), f(B, U, 4), f(B, U, 4), f(B, U, 4), f(B, U)
    Wc, part = f(D, U, 4), f(U // 16, B, D)
    fwd = lambda B_, U_, h_: be.lstm_step_fwd(xz, h0, c0, Ur, None, None, 0, None, 0, 0, None, h_, c, out, gates, B_, U_)
    bwd = lambda B_, U_, dz_, **kw: be.lstm_step_bwd(dzn, Ur, None, h0, c0, None, None, None, 0, 0, gates, c, c0, dz_, None, dc_o,
                                                     None, B_, U_, **kw)
    for args in ((B, 24, h), (0, U, h), (B, U, h0)):
        with pytest.raises(KernelLibraryError):
            fwd(*args)
    for args in ((B, 24, dz), (0, U, dz), (B, U, dzn)):
        with pytest.raises(KernelLibraryError):
            bwd(*args)
    with pytest.raises(KernelLibraryError):
        bwd(B, U, dz, Wc=Wc, D=D, dctx_part=part)
    torch.cuda.synchronize()
    assert all(float(t.min()) == 7.0 == float(t.max()) for t in (h0, h, c, out, gates, dz, dzn, dc_o, part))
