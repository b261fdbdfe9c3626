"""The masked LSTM layer of the dense models (nic, fc_nic, think_and_tell), forward and BPTT, as the one persistent chain launch
(tnt_lstm_seq_fwd_f32 / tnt_lstm_seq_bwd_f32) or as S launches of the step kernels: which, the model says with ``chain``.  Plain
functions of the backend, so the kernel tests (tests/test_gpu_lstm_paths.py) drive the models' own loop.
Step s < mask_s0 is unmasked; step s >= mask_s0 is sequence step t = s - mask_s0: it advances row b only where ids[b][t] != 0
(every row without ids) and writes out[t], the new h of an advancing row, the carried out[t-1] of a masked one.
Per-step buffers (xz, gates, dz [.., U, 4]; out, dout [.., U]) are held [S][B][..] or as [S*B] rows; hs, cs are [S+1][B][U]."""


def _steps(x, B, *tail):
    return None if x is None else x.view(-1, B, *tail)


def lstm_layer_step_fwd(be, s, xz, hs, cs, Ur, bias, ids, mask_T, mask_s0, out, gates, B, U, carry_out=True):
    """Step s as one tnt_lstm_step_fwd_f32 launch.  ``bias``: added by the kernel (None: the projection added it); ``gates``
    without a step axis: one slab for all steps; ``carry_out=False``: a masked row's output is zero, not the carried one."""
    t = s - mask_s0
    xz, out = _steps(xz, B, U, 4), _steps(out, B, U)
    carry = carry_out and t > 0 and ids is not None
    be.lstm_step_fwd(xz[s], hs[s], cs[s], Ur, None, None, 0, ids if t >= 0 else None, mask_T, max(t, 0),
                     out[t - 1] if carry else None, hs[s + 1], cs[s + 1], out[t] if t >= 0 and out is not None else None,
                     gates if gates.dim() == 3 else gates[s], B, U, xz_bias=bias)


def lstm_layer_fwd(be, xz, hs, cs, Ur, bias, ids, mask_T, mask_s0, out, gates, S, B, U, chain=None, out_pos=None,
                   carry_out=True):
    """The S steps.  ``chain`` = (sync, guard_out): ONE persistent launch (an XCD-local barrier per dependent step instead
    of a kernel launch, the recurrent weights stay in VGPRs), writing `out` by compacted row with ``out_pos``; None: S launches."""
    if chain is not None:
        be.lstm_seq_fwd(xz, hs, cs, Ur, bias, ids, mask_T, mask_s0, out, gates, S, B, U, *chain, out_pos=out_pos)
        return
    for s in range(S):
        lstm_layer_step_fwd(be, s, xz, hs, cs, Ur, bias, ids, mask_T, mask_s0, out, gates, B, U, carry_out)


def lstm_layer_bwd(be, Ur, dout, ids, mask_T, mask_s0, gates, cs, dz, scratch, S, B, U, chain=None, dout_pos=None,
                   pass_out_last=True):
    """BPTT: dz of every step from ``dout``, the gradient of `out`.  ``chain`` = (sync, guard_out, exchange buffer): ONE
    persistent launch, reading `dout` by compacted row with ``dout_pos``; None: S launches of tnt_lstm_step_bwd_f32 from step
    S-1 down, handing the pending gradients of h, c and the carried output on through ``scratch`` = (da_pass, dc, dout-carry
    or None: no carry).  ``pass_out_last=False``: step 0's launch, which nothing follows, gets null pointers for them."""
    if chain is not None:
        be.lstm_seq_bwd(Ur, dout, ids, mask_T, mask_s0, gates, cs, dz, chain[2], S, B, U, *chain[:2], dout_pos=dout_pos)
        return
    dout, dz = _steps(dout, B, U), _steps(dz, B, U, 4)
    da, dc, dcarry = scratch
    for s in range(S - 1, -1, -1):
        t = s - mask_s0
        first, seq = s == S - 1, t >= 0
        da_o, dc_o, dcarry_o = (da, dc, dcarry if seq else None) if (s > 0 or pass_out_last) else (None, None, None)
        be.lstm_step_bwd(None if first else dz[s + 1], Ur, None if first else da, None, None if first else dc,
                         None if first or not seq else dcarry, dout[t] if seq else None, ids if seq else None, mask_T,
                         max(t, 0), gates[s], cs[s + 1], cs[s], dz[s], da_o, dc_o, dcarry_o, B, U)
