"""Timing of the learned initial LSTM state (lc_nic.NIC(init_state=LearnedInitState())) on config 3 (bench.py's attention model
and batch), all in one process, device events around windows that end in a synchronise, every window warmed first, medians:

  1. each new launch alone at config 3's sizes (B = 64, R = 360, D = 32, U = 512) -- tnt_init_state_fwd_f32,
     tnt_init_state_bwd_f32 with and without dF -- against tnt_attention_coverage_f32 on config 3's attention weights, the
     launch-latency-bound yardstick of profiles/coverage_bench.txt;
  2. the persistent backward chain on the buffers a training step left, with dc0 = NULL and with dc0, alternating windows;
  3. config 3's training step and a 64 x 15 greedy decode with the feature on against off, alternating windows.

    python tools/init_state_bench.py        # prints, and writes its section of profiles/init_state_bench.txt

The file's first section, the feature-off step against the parent commit (bench.py, alternating runs), is kept.

Every expectation of the feature's design is marked held or missed in the output; none is a gate."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from masters_thesis_amd import _lib, ops  # noqa: E402
from masters_thesis_amd.lc_nic import NIC, synthetic_groups, S_ATTN, S_LSTM_IN, S_LSTM_OUT  # noqa: E402
from masters_thesis_amd.model_base import LearnedInitState  # noqa: E402
from masters_thesis_amd.optimizers import Adam  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "init_state_bench.txt")
MARK = "# ---- the feature's launches, the chain and the step (tools/init_state_bench.py)"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n          # us per call


def median(v):
    return sorted(v)[len(v) // 2]


def alternate(arms, n, reps=5, warm=20):
    """arms: {name: fn}; reps alternating windows of n calls each -> {name: [us per call]}"""
    out = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(warm):
            fn()
    for _ in range(reps):
        for k, fn in arms.items():
            for _ in range(3):
                fn()
            out[k].append(window(fn, n))
    return out


def make(init):
    """bench.make_model("attention"), with or without the learned initial state"""
    groups = synthetic_groups(bench.N_VOX, 360, 32, seed=42)
    m = NIC(groups, bench.U, 512, bench.E, 32, bench.V, bench.T, 0.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 0.00003, 0.00001,
            device="cuda", seed=42, **({"init_state": init} if init is not None else {}))
    m.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def launches():
    be = ops.backend()
    B, R, D, U, T = bench.B, 360, 32, bench.U, bench.T
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s, sc=1.0: torch.randn(*s, device="cuda", generator=g) * sc
    F, Wh, Wc, bh, bc = rnd(B, R, D), rnd(D, U, sc=0.1), rnd(D, U, sc=0.1), rnd(U, sc=0.1), rnd(U, sc=0.1)
    fm, h0, c0 = torch.zeros(B, D, device="cuda"), torch.zeros(B, U, device="cuda"), torch.zeros(B, U, device="cuda")
    dh0, dc0, dF = rnd(B, U, sc=0.1), rnd(B, U, sc=0.1), torch.zeros(B, R, D, device="cuda")
    dW = [torch.zeros(D, U, device="cuda"), torch.zeros(U, device="cuda"), torch.zeros(D, U, device="cuda"),
          torch.zeros(U, device="cuda")]
    alpha = torch.softmax(rnd(T, B, R), dim=-1)
    ext, met = torch.zeros(B * R, device="cuda"), torch.zeros(1, device="cuda")
    work = torch.zeros(ops.attention_coverage_work_floats(T, B, R, 0), device="cuda")
    be.init_state_fwd(F, Wh, bh, Wc, bc, fm, h0, c0, B, R, D, U)
    arms = {
        "tnt_attention_coverage_f32 (yardstick, 2 launches)": lambda: be.attention_coverage(alpha, T, B, R, 0, 1e-3, ext, met, work),
        "tnt_attention_coverage_f32 ext only (1 launch)": lambda: be.attention_coverage(alpha, T, B, R, 0, 1e-3, ext, None, work),
        "tnt_init_state_fwd_f32 (1 launch)": lambda: be.init_state_fwd(F, Wh, bh, Wc, bc, fm, h0, c0, B, R, D, U),
        "tnt_init_state_bwd_f32 (2 launches)": lambda: be.init_state_bwd(dh0, dc0, h0, c0, fm, Wh, Wc, *dW, dF, B, R, D, U),
        "tnt_init_state_bwd_f32, dF = NULL (1 launch)": lambda: be.init_state_bwd(dh0, dc0, h0, c0, fm, Wh, Wc, *dW, None, B, R, D, U),
        "tnt_init_state_bwd_f32, frozen layers (1 launch)": lambda: be.init_state_bwd(dh0, dc0, h0, c0, fm, Wh, Wc, None, None, None,
                                                                                      None, dF, B, R, D, U),
    }
    res = alternate(arms, 500)
    say(f"1. launches alone, B = {B}, R = {R}, D = {D}, U = {U} (T = {T} for the yardstick): back-to-back launches in windows of "
        "500, 5 alternating windows, median us per call")
    med = {k: median(v) for k, v in res.items()}
    for k, v in res.items():
        say(f"  {k:52s}: {med[k]:6.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    keys = list(arms)
    per_launch = med[keys[1]]
    say(f"  expectation: both new entries are launch-latency bound, like the yardstick ({per_launch:.2f} us for its one-launch form)")
    for k, nl in ((keys[2], 1), (keys[3], 2)):
        ok = med[k] <= 2.0 * nl * per_launch
        say(f"    {k.split(' ')[0]}: {med[k]:.2f} us for {nl} launch(es), {med[k] / (nl * per_launch):.2f} x the yardstick's launch: "
            f"{'held' if ok else 'missed'} (held = within 2 x)")
    return med


def chain(m, batch):
    """the backward chain of a training step, re-issued on the buffers the step left"""
    be, a = ops.backend(), m.arena
    B, T = bench.B, bench.T
    R, D, A, U, Et = m.R, m.D, m.A, m.U, m.Et
    assert m._lc_seq_bwd_ok(), "config 3 runs the persistent backward chain"
    keep = m.att_keep if m._keep_stored else None
    dc0 = torch.zeros(B, U, device="cuda")

    def run(**kw):
        be.lc_seq_bwd(m.F, m.P, a.p("attention/W2/kernel"), a.p("attention/V/kernel"), m.qpre, m.alpha, keep,
                      B * R * A // 4 if keep is not None else 0, m.dP, m.dF, m.dvb, m.dqpre, a.p("lstm/recurrent_kernel"),
                      a.p("lstm/kernel")[:D], m.dHs, m.gates, m.Cs, m.dZ, m.lc_xch, T, B, R, D, A, U, 0.2, m.r_attn, m.r_lstm,
                      D + Et, m.seed, S_ATTN, S_LSTM_IN, m.drop_step, 0.0, m.seq_sync, m._guard_out(),
                      out_drop=(m.r_lstm, S_LSTM_OUT), **kw)
    res = alternate({"dc0 = NULL": run, "dc0": lambda: run(dc0=dc0)}, 200)
    m.check_device_errors()
    med = {k: median(v) for k, v in res.items()}
    say()
    say(f"2. lc_seq_bwd_kernel at config 3 (T = {T}), windows of 200 launches, 5 alternating windows, median us per launch")
    for k, v in res.items():
        say(f"  {k:12s}: {med[k]:7.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    spread = max(res["dc0 = NULL"]) - min(res["dc0 = NULL"])
    diff = med["dc0"] - med["dc0 = NULL"]
    say(f"  dc0 - NULL = {diff:+.2f} us; the plain arm's own spread is {spread:.2f} us")
    say(f"  expectation: the dc0 store costs the chain nothing outside the plain arm's own spread: "
        f"{'held' if diff <= spread else 'missed'}")


def steps(models, batch, launch_us):
    res = alternate({k: (lambda m=m: m.train_step(batch)) for k, m in models.items()}, 200, warm=30)
    med = {k: median(v) for k, v in res.items()}
    say()
    say("3a. train_step attention (config 3): windows of 200 steps, 5 alternating windows, median us per step")
    for k, v in res.items():
        say(f"  init_state {k:4s}: {med[k]:8.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    diff = med["on"] - med["off"]
    want = launch_us["fwd"] + launch_us["bwd"] + 2 * launch_us["one"]
    say(f"  on - off = {diff:+.2f} us; the added launches alone (one forward, two small products at about a launch each, "
        f"the two backward launches): about {want:.1f} us")
    say(f"  expectation: the step pays about the added launches: {'held' if diff <= 1.5 * want + 2.0 else 'missed'} "
        "(held = within 1.5 x + 2 us)")
    for m in models.values():
        m.check_device_errors()
    x, cap, a0, c0 = batch[0]
    start = torch.ones(bench.B, dtype=torch.int64)
    dec = {k: (lambda m=m: m._decode(x, a0, c0, start, bench.T, return_s=False)) for k, m in models.items()}
    res = alternate(dec, 50, warm=5)
    med = {k: median(v) for k, v in res.items()}
    say()
    say(f"3b. greedy decode {bench.B} x {bench.T} (device part, ids left on the device): windows of 50 decodes, 5 alternating "
        "windows, median us per decode")
    for k, v in res.items():
        say(f"  init_state {k:4s}: {med[k]:8.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    diff = med["on"] - med["off"]
    say(f"  on - off = {diff:+.2f} us; the added launch alone: {launch_us['fwd']:.1f} us")
    say(f"  expectation: the decode pays about one launch: {'held' if diff <= 1.5 * launch_us['fwd'] + 2.0 else 'missed'} "
        "(held = within 1.5 x + 2 us)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(MARK)
    say(f"tools/init_state_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say()
    med = launches()
    keys = list(med)
    launch_us = dict(one=med[keys[1]], fwd=med[keys[2]], bwd=med[keys[3]])
    batch, _ = bench.synth(0, "cuda")
    models = {"off": make(None), "on": make(LearnedInitState())}
    for m in models.values():
        for _ in range(5):
            m.train_step(batch)
    chain(models["on"], batch)
    steps(models, batch, launch_us)
    head = open(OUT).read().split(MARK)[0] if os.path.exists(OUT) else ""      # the first section is kept
    with open(OUT, "w") as f:
        f.write(head + "\n".join(LINES) + "\n")
