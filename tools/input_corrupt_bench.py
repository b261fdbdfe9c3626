"""Timing of the training-time input corruption (scan_dropout= / word_dropout= of nic.NIC and lc_nic.NIC): ONE launch,
tnt_input_corrupt_f32, on the staged batch behind the staging launch and outside the recorded step.  Scan dropout also
declines the stage_fwd ride of config 2, so its staging comes back as a launch of its own.

  * the launch alone at config 2's shapes (64 x 20 000 betas, T = 15) and at config 3's (the same, with the voxel-major
    copy xT), at rates 0.1 and 0.25: scan part only, word part only, both;
  * the training step of config 2 and config 3 (bench.py's models) in four arms -- without either option, word dropout
    only, scan dropout only, both -- with the plain arm measured twice: what its two measurements and its own windows
    differ by is the margin each arm is judged against.

Alternating windows in one process, medians; device events around windows that end in a synchronise; every window is
warmed first (tools/weight_decay_bench.py's helpers).  The launch arms repeat one step word on one buffer: the same rows
fire in every launch, so the traffic is that of one step.

    python tools/input_corrupt_bench.py [--no-steps]        # prints, and writes profiles/input_corrupt_bench.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.model_base import S_SCAN_DROP, S_WORD_DROP, ScanDropout, WordDropout  # noqa: E402
from weight_decay_bench import LINES, alternate, say, window  # noqa: E402

RATES = (0.1, 0.25)
STEP_RATE, UNK = 0.1, 3


def med(v):
    return sorted(v)[len(v) // 2]


def kernel(config, with_xT, n=2000, reps=7):
    be = ops.backend()
    (x, cap, _, _), _ = bench.synth(0, "cuda")[0]
    B, N = x.shape
    T = cap.shape[1]
    xs, caps = x.clone(), cap.clone()
    xT = torch.zeros(N, (B + 3) // 4 * 4, device="cuda") if with_xT else None
    null = torch.randn(N, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = lambda sr, wr: (lambda: be.input_corrupt(xs, N, xT, xT.shape[1] if with_xT else 0, caps, B, T, N, bench.V, sr, null, wr,
                                                   UNK, 42, S_SCAN_DROP, S_WORD_DROP, step))
    arms = {}
    for r in RATES:
        arms[f"scan part only, rate {r}"] = run(r, 0.0)
        arms[f"word part only, rate {r}"] = run(0.0, r)
        arms[f"both parts, rate {r}"] = run(r, r)
    t = alternate(arms, n, reps)
    say(f"tnt_input_corrupt_f32 alone at config {config}'s shapes: x {B} x {N}{', xT ' + str(N) + ' x ' + str(xT.shape[1]) if with_xT else ''}, "
        f"cap {B} x {T}; {reps} alternating windows of {n} back-to-back eager launches, median us per launch")
    for k, v in t.items():
        say(f"  {k:46s}: {med(v):9.4f} us   (windows {min(v):.4f} .. {max(v):.4f})")
    from oracle.philox import uniform24
    elig = cap.cpu().numpy() != 0
    elig[:, 0] = False
    for r in RATES:
        rows = uniform24(B, 42, S_SCAN_DROP, 0) < np.float32(r)
        words = (uniform24(B * T, 42, S_WORD_DROP, 0).reshape(B, T) < np.float32(r)) & elig
        say(f"  rate {r} at this step word: {int(rows.sum())} of {B} rows and {int(words.sum())} of {int(elig.sum())} eligible "
            f"tokens fire")


def steps(workload, n=200, warm=30, reps=5):
    batch, _ = bench.synth(0, "cuda")
    arms = {"without either option": (None, None), "word dropout only": (None, STEP_RATE), "scan dropout only": (STEP_RATE, None),
            "both": (STEP_RATE, STEP_RATE), "without either option, again": (None, None)}
    models = {}
    for name, (sr, wr) in arms.items():
        m = bench.make_model(workload, "cuda")
        m.scan_dropout = None if sr is None else ScanDropout(sr)
        m.word_dropout = None if wr is None else WordDropout(wr, UNK)
        for _ in range(warm):
            m.train_step(batch)
        models[name] = m
    out = {k: [] for k in arms}
    for _ in range(reps):
        for name, m in models.items():
            for _ in range(5):
                m.train_step(batch)
            out[name].append(window(lambda: m.train_step(batch), n) / 1e3)
    for m in models.values():
        m.check_device_errors()
    say(f"train_step {workload} (config {'2' if workload == 'dense' else '3'}), rates {STEP_RATE}: {reps} alternating windows of {n} "
        f"steps each, median ms per step")
    names = list(arms)
    for k in names:
        say(f"  {k:46s}: {med(out[k]):9.4f} ms   (windows {min(out[k]):.4f} .. {max(out[k]):.4f})")
    plain, again = names[0], names[-1]
    margin = max(abs(med(out[again]) - med(out[plain])), max(out[plain]) - min(out[plain]), max(out[again]) - min(out[again]))
    say(f"  plain against plain = {(med(out[again]) - med(out[plain])) * 1e3:+.2f} us; margin (that, or the plain arm's own windows) "
        f"{margin * 1e3:.2f} us")
    for k in names[1:-1]:
        d = (med(out[k]) - med(out[plain])) * 1e3
        say(f"  {k:24s} - plain = {d:+7.2f} us: {'inside' if abs(d) <= margin * 1e3 else 'OUTSIDE'} the margin")
    if workload == "dense":
        say(f"  the staging rode in the encoder forward (stage_fwd): "
            + ", ".join(f"{k}: {'yes' if models[k]._route.stage_fwd_done else 'no'}" for k in names[:-1]))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/input_corrupt_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    kernel(2, False)
    kernel(3, True)
    if "--no-steps" not in sys.argv:
        for wl in ("dense", "attention"):
            say("")
            steps(wl)
    with open(os.path.join(ROOT, "profiles", "input_corrupt_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
