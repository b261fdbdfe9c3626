"""Timing of the attention coverage penalty (lc_nic.NIC(attention_coverage=...)) on config 3 (bench.py's attention model and
batch): the training step with the term on the time axis and on the batch axis against the default step, alternating windows
in one process (device events around windows of steps that end in a synchronise; every window is warmed first), medians.
Then, from kernel traces taken in runs of their own (one profiler run per arm), the average time per launch of
attention_coverage_kernel and of the final sum behind it, of dropout4_metric_kernel (which carries the step's attention metric:
the launch-bound yardstick in the same trace) and of lc_seq_bwd_kernel with the rider off and on.

    python tools/coverage_bench.py                     # prints, and writes the step-time section of profiles/coverage_bench.txt
    for arm in off time batch; do                      # the traces: runs of their own
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR/$arm -- python tools/coverage_bench.py --steps-only $arm 200
    done
    python tools/coverage_bench.py --trace-summary DIR 200        # appends the per-launch section (needs no GPU)

The file's first section, the feature-off step against the parent commit (bench.py, alternating runs), is kept by both.
"""
import csv
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.lc_nic import NIC, synthetic_groups  # noqa: E402
from masters_thesis_amd.model_base import AttentionCoverage  # noqa: E402
from masters_thesis_amd.optimizers import Adam  # noqa: E402

WEIGHT = 1.0
ARMS = {"off": None, "time": AttentionCoverage(WEIGHT, "time"), "batch": AttentionCoverage(WEIGHT, "batch")}
OUT = os.path.join(ROOT, "profiles", "coverage_bench.txt")
MARK = "# ---- step time with the feature on (tools/coverage_bench.py)"
TRACE_MARK = "# ---- per-launch times (tools/coverage_bench.py --trace-summary)"
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n          # ms per call


def make(cov):
    """bench.make_model("attention"), with the coverage term"""
    groups = synthetic_groups(bench.N_VOX, 360, 32, seed=42)
    m = NIC(groups, bench.U, 512, bench.E, 32, bench.V, bench.T, 0.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 0.00003, 0.00001,
            device="cuda", seed=42, attention_coverage=cov)
    m.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def steps(n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
    models = {}
    for name, cov in ARMS.items():
        m = make(cov)
        for _ in range(warm):
            m.train_step(batch)
        models[name] = m
    out = {k: [] for k in ARMS}
    for _ in range(reps):
        for name, m in models.items():
            for _ in range(5):
                m.train_step(batch)
            out[name].append(window(lambda: m.train_step(batch), n))
    last = {}
    for name, m in models.items():
        m.check_device_errors()
        last[name] = m.train_step(batch).as_floats()
    say(f"train_step attention (config 3), weight {WEIGHT}: {reps} alternating windows of {n} steps each, median ms per step")
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    for k, v in out.items():
        extra = "" if k == "off" else f"   on - off = {1e3 * (med[k] - med['off']):+.1f} us   coverage {last[k]['coverage']:.4f}"
        say(f"  {'default step' if k == 'off' else 'attention_coverage, axis ' + k:34s}: {med[k]:.4f}   "
            f"(windows {min(v):.4f} .. {max(v):.4f}){extra}")
    say(f"  largest spread between the windows of one arm: {1e3 * max(max(v) - min(v) for v in out.values()):.1f} us")


def trace_summary(root, n):
    """per-launch averages from the kernel stats of one profiler run per arm, <root>/<arm>/**/*kernel_stats.csv"""
    say(f"kernel trace (rocprofv3 --kernel-trace --stats, one run of {n} steps per arm): average us per launch")
    for arm in ARMS:
        files = glob.glob(f"{root}/{arm}/**/*kernel_stats.csv", recursive=True)
        if not files:
            say(f"  {arm}: no kernel stats under {root}/{arm}")
            continue
        rows = list(csv.DictReader(open(files[0])))
        parts = []
        # (the step's attention metric rides in dropout4_metric_kernel, a launch-bound launch of the same trace: the yardstick)
        for key in ("attention_coverage_kernel", "attention_metric_final_kernel", "dropout4_metric_kernel", "lc_seq_bwd_kernel",
                    "lc_seq_fwd_kernel"):
            got = [(int(x["Calls"]), float(x["AverageNs"]) / 1e3) for x in rows if key in x["Name"]]
            if got:
                calls = sum(c for c, _ in got)
                parts.append(f"{key} {sum(c * a for c, a in got) / calls:.2f} ({calls / n:.2f} launches per step)")
        say(f"  {arm:5s}: " + "; ".join(parts))


def write(mark):
    """the file is kept up to ``mark``; what was said replaces the rest"""
    head = open(OUT).read().split(mark)[0] if os.path.exists(OUT) else ""
    with open(OUT, "w") as f:
        f.write(head + "\n".join(LINES) + "\n")


if __name__ == "__main__":
    if "--trace-summary" in sys.argv:                  # no GPU needed
        i = sys.argv.index("--trace-summary")
        say(TRACE_MARK)
        trace_summary(sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 200)
        write(TRACE_MARK)
        sys.exit(0)
    assert torch.cuda.is_available(), "needs a GPU"
    if "--steps-only" in sys.argv:
        i = sys.argv.index("--steps-only")
        arm, n = sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 200
        batch, _ = bench.synth(0, "cuda")
        m = make(ARMS[arm])
        for _ in range(n):
            m.train_step(batch)
        torch.cuda.synchronize()
        m.check_device_errors()
        sys.exit(0)
    say(MARK)
    say(f"tools/coverage_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    steps()
    write(MARK)
