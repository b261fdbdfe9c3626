"""Timing of the on-device learning-rate schedule: the training step of config 2 and config 3 (bench.py's models) with a
float learning rate -- the launch sequence the step had before schedules existed, tests/test_host_lr_schedule.py holds
that, so it is the baseline -- and with Warmup(CosineDecay), which adds one tnt_lr_schedule_f32 launch in front of the
step's first reader of lr_dev; and that launch alone next to tnt_step_tick, the other one-thread launch of the update,
on counters of their own.  Alternating windows in one process, medians; device events around windows that end in a
synchronise; every window is warmed first.

A launch alone in a window is a launch behind an identical launch, back to back in one stream: the figure is the cost of
one minimum-length dependent launch, which is what it is inside the step too.

    python tools/lr_schedule_bench.py [--no-steps]        # prints, and writes profiles/lr_schedule_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.optimizers import Adam  # noqa: E402
from masters_thesis_amd.schedules import CosineDecay, Warmup  # noqa: E402

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
    return a.elapsed_time(b) / n * 1e3          # us per call


def adam(lr):
    return Adam(learning_rate=lr, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def schedule():
    """1000 warm-up steps to 1e-4, then a cosine over 100 000 steps: the timed windows stay inside the schedule"""
    return Warmup(CosineDecay(1e-4, 100_000, alpha=0.01), 1000)


def launches(n=2000, reps=5):
    be = ops.backend()
    params = torch.tensor(schedule().params(), dtype=torch.float64, device="cuda")
    counters = {"in the warm-up": 500, "in the cosine": 50_000}
    step = {k: torch.full((1,), v, dtype=torch.int64, device="cuda") for k, v in counters.items()}
    lr, lr_t = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    t_tick = torch.zeros(1, dtype=torch.int64, device="cuda")
    drop = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.full((1,), 1e-4, device="cuda")
    arms = {f"tnt_lr_schedule_f32, {k}": (lambda s=s: be.lr_schedule(s, params, lr)) for k, s in step.items()}
    arms["tnt_step_tick (yardstick)"] = lambda: be.step_tick(t_tick, drop, one, lr_t, 0.9, 0.98)
    for f in arms.values():
        window(f, 100)
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    say(f"the launch alone: {reps} alternating windows of {n} eager launches each, median us per launch")
    for k, v in t.items():
        say(f"  {k:38s}: {sorted(v)[len(v) // 2]:6.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    # the same launches recorded once and replayed as one hipGraph of n nodes: the device-side cost of a dependent launch
    graphs = {}
    for k, f in arms.items():
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            for _ in range(n):
                f()
        g.replay()
        graphs[k] = g
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, g in graphs.items():
            t[k].append(window(g.replay, 3) / n)
    say(f"inside a captured sequence: {reps} alternating windows of 3 replays of a hipGraph of {n} such launches, median us per launch")
    for k, v in t.items():
        say(f"  {k:38s}: {sorted(v)[len(v) // 2]:6.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    assert torch.isfinite(lr).all()


def steps(workload, n=200, warm=30, reps=5):
    batch, _ = bench.synth(0, "cuda")
    arms = {"float learning rate": lambda: adam(1e-4), "Warmup(CosineDecay)": lambda: adam(schedule())}
    models = {}
    for name, make in arms.items():
        m = bench.make_model(workload, "cuda")
        m.compile(make())
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
    say(f"train_step {workload}: {reps} alternating windows of {n} steps each, median ms per step")
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    base = med[next(iter(arms))]
    for k, v in out.items():
        say(f"  {k:28s}: {med[k]:.4f}   (windows {min(v):.4f} .. {max(v):.4f})   {(med[k] - base) * 1e3:+6.1f} us")
    m = models["Warmup(CosineDecay)"]
    say(f"  after {m.iterations} updates lr = {float(m.lr_dev.item()):.6g} (host: {schedule()(m.iterations - 1):.6g})")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/lr_schedule_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    launches()
    if "--no-steps" not in sys.argv:
        for wl in ("dense", "attention"):
            say("")
            steps(wl)
    with open(os.path.join(ROOT, "profiles", "lr_schedule_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
