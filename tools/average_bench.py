"""Timing of weight averaging: the tnt_weight_average_f32 launch alone over the parameter arenas of config 2 and config 3
(bench.py's models), blending, seeding (copy) and skipping, and the bytes/s that implies at 12 B per parameter (8 B for a
copy) -- against tnt_adam_fin_f32, the unchanged optimizer stream, over the same arena at its 28 B per parameter, in the
same run; tnt_swap_f32 (16 B per parameter); then the training step of both configs with averaging off, every = 1 and
every = 10.  Alternating windows in one process, medians; device events around windows of launches that end in a
synchronise; every window is warmed first.

A launch repeated in a window finds whatever fits of its own operands in the 256 MiB Infinity Cache, so the launch-alone
figures are an upper bound on what the launch reaches inside a step, where ~160 MB of other traffic lie between two of its
runs (non-temporal avg, see csrc/tnt_common.h); the step figures are the ones that count.

    python tools/average_bench.py [--no-steps]        # prints, and writes profiles/average_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.optimizers import Adam, MovingAverage  # noqa: E402

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


def adam():
    return Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def launches(workload, n=300, reps=5):
    """the launches alone, over the arena of a model that has trained a few steps (real span table, norms and moments)"""
    be = ops.backend()
    batch, _ = bench.synth(0, "cuda")
    m = bench.make_model(workload, "cuda")
    m.compile(MovingAverage(adam(), 0.99))
    for _ in range(5):
        m.train_step(batch)
    torch.cuda.synchronize()
    a, sp, opt = m.arena, m.arena.spans, m.optimizer
    N = a.total
    t_blend = torch.full((1,), 1000, dtype=torch.int64, device="cuda")      # every = 1: every launch blends
    t_skip = torch.full((1,), 1001, dtype=torch.int64, device="cuda")       # every = 7: r = 1000, r % 7 != 0
    t_copy = torch.zeros(1, dtype=torch.int64, device="cuda")               # t <= s: every launch seeds
    # tnt_adam_fin_f32 over the WHOLE arena (in the step the dense encoder kernel has an update launch of its own), with
    # counters of its own so that the model's are left alone
    t_fin = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    arrive = torch.zeros(16, dtype=torch.int32, device="cuda")
    desc = be.finalize_desc(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, m.met[2:3], a.nseg, arrive, adam_t=t_fin,
                            lr=m.lr_dev, lr_t=m.lr_t_dev, beta1=opt.beta_1, beta2=opt.beta_2)
    arms = {
        "tnt_weight_average_f32, blend": (12, lambda: be.weight_average(a.theta, m.opt_avg, N, t_blend, 0, 0.99, False, 0, 1)),
        "tnt_weight_average_f32, copy": (8, lambda: be.weight_average(a.theta, m.opt_avg, N, t_copy, 0, 0.99, False, 0, 1)),
        "tnt_weight_average_f32, skipped step": (0, lambda: be.weight_average(a.theta, m.opt_avg, N, t_skip, 0, 0.99, False, 0, 7)),
        "tnt_swap_f32": (16, lambda: be.swap(a.theta, m.opt_avg, N)),
        "tnt_adam_fin_f32 (yardstick)": (28, lambda: be.adam_fin(a.theta, m.opt_m, m.opt_v, a.grad, sp.span_seg, sp.span_off, sp.span_len,
                                                                  a.sq_override, sp.nspan, opt.epsilon, 0.1, desc)),
    }
    for _, f in arms.values():
        window(f, 30)
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, (_, f) in arms.items():
            t[k].append(window(f, n))
    say(f"{workload}: arena of {N:,d} parameters ({N * 4 / 1e6:.1f} MB per buffer); {reps} alternating windows of {n} launches each, "
        "median us per launch")
    med = {}
    for k, (bpp, _) in arms.items():
        med[k] = sorted(t[k])[len(t[k]) // 2]
        rate = f"{N * bpp / med[k] / 1e6:6.2f} TB/s at {bpp} B per parameter" if bpp else "no parameter traffic"
        say(f"  {k:38s}: {med[k]:7.2f}   (windows {min(t[k]):.2f} .. {max(t[k]):.2f})   {rate}")
    wa, fin = med["tnt_weight_average_f32, blend"], med["tnt_adam_fin_f32 (yardstick)"]
    say(f"  bytes/s of the blend / bytes/s of the yardstick: {(12 / wa) / (28 / fin):.3f}")
    assert torch.isfinite(m.opt_avg).all()
    del m


def steps(workload, arms, n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
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


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/average_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    for wl in ("dense", "attention"):
        launches(wl)
    if "--no-steps" not in sys.argv:
        arms = {"averaging off": adam, "MovingAverage, every = 1": lambda: MovingAverage(adam(), 0.99),
                "MovingAverage, every = 10": lambda: MovingAverage(adam(), 0.99, every=10)}
        say("")
        steps("dense", arms)
        steps("attention", arms)
    with open(os.path.join(ROOT, "profiles", "average_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
