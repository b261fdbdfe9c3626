"""Timing of gradient accumulation (gradient_accumulation_steps=): the tnt_grad_accumulate_f32 launch alone over the arenas
of config 2 and config 3 (bench.py's models), per phase -- OPEN moves 8 B per parameter, ADD and CLOSE 12 -- against
tnt_weight_average_f32 blending (12 B per parameter) over the same arena in the same run; then the training step per
micro-step at k = 4 against the plain fused step at B = 64, and against the only alternative for an effective batch of
256 without accumulation, one plain step at B = 256, in caption tokens per second.  Alternating windows in one process,
medians; device events around windows of launches that end in a synchronise; every window is warmed first.

A launch repeated in a window finds whatever fits of its own operands in the 256 MiB Infinity Cache, so the launch-alone
figures are an upper bound on what the launch reaches inside a step (see tools/average_bench.py); the step figures are the
ones that count.

    python tools/grad_accum_bench.py [--no-steps]        # prints, and writes profiles/grad_accum_bench.txt
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
K = 4


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


def adam(**kw):
    return Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1, **kw)


def launches(workload, n=300, reps=5):
    """the launches alone, over the arena of a model that has trained a few steps; buffers of their own take the
    accumulator's and the gradient's place, so the model's state is left alone"""
    be = ops.backend()
    batch, _ = bench.synth(0, "cuda")
    m = bench.make_model(workload, "cuda")
    m.compile(MovingAverage(adam(), 0.99))
    for _ in range(5):
        m.train_step(batch)
    torch.cuda.synchronize()
    a = m.arena
    N = a.total
    acc, grad = torch.zeros_like(a.grad), (1e-3 * torch.randn_like(a.grad))
    grad2 = grad.clone()        # CLOSE writes its gradient operand: one of its own, so that ADD's stays constant
    sq_acc, sq_slot = torch.zeros(1, device="cuda"), torch.full((1,), 1e-6, device="cuda")
    tick = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_blend = torch.full((1,), 1000, dtype=torch.int64, device="cuda")      # every = 1: every launch blends
    arms = {
        "tnt_grad_accumulate_f32, OPEN": (8, lambda: be.grad_accumulate(acc, grad, N, 0, sq_acc, sq_slot, tick)),
        "tnt_grad_accumulate_f32, ADD": (12, lambda: be.grad_accumulate(acc, grad, N, 1, sq_acc, sq_slot, tick)),
        "tnt_grad_accumulate_f32, CLOSE": (12, lambda: be.grad_accumulate(acc, grad2, N, 2, sq_acc, sq_slot, tick)),
        "tnt_weight_average_f32, blend (yardstick)": (12, lambda: be.weight_average(a.theta, m.opt_avg, N, t_blend, 0, 0.99, False, 0, 1)),
    }
    # (ADD repeated grows acc linearly and CLOSE grad2 quadratically: 1e-3 x 1530^2 launches stays far from overflow)
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
        say(f"  {k:42s}: {med[k]:7.2f}   (windows {min(t[k]):.2f} .. {max(t[k]):.2f})   "
            f"{N * bpp / med[k] / 1e6:6.2f} TB/s at {bpp} B per parameter")
    wa = "tnt_weight_average_f32, blend (yardstick)"
    spread = max(t[wa]) / min(t[wa])
    for ph in ("ADD", "CLOSE"):
        say(f"  time of {ph} / time of the yardstick (the same 12 B per parameter): {med[f'tnt_grad_accumulate_f32, {ph}'] / med[wa]:.3f}")
    say(f"  time of OPEN x 12 / 8 / time of the yardstick: {med['tnt_grad_accumulate_f32, OPEN'] * 1.5 / med[wa]:.3f}")
    say(f"  the yardstick's own spread between its windows (max / min): {spread:.3f}")
    assert torch.isfinite(grad2).all() and torch.isfinite(acc).all()
    del m


def big_batch(batch, k):
    (x, cap, a0, c0), tgt = batch
    rep = lambda t: torch.cat([t] * k).contiguous()
    return (rep(x), rep(cap), rep(a0), rep(c0)), rep(tgt)


def steps(workload, n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
    tokens = bench.B * bench.T
    arms = {"plain fused step, B = 64": (adam, batch, tokens),
            f"accumulating micro-step, k = {K}, B = 64": (lambda: adam(gradient_accumulation_steps=K), batch, tokens),
            f"plain step, B = {K * bench.B}": (adam, big_batch(batch, K), K * tokens)}
    models = {}
    for name, (make, data, _) in arms.items():
        m = bench.make_model(workload, "cuda")
        m.compile(make())
        for _ in range(warm + (-warm) % K):
            m.train_step(data)
        models[name] = m
    out = {k: [] for k in arms}
    for _ in range(reps):
        for name, m in models.items():
            data = arms[name][1]
            for _ in range(K):
                m.train_step(data)
            out[name].append(window(lambda: m.train_step(data), n - n % K) / 1e3)
    for m in models.values():
        m.check_device_errors()
    say(f"train_step {workload}: {reps} alternating windows of {n - n % K} steps each, median ms per train_step call")
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    base = med[next(iter(arms))]
    for k, v in out.items():
        say(f"  {k:40s}: {med[k]:.4f}   (windows {min(v):.4f} .. {max(v):.4f})   x{med[k] / base:.3f} the plain step   "
            f"{arms[k][2] / med[k] / 1e3:8.2f} M caption tokens/s")
    chains = {k: bool(m.__dict__.get("_seq_lstm")) for k, m in models.items()}
    say(f"  persistent LSTM chains in use: {chains}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/grad_accum_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    for wl in ("dense", "attention"):
        launches(wl)
    if "--no-steps" not in sys.argv:
        say("")
        steps("dense")
        steps("attention")
    with open(os.path.join(ROOT, "profiles", "grad_accum_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
