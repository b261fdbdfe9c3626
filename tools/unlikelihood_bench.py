"""Timing of the unlikelihood head: tnt_softmax_cce_unlikely_f32 against tnt_softmax_cce_f32 and
tnt_softmax_cce_smooth_f32 at the workload shape (960 x 5001 = T 15 x B 64, ld 5004, dlogits aliasing logits, captions of
8 to 14 words and padding behind them), alternating in one process; the new launch also with alpha = 0 (no candidate set
is formed) and with all-zero targets (the set is formed and is empty), which splits its extra time into candidate
formation and the Q / patch part of the write pass; then the training step of config 2 and config 3 (bench.py's models
and batch) with unlikelihood 1.0 against the default step and, for config 2, the teacher-forced step with the compact
head off, alternating.  Device events around windows of launches that end in a synchronise; every window is warmed first.

    python tools/unlikelihood_bench.py [--no-steps]        # prints, and writes profiles/unlikelihood_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.optimizers import Adam, CategoricalCrossentropy  # noqa: E402

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


def captions(B, T, V, gen):
    """t-major targets of B captions: 8 to 14 words from a Zipf-like vocabulary (frequent words repeat), then 0"""
    tg = torch.zeros(T, B, dtype=torch.int32)
    for b in range(B):
        L = int(torch.randint(8, 15, (1,), generator=gen))
        w = (torch.rand(L, generator=gen) ** 3 * (V - 3)).long() + 3
        tg[:L, b] = w.int()
    return tg.reshape(-1).cuda()


def head():
    be = ops.backend()
    B, T, V, ld = 64, 15, 5001, 5004
    rows = B * T
    gen = torch.Generator().manual_seed(1)
    x0 = torch.randn(rows, ld, device="cuda")
    x = x0.clone()
    tgt = captions(B, T, V, gen)
    zero = torch.zeros_like(tgt)
    loss, corr = torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    gs = 1.0 / rows
    tg = tgt.cpu().view(T, B)
    ncand = sum(len(set(tg[:t, b].tolist()) - {0, int(tg[t, b])}) for t in range(T) for b in range(B)) / rows

    # in place: the row a launch reads is the dlogits the launch before wrote: refill it from x0 in a window of its own
    # and subtract, so every kernel sees unit-scale logits on every call
    arms = {
        "refill copy alone": lambda: x.copy_(x0),
        "tnt_softmax_cce_f32": lambda: (x.copy_(x0), be.softmax_cce(x, tgt, None, loss, corr, x, rows, V, ld, gs)),
        "tnt_softmax_cce_smooth_f32": lambda: (x.copy_(x0), be.softmax_cce_smooth(x, tgt, None, loss, corr, x, rows, V, ld, gs, 0.1)),
        "tnt_softmax_cce_unlikely_f32": lambda: (x.copy_(x0), be.softmax_cce_unlikely(x, tgt, None, loss, corr, x, B, T, V, ld, gs, 1.0)),
        "  the same, alpha = 0": lambda: (x.copy_(x0), be.softmax_cce_unlikely(x, tgt, None, loss, corr, x, B, T, V, ld, gs, 0.0)),
        "  the same, all targets 0": lambda: (x.copy_(x0), be.softmax_cce_unlikely(x, zero, None, loss, corr, x, B, T, V, ld, gs, 1.0)),
    }
    for f in arms.values():
        window(f, 50)
    n, reps = 500, 6
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    ref = med["refill copy alone"]
    say(f"head 960 x 5001 (B 64, T 15, ld 5004), dlogits in place, captions of 8 to 14 words ({ncand:.2f} candidates per row),")
    say(f"{reps} alternating windows of {n} launches each, median us per launch, the refill copy subtracted")
    for k in arms:
        v = med[k] - (0.0 if k == "refill copy alone" else ref)
        say(f"  {k:30s}: {v:6.2f}   (windows {min(t[k]):.2f} .. {max(t[k]):.2f}{'' if k == 'refill copy alone' else ' with refill'})")
    u, p, s = (med[k] - ref for k in ("tnt_softmax_cce_unlikely_f32", "tnt_softmax_cce_f32", "tnt_softmax_cce_smooth_f32"))
    a0, z = med["  the same, alpha = 0"] - ref, med["  the same, all targets 0"] - ref
    say(f"  ratio unlikely / plain {u / p:.3f}, unlikely / smooth {u / s:.3f}")
    say(f"  split of unlikely - plain = {u - p:+.2f} us: kernel without a candidate set {a0 - p:+.2f}, forming the (empty) set "
        f"{z - a0:+.2f}, x_c fetch + Q + loss terms + patching the candidate columns {u - z:+.2f}")


def steps(workload, arms, n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
    models = {}
    for name, (alpha, attrs) in arms.items():
        m = bench.make_model(workload, "cuda")
        for k, v in attrs.items():
            setattr(m, k, v)
        m.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1),
                  CategoricalCrossentropy(unlikelihood=alpha))
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
    for k, v in out.items():
        say(f"  {k:44s}: {sorted(v)[len(v) // 2]:.4f}   (windows {min(v):.4f} .. {max(v):.4f})")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/unlikelihood_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    head()
    if "--no-steps" not in sys.argv:
        steps("dense", {"default step (compact head)": (0.0, {}),
                        "teacher-forced step, compact head off": (0.0, {"compact_head": False}),
                        "unlikelihood 1.0": (1.0, {})})
        steps("attention", {"default step": (0.0, {}), "unlikelihood 1.0": (1.0, {})})
    with open(os.path.join(ROOT, "profiles", "unlikelihood_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
