"""Timing of knowledge distillation (CategoricalCrossentropy(distillation=...) / set_teacher): the
tnt_softmax_cce_distill_f32 launch alone at 960 x 5001 (config 2's B * T rows) against tnt_softmax_cce_f32 and
tnt_softmax_cce_smooth_f32 on the same rows -- it moves three row passes of bytes (two reads, one write) where they move
two, so the expectation under test is <= 1.5 x the plain launch's time plus the spread the plain launch shows between
its own windows --; then the teacher's inference forward alone and the whole distilled train_step at config 2 (dense
student under a dense and under an attention teacher) and config 3 (attention student, attention teacher) against the
plain step, and the plain dense step without the compact head and the staging ride, which a distilled step gives up.
Alternating windows in one process, medians; device events around windows of launches that end in a synchronise; every
window is warmed first.

A launch repeated in a window finds its operands (19 MB per row pass) in the 256 MiB Infinity Cache, so the
launch-alone bytes/s are an upper bound on what the launch reaches inside a step; the step figures are the ones that
count.

    python tools/distill_bench.py [--no-steps]        # prints, and writes profiles/distill_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.optimizers import Adam, CategoricalCrossentropy, Distillation  # noqa: E402

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


def median(v):
    return sorted(v)[len(v) // 2]


def launches(n=300, reps=5):
    """the head launches alone, out of place so that every launch reads the same logits"""
    be = ops.backend()
    rows, V = bench.B * bench.T, bench.V
    ld = (V + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 3.0 * torch.randn(rows, ld, device="cuda", generator=g)
    u = 4.0 * torch.randn(rows, ld, device="cuda", generator=g)
    y = torch.randint(0, V, (rows,), device="cuda", generator=g).to(torch.int32)
    dl = torch.zeros(rows, ld, device="cuda")
    loss, kl, corr = (torch.zeros(rows, device="cuda") for _ in range(3))
    gs = 1.0 / rows
    row_pass = rows * V * 4
    arms = {
        "tnt_softmax_cce_f32 (plain)": (2, lambda: be.softmax_cce(x, y, None, loss, corr, dl, rows, V, ld, gs)),
        "tnt_softmax_cce_smooth_f32, eps 0.1": (2, lambda: be.softmax_cce_smooth(x, y, None, loss, corr, dl, rows, V, ld, gs, 0.1)),
        "tnt_softmax_cce_distill_f32, a 0.5 t 2": (3, lambda: be.softmax_cce_distill(x, u, y, loss, kl, corr, dl, rows, V, ld, ld, gs,
                                                                                      0.5, 2.0)),
        "tnt_softmax_cce_distill_f32, a 0.5 t 1": (3, lambda: be.softmax_cce_distill(x, u, y, loss, kl, corr, dl, rows, V, ld, ld, gs,
                                                                                      0.5, 1.0)),
    }
    for _, f in arms.values():
        window(f, 30)
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, (_, f) in arms.items():
            t[k].append(window(f, n))
    assert torch.isfinite(dl).all() and torch.isfinite(kl).all()
    say(f"head launches alone, {rows} x {V} (ld {ld}), training form out of place: {reps} alternating windows of {n} launches "
        "each, median us per launch")
    med = {k: median(v) for k, v in t.items()}
    for k, (passes, _) in arms.items():
        say(f"  {k:42s}: {med[k]:7.2f}   (windows {min(t[k]):.2f} .. {max(t[k]):.2f})   "
            f"{passes * row_pass / med[k] / 1e6:6.2f} TB/s at {passes} row passes of {row_pass / 1e6:.1f} MB")
    plain = "tnt_softmax_cce_f32 (plain)"
    spread = max(t[plain]) - min(t[plain])
    bound = 1.5 * med[plain] + spread
    say(f"  the plain launch's own spread between its windows: {spread:.2f} us (max / min {max(t[plain]) / min(t[plain]):.3f})")
    for k in list(arms)[2:]:
        verdict = "meets" if med[k] <= bound else "MISSES"
        say(f"  {k}: x{med[k] / med[plain]:.3f} the plain launch; {verdict} the expectation <= 1.5 x plain + spread = {bound:.2f} us")
    say(f"  tnt_softmax_cce_smooth_f32: x{med['tnt_softmax_cce_smooth_f32, eps 0.1'] / med[plain]:.3f} the plain launch")


def adam():
    return Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1)


def steps(n=200, warm=40, reps=3):
    batch, _ = bench.synth(0, "cuda")
    B, T = bench.B, bench.T
    loss = lambda: CategoricalCrossentropy(from_logits=False, reduction="none", distillation=Distillation(0.5, 2.0))

    def student(workload, teacher=None, **attrs):
        m = bench.make_model(workload, "cuda")
        for k, v in attrs.items():
            setattr(m, k, v)
        if teacher is not None:
            m.compile(adam(), loss())
            m.set_teacher(bench.make_model(teacher, "cuda"))
        return m
    models = {
        "config 2, plain step": student("dense"),
        "config 2, plain step, compact_head and stage_fwd off": student("dense", compact_head=False, stage_fwd=False),
        "config 2, distilled, dense teacher": student("dense", "dense"),
        "config 2, distilled, attention teacher": student("dense", "attention"),
        "config 3, plain step": student("attention"),
        "config 3, distilled, attention teacher": student("attention", "attention"),
    }
    arms = {k: (lambda m=m: m.train_step(batch)) for k, m in models.items()}
    for k in ("config 2, distilled, dense teacher", "config 2, distilled, attention teacher"):
        m = models[k]
        arms[k.replace("distilled, ", "the ") + "'s forward alone (_teach)"] = lambda m=m: m._teach(batch, B, T)
    for f in arms.values():
        for _ in range(warm):
            f()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            for _ in range(5):
                f()
            out[k].append(window(f, n) / 1e3)
    for m in models.values():
        m.check_device_errors()
        if m.teacher is not None:
            m.teacher.check_device_errors()
    say(f"train_step at B = {B}, T = {T}, V = {bench.V}: {reps} alternating windows of {n} calls each, median ms per call")
    med = {k: median(v) for k, v in out.items()}
    for k, v in out.items():
        base = med["config 3, plain step" if k.startswith("config 3") else "config 2, plain step"]
        say(f"  {k:62s}: {med[k]:.4f}   (windows {min(v):.4f} .. {max(v):.4f})   x{med[k] / base:.3f} the plain step")
    p2 = med["config 2, plain step"]
    say(f"  config 2: the loss of the compact head and the staging ride costs {med['config 2, plain step, compact_head and stage_fwd off'] - p2:+.4f} ms; "
        f"a distilled step costs {med['config 2, distilled, dense teacher'] - p2:+.4f} ms (dense teacher) / "
        f"{med['config 2, distilled, attention teacher'] - p2:+.4f} ms (attention teacher) over the plain step")
    say(f"  config 3: a distilled step costs {med['config 3, distilled, attention teacher'] - med['config 3, plain step']:+.4f} ms "
        "over the plain step")
    chains = {k: (bool(m.__dict__.get("_seq_lstm")), None if m.teacher is None else bool(m.teacher.__dict__.get("_seq_lstm")))
              for k, m in models.items()}
    say(f"  persistent LSTM chains in use (student, teacher): {chains}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/distill_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    launches()
    if "--no-steps" not in sys.argv:
        say("")
        steps()
    with open(os.path.join(ROOT, "profiles", "distill_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
