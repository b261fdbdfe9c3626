"""Timing of decoupled weight decay (Adam / SGD weight_decay=, AdamW): the decay is applied where theta is already read and
written once per step, inside the update kernels, so it adds no bytes -- the expectation is "no measurable difference",
and the margin that decides "measurable" is the spread the PLAIN arm shows between its own windows in the same run.

  * the span kernel: tnt_adamw_fin_f32 against tnt_adam_fin_f32 over the spans config 2's step hands it (every variable
    behind the encoder kernel), per launch;
  * the encoder's fused update: tnt_dense_dw_adamw_fin_f32 against tnt_dense_dw_adam_fin_f32 on config 2's encoder
    kernel (20000 x 512, 64 rows), per launch;
  * the training step of config 2 and config 3 (bench.py's models) with AdamW(weight_decay=0.01, biases and
    normalisation parameters excluded) against Adam.

Alternating windows in one process, medians; device events around windows that end in a synchronise; every window is
warmed first.  Each arm has its own copy of theta / m / v, so the launch comparisons carry a control arm, the plain
launch on a third copy: it shows what two arms differ by through the placement of their buffers alone.  The learning
rate of the launch arms is 1e-7, so that thousands of updates on one fixed gradient leave the values where they are.

    python tools/weight_decay_bench.py [--no-steps]        # prints, and writes profiles/weight_decay_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.optimizers import Adam, AdamW  # noqa: E402

LINES = []
B1, B2, EPS, CLIP = 0.9, 0.98, 1e-8, 0.1


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


def report(title, t, unit="us", scale=1.0):
    """medians per arm, the plain arm's own spread, and whether the difference of the medians lies inside it"""
    say(title)
    med = {k: sorted(v)[len(v) // 2] * scale for k, v in t.items()}
    names = list(t)
    for k in names:
        say(f"  {k:42s}: {med[k]:9.4f} {unit}   (windows {min(t[k]) * scale:.4f} .. {max(t[k]) * scale:.4f})")
    plain, decay = names[0], names[1]
    spread = (max(t[plain]) - min(t[plain])) * scale
    diff = med[decay] - med[plain]
    verdict = "inside" if abs(diff) <= spread else "OUTSIDE"
    say(f"  decaying - plain = {diff:+.4f} {unit}; the plain arm's own spread is {spread:.4f} {unit}: {verdict} the margin")
    if len(names) > 2:           # the same plain launch on a second copy of the state: what two arms differ by on their own
        say(f"  control - plain  = {med[names[2]] - med[plain]:+.4f} {unit}")


def alternate(arms, n, reps):
    for f in arms.values():
        window(f, 50)
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    return t


def launches(n=500, reps=7):
    be = ops.backend()
    model = bench.make_model("dense", "cuda")
    batch, _ = bench.synth(0, "cuda")
    for _ in range(3):
        model.train_step(batch)                  # builds the arena, the optimizer state and a real gradient
    torch.cuda.synchronize()
    a, sp = model.arena, model.arena.spans
    e = a.entries["dense_img/kernel"]
    s1 = sp.first_host[e.seg + 1]
    lr, lr_t = torch.full((1,), 1e-7, device="cuda"), torch.full((1,), 1e-7, device="cuda")
    wd = torch.full((a.nseg,), 0.01, device="cuda")
    l2_out = torch.zeros(1, device="cuda")
    be.span_sqnorm(a.theta, a.grad, sp.span_seg, sp.span_off, sp.span_len, a.seg_l2, a.partial, sp.nspan)

    def span_arm(decay):
        th, m, v = a.theta.clone(), model.opt_m.clone(), model.opt_v.clone()
        arrive = torch.zeros(16, dtype=torch.int32, device="cuda")
        t, drop = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        fin = be.finalize_desc(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, l2_out, a.nseg, arrive, adam_t=t, drop_step=drop,
                               lr=lr, lr_t=lr_t, beta1=B1, beta2=B2)
        args = (th, m, v, a.grad, sp.span_seg[s1:], sp.span_off[s1:], sp.span_len[s1:], a.sq_override, sp.nspan - s1, EPS, CLIP, fin)
        return (lambda: be.adamw_fin(*args, wd)) if decay else (lambda: be.adam_fin(*args))

    say(f"the span kernel over config 2's arena behind the encoder kernel: {sp.nspan - s1} spans, "
        f"{a.total - e.size} floats, {a.nseg - 1} variables")
    report(f"  {reps} alternating windows of {n} eager launches each, median us per launch",
           alternate({"tnt_adam_fin_f32 (plain)": span_arm(False), "tnt_adamw_fin_f32 (decaying)": span_arm(True),
                      "tnt_adam_fin_f32 (plain, control)": span_arm(False)}, n, reps))

    N, E, rows = model.N, model.E, 64
    x = torch.randn(rows, model.ldx, device="cuda")
    dpre = torch.randn(rows, E, device="cuda") * 0.01
    sl = slice(e.off, e.off + e.size)
    k0, k1 = sp.first_host[e.seg], sp.first_host[e.seg + 1]
    ovr = a.sq_override[e.seg:e.seg + 1]

    def enc_arm(decay):
        th, m, v = a.theta[sl].clone(), model.opt_m[sl].clone(), model.opt_v[sl].clone()
        args = (x, dpre, th, m, v, e.l2, a.partial, k0, k1, ovr, lr_t, B1, B2, EPS, CLIP, N, E, rows, model.ldx)
        return (lambda: be.dense_dw_adamw_fin(*args, lr, 0.01)) if decay else (lambda: be.dense_dw_adam_fin(*args))

    say("")
    say(f"the encoder's fused update: X^T D ({N} x {E}, {rows} rows) + clip + Adam on the strips, {e.size} floats")
    report(f"  {reps} alternating windows of {n} eager launches each, median us per launch",
           alternate({"tnt_dense_dw_adam_fin_f32 (plain)": enc_arm(False), "tnt_dense_dw_adamw_fin_f32 (decaying)": enc_arm(True),
                      "tnt_dense_dw_adam_fin_f32 (plain, control)": enc_arm(False)}, n, reps))
    model.check_device_errors()


def adam():
    return Adam(learning_rate=1e-4, beta_1=B1, beta_2=B2, epsilon=EPS, clipnorm=CLIP)


def adamw():
    opt = AdamW(learning_rate=1e-4, weight_decay=0.01, beta_1=B1, beta_2=B2, epsilon=EPS, clipnorm=CLIP)
    opt.exclude_from_weight_decay(var_names=["bias", "gamma", "beta"])
    return opt


def steps(workload, n=200, warm=30, reps=5):
    batch, _ = bench.synth(0, "cuda")
    arms = {"Adam": adam, "AdamW(weight_decay=0.01)": adamw}
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
    report(f"train_step {workload}: {reps} alternating windows of {n} steps each, median ms per step", out, unit="ms")
    m = models["AdamW(weight_decay=0.01)"]
    say(f"  decayed variables: {int((m.seg_wd > 0).sum())} of {m.arena.nseg}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/weight_decay_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    launches()
    if "--no-steps" not in sys.argv:
        for wl in ("dense", "attention"):
            say("")
            steps(wl)
    with open(os.path.join(ROOT, "profiles", "weight_decay_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
