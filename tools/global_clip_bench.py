"""Timing of global-norm gradient clipping (Adam / SGD global_clipnorm=).  The update kernels read one word in the place of
their per-variable clip norm, so the gclip launches should cost what the plain ones cost or less; what the mode adds is
ONE dependent launch per step, tnt_global_sqnorm_f32 (one workgroup), between the norm launch and the first update.

  * the reduction launch alone, both input forms, at the span tables of config 2 and config 3 (bench.py's models);
  * each gclip update launch against its plain arm over config 2's arena: tnt_adam_fin_gclip_f32 / tnt_adam_fin_f32 on
    the spans behind the encoder kernel, tnt_dense_dw_adam_fin_gclip_f32 / tnt_dense_dw_adam_fin_f32 on the encoder
    kernel, tnt_adam_gclip_f32 / tnt_adam_f32 and tnt_sgd_gclip_f32 / tnt_sgd_f32 over the same spans.  The plain arm is
    measured twice (a second copy of the state): the difference of the two plain arms is the margin;
  * the training step of config 2 and config 3 with Adam(global_clipnorm=5.0) against Adam(clipnorm=0.1), the plain arm
    twice again.

Alternating windows in one process, medians; device events around windows that end in a synchronise; every window is
warmed first (tools/weight_decay_bench.py's helpers).  The learning rate of the launch arms is 1e-7, so that thousands
of updates on one fixed gradient leave the values where they are.

    python tools/global_clip_bench.py [--no-steps]        # prints, and writes profiles/global_clip_bench.txt
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
from weight_decay_bench import B1, B2, CLIP, EPS, LINES, alternate, say, window  # noqa: E402

GCLIP = 5.0


def report(title, t, unit="us", scale=1.0):
    """medians per arm (plain, gclip, plain again); the margin is what the two plain arms differ by"""
    say(title)
    med = {k: sorted(v)[len(v) // 2] * scale for k, v in t.items()}
    names = list(t)
    for k in names:
        say(f"  {k:46s}: {med[k]:9.4f} {unit}   (windows {min(t[k]) * scale:.4f} .. {max(t[k]) * scale:.4f})")
    plain, gc, again = names
    margin = max(abs(med[again] - med[plain]), (max(t[plain]) - min(t[plain])) * scale)
    diff = med[gc] - med[plain]
    say(f"  gclip - plain = {diff:+.4f} {unit}; plain against plain = {med[again] - med[plain]:+.4f} {unit}, margin {margin:.4f} {unit}: "
        f"{'inside' if abs(diff) <= margin else 'OUTSIDE'} the margin")


def reduction(workload, n=2000, reps=7):
    be = ops.backend()
    model = bench.make_model(workload, "cuda")
    batch, _ = bench.synth(0, "cuda")
    for _ in range(3):
        model.train_step(batch)
    torch.cuda.synchronize()
    a, sp = model.arena, model.arena.spans
    gsq = torch.zeros(1, device="cuda")
    arms = {"tnt_global_sqnorm_f32 (fin form)": lambda: be.global_sqnorm(gsq, a.nseg, sq_override=a.sq_override, partial=a.partial,
                                                                          seg_first=sp.seg_first),
            "tnt_global_sqnorm_f32 (table form)": lambda: be.global_sqnorm(gsq, a.nseg, sq_override=a.sq_override, sq=a.sq)}
    t = alternate(arms, n, reps)
    say(f"the reduction launch at config {'2' if workload == 'dense' else '3'}'s span table ({workload}): {a.nseg} variables, "
        f"{sp.nspan} spans; {reps} alternating windows of {n} back-to-back eager launches, median us per launch")
    for k, v in t.items():
        say(f"  {k:46s}: {sorted(v)[len(v) // 2]:9.4f} us   (windows {min(v):.4f} .. {max(v):.4f})")
    model.check_device_errors()
    return model


def launches(model, n=500, reps=7):
    be = ops.backend()
    a, sp = model.arena, model.arena.spans
    e = a.entries["dense_img/kernel"]
    s1 = sp.first_host[e.seg + 1]
    lr, lr_t = torch.full((1,), 1e-7, device="cuda"), torch.full((1,), 1e-7, device="cuda")
    gsq = torch.full((1,), 4 * GCLIP * GCLIP, device="cuda")             # cs = 0.5: the clip is active
    l2_out = torch.zeros(1, device="cuda")
    be.seg_sqnorm(a.theta, a.grad, sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, a.seg_l2, a.partial, a.sq, a.wsq, None,
                  sp.nspan, a.nseg)
    spans = (sp.span_seg[s1:], sp.span_off[s1:], sp.span_len[s1:])
    title = f"  {reps} alternating windows of {n} eager launches each, median us per launch"

    def fin_arm(gc):
        th, m, v = a.theta.clone(), model.opt_m.clone(), model.opt_v.clone()
        arrive = torch.zeros(16, dtype=torch.int32, device="cuda")
        t, drop = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        fin = be.finalize_desc(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, l2_out, a.nseg, arrive, adam_t=t, drop_step=drop,
                               lr=lr, lr_t=lr_t, beta1=B1, beta2=B2)
        args = (th, m, v, a.grad, *spans, a.sq_override, sp.nspan - s1, EPS)
        return (lambda: be.adam_fin_gclip(*args, GCLIP, fin, gsq)) if gc else (lambda: be.adam_fin(*args, CLIP, fin))

    def ring_arm(gc):
        th, m, v = a.theta.clone(), model.opt_m.clone(), model.opt_v.clone()
        args = (th, m, v, a.grad, *spans, a.seg_l2, a.sq, a.sq_override, sp.nspan - s1, 0.0, lr_t, B1, B2, EPS)
        return (lambda: be.adam_gclip(*args, GCLIP, gsq)) if gc else (lambda: be.adam(*args, CLIP))

    def sgd_arm(gc):
        th, m = a.theta.clone(), model.opt_m.clone()
        args = (th, m, a.grad, *spans, a.seg_l2, a.sq, a.sq_override, sp.nspan - s1, 0.0, lr, 0.9)
        return (lambda: be.sgd_gclip(*args, GCLIP, gsq)) if gc else (lambda: be.sgd(*args, CLIP))

    N, E, rows = model.N, model.E, 64
    x = torch.randn(rows, model.ldx, device="cuda")
    dpre = torch.randn(rows, E, device="cuda") * 0.01
    sl = slice(e.off, e.off + e.size)
    k0, k1 = sp.first_host[e.seg], sp.first_host[e.seg + 1]
    ovr = a.sq_override[e.seg:e.seg + 1]

    def enc_arm(gc):
        th, m, v = a.theta[sl].clone(), model.opt_m[sl].clone(), model.opt_v[sl].clone()
        args = (x, dpre, th, m, v, e.l2, a.partial, k0, k1, ovr, lr_t, B1, B2, EPS)
        tail = (N, E, rows, model.ldx)
        return (lambda: be.dense_dw_adam_fin_gclip(*args, GCLIP, *tail, gsq)) if gc else (lambda: be.dense_dw_adam_fin(*args, CLIP, *tail))

    say("")
    say(f"the update launches over config 2's arena: {sp.nspan - s1} spans behind the encoder kernel ({a.total - e.size} floats, "
        f"{a.nseg - 1} variables); the encoder kernel {N} x {E}, {rows} rows ({e.size} floats)")
    for plain, gc, arm in (("tnt_adam_fin_f32", "tnt_adam_fin_gclip_f32", fin_arm),
                           ("tnt_dense_dw_adam_fin_f32", "tnt_dense_dw_adam_fin_gclip_f32", enc_arm),
                           ("tnt_adam_f32", "tnt_adam_gclip_f32", ring_arm), ("tnt_sgd_f32", "tnt_sgd_gclip_f32", sgd_arm)):
        report(title, alternate({f"{plain} (plain)": arm(False), f"{gc} (gclip)": arm(True), f"{plain} (plain again)": arm(False)},
                                n, reps))
    model.check_device_errors()


def adam(**clip):
    return Adam(learning_rate=1e-4, beta_1=B1, beta_2=B2, epsilon=EPS, **clip)


def steps(workload, n=200, warm=30, reps=5):
    batch, _ = bench.synth(0, "cuda")
    arms = {"Adam(clipnorm=0.1)": dict(clipnorm=CLIP), f"Adam(global_clipnorm={GCLIP})": dict(global_clipnorm=GCLIP),
            "Adam(clipnorm=0.1) again": dict(clipnorm=CLIP)}
    models = {}
    for name, clip in arms.items():
        m = bench.make_model(workload, "cuda")
        m.compile(adam(**clip))
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
    say(f"  global gradient norm of the last step: {models[f'Adam(global_clipnorm={GCLIP})'].global_grad_norm():.4g}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/global_clip_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    dense = reduction("dense")
    reduction("attention")
    launches(dense)
    if "--no-steps" not in sys.argv:
        for wl in ("dense", "attention"):
            say("")
            steps(wl)
    with open(os.path.join(ROOT, "profiles", "global_clip_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
