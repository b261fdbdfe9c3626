"""Timing of layer freezing and per-variable learning-rate multipliers (freeze / set_lr_multipliers; the *_lrmul_f32
entries).  Nothing here is held to a figure fixed in advance.  The expectations that the numbers are read against: a
table of ones costs an update launch no more than the spread the PLAIN arm shows between its own windows; a frozen
variable's spans cost next to nothing; the decoder-frozen step is faster than the plain step by about the time of the
launches it leaves out.

  * the update launch over config 2's whole arena: tnt_adam_fin_lrmul_f32 against tnt_adam_fin_f32, tnt_adam_lrmul_f32
    against tnt_adam_f32, tnt_sgd_lrmul_f32 against tnt_sgd_f32, and the norm launch tnt_span_sqnorm_lrmul_f32 against
    tnt_span_sqnorm_lr_f32, tnt_seg_sqnorm_lrmul_f32 against tnt_seg_sqnorm_f32 and the reduction
    tnt_global_sqnorm_lrmul_f32 against tnt_global_sqnorm_f32, per launch, for three tables: all ones, decoder frozen
    (emb_text, lstm, head), encoder kernel frozen;
  * the encoder's fused update on config 2's encoder kernel (20000 x 512, 64 rows): tnt_dense_dw_adam_fin_lrmul_f32 at
    the scalar multipliers 1 and 0.1 against tnt_dense_dw_adam_fin_f32;
  * the training step of config 2 and config 3 (bench.py's models): plain, decoder frozen, encoder frozen, and multipliers
    only (every decoder variable at 0.1).

Alternating windows in one process, medians; device events around windows that end in a synchronise; every window is
warmed first.  Each arm has its own copy of theta / m / v.  The learning rate of the launch arms is 1e-7, so that
thousands of updates on one fixed gradient leave the values where they are.

    python tools/finetune_bench.py [--no-steps]        # prints, and writes profiles/finetune_bench.txt
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

LINES = []
B1, B2, EPS, CLIP = 0.9, 0.98, 1e-8, 0.1
DECODER = ("emb_text", "lstm", "time_distributed_softmax")


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


def alternate(arms, n, reps):
    for f in arms.values():
        window(f, 30)
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    return t


def report(title, t, unit="us", scale=1.0):
    """medians per arm against the first (plain) arm, whose own spread between its windows is the margin"""
    say(title)
    med = {k: sorted(v)[len(v) // 2] * scale for k, v in t.items()}
    names = list(t)
    plain = names[0]
    spread = (max(t[plain]) - min(t[plain])) * scale
    for k in names:
        line = f"  {k:46s}: {med[k]:9.4f} {unit}   (windows {min(t[k]) * scale:.4f} .. {max(t[k]) * scale:.4f})"
        if k != plain:
            d = med[k] - med[plain]
            line += f"   {d:+.4f} against plain: {'inside' if abs(d) <= spread else 'OUTSIDE'} the margin"
        say(line)
    say(f"  margin (the plain arm's own spread): {spread:.4f} {unit}")


def tables(model):
    a = model.arena
    tabs = {"all ones": torch.ones(a.nseg, device="cuda")}
    dec = torch.ones(a.nseg, device="cuda")
    for n, e in a.entries.items():
        if n.split("/")[0] in DECODER:
            dec[e.seg] = 0
    enc = torch.ones(a.nseg, device="cuda")
    enc[a.entries["dense_img/kernel"].seg] = 0
    tabs["decoder frozen"], tabs["encoder kernel frozen"] = dec, enc
    return tabs


def launches(n=300, reps=5):
    be = ops.backend()
    model = bench.make_model("dense", "cuda")
    model.fuse_enc_update = False               # the encoder kernel's gradient is written: the launches walk the whole arena
    batch, _ = bench.synth(0, "cuda")
    for _ in range(3):
        model.train_step(batch)
    torch.cuda.synchronize()
    a, sp = model.arena, model.arena.spans
    spans = (sp.span_seg, sp.span_off, sp.span_len)
    lr, lr_t = torch.full((1,), 1e-7, device="cuda"), torch.full((1,), 1e-7, device="cuda")
    l2_out = torch.zeros(1, device="cuda")
    be.seg_sqnorm(a.theta, a.grad, *spans, sp.seg_first, a.seg_l2, a.partial, a.sq, a.wsq, None, sp.nspan, a.nseg)
    tabs = tables(model)
    say(f"config 2's whole arena: {sp.nspan} spans, {a.total} floats, {a.nseg} variables")
    for name, tab in tabs.items():
        live = sum(e.size for e in a.entries.values() if float(tab[e.seg]) != 0)
        say(f"  table '{name}': {live} of {a.total} floats are updated")

    def state():
        return a.theta.clone(), model.opt_m.clone(), model.opt_v.clone()

    def fin_arm(tab):
        th, m, v = state()
        arrive = torch.zeros(16, dtype=torch.int32, device="cuda")
        t, drop = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        fin = be.finalize_desc(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, l2_out, a.nseg, arrive, adam_t=t, drop_step=drop,
                               lr=lr, lr_t=lr_t, beta1=B1, beta2=B2)
        args = (th, m, v, a.grad, *spans, a.sq_override, sp.nspan, EPS, CLIP, fin)
        return (lambda: be.adam_fin(*args)) if tab is None else (lambda: be.adam_fin_lrmul(*args, tab))

    def ring_arm(tab):
        th, m, v = state()
        args = (th, m, v, a.grad, *spans, a.seg_l2, a.sq, a.sq_override, sp.nspan, 0.0, lr_t, B1, B2, EPS, CLIP)
        return (lambda: be.adam(*args)) if tab is None else (lambda: be.adam_lrmul(*args, tab))

    def sgd_arm(tab):
        th, m, _ = state()
        args = (th, m, a.grad, *spans, a.seg_l2, a.sq, a.sq_override, sp.nspan, 0.0, lr, 0.9, CLIP)
        return (lambda: be.sgd(*args)) if tab is None else (lambda: be.sgd_lrmul(*args, tab))

    def norm_arm(tab):
        part = torch.zeros_like(a.partial)
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        out = torch.zeros(1, device="cuda")
        args = (a.theta, a.grad, *spans, a.seg_l2, part, sp.nspan)
        if tab is None:
            return lambda: be.span_sqnorm_lr(*args, t, lr, out, B1, B2, skip=a.sq_override)
        return lambda: be.span_sqnorm_lrmul(*args, tab, lr_job=(t, lr, out, B1, B2), skip=a.sq_override)

    def seg_arm(tab):
        part, sq, wsq = torch.zeros_like(a.partial), torch.zeros_like(a.sq), torch.zeros_like(a.wsq)
        args = (a.theta, a.grad, *spans, sp.seg_first, a.seg_l2, part, sq, wsq, l2_out, sp.nspan, a.nseg)
        return (lambda: be.seg_sqnorm(*args)) if tab is None else (lambda: be.seg_sqnorm_lrmul(*args, tab))

    def gsq_arm(tab):
        out = torch.zeros(1, device="cuda")
        kw = dict(sq_override=a.sq_override, sq=a.sq)
        return (lambda: be.global_sqnorm(out, a.nseg, **kw)) if tab is None else (lambda: be.global_sqnorm_lrmul(out, a.nseg, tab, **kw))

    for title, plain, arm in (("tnt_seg_sqnorm_f32 (three launches)", "tnt_seg_sqnorm_f32 (plain)", seg_arm),
                              ("tnt_global_sqnorm_f32, table form", "tnt_global_sqnorm_f32 (plain)", gsq_arm),
                              ("tnt_adam_fin_f32", "tnt_adam_fin_f32 (plain)", fin_arm), ("tnt_adam_f32", "tnt_adam_f32 (plain)", ring_arm),
                              ("tnt_sgd_f32", "tnt_sgd_f32 (plain)", sgd_arm),
                              ("tnt_span_sqnorm_lr_f32", "tnt_span_sqnorm_lr_f32 (plain)", norm_arm)):
        arms = {plain: arm(None)}
        arms.update({f"_lrmul form, {k}": arm(tab) for k, tab in tabs.items()})
        say("")
        report(f"{title} and its _lrmul form: {reps} alternating windows of {n} eager launches each, median us per launch",
               alternate(arms, n, reps))
    e = a.entries["dense_img/kernel"]
    N, E, rows = model.N, model.E, 64
    x = torch.randn(rows, model.ldx, device="cuda")
    dpre = torch.randn(rows, E, device="cuda") * 0.01
    sl = slice(e.off, e.off + e.size)
    k0, k1 = sp.first_host[e.seg], sp.first_host[e.seg + 1]
    ovr = a.sq_override[e.seg:e.seg + 1]

    def enc_arm(mul):
        th, m, v = a.theta[sl].clone(), model.opt_m[sl].clone(), model.opt_v[sl].clone()
        args = (x, dpre, th, m, v, e.l2, a.partial, k0, k1, ovr, lr_t, B1, B2, EPS, CLIP, N, E, rows, model.ldx)
        return (lambda: be.dense_dw_adam_fin(*args)) if mul is None else (lambda: be.dense_dw_adam_fin_lrmul(*args, mul))

    say("")
    report(f"the encoder's fused update, X^T D ({N} x {E}, {rows} rows) + clip + Adam on the strips, {e.size} floats: "
           f"{reps} alternating windows of {n} eager launches each, median us per launch",
           alternate({"tnt_dense_dw_adam_fin_f32 (plain)": enc_arm(None), "_fin_lrmul form, multiplier 1": enc_arm(1.0),
                      "_fin_lrmul form, multiplier 0.1": enc_arm(0.1),
                      "tnt_dense_dw_adam_fin_f32 (plain, control)": enc_arm(None)}, n, reps))
    model.check_device_errors()


def steps(workload, n=200, warm=30, reps=5):
    batch, _ = bench.synth(0, "cuda")
    enc = ["dense_img/kernel"] if workload == "dense" else ["dense_in"]
    cases = {"plain": None, "decoder frozen": {k: 0.0 for k in DECODER}, "encoder frozen": {k: 0.0 for k in enc},
             "multipliers only (decoder at 0.1)": {k: 0.1 for k in DECODER}}
    models = {}
    for name, tab in cases.items():
        m = bench.make_model(workload, "cuda")
        m.compile(Adam(learning_rate=1e-4, beta_1=B1, beta_2=B2, epsilon=EPS, clipnorm=CLIP))
        if tab is not None:
            m.set_lr_multipliers(tab)
        for _ in range(warm):
            m.train_step(batch)
        models[name] = m
    out = {k: [] for k in cases}
    for _ in range(reps):
        for name, m in models.items():
            for _ in range(5):
                m.train_step(batch)
            out[name].append(window(lambda: m.train_step(batch), n) / 1e3)
    for m in models.values():
        m.check_device_errors()
    report(f"train_step {workload}: {reps} alternating windows of {n} steps each, median ms per step", out, unit="ms")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/finetune_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    launches()
    if "--no-steps" not in sys.argv:
        for wl in ("dense", "attention"):
            say("")
            steps(wl)
    with open(os.path.join(ROOT, "profiles", "finetune_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
