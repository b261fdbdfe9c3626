"""Timing of the contrastive sentence-embedding loss (nic.NIC(semantic=SemanticTarget(loss="contrastive"))), all in one process,
with tools/semantic_bench.py's windows (device events around windows that end in a synchronise, every window warmed first,
medians of alternating windows):

  1. tnt_contrastive_loss_f32 alone at B = 64, G = 512: hard / soft targets, symmetric / one-way, with and without dz, beside
     tnt_cosine_loss_f32 (the reference point) and tnt_attention_coverage_f32 (the launch-bound yardstick of
     profiles/semantic_bench.txt);
  2. config 2's training step (bench.py's dense model and batch) with loss="contrastive" against loss="cosine" and against no
     ``semantic``.

    python tools/contrastive_bench.py       # prints, and writes its section of profiles/contrastive_bench.txt

The file's first sections -- the resource usage of the new kernels and the feature-off step against the parent commit (bench.py,
alternating runs of whole processes) -- are kept.

Expectations, stated before measuring and marked held or missed in the output; none is a gate:
  a. the entry costs about its number of launches (3 without dz, 4 with, one of them the means) times the yardstick: held =
     no more than 1.25 x that product;
  b. the contrastive step pays, over the cosine step, the entry's time less the cosine launch's plus the two-word launch that
     files the means: held = within 1.25 x + 2 us of that sum."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import semantic_bench as SB  # noqa: E402
from masters_thesis_amd import _lib, ops  # noqa: E402
from masters_thesis_amd.model_base import SemanticTarget  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "contrastive_bench.txt")
MARK = "# ---- the entry alone and the step (tools/contrastive_bench.py)"
G = 512
say = SB.say


def entry():
    be = ops.backend()
    B, T, R = bench.B, bench.T, 360
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    z, tg, dz = rnd(B, G), rnd(B, G), torch.zeros(B, G, device="cuda")
    loss, cs, out = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(2, device="cuda")
    hit = torch.zeros(B, dtype=torch.int32, device="cuda")
    cwork = torch.zeros(ops.contrastive_work_floats(B, True), device="cuda")
    alpha = torch.softmax(rnd(T, B, R), dim=-1)
    ext = torch.zeros(B * R, device="cuda")
    work = torch.zeros(ops.attention_coverage_work_floats(T, B, R, 0), device="cuda")
    it, st = 1.0 / 0.07, 1.0 / 0.5
    con = lambda d, soft, sym: lambda: be.contrastive_loss(z, G, tg, G, d, cwork, loss, hit, out, B, G, it, soft, sym, 1.0)
    arms = {
        "tnt_attention_coverage_f32 ext only (yardstick, 1 launch)": lambda: be.attention_coverage(alpha, T, B, R, 0, 1e-3, ext, None, work),
        "tnt_cosine_loss_f32 with dz (reference point, 1 launch)": lambda: be.cosine_loss(z, G, tg, G, dz, loss, cs, out, B, G, 1.0 / B),
        "contrastive hard, symmetric, dz (4 launches)": con(dz, 0.0, True),
        "contrastive hard, one-way, dz (4 launches)": con(dz, 0.0, False),
        "contrastive soft, symmetric, dz (4 launches)": con(dz, st, True),
        "contrastive soft, one-way, dz (4 launches)": con(dz, st, False),
        "contrastive hard, symmetric, no dz (3 launches)": con(None, 0.0, True),
        "contrastive soft, symmetric, no dz (3 launches)": con(None, st, True),
    }
    res = SB.alternate(arms, 500)
    say(f"1. the entry alone, B = {B}, G = {G}, temperature 0.07, soft_temperature 0.5: back-to-back calls in windows of 500, 5 "
        "alternating windows, median us per call")
    med = SB.report(res)
    keys = list(arms)
    yard, cos = med[keys[0]], med[keys[1]]
    say(f"  the cosine launch is {cos / yard:.2f} x the yardstick")
    for k in keys[2:]:
        n = 4 if "(4 " in k else 3
        say(f"  {k}: {med[k] / (n * yard):.2f} x (launches x yardstick), {med[k] / cos:.2f} x the cosine launch; expectation a: "
            f"{'held' if med[k] <= 1.25 * n * yard else 'missed'}")
    return med[keys[4]], cos


def steps(entry_us, cos_us):
    batch, _ = bench.synth(0, "cuda")
    B = bench.B
    g = torch.Generator(device="cuda").manual_seed(3)
    guse = torch.randn(B, G, device="cuda", generator=g)
    with5 = (batch[0] + (guse,), batch[1])
    models = {"off": SB.make(None), "cosine": SB.make(SemanticTarget(G)),
              "contrastive": SB.make(SemanticTarget(G, loss="contrastive", temperature=0.07, soft_temperature=0.5))}
    arms = {k: (lambda m=m, b=(batch if k == "off" else with5): m.train_step(b)) for k, m in models.items()}
    res = SB.alternate(arms, 200, warm=40)
    say()
    say("2. train_step dense (config 2): windows of 200 steps, 5 alternating windows, median us per step (contrastive: soft, "
        "symmetric)")
    med = SB.report({f"semantic {k}": v for k, v in res.items()}, 22)
    for m in models.values():
        m.check_device_errors()
    m = models["contrastive"]
    be = ops.backend()
    mover = SB.alternate({"the two-word launch that files the means": lambda: be.sum2(m.sem_out[0:1], m.met[6:7], m.sem_out[1:2],
                                                                                      m.met[5:6], 1, 1.0)}, 500)
    mv = SB.report(mover)["the two-word launch that files the means"]
    want = entry_us - cos_us + mv
    diff = med["semantic contrastive"] - med["semantic cosine"]
    say(f"  contrastive - cosine = {diff:+.2f} us; entry {entry_us:.2f} - cosine launch {cos_us:.2f} + filing launch {mv:.2f} = "
        f"{want:.2f} us")
    say(f"  expectation b: {'held' if diff <= 1.25 * want + 2.0 else 'missed'}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(MARK)
    say(f"tools/contrastive_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say()
    steps(*entry())
    head = open(OUT).read().split(MARK)[0] if os.path.exists(OUT) else ""           # the first sections are kept
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(head + "\n".join(SB.LINES) + "\n")
