"""Timing of the label-smoothed head: tnt_softmax_cce_smooth_f32 against tnt_softmax_cce_f32 at the workload shape
(960 x 5001, ld 5004, dlogits aliasing logits), alternating in one process; then the training step of config 2 and
config 3 (bench.py's models and batch) with label_smoothing 0 and 0.1, alternating.  Device events around windows of
launches that end in a synchronise; every window is warmed first.

    python tools/smooth_head_bench.py [--no-steps]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd.optimizers import Adam, CategoricalCrossentropy  # noqa: E402


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def head():
    be = ops.backend()
    rows, V, ld = 960, 5001, 5004
    x0 = torch.randn(rows, ld, device="cuda")
    x = x0.clone()
    tgt = torch.randint(0, V, (rows,), dtype=torch.int32, device="cuda")
    loss, corr = torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    gs = 1.0 / rows

    # in place: the row a launch reads is the dlogits the launch before wrote (|values| <= 1e-3): refill it from x0 in a
    # window of its own and subtract, so both kernels see unit-scale logits on every call
    def plain():
        x.copy_(x0); be.softmax_cce(x, tgt, None, loss, corr, x, rows, V, ld, gs)

    def smooth():
        x.copy_(x0); be.softmax_cce_smooth(x, tgt, None, loss, corr, x, rows, V, ld, gs, 0.1)

    def refill():
        x.copy_(x0)

    for f in (plain, smooth, refill):
        window(f, 50)
    n, reps = 500, 6
    t = {"plain": [], "smooth": [], "refill": []}
    for _ in range(reps):
        t["plain"].append(window(plain, n)); t["smooth"].append(window(smooth, n)); t["refill"].append(window(refill, n))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    p, s = med["plain"] - med["refill"], med["smooth"] - med["refill"]
    print(f"head 960 x 5001 (ld 5004), dlogits in place, {reps} windows of {n} launches each, median us per launch")
    print(f"  refill copy alone            : {med['refill']:.2f}   (windows {min(t['refill']):.2f} .. {max(t['refill']):.2f})")
    print(f"  tnt_softmax_cce_f32          : {p:.2f}   (with refill {min(t['plain']):.2f} .. {max(t['plain']):.2f})")
    print(f"  tnt_softmax_cce_smooth_f32   : {s:.2f}   (with refill {min(t['smooth']):.2f} .. {max(t['smooth']):.2f})")
    print(f"  ratio smooth / plain         : {s / p:.3f}")
    print(f"  bytes moved per launch       : {2 * rows * ld * 4 / 1e6:.1f} MB -> plain {2 * rows * ld * 4 / p / 1e6:.2f} TB/s, "
          f"smooth {2 * rows * ld * 4 / s / 1e6:.2f} TB/s")


def steps(workload, n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
    model = bench.make_model(workload, "cuda")
    out = {0.0: [], 0.1: []}
    for _ in range(reps):
        for eps in (0.0, 0.1):
            model.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1),
                          CategoricalCrossentropy(label_smoothing=eps))
            for _ in range(warm):
                model.train_step(batch)
            out[eps].append(window(lambda: model.train_step(batch), n) / 1e3)
    model.check_device_errors()
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    print(f"train_step {workload}: {reps} windows of {n} steps each, median ms per step")
    for eps in (0.0, 0.1):
        print(f"  label_smoothing {eps}: {med[eps]:.4f}   (windows {min(out[eps]):.4f} .. {max(out[eps]):.4f})")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    head()
    if "--no-steps" not in sys.argv:
        steps("dense")
        steps("attention")
