"""Timing of the weighted head: tnt_softmax_cce_weighted_f32 against tnt_softmax_cce_f32 and tnt_softmax_cce_smooth_f32
at the workload shape (960 x 5001 = T 15 x B 64, ld 5004, dlogits aliasing logits, captions of 8 to 14 words and padding
behind them), alternating in one process: the new launch with neutral settings (no weights, gamma 0, "count"), with
weights and gamma 2 (no powf) or 0.5 (powf) under "count", and with a zero pad weight (a quarter of the rows) and gamma 2
under "weights", which adds the gather pass of the weight sum and lets the zero-weight rows skip their row walk -- the
same launch in its evaluation form (probabilities in place) keeps the walk; then the training step
of config 2 and config 3 (bench.py's models and batch) with the option on against the default step and, for config 2,
the teacher-forced step with the compact head off, alternating.  Device events around windows of launches that end in a
synchronise; every window is warmed first.

    python tools/weighted_loss_bench.py [--no-steps]        # prints, and writes profiles/weighted_loss_bench.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import masters_thesis_amd.ops as ops  # noqa: E402
from masters_thesis_amd import _lib  # noqa: E402
from masters_thesis_amd.data import token_class_weights  # noqa: E402
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
    loss, corr = torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    gs = 1.0 / rows
    w = token_class_weights(tgt.cpu().numpy(), V, scheme="inverse_sqrt", pad_weight=1.0)
    cw = torch.from_numpy(w).cuda()                  # every row weighted
    w[0] = 0.0
    cw0 = torch.from_numpy(w).cuda()                 # the padding rows at weight 0
    pad = float((tgt == 0).float().mean())

    # in place: the row a launch reads is the dlogits the launch before wrote: refill it from x0 in a window of its own
    # and subtract, so every kernel sees unit-scale logits on every call
    wt = lambda c, g, n: (x.copy_(x0), be.softmax_cce_weighted(x, tgt, c, None, loss, corr, x, rows, V, ld, gs, g, n))
    arms = {
        "refill copy alone": lambda: x.copy_(x0),
        "tnt_softmax_cce_f32": lambda: (x.copy_(x0), be.softmax_cce(x, tgt, None, loss, corr, x, rows, V, ld, gs)),
        "tnt_softmax_cce_smooth_f32": lambda: (x.copy_(x0), be.softmax_cce_smooth(x, tgt, None, loss, corr, x, rows, V, ld, gs, 0.1)),
        "weighted: no weights, gamma 0, count": lambda: wt(None, 0.0, False),
        "weighted: weights, gamma 2, count": lambda: wt(cw, 2.0, False),
        "weighted: weights, gamma 0.5, count": lambda: wt(cw, 0.5, False),
        "weighted: pad weight 0, gamma 2, weights": lambda: wt(cw0, 2.0, True),
        "  the same without the row skip (probs)": lambda: (x.copy_(x0), be.softmax_cce_weighted(
            x, tgt, cw0, x, loss, corr, None, rows, V, ld, 0.0, 2.0, True)),
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
    say(f"head 960 x 5001 (B 64, T 15, ld 5004), dlogits in place, captions of 8 to 14 words ({100 * pad:.0f} % padding rows),")
    say(f"{reps} alternating windows of {n} launches each, median us per launch, the refill copy subtracted")
    for k in arms:
        v = med[k] - (0.0 if k == "refill copy alone" else ref)
        say(f"  {k:42s}: {v:6.2f}   (windows {min(t[k]):.2f} .. {max(t[k]):.2f}{'' if k == 'refill copy alone' else ' with refill'})")
    s = med["tnt_softmax_cce_smooth_f32"] - ref
    spread = max(max(v) - min(v) for v in t.values())
    say(f"  largest spread between the windows of one arm: {spread:.2f} us")
    for k in list(arms)[3:7]:
        say(f"  {k.strip()} - smooth = {med[k] - ref - s:+.2f} us")


def steps(workload, arms, n=200, warm=30, reps=3):
    batch, _ = bench.synth(0, "cuda")
    tgt = batch[1]
    tgt = tgt.cpu().numpy() if hasattr(tgt, "cpu") else tgt
    ids = tgt if tgt.ndim == 2 else tgt.argmax(-1)
    models = {}
    for name, (kw, attrs) in arms.items():
        m = bench.make_model(workload, "cuda")
        for k, v in attrs.items():
            setattr(m, k, v)
        kw = dict(kw)
        if kw.get("class_weight") == "corpus":
            kw["class_weight"] = token_class_weights(ids.astype("int64"), m.V, scheme="inverse_sqrt", pad_weight=0.0)
        m.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1), CategoricalCrossentropy(**kw))
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
        say(f"  {k:50s}: {sorted(v)[len(v) // 2]:.4f}   (windows {min(v):.4f} .. {max(v):.4f})")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(f"tools/weighted_loss_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say("")
    head()
    if "--no-steps" not in sys.argv:
        on = dict(class_weight="corpus", focal_gamma=2.0, normalise="weights")
        steps("dense", {"default step (compact head)": ({}, {}),
                        "teacher-forced step, compact head off": ({}, {"compact_head": False}),
                        "weights (pad 0), gamma 2, count": (dict(on, normalise="count"), {}),
                        "weights (pad 0), gamma 2, weights": (on, {})})
        steps("attention", {"default step": ({}, {}),
                            "weights (pad 0), gamma 2, count": (dict(on, normalise="count"), {}),
                            "weights (pad 0), gamma 2, weights": (on, {})})
    with open(os.path.join(ROOT, "profiles", "weighted_loss_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
