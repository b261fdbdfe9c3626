"""Caption scoring at the BASELINE shapes (config 2 and config 3, B = 64, T = 15), in one process per run.

    python tools/score_bench.py [--windows 5] [--calls 20] [--warmup 5] [--workloads dense,attention]
        per workload, alternating timed windows of
          model(data)        the inference forward + softmax + the (B, T, V) probabilities to the host: the nearest thing
                             to a caption likelihood without score_captions
          score_captions     C = 1: the same forward stopped at the logits + tnt_caption_score_f32, (B,) results to the host
        then evaluate.identification (C = B = 64, default max_rows): ms per call and the peak extra device memory.
    python tools/score_bench.py --kernel [--calls 20]
        tnt_caption_score_f32 and tnt_softmax_cce_f32 (in place, no target) on the same 960 x 5001 logits, alternating;
        meant to run under `rocprofv3 --kernel-trace --stats -- python tools/score_bench.py --kernel`.

Run each invocation under a time limit of its own; nothing here retries."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

END = 2     # <end> in bench.synth's captions


def kernel_run(calls):
    import masters_thesis_amd.ops as ops
    be = ops.backend()
    R, T, V, ld = bench.B, bench.T + 1, bench.V, (bench.V + 3) // 4 * 4
    steps = T - 1                                       # 15 x 64 = 960 rows, every one counted
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randn(steps * R, ld, device="cuda", generator=g) * 3
    cap = torch.randint(3, V, (R, T), device="cuda", dtype=torch.int32, generator=g)
    tok, lp = torch.zeros(steps * R, device="cuda"), torch.zeros(R, device="cuda")
    ln = torch.zeros(R, dtype=torch.int32, device="cuda")
    work = torch.empty_like(src)
    for _ in range(calls):
        work.copy_(src)
        be.caption_score(work, ld, V, cap, T, steps, R, END, tok, lp, ln)
        be.softmax_cce(work, None, work, None, None, None, steps * R, V, ld, 0.0)
    torch.cuda.synchronize()
    print(f"{calls} x (caption_score, softmax_cce) on {steps * R} rows x {V} columns (ld {ld}); sum of logprob {float(lp.sum()):.3f}")


def windows(arms, n_windows, calls):
    times = {k: [] for k in arms}
    for _ in range(n_windows):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="dense,attention")
    ap.add_argument("--kernel", action="store_true")
    args = ap.parse_args()
    if args.kernel:
        kernel_run(args.calls)
        return
    from masters_thesis_amd import evaluate
    dev = torch.device("cuda", 0)
    for wl in args.workloads.split(","):
        model = bench.make_model(wl, dev, None)
        (data, _), _ = bench.synth(0, dev)
        x, cap, z, _ = data
        caps = cap.cpu().numpy()

        def forward():
            out = model(data)
            return (out[0] if isinstance(out, tuple) else out).cpu()
        arms = {"model(data) -> probabilities on the host": forward,
                "score_captions C = 1": lambda: model.score_captions(x, z, z, caps, end_id=END)}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        model.check_device_errors()
        for name, ts in windows(arms, args.windows, args.calls).items():
            print(f"{wl:9s} {name:42s} best {ts[0]:.3f} ms/call, median {ts[len(ts) // 2]:.3f} ms/call "
                  f"({args.windows} windows x {args.calls} calls)")
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ident = lambda: evaluate.identification(model, x, z, z, caps, END)
        for _ in range(3):
            res = ident()
        peak = torch.cuda.max_memory_allocated() - base
        ts = windows({"identification": ident}, args.windows, max(1, args.calls // 4))["identification"]
        rows = model._score["key"][0] * model._score["key"][1]
        print(f"{wl:9s} identification C = B = {len(caps)} ({rows} decoder rows per pass, {-(-len(caps) // model._score['key'][1])} "
              f"passes): best {ts[0]:.3f} ms/call, median {ts[len(ts) // 2]:.3f} ms/call; peak extra device memory "
              f"{peak / 2 ** 20:.0f} MiB; top-1 {res['top1']:.3f} (untrained weights)")
        model.check_device_errors()
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
