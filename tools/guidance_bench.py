"""Timing of classifier-free guidance for caption decoding.  Part "kernel": tnt_guidance_mix_f32 at Rm = 64, V = 5001
(ld 5004) next to the tnt_softmax_cce_f32 + tnt_argmax_rows_f32 pair on the 64 rows of a plain decode (which the mix
launch replaces), the same pair on the 128 member rows, and tnt_consensus_mix_f32 at G = 2 on the same 128 rows;
alternating windows in one process, device events around windows of launches that end in a synchronise.  Parts "dense" /
"attention": the 15-token guided greedy decode of config 2 / config 3 (bench.py's models) of M = 64 scans, which runs 128
decoder rows, next to the plain greedy decode of the same 64 scans; alternating windows, host clock around calls that end
in the copy of the outputs to the host (both return 64 rows of probabilities per token).

    python tools/guidance_bench.py             # every part in a child process of its own, each under its own time limit;
                                               # writes profiles/guidance_bench.txt
    python tools/guidance_bench.py --part kernel | dense | attention
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = (("kernel", 240), ("dense", 420), ("attention", 420))       # (part, its time limit in seconds)


def window(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def kernel():
    import torch
    import masters_thesis_amd.ops as ops
    be = ops.backend()
    Rm, V, ld = 64, 5001, 5004
    rows = 2 * Rm
    n, reps = 500, 7
    print(f"guidance mix launch against the launches it replaces, Rm = {Rm}, V = {V} (ld {ld}): {reps} alternating windows of "
          f"{n} launches, median us per launch (min .. max)")
    x = torch.randn(rows, ld, device="cuda") * 3
    probs = torch.zeros(rows, ld, device="cuda")
    mix = torch.zeros(Rm, ld, device="cuda")
    tok, ids = torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
    pair = lambda r: (be.softmax_cce(x, None, probs, None, None, None, r, V, ld, 0.0), be.argmax_rows(probs, ids, r, V, ld))
    arms = {"guidance mix, scale 1.5": lambda: be.guidance_mix(x, ld, V, Rm, 1.5, 0.0, mix, ld, tok),
            "guidance mix, scale 1.5, plaus 0.1": lambda: be.guidance_mix(x, ld, V, Rm, 1.5, 0.1, mix, ld, tok),
            "softmax_cce + argmax_rows, 64 rows": lambda: pair(Rm),
            "softmax_cce + argmax_rows, 128 rows": lambda: pair(rows),
            "consensus mix mean, G = 2": lambda: be.consensus_mix(x, ld, V, Rm, 2, None, 0, mix, ld, tok),
            "consensus mix logmean, G = 2": lambda: be.consensus_mix(x, ld, V, Rm, 2, None, 1, mix, ld, tok)}
    t = {k: [] for k in arms}
    for f in arms.values():
        window(f, 50)
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    for k, v in t.items():
        print(f"  {k:36s}: {sorted(v)[len(v) // 2]:6.2f}   ({min(v):.2f} .. {max(v):.2f})")


def decode(workload):
    import numpy as np
    import torch
    import bench
    from masters_thesis_amd.model_base import Guidance
    Mn, WINDOWS, CALLS = 64, 7, 10
    dev = torch.device("cuda", 0)
    model = bench.make_model(workload, dev, None)
    (data, _), _ = bench.synth(0, dev)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((Mn, int(data[0].shape[1]))).astype(np.float32)
    z = np.zeros((Mn, bench.U), np.float32)
    start = np.ones(Mn, np.int64)
    kw = {} if workload == "dense" else dict(return_s=False)
    arms = {"plain greedy, 64 rows": lambda: model.greedy_predict(x, z, z, start, bench.T, bench.U, None, **kw),
            "guided greedy, 64 scans (128 rows)": lambda: model.greedy_predict(x, z, z, start, bench.T, bench.U, None,
                                                                             guidance=Guidance(1.5, None, 0.1), **kw)}
    for f in arms.values():
        for _ in range(4):                         # eager warm-up, capture, replays
            f()
    t = {k: [] for k in arms}
    for _ in range(WINDOWS):
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / CALLS * 1e3)
    model.check_device_errors()
    print(f"{workload} ({'config 2' if workload == 'dense' else 'config 3'}), {bench.T}-token greedy decode of {Mn} scans: "
          f"{WINDOWS} alternating windows of {CALLS} calls, median ms per call (min .. max), incl. staging and the copy of the "
          f"{Mn} rows of probabilities per token to the host")
    for k, v in t.items():
        print(f"  {k:36s}: {sorted(v)[len(v) // 2]:7.3f}   ({min(v):.3f} .. {max(v):.3f})")


def main():
    out = ["tools/guidance_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("GUIDANCE_BENCH_OUT", os.path.join("profiles", "guidance_bench.txt")))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if "--part" in sys.argv:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        part = sys.argv[sys.argv.index("--part") + 1]
        kernel() if part == "kernel" else decode(part)
    else:
        main()
