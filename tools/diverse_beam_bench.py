"""Timing of diverse (group) beam search.  Part "kernel": tnt_beam_step_diverse_f32 at B = 64, V = 5001 (ld 5004),
U = 512, (k, Gd) in {(6, 1), (6, 2), (6, 3), (16, 4)}, next to tnt_beam_step_f32 at the same (B, k) -- and at k = 5, the
shape of the figure recorded for it (profiles/r06_beam_kernel_stats.txt); alternating windows in one process, device
events around windows of launches that end in a synchronise.  Part "dense": the 15-token beam search of config 2
(bench.py's model, its output layer sharpened as tests/test_gpu_beam.py does) over 64 scans, (k, Gd) = (6, 3) next to the
plain searches of width 6 and width 2, alternating windows, host clock around calls that end in the copy of the results
to the host; and evaluate.distinct_n (n = 1, 2) of each scan's six results under the diverse and the plain search.

    python tools/diverse_beam_bench.py            # every part in a child process of its own, each under its own time limit;
                                                  # writes profiles/diverse_beam_bench.txt
    python tools/diverse_beam_bench.py --part kernel | dense
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = (("kernel", 240), ("dense", 420))       # (part, its time limit in seconds)
LAM = 0.8


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
    B, V, ld, U = 64, 5001, 5004, 512
    n, reps = 500, 7
    print(f"diverse step against tnt_beam_step_f32, B = {B}, V = {V} (ld {ld}), U = {U}, lambda = {LAM}: {reps} alternating "
          f"windows of {n} launches, median us per launch (min .. max)")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    arms = {}

    def arm(k, gd):
        Bk = B * k
        probs = torch.softmax(2.5 * torch.randn(Bk, ld, generator=g, device="cuda"), dim=1)
        score = -10 * torch.rand(Bk, generator=g, device="cuda")
        fin = torch.zeros(Bk, dtype=torch.int32, device="cuda")
        so, pa, to, fo = torch.zeros(Bk, device="cuda"), *(torch.zeros(Bk, dtype=torch.int32, device="cuda") for _ in range(3))
        h = [torch.randn(Bk, U, generator=g, device="cuda") for _ in range(4)]
        args = (probs, ld, score, fin, B, V, k, 2, so, pa, to, fo, h[0], h[1], U, U, h[2], h[3])
        if gd is None:
            return lambda: be.beam_step(*args)
        return lambda: be.beam_step_diverse(*args, gd, LAM)
    arms["beam_step k = 5"] = arm(5, None)
    for k, gds in ((6, (1, 2, 3)), (16, (4,))):
        arms[f"beam_step k = {k}"] = arm(k, None)
        for gd in gds:
            arms[f"diverse   k = {k}, Gd = {gd}"] = arm(k, gd)
    t = {name: [] for name in arms}
    for f in arms.values():
        window(f, 50)
    for _ in range(reps):
        for name, f in arms.items():
            t[name].append(window(f, n))
    med = {name: sorted(v)[len(v) // 2] for name, v in t.items()}
    for name, v in t.items():
        ratio = ""
        if name.startswith("diverse"):
            k = name.split("k = ")[1].split(",")[0]
            ratio = f"   {med[name] / med[f'beam_step k = {k}']:.2f} x beam_step k = {k}"
        print(f"  {name:24s}: {med[name]:7.2f}   ({min(v):.2f} .. {max(v):.2f}){ratio}")


def dense():
    import numpy as np
    import torch
    import bench
    from masters_thesis_amd.evaluate import distinct_n
    from masters_thesis_amd.model_base import BeamDiversity
    Bn, WINDOWS, CALLS, K, GD = 64, 7, 10, 6, 3
    dev = torch.device("cuda", 0)
    model = bench.make_model("dense", dev, None)
    (data, _), _ = bench.synth(0, dev)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((Bn, int(data[0].shape[1]))).astype(np.float32)
    z = np.zeros((Bn, bench.U), np.float32)
    start = np.ones(Bn, np.int64)
    p0 = model.greedy_predict(x, z, z, start, 1)[0, :, 0]
    f = 2.5 / np.log(np.maximum(p0, 1e-30)).std(-1).mean()       # the logits spread like a trained model's
    for key in ("time_distributed_softmax/kernel", "time_distributed_softmax/bias"):
        model.set_weight(key, model.get_weight(key) * f)
    search = lambda k, **kw: model.beam_search(x, z, z, start, bench.T, beam_width=k, end_id=2, **kw)
    arms = {"plain, width 2": lambda: search(K // GD),
            "plain, width 6": lambda: search(K),
            f"diverse, (k, Gd) = ({K}, {GD}), lambda = {LAM}": lambda: search(K, diversity=BeamDiversity(GD, LAM))}
    for fn in arms.values():
        for _ in range(4):                         # eager warm-up, capture, replays
            fn()
    t = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / CALLS * 1e3)
    model.check_device_errors()
    print(f"dense (config 2), {bench.T}-token beam search of {Bn} scans: {WINDOWS} alternating windows of {CALLS} calls, median ms "
          f"per call (min .. max), incl. staging and the copy of the results to the host")
    for name, v in t.items():
        print(f"  {name:42s}: {sorted(v)[len(v) // 2]:7.3f}   ({min(v):.3f} .. {max(v):.3f})")
    print(f"distinct-n of each scan's {K} results (cut at end_id = 2), mean over the {Bn} scans:")
    cut = lambda s: list(s[:list(s).index(2)]) if 2 in s else list(s)
    for name in list(arms)[1:]:
        seqs = arms[name]()[0]
        d = [[distinct_n([cut(s) for s in seqs[b]], n) for b in range(Bn)] for n in (1, 2)]
        print(f"  {name:42s}: distinct-1 {np.mean(d[0]):.3f}   distinct-2 {np.mean(d[1]):.3f}")


def main():
    out = ["tools/diverse_beam_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("DIVERSE_BEAM_BENCH_OUT", os.path.join("profiles", "diverse_beam_bench.txt")))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if "--part" in sys.argv:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        part = sys.argv[sys.argv.index("--part") + 1]
        kernel() if part == "kernel" else dense()
    else:
        main()
