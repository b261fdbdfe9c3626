"""Timing of consensus decoding.  Part "kernel": tnt_consensus_mix_f32 at Rm = 64, V = 5001 (ld 5004), G in {2, 3, 8},
next to the tnt_softmax_cce_f32 + tnt_argmax_rows_f32 pair on the same G * 64 rows, which the mix launch replaces in a
decode; alternating windows in one process, device events around windows of launches that end in a synchronise.  Parts
"dense" / "attention": the 15-token consensus greedy decode of config 2 / config 3 (bench.py's models) with G = 3 members
of M = 64 images, next to the plain greedy decode of the same 192 rows (consensus=None: the launches and capture keys of
the decode as it was before the keyword existed), alternating windows, host clock around calls that end in the copy of
the outputs to the host.

    python tools/consensus_bench.py            # every part in a child process of its own, each under its own time limit;
                                               # writes profiles/consensus_bench.txt
    python tools/consensus_bench.py --part kernel | dense | attention
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
    n, reps = 500, 7
    print(f"mix launch against the pair it replaces, Rm = {Rm}, V = {V} (ld {ld}): {reps} alternating windows of {n} launches, "
          f"median us per launch (min .. max)")
    for G in (2, 3, 8):
        rows = G * Rm
        x = torch.randn(rows, ld, device="cuda") * 3
        probs = torch.zeros(rows, ld, device="cuda")
        mix = torch.zeros(Rm, ld, device="cuda")
        tok, ids = torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
        arms = {"mix mean": lambda: be.consensus_mix(x, ld, V, Rm, G, None, 0, mix, ld, tok),
                "mix logmean": lambda: be.consensus_mix(x, ld, V, Rm, G, None, 1, mix, ld, tok),
                "softmax_cce": lambda: be.softmax_cce(x, None, probs, None, None, None, rows, V, ld, 0.0),
                "argmax_rows": lambda: be.argmax_rows(probs, ids, rows, V, ld)}
        arms["softmax_cce + argmax_rows"] = lambda: (arms["softmax_cce"](), arms["argmax_rows"]())
        t = {k: [] for k in arms}
        for f in arms.values():
            window(f, 50)
        for _ in range(reps):
            for k, f in arms.items():
                t[k].append(window(f, n))
        for k, v in t.items():
            print(f"  G = {G} ({rows:3d} rows)  {k:26s}: {sorted(v)[len(v) // 2]:6.2f}   ({min(v):.2f} .. {max(v):.2f})")


def decode(workload):
    import numpy as np
    import torch
    import bench
    from masters_thesis_amd.model_base import Consensus
    G, Mn, WINDOWS, CALLS = 3, 64, 7, 10
    dev = torch.device("cuda", 0)
    model = bench.make_model(workload, dev, None)
    (data, _), _ = bench.synth(0, dev)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((G * Mn, int(data[0].shape[1]))).astype(np.float32)
    z = np.zeros((G * Mn, bench.U), np.float32)
    kw = {} if workload == "dense" else dict(return_s=False)
    arms = {"plain greedy, 192 rows": lambda: model.greedy_predict(x, z, z, np.ones(G * Mn, np.int64), bench.T, bench.U, None, **kw),
            "consensus mean, G = 3 x M = 64": lambda: model.greedy_predict(x, z, z, np.ones(Mn, np.int64), bench.T, bench.U, None,
                                                                         consensus=Consensus(G), **kw),
            "consensus logmean, G = 3 x M = 64": lambda: model.greedy_predict(x, z, z, np.ones(Mn, np.int64), bench.T, bench.U, None,
                                                                            consensus=Consensus(G, "logmean"), **kw)}
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
    print(f"{workload} ({'config 2' if workload == 'dense' else 'config 3'}), {bench.T}-token greedy decode of {G * Mn} decoder rows: "
          f"{WINDOWS} alternating windows of {CALLS} calls, median ms per call (min .. max), incl. staging and the copy of the "
          f"outputs to the host (plain: 192 rows of probabilities; consensus: the 64 mixtures)")
    for k, v in t.items():
        print(f"  {k:34s}: {sorted(v)[len(v) // 2]:7.3f}   ({min(v):.3f} .. {max(v):.3f})")


def main():
    out = [f"tools/consensus_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("CONSENSUS_BENCH_OUT", os.path.join("profiles", "consensus_bench.txt")))
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
