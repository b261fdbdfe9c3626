"""Timing of minimum Bayes risk caption decoding.  Part "kernel": tnt_mbr_select_f32 at B = 64 scans, L = 15 tokens,
(Nc, Nr) = (5, 4), (17, 16), (33, 32), both utilities, on random captions of 5 .. 15 tokens over a vocabulary of 40 words;
alternating windows in one process, device events around windows of launches that end in a synchronise; next to it the
host time of the same selection in Python (tests/mbr_oracle.py, the restatement the tests use: Counter n-grams and
evaluate.sentence_bleu), once per arm.  Parts "dense" / "attention": mbr_decode of config 2 / config 3 (bench.py's models)
of M = 64 scans, 15 tokens, N = 16 samples (top-k 50, top-p 0.95) plus the greedy caption, next to the same N + 1 candidate
decodes alone (no copies into the candidate buffer, no selection launch, no result copy); alternating windows, host clock
around calls that end in a synchronise; and the Python selection on that call's candidates.

    python tools/mbr_bench.py             # every part in a child process of its own, each under its own time limit;
                                          # writes profiles/mbr_bench.txt
    python tools/mbr_bench.py --part kernel | dense | attention
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PARTS = (("kernel", 240), ("dense", 420), ("attention", 420))       # (part, its time limit in seconds)
END = 2


def window(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def med(v):
    return sorted(v)[len(v) // 2]


def kernel():
    import numpy as np
    import torch
    import masters_thesis_amd.ops as ops
    import mbr_oracle as MO
    be = ops.backend()
    B, L, order = 64, 15, 4
    n, reps = 500, 7
    rng = np.random.default_rng(0)
    print(f"tnt_mbr_select_f32, B = {B}, L = {L}, order = {order}: {reps} alternating windows of {n} launches, median us per "
          f"launch (min .. max); Python: the same selection by tests/mbr_oracle.py on the host, ms, one run")
    arms = {}
    for Nc, Nr in ((5, 4), (17, 16), (33, 32)):
        ids = rng.integers(3, 43, (Nc, L, B)).astype(np.int32)
        for c in range(Nc):
            for b in range(B):
                ids[c, int(rng.integers(5, L + 1)):, b] = 0
                ids[c, min(int((ids[c, :, b] != 0).sum()), L - 1), b] = END
        d = torch.from_numpy(ids).to("cuda")
        expected, best = torch.zeros(B, Nc, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.zeros(L, B, dtype=torch.int32, device="cuda")
        for kind in (0, 1):
            name = f"Nc = {Nc:2d}, Nr = {Nr:2d}, {MO.KINDS[kind]}"
            arms[name] = (lambda d=d, Nc=Nc, Nr=Nr, kind=kind, e=expected, bb=best, o=out:
                          be.mbr_select(d, B, B, Nc, Nr, L, END, order, kind, e, bb, o, B), ids, Nr, kind)
    t = {k: [] for k in arms}
    for f, *_ in arms.values():
        window(f, 50)
    for _ in range(reps):
        for k, (f, *_) in arms.items():
            t[k].append(window(f, n))
    for k, (f, ids, Nr, kind) in arms.items():
        t0 = time.perf_counter()
        MO.select(ids, B, Nr, END, order, kind)
        py = (time.perf_counter() - t0) * 1e3
        v = t[k]
        print(f"  {k:28s}: {med(v):7.2f} us   ({min(v):.2f} .. {max(v):.2f})    Python {py:8.1f} ms = {py * 1e3 / med(v):8.0f} x")


def decode(workload):
    import numpy as np
    import torch
    import bench
    import mbr_oracle as MO
    from masters_thesis_amd.model_base import MBR
    Mn, N, WINDOWS, CALLS = 64, 16, 7, 5
    dev = torch.device("cuda", 0)
    model = bench.make_model(workload, dev, None)
    (data, _), _ = bench.synth(0, dev)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((Mn, int(data[0].shape[1]))).astype(np.float32)
    z = np.zeros((Mn, bench.U), np.float32)
    start = np.ones(Mn, np.int64)
    mbr = MBR(END, n_samples=N, top_k=50, top_p=0.95)

    def decodes_alone():
        for c in range(N + 1):
            model._mbr_candidate(x, z, z, start, bench.T, (mbr.temperature, mbr.top_k, mbr.top_p, c) if c < N else None)
    arms = {"mbr_decode": lambda: model.mbr_decode(x, z, z, start, bench.T, mbr),
            f"the {N + 1} candidate decodes alone": decodes_alone}
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
    st = next(iter(model._mbr_bufs.values()))
    sel = lambda: model.be.mbr_select(st["cand"], Mn, Mn, N + 1, N, bench.T, END, mbr.order, mbr.kind, st["expected"], st["best"],
                                      st["out"], Mn)
    window(sel, 50)
    launch = med([window(sel, 500) for _ in range(WINDOWS)])
    cand = model.mbr_decode(x, z, z, start, bench.T, mbr, return_candidates=True)[1]["candidates"]
    t0 = time.perf_counter()
    MO.select(cand.transpose(1, 2, 0), Mn, N, END, mbr.order, mbr.kind)
    py = (time.perf_counter() - t0) * 1e3
    print(f"{workload} ({'config 2' if workload == 'dense' else 'config 3'}), mbr_decode of {Mn} scans, {bench.T} tokens, "
          f"{N} samples + greedy: {WINDOWS} alternating windows of {CALLS} calls, median ms per call (min .. max), host clock "
          f"incl. staging")
    for k, v in t.items():
        print(f"  {k:36s}: {med(v):8.3f}   ({min(v):.3f} .. {max(v):.3f})")
    alone = med(t[f"the {N + 1} candidate decodes alone"])
    print(f"  {'selection launch on its candidates':36s}: {launch / 1e3:8.4f}   = {launch / 1e3 / alone * 100:.3f} % of the decodes alone")
    print(f"  {'Python selection (tests/mbr_oracle)':36s}: {py:8.1f}   = {py * 1e3 / launch:.0f} x the launch")


def main():
    out = ["tools/mbr_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("MBR_BENCH_OUT", os.path.join("profiles", "mbr_bench.txt")))
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
