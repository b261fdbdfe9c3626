"""Decode latency / throughput of both model forms at the BASELINE shapes (B = 64, max_len = 15): greedy decoding and
top-p sampled decoding (sample_predict(top_p=0.9), a fresh Philox stream step per call), in one process."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
import bench


def timed(fn, n=20):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(3 + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def line(label, el):
    print(f"{label:24s}: {el * 1e3:7.3f} ms per batch of {bench.B} captions x {bench.T} tokens = "
          f"{bench.B * bench.T / el:9.0f} tokens/s (incl. D2H of the outputs)")


for wl in ("dense", "attention"):
    dev = torch.device("cuda", 0)
    model = bench.make_model(wl, dev, None)
    (data, tgt), _ = bench.synth(0, dev)
    x, cap, z, _ = data
    start = np.ones(bench.B, np.int64)
    kw = {} if wl == "dense" else dict(return_s=False)     # s: analysis output, 44 MB of D2H per call
    line(f"{wl} greedy", timed(lambda i: model.greedy_predict(x, z, z, start, bench.T, bench.U, None, **kw)))
    if wl == "attention":
        line(f"{wl} greedy (return_s)", timed(lambda i: model.greedy_predict(x, z, z, start, bench.T, bench.U, None)))
    line(f"{wl} top-p 0.9", timed(lambda i: model.sample_predict(x, z, z, start, bench.T, bench.U, None, top_p=0.9,
                                                                sample_step=i, **kw)))
    line(f"{wl} top-k 50", timed(lambda i: model.sample_predict(x, z, z, start, bench.T, bench.U, None, top_k=50,
                                                               sample_step=i, **kw)))
