"""Decode latency / throughput of both model forms at the BASELINE shapes (B = 64, max_len = 15): greedy decoding,
top-p sampled decoding (sample_predict(top_p=0.9), a fresh Philox stream step per call) and beam search of width 5
(the dense model's captured decode on tnt_beam_step_f32, with and without length normalisation; the attention model's
eager path on tnt_beam_topk_f32 + state gathers), in one process.  --beam-only: the beam rows alone (profiling)."""
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
    print(f"{label:34s}: {el * 1e3:7.3f} ms per batch of {bench.B} captions x {bench.T} tokens = "
          f"{bench.B * bench.T / el:9.0f} tokens/s (incl. D2H of the outputs)")


beam_only = "--beam-only" in sys.argv
for wl in ("dense", "attention"):
    dev = torch.device("cuda", 0)
    model = bench.make_model(wl, dev, None)
    (data, tgt), _ = bench.synth(0, dev)
    x, cap, z, _ = data
    start = np.ones(bench.B, np.int64)
    kw = {} if wl == "dense" else dict(return_s=False)     # s: analysis output, 44 MB of D2H per call
    if not beam_only:
        line(f"{wl} greedy", timed(lambda i: model.greedy_predict(x, z, z, start, bench.T, bench.U, None, **kw)))
        if wl == "attention":
            line(f"{wl} greedy (return_s)", timed(lambda i: model.greedy_predict(x, z, z, start, bench.T, bench.U, None)))
        line(f"{wl} top-p 0.9", timed(lambda i: model.sample_predict(x, z, z, start, bench.T, bench.U, None, top_p=0.9,
                                                                    sample_step=i, **kw)))
        line(f"{wl} top-k 50", timed(lambda i: model.sample_predict(x, z, z, start, bench.T, bench.U, None, top_k=50,
                                                                   sample_step=i, **kw)))
    zb = z if wl == "dense" else z.cpu().numpy()           # the attention path repeats its inputs on the host
    beam = lambda lp: (lambda i: model.beam_search(x, zb, zb, start, bench.T, beam_width=5, end_id=2, length_penalty=lp))
    line(f"{wl} beam 5", timed(beam(0.0)))
    if wl == "dense":
        line(f"{wl} beam 5, length_penalty 0.6", timed(beam(0.6)))
