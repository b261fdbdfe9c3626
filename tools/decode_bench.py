"""Decode latency / throughput of both model forms at the BASELINE shapes (B = 64, max_len = 15): greedy decoding,
top-p sampled decoding (sample_predict(top_p=0.9), a fresh Philox stream step per call) and beam search of width 5
(the dense model's captured decode on tnt_beam_step_f32, with and without length normalisation; the attention model's
eager path on tnt_beam_topk_f32 + state gathers), in one process.  --beam-only: the beam rows alone (profiling).
--constrained: instead, each of the six decode paths with constraints=DecodeConstraints(no_repeat_ngram_size=2,
repetition_penalty=1.2, min_length=3, three bad ids) against the same path with constraints=None, in alternating timed
windows (medians); --constrained --kernel: the constrained greedy decodes alone, for a rocprofv3 --kernel-trace --stats run."""
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


def constrained_arm(kernel_only):
    """six paths x {constraints=None, constrained}: WINDOWS alternating windows of CALLS calls each, median per call"""
    from masters_thesis_amd.model_base import DecodeConstraints
    WINDOWS, CALLS = 7, 10
    c = DecodeConstraints(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3, bad_ids=(0, 1, 3), end_id=2)
    cb = DecodeConstraints(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3, bad_ids=(0, 1, 3))
    for wl in ("dense", "attention"):
        model = bench.make_model(wl, torch.device("cuda", 0), None)
        (data, _), _ = bench.synth(0, torch.device("cuda", 0))
        x, _, z, _ = data
        start = np.ones(bench.B, np.int64)
        kw = {} if wl == "dense" else dict(return_s=False)
        zb = z if wl == "dense" else z.cpu().numpy()
        paths = {"greedy": lambda i, cc: model.greedy_predict(x, z, z, start, bench.T, bench.U, None, constraints=cc, **kw),
                 "top-k 50": lambda i, cc: model.sample_predict(x, z, z, start, bench.T, bench.U, None, top_k=50, sample_step=i,
                                                                constraints=cc, **kw),
                 "beam 5": lambda i, cc: model.beam_search(x, zb, zb, start, bench.T, beam_width=5, end_id=2,
                                                           constraints=cb if cc is not None else None)}
        if kernel_only:
            for i in range(40):
                paths["greedy"](i, c)
            torch.cuda.synchronize()
            continue
        for name, fn in paths.items():
            for cc in (None, c):
                for i in range(3):
                    fn(i, cc)
            t = {False: [], True: []}
            for w in range(WINDOWS):
                for on in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(CALLS):
                        fn(3 + w * CALLS + i, c if on else None)
                    torch.cuda.synchronize()
                    t[on].append((time.perf_counter() - t0) / CALLS)
            a, b = float(np.median(t[False])), float(np.median(t[True]))
            print(f"{wl + ' ' + name:22s}: constraints=None {a * 1e3:7.3f} ms, constrained {b * 1e3:7.3f} ms, "
                  f"+{(b - a) * 1e6:6.1f} us per {bench.T}-token decode ({(b - a) * 1e6 / bench.T:5.2f} us per token; "
                  f"median of {WINDOWS} alternating windows of {CALLS} calls, B = {bench.B}, incl. D2H of the outputs)")


if "--constrained" in sys.argv:
    constrained_arm("--kernel" in sys.argv)
    sys.exit(0)
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
