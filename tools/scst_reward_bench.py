"""Timing of the self-critical step's rewards on the device.  Part "kernel": tnt_caption_reward_f32 alone at B = 64 scans,
T = 15 tokens, K = 1 ("greedy" baseline), 4 and 16 ("mean") samples and M = 1 and 5 references per scan, both kinds,
against the table of a synthetic corpus of 9000 documents x 5 references (captions of 6 .. 13 words, drawn with a skew
over a vocabulary of 5001 so that n-grams repeat across documents); alternating windows in one process, device events
around windows of launches that end in a synchronise.  Part "step": config 2's self-critical step (bench.py's dense
model, CIDEr-D with that corpus, each row's own caption as its reference) with score_on="host" and score_on="device" in
one process, K = 1 "greedy" and K = 4 "mean", every arm with its own warm-up, alternating windows, host clock around
windows that end in a synchronise; then the device-scored step's three device segments, each ended by a synchronise
(staging + greedy decode, rollout, reward + loss + backward + update), and the reward launch alone on the step's buffers.
The expectations are printed as hit or miss, not tuned.

    python tools/scst_reward_bench.py           # both parts in child processes of their own, each under its own time
                                                # limit; writes profiles/scst_reward_bench.txt
    python tools/scst_reward_bench.py --part kernel | step
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = (("kernel", 240), ("step", 420))       # (part, its time limit in seconds)
END, VOCAB, NDOC, NREF = 2, 5001, 9000, 5


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


def words(rng, n):
    """n word ids in [3, VOCAB), skewed towards the small ids"""
    return (3 + (VOCAB - 3) * rng.random(n) ** 3).astype(int).clip(3, VOCAB - 1)


def synthetic_corpus(seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    return [[[int(w) for w in words(rng, int(rng.integers(6, 14)))] for _ in range(NREF)] for _ in range(NDOC)]


def kernel():
    import numpy as np
    import torch
    import masters_thesis_amd.ops as ops
    from masters_thesis_amd.evaluate import RewardTable, pack_references
    be = ops.backend()
    B, T, Lr = 64, 15, 15
    n, reps = 500, 7
    rng = np.random.default_rng(1)
    corpus = synthetic_corpus()
    t0 = time.perf_counter()
    table = RewardTable(corpus)
    keys, idf, params = table.device("cuda")
    print(f"table of {NDOC} documents x {NREF} references: {len(table)} entries ({len(table) * 16 / 2 ** 20:.1f} MiB), built on the "
          f"host in {time.perf_counter() - t0:.1f} s")
    print(f"tnt_caption_reward_f32, B = {B}, T = {T}, Lr = {Lr}: {reps} alternating windows of {n} launches, median us per launch "
          f"(min .. max)")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    arms = {}
    for K in (1, 4, 16):
        R = B * K
        w = np.zeros((R, T + 1), np.int32)
        for r in range(R):                                  # half of a sample's words come from its scan's first reference
            L = int(rng.integers(6, 14))
            ref = corpus[r // K][0]
            own = words(rng, L)
            w[r, 1:1 + L] = [ref[i] if i < len(ref) and rng.random() < 0.5 else own[i] for i in range(L)]
            w[r, 1 + L] = END
        fed, last = up(w[:, :T]), up(w[:, T])
        greedy = up(np.ascontiguousarray(w[::K, 1:].T))
        adv = torch.zeros(R, device="cuda")
        score = torch.zeros(B, K + 1, dtype=torch.float64, device="cuda")
        counted = torch.zeros(R, dtype=torch.int32, device="cuda")
        for M in (1, 5):
            refs, n_refs = np.zeros((B, M, Lr), np.int32), np.zeros(B, np.int32)
            pack_references([corpus[b][:M] for b in range(B)], refs, n_refs)
            d_refs, d_n = up(refs), up(n_refs)
            for kind, name in ((0, "cider-d"), (1, "bleu4")):
                arms[f"K = {K:2d}, M = {M}, {name}"] = (
                    lambda fed=fed, last=last, greedy=greedy, d_refs=d_refs, d_n=d_n, M=M, K=K, kind=kind, adv=adv, score=score,
                    counted=counted: be.caption_reward(fed, T, last, greedy, B, d_refs, d_n, M, Lr, keys, idf, len(table), params,
                                                       B, K, END, kind, 0 if K == 1 else 1, adv, score, counted))
    t = {k: [] for k in arms}
    for f in arms.values():
        window(f, 50)
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    for k, v in t.items():
        print(f"  {k:26s}: {med(v):7.2f} us   ({min(v):.2f} .. {max(v):.2f})")


def make_scst(device, K, baseline, score_on, corpus):
    import bench
    from masters_thesis_amd.model_base import SelfCritical
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    # the shapes and rates of bench.make_model("dense"); <end> is id 2 in bench.synth's captions
    sc = SelfCritical(END, n_samples=K, baseline=baseline, reward="cider-d", corpus=corpus, score_on=score_on)
    model = NIC(bench.N_VOX, bench.U, bench.E, bench.V, bench.T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, device=device,
                seed=42, self_critical=sc)
    model.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return model


def segments(m, batch):
    """one device-scored step split at device synchronises, in the order of nic.NIC.train_step_scst; seconds per segment"""
    import numpy as np
    import torch
    sc = m.self_critical
    sync = torch.cuda.synchronize
    sync()
    t = [time.perf_counter()]
    B, T = m._stage_scst(batch[0])
    R = B * sc.n_samples
    m._scst_stage_refs(None, B, T)
    m._sync_lr()
    m._enc_grad_stale = None
    run = m._step_runner()
    if sc.baseline == "greedy":
        run(("scst_greedy", B, T), lambda: m._scst_greedy(B, T))
    sync()
    t.append(time.perf_counter())
    run(("scst_rollout", R, T), lambda: m._scst_rollout(R, T))
    sync()
    t.append(time.perf_counter())
    m._run_step(run, ("scst_update", R, T), lambda: m._scst_update(R, T))
    m._enc_grad_stale = m.__dict__.get("_enc_last_fused")
    m.optimizer.iterations += 1
    sync()
    t.append(time.perf_counter())
    return np.diff(t)


def step():
    import numpy as np
    import torch
    import bench
    WINDOWS, STEPS, WARMUP = 5, 30, 20
    dev = torch.device("cuda", 0)
    corpus = synthetic_corpus()
    batch, _ = bench.synth(0, dev)
    models = {}
    for K, baseline in ((1, "greedy"), (4, "mean")):
        for score_on in ("host", "device"):
            models[(K, baseline, score_on)] = make_scst(dev, K, baseline, score_on, corpus)
    for m in models.values():                              # every arm's own warm-up: eager, record, replays
        for _ in range(WARMUP):
            m.train_step(batch)
        m.check_device_errors()
    times = {k: [] for k in models}
    for _ in range(WINDOWS):
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                m.train_step(batch)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / STEPS * 1e3)
    print(f"config 2 self-critical step, CIDEr-D, B = {bench.B}, T = {bench.T}: {WINDOWS} alternating windows of {STEPS} steps, median "
          f"ms per step (min .. max), host clock incl. staging")
    for (K, baseline, score_on), v in times.items():
        print(f"  K = {K} {baseline:6s} score_on = {score_on:6s}: {med(v):8.3f}   ({min(v):.3f} .. {max(v):.3f})")
    for K, baseline in ((1, "greedy"), (4, "mean")):
        m = models[(K, baseline, "device")]
        seg = np.median(np.array([segments(m, batch) for _ in range(STEPS)]), 0) * 1e3
        st = m._scst
        R = bench.B * K
        launch = lambda: m._scst_reward(R, bench.T)
        window(launch, 50)
        us = med([window(launch, 500) for _ in range(WINDOWS)])
        host, device = med(times[(K, baseline, "host")]), med(times[(K, baseline, "device")])
        print(f"  K = {K} {baseline}: device segments, each ended by a synchronise (median of {STEPS} steps, ms): staging + greedy decode "
              f"{seg[0]:.3f}, rollout {seg[1]:.3f}, reward + loss + backward + update {seg[2]:.3f}; sum {seg.sum():.3f}")
        print(f"    the reward launch alone on the step's buffers (M = 8, Lr = 64 extents, 1 reference): {us:.2f} us")
        print(f"    device-scored step {device:.3f} ms against the segments' sum {seg.sum():.3f} ms: "
              f"{'hit' if device <= 1.1 * seg.sum() else 'MISS'} (expected: about the sum)")
        print(f"    device-scored {device:.3f} ms against host-scored {host:.3f} ms: {'hit' if device < host else 'MISS'} "
              f"({host / device:.2f} x)")
        if baseline == "greedy":
            print(f"    the reward launch {us / 1e3:.4f} ms against the staging + greedy decode it follows {seg[0]:.3f} ms: "
                  f"{'hit' if us / 1e3 <= seg[0] else 'MISS'}")
        assert st["score"].shape == (bench.B, K + 1)
    for m in models.values():
        m.check_device_errors()


def main():
    out = ["tools/scst_reward_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("SCST_REWARD_BENCH_OUT", os.path.join("profiles", "scst_reward_bench.txt")))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if "--part" in sys.argv:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        kernel() if sys.argv[sys.argv.index("--part") + 1] == "kernel" else step()
    else:
        main()
