"""Timing of ROUGE-L on the device.  Part "kernel": tnt_caption_rouge_f32 alone at B = 64 scans, T = 15 tokens, K = 1
("greedy" baseline), 4 and 16 ("mean") samples and M = 1 and 5 references per scan, against tnt_caption_reward_f32 with kind
BLEU-4 on the same buffers in the same process (tools/scst_reward_bench.py's synthetic captions); alternating windows,
device events around windows of launches that end in a synchronise.  Part "step": config 2's self-critical step (bench.py's
dense model, each row's own caption as its reference) with reward "rouge-l" and reward "bleu4", both scored on the device,
K = 1 "greedy" and K = 4 "mean", every arm with its own warm-up, alternating windows, host clock around windows that end
in a synchronise.  Part "epoch": at config 2, the time fit(validation_captions=CaptionValidation(end_id)) adds per validation
batch (decode, two scoring launches, one sum each; the pass's one read-back at its end) against the greedy decode of the
same batch alone; the references are the model's own greedy captions with every third word replaced, so the logged scores
are not zero.  The expectation of parts "kernel" and "step" -- the ROUGE-L arm is no slower than the BLEU-4 arm, within
the spread the BLEU-4 arm shows between its own windows -- is printed as held or MISSED for every shape, not tuned; part
"epoch" reports and fixes no bound.

    python tools/rouge_bench.py           # the parts in child processes of their own, each under its own time limit;
                                          # writes profiles/rouge_bench.txt
    python tools/rouge_bench.py --part kernel | step | epoch
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARTS = (("kernel", 240), ("step", 420), ("epoch", 300))       # (part, its time limit in seconds)
END = 2


def med(v):
    return sorted(v)[len(v) // 2]


def verdict(new, old):
    """the expectation "no slower than the yardstick arm", the margin being the yardstick's own window-to-window spread"""
    margin = max(old) - min(old)
    ok = med(new) <= med(old) + margin
    return f"{'held' if ok else 'MISSED'} ({med(new) / med(old):.2f} x the BLEU-4 arm; its own spread {margin:.3g})"


def kernel():
    import numpy as np
    import torch
    import masters_thesis_amd.ops as ops
    from masters_thesis_amd.evaluate import ROUGE_BETA, pack_references
    from scst_reward_bench import synthetic_corpus, window, words
    be = ops.backend()
    B, T, Lr = 64, 15, 15
    n, reps = 500, 7
    rng = np.random.default_rng(1)
    corpus = synthetic_corpus()
    print(f"tnt_caption_rouge_f32 against tnt_caption_reward_f32 (kind BLEU-4) on the same buffers, B = {B}, T = {T}, Lr = {Lr}: "
          f"{reps} alternating windows of {n} launches, median us per launch (min .. max)")
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
        base = 0 if K == 1 else 1
        for M in (1, 5):
            refs, n_refs = np.zeros((B, M, Lr), np.int32), np.zeros(B, np.int32)
            pack_references([corpus[b][:M] for b in range(B)], refs, n_refs)
            d_refs, d_n = up(refs), up(n_refs)
            arms[(K, M, "bleu4")] = (lambda fed=fed, last=last, greedy=greedy, d_refs=d_refs, d_n=d_n, M=M, K=K, base=base, adv=adv,
                                     score=score, counted=counted: be.caption_reward(
                                         fed, T, last, greedy, B, d_refs, d_n, M, Lr, None, None, 0, None, B, K, END, 1, base, adv,
                                         score, counted))
            arms[(K, M, "rouge-l")] = (lambda fed=fed, last=last, greedy=greedy, d_refs=d_refs, d_n=d_n, M=M, K=K, base=base, adv=adv,
                                       score=score, counted=counted: be.caption_rouge(
                                           fed, T, last, greedy, B, d_refs, d_n, M, Lr, B, K, END, ROUGE_BETA, base, adv, score,
                                           counted))
    t = {k: [] for k in arms}
    for f in arms.values():
        window(f, 50)
    for _ in range(reps):
        for k, f in arms.items():
            t[k].append(window(f, n))
    for (K, M, name), v in t.items():
        print(f"  K = {K:2d}, M = {M}, {name:8s}: {med(v):7.2f} us   ({min(v):.2f} .. {max(v):.2f})")
    for K in (1, 4, 16):
        for M in (1, 5):
            print(f"  K = {K:2d}, M = {M}: no slower than BLEU-4: {verdict(t[(K, M, 'rouge-l')], t[(K, M, 'bleu4')])}")


def make_scst(device, K, baseline, reward):
    import bench
    from masters_thesis_amd.model_base import SelfCritical
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    # the shapes and rates of bench.make_model("dense"); <end> is id 2 in bench.synth's captions
    sc = SelfCritical(END, n_samples=K, baseline=baseline, reward=reward, score_on="device")
    model = NIC(bench.N_VOX, bench.U, bench.E, bench.V, bench.T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, device=device,
                seed=42, self_critical=sc)
    model.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return model


def step():
    import torch
    import bench
    WINDOWS, STEPS, WARMUP = 5, 30, 20
    dev = torch.device("cuda", 0)
    batch, _ = bench.synth(0, dev)
    models = {}
    for K, baseline in ((1, "greedy"), (4, "mean")):
        for reward in ("bleu4", "rouge-l"):
            models[(K, baseline, reward)] = make_scst(dev, K, baseline, reward)
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
    print(f"config 2 self-critical step scored on the device, B = {bench.B}, T = {bench.T}: {WINDOWS} alternating windows of {STEPS} "
          f"steps, median ms per step (min .. max), host clock incl. staging")
    for (K, baseline, reward), v in times.items():
        print(f"  K = {K} {baseline:6s} reward = {reward:8s}: {med(v):8.3f}   ({min(v):.3f} .. {max(v):.3f})")
    for K, baseline in ((1, "greedy"), (4, "mean")):
        print(f"  K = {K} {baseline}: no slower than BLEU-4: {verdict(times[(K, baseline, 'rouge-l')], times[(K, baseline, 'bleu4')])}")
    for m in models.values():
        m.check_device_errors()


def epoch():
    import torch
    import bench
    from masters_thesis_amd.evaluate import CaptionValidation
    WINDOWS, NV, WARMUP = 5, 8, 3
    dev = torch.device("cuda", 0)
    model = bench.make_model("dense", dev)
    batch, _ = bench.synth(0, dev)
    val = [batch] * NV
    x, cap, a0, c0 = batch[0][:4]
    L = int(cap.shape[1]) - 1
    sync = torch.cuda.synchronize
    # references that share words with what the model decodes, so that the logs printed below are a check and not zeros:
    # each scan's reference is its own greedy caption with every third word replaced, behind two words of the batch's caption
    ids = CaptionValidation(END)._decode_ids(model, x, a0, c0, cap[:, 0].cpu().numpy(), L).cpu().numpy()[:, :bench.B].T
    own = cap.cpu().numpy()
    docs = []
    for b in range(bench.B):
        words = [int(w) for w in ids[b] if w not in (0, END)] or [3]
        docs.append([[int(own[b, 1]), int(own[b, 2])] + [3 if i % 3 == 2 else w for i, w in enumerate(words)][:L]])
    cv = CaptionValidation(END, references=[docs] * NV)

    def decode_alone():                                    # what epoch_logs does for a batch in front of its scoring launches
        for _ in range(NV):
            d_cap = model._to_dev(cap, torch.int32)
            cv._decode_ids(model, x, a0, c0, d_cap[:, 0].cpu().numpy(), L)
        sync()

    def test_pass():
        for b in val:
            model.test_step(b).as_floats()

    arms = {"greedy decode alone": decode_alone, "validation_captions (bleu4, rouge-l)": lambda: cv.epoch_logs(model, val, NV),
            "test_step pass": test_pass}
    for f in arms.values():
        for _ in range(WARMUP):
            f()
    t = {k: [] for k in arms}
    for _ in range(WINDOWS):
        for k, f in arms.items():
            test_pass()                                    # as in fit: every arm starts behind a test_step pass (untimed here)
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            t[k].append((time.perf_counter() - t0) / NV * 1e3)
    print(f"config 2 validation, B = {bench.B}, {L} decoded positions: {WINDOWS} alternating windows of {NV} validation batches, "
          f"median ms per batch (min .. max), host clock around work that ends in a synchronise")
    for k, v in t.items():
        print(f"  {k:38s}: {med(v):8.3f}   ({min(v):.3f} .. {max(v):.3f})")
    d, c = med(t["greedy decode alone"]), med(t["validation_captions (bleu4, rouge-l)"])
    print(f"  validation_captions costs {c:.3f} ms per validation batch, {c / d:.2f} x the greedy decode of the same batch alone "
          f"({c - d:+.3f} ms: the staging of the caption, two scoring launches and their sums); logs {cv.epoch_logs(model, val, NV)}")
    model.check_device_errors()


def main():
    out = ["tools/rouge_bench.py on one MI355X (gfx950).", ""]
    for part, limit in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part],
                           cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        out.append(r.stdout.rstrip())
        if r.returncode != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"part {part} ended with status {r.returncode}")
    path = os.path.join(ROOT, os.environ.get("ROUGE_BENCH_OUT", os.path.join("profiles", "rouge_bench.txt")))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if "--part" in sys.argv:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        {"kernel": kernel, "step": step, "epoch": epoch}[sys.argv[sys.argv.index("--part") + 1]]()
    else:
        main()
