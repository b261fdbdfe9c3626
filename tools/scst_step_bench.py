"""ms/step of config 2's self-critical training step (nic.NIC(self_critical=SelfCritical(2, ...)), CIDEr-D reward against
each row's own caption) with K = 1 "greedy" and K = 4 "mean", next to the teacher-forced step (bench.make_model), in one
process with alternating timed windows; then a per-phase breakdown of each SCST arm, every phase ended by a device
synchronise: the greedy baseline decode, the rollout, the host round trip with the rewards, and loss + backward + update.

    python tools/scst_step_bench.py [--windows 5] [--steps 50] [--warmup 20] [--arms greedy1,mean4]

Prints one line per arm (best and median window) and one breakdown line per SCST arm (medians over --steps steps)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ARMS = {"greedy1": (1, "greedy"), "mean4": (4, "mean")}


def make_scst(device, K, baseline):
    from masters_thesis_amd.model_base import SelfCritical
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    # the shapes and rates of bench.make_model("dense"); <end> is id 2 in bench.synth's captions
    model = NIC(bench.N_VOX, bench.U, bench.E, bench.V, bench.T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, device=device,
                seed=42, self_critical=SelfCritical(2, n_samples=K, baseline=baseline))
    model.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return model


def phases(m, batch):
    """one SCST step split at device synchronises, in the order of nic.NIC.train_step_scst; seconds per phase"""
    sc = m.self_critical
    sync = torch.cuda.synchronize
    t = [time.perf_counter()]
    B, T = m._stage_scst(batch[0])
    R = B * sc.n_samples
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
    samples, greedy, cap0 = m._scst_round_trip(B, T)
    refs = [[sc.truncate(row[1:])] for row in cap0]
    adv, _, _, _ = sc.advantages(samples, refs, greedy if sc.baseline == "greedy" else None)
    m._scst["h_adv"].copy_(torch.from_numpy(adv.astype(np.float32)))
    m._scst["adv"].copy_(m._scst["h_adv"], non_blocking=True)
    sync()
    t.append(time.perf_counter())
    m._run_step(run, ("scst_update", R, T), lambda: m._scst_update(R, T))
    m._enc_grad_stale = m.__dict__.get("_enc_last_fused")
    m.optimizer.iterations += 1
    sync()
    t.append(time.perf_counter())
    return np.diff(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--arms", default="greedy1,mean4")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    models = {"teacher-forced": bench.make_model("dense", dev)}
    for a in args.arms.split(","):
        K, baseline = ARMS[a]
        models[f"scst K={K} {baseline}"] = make_scst(dev, K, baseline)
    batch, _ = bench.synth(0, dev)
    for m in models.values():
        for _ in range(args.warmup):
            m.train_step(batch)
        m.check_device_errors()
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(args.windows):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                m.train_step(batch)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    for name, ts in times.items():
        ts = sorted(ts)
        print(f"{name:17s} best {ts[0]:.4f} ms/step, median {ts[len(ts) // 2]:.4f} ms/step "
              f"({args.windows} windows x {args.steps} steps)")
    for name, m in models.items():
        if m.__dict__.get("self_critical") is None:
            continue
        ph = np.median(np.array([phases(m, batch) for _ in range(args.steps)]), 0) * 1e3
        print(f"{name:17s} breakdown (median of {args.steps} synchronised steps, ms): staging + baseline decode {ph[0]:.3f}, "
              f"rollout {ph[1]:.3f}, round trip + reward {ph[2]:.3f}, loss + backward + update {ph[3]:.3f}; "
              f"sum {ph.sum():.3f}")
    for m in models.values():
        m.check_device_errors()


if __name__ == "__main__":
    main()
