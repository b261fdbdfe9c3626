"""ms/step of the config-2 (--workload dense, the default) or config-3 (--workload attention) training step, teacher-forced
(bench.py's make_model) and with scheduled sampling at p = 0.25 in greedy and in sample mode (the same model with
scheduled_sampling=ScheduledSampling.linear(0.25, 0)), in one process with alternating timed windows:

    python tools/ss_step_bench.py [--workload dense|attention] [--windows 5] [--steps 100] [--warmup 30]

Prints one line per mode: the best and the median window."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def make_ss(workload, device, mode):
    from masters_thesis_amd.model_base import ScheduledSampling
    from masters_thesis_amd.optimizers import Adam
    ss = ScheduledSampling.linear(0.25, 0.0, mode=mode)
    # the shapes and rates of bench.make_model(workload)
    if workload == "dense":
        from masters_thesis_amd.nic import NIC
        model = NIC(bench.N_VOX, bench.U, bench.E, bench.V, bench.T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, device=device,
                    seed=42, scheduled_sampling=ss)
    else:
        from masters_thesis_amd.lc_nic import NIC as LcNIC, synthetic_groups
        groups = synthetic_groups(bench.N_VOX, 360, 32, seed=42)
        model = LcNIC(groups, bench.U, 512, bench.E, 32, bench.V, bench.T, 0.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001,
                      0.00003, 0.00001, device=device, seed=42, scheduled_sampling=ss)
    model.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("dense", "attention"), default="dense")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    w = args.workload
    models = {"teacher-forced": bench.make_model(w, dev), "ss greedy p=0.25": make_ss(w, dev, "greedy"),
              "ss sample p=0.25": make_ss(w, dev, "sample")}
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
    for m in models.values():
        m.check_device_errors()


if __name__ == "__main__":
    main()
