"""Timing of the sentence-embedding target (nic.NIC(semantic=SemanticTarget())) and of retrieval in embedding space, all in one
process, device events around windows that end in a synchronise, every window warmed first, medians of alternating windows:

  1. the loss launch at B = 64, G = 512 (tnt_cosine_loss_f32, with and without dz) beside tnt_attention_coverage_f32 on config
     3's attention weights, the launch-latency-bound yardstick of profiles/coverage_bench.txt;
  2. the selection launch at B = 64, k = 5 and M = 10 000 / 50 000 (tnt_cosine_topk_f32) beside one streaming read of the same
     S by an existing row kernel (tnt_argmax_rows_f32), and tnt_row_inv_norm_f32 over the bank;
  3. config 2's training step (bench.py's dense model and batch) with the term against the plain step -- the plain arm runs
     the parent commit's launches (tests/test_host_semantic.py: the same recorded calls);
  4. predict_embedding plus retrieval for 64 scans against a 50 000-row bank, host to host.

    python tools/semantic_bench.py          # prints, and writes its section of profiles/semantic_bench.txt
    python tools/semantic_bench.py 3        # the named sections only; prints, writes nothing

The file's first section, the feature-off step against the parent commit (bench.py, alternating runs), is kept.

Every expectation of the feature's design is marked held or missed in the output; none is a gate."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from masters_thesis_amd import _lib, evaluate, ops  # noqa: E402
from masters_thesis_amd.model_base import SemanticTarget  # noqa: E402
from masters_thesis_amd.nic import NIC  # noqa: E402
from masters_thesis_amd.optimizers import Adam  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "semantic_bench.txt")
MARK = "# ---- the feature's launches, the step and retrieval (tools/semantic_bench.py)"
G = 512
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n          # us per call


def median(v):
    return sorted(v)[len(v) // 2]


def alternate(arms, n, reps=5, warm=20):
    """arms: {name: fn}; reps alternating windows of n calls each -> {name: [us per call]}"""
    out = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(warm):
            fn()
    for _ in range(reps):
        for k, fn in arms.items():
            for _ in range(3):
                fn()
            out[k].append(window(fn, n))
    return out


def report(res, width=58):
    med = {k: median(v) for k, v in res.items()}
    for k, v in res.items():
        say(f"  {k:{width}s}: {med[k]:8.2f}   (windows {min(v):.2f} .. {max(v):.2f})")
    return med


def loss_launch():
    be = ops.backend()
    B, T, R = bench.B, bench.T, 360
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    z, tg, dz = rnd(B, G), rnd(B, G), torch.zeros(B, G, device="cuda")
    loss, cs, out = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(1, device="cuda")
    alpha = torch.softmax(rnd(T, B, R), dim=-1)
    ext, met = torch.zeros(B * R, device="cuda"), torch.zeros(1, device="cuda")
    work = torch.zeros(ops.attention_coverage_work_floats(T, B, R, 0), device="cuda")
    arms = {
        "tnt_attention_coverage_f32 ext only (yardstick, 1 launch)": lambda: be.attention_coverage(alpha, T, B, R, 0, 1e-3, ext, None, work),
        "tnt_cosine_loss_f32 with dz (1 launch)": lambda: be.cosine_loss(z, G, tg, G, dz, loss, cs, out, B, G, 1.0 / B),
        "tnt_cosine_loss_f32 without dz (1 launch)": lambda: be.cosine_loss(z, G, tg, G, None, loss, cs, out, B, G, 1.0 / B),
    }
    res = alternate(arms, 500)
    say(f"1. the loss launch alone, B = {B}, G = {G}: back-to-back launches in windows of 500, 5 alternating windows, median us "
        "per call")
    med = report(res)
    keys = list(arms)
    spread = max(max(res[k]) - min(res[k]) for k in keys[:2])
    diff = med[keys[1]] - med[keys[0]]
    say(f"  loss - yardstick = {diff:+.2f} us; the two arms' own windows spread over {spread:.2f} us")
    say(f"  expectation: launch bound, the yardstick's time within the spread of the two arms' own windows: "
        f"{'held' if abs(diff) <= spread else 'missed'}")
    return med[keys[1]]


def selection():
    be = ops.backend()
    B, k = bench.B, 5
    out = {}
    say()
    say(f"2. the selection launch, B = {B}, k = {k}: windows of 200 launches, 5 alternating windows, median us per call")
    for M in (10000, 50000):
        g = torch.Generator(device="cuda").manual_seed(M)
        S = torch.randn(B, M, device="cuda", generator=g)
        qinv = torch.rand(B, device="cuda", generator=g) + 0.5
        bank = torch.randn(M, G, device="cuda", generator=g)
        binv = torch.zeros(M, device="cuda")
        idx = torch.zeros(B, k, dtype=torch.int32, device="cuda")
        sim = torch.zeros(B, k, device="cuda")
        am = torch.zeros(B, dtype=torch.int32, device="cuda")
        arms = {
            f"M = {M}: tnt_argmax_rows_f32 (one streaming read of S)": lambda: be.argmax_rows(S, am, B, M, M),
            f"M = {M}: tnt_cosine_topk_f32": lambda: be.cosine_topk(S, M, qinv, binv, idx, sim, B, M, k),
            f"M = {M}: tnt_row_inv_norm_f32 over the bank ({M} x {G})": lambda: be.row_inv_norm(bank, G, binv, M, G),
        }
        be.row_inv_norm(bank, G, binv, M, G)
        res = alternate(arms, 200)
        med = report(res)
        keys = list(arms)
        ratio = med[keys[1]] / med[keys[0]]
        gbs = B * M * 4 / med[keys[1]] * 1e-3
        say(f"  selection / streaming read = {ratio:.2f}; the selection reads S at {gbs:.0f} GB/s counted once "
            f"({k} passes over a row that stays in the L2)")
        say(f"  expectation: bandwidth bound, no more than twice the streaming read: {'held' if ratio <= 2.0 else 'missed'}")
        bank_gbs = M * G * 4 / med[keys[2]] * 1e-3
        say(f"  the bank's norms: {bank_gbs:.0f} GB/s")
        out[M] = med[keys[1]]
    return out


def make(sem):
    m = NIC(bench.N_VOX, bench.U, bench.E, bench.V, bench.T, 0.0, 0.2, 0.2, 0.01, 0.00003, 0.00001, device="cuda", seed=42,
            **({"semantic": sem} if sem is not None else {}))
    m.compile(Adam(learning_rate=0.0001, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def steps(loss_us):
    be = ops.backend()
    batch, _ = bench.synth(0, "cuda")
    B = bench.B
    g = torch.Generator(device="cuda").manual_seed(3)
    guse = torch.randn(B, G, device="cuda", generator=g)
    with5 = (batch[0] + (guse,), batch[1])
    models = {"off": make(None), "on": make(SemanticTarget(G))}
    arms = {"off": lambda: models["off"].train_step(batch), "on": lambda: models["on"].train_step(with5)}
    res = alternate(arms, 200, warm=40)
    say()
    say("3. train_step dense (config 2): windows of 200 steps, 5 alternating windows, median us per step")
    med = report({f"semantic {k}": v for k, v in res.items()}, 14)
    for m in models.values():
        m.check_device_errors()
    # the added launches alone, on the buffers the step left: the forward product, the loss, dW + db, the accumulating dx
    m = models["on"]
    a, E, ldG = m.arena, m.E, m.ldG
    # the feature rows the step fed: a replayed step leaves no route record (_forward did not run), so name the buffer here
    x = m._route.xin_used = m.Xin_d if m.r_lstm > 0 else m.Xin
    added = {
        "z = x W + bias": lambda: m.gemm_sk(x, a.p("guse_out/kernel"), m.sem_z, B, G, E, E, ldG, ldG, bias=a.p("guse_out/bias")),
        "dW = x^T dz with the bias rider": lambda: m._semantic_bwd_w(B),
        "dXin[:B] += dz W^T": lambda: m._semantic_bwd_x(B),
        "the target's copy into its static buffer": lambda: m._semantic_stage(guse),
    }
    res2 = alternate(added, 500)
    say("  the added launches alone, windows of 500, median us per call")
    med2 = report(res2)
    want = sum(med2.values()) + loss_us
    diff = med["semantic on"] - med["semantic off"]
    say(f"  on - off = {diff:+.2f} us; the added launches' own times sum to {want:.2f} us (with the loss launch, {loss_us:.2f})")
    say(f"  expectation: the step pays the sum of the added launches' own times: {'held' if diff <= 1.25 * want + 2.0 else 'missed'} "
        "(held = within 1.25 x + 2 us)")
    return models["on"]


def retrieval(model):
    B, M = 64, 50000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, bench.N_VOX)).astype(np.float32)
    bank_rows = rng.standard_normal((M, G)).astype(np.float32)
    bank = evaluate.SemanticBank(bank_rows, device="cuda")
    xd = torch.as_tensor(x).cuda()
    import time
    evaluate.semantic_retrieve(model, xd, bank, k=5)
    ts = []
    for _ in range(9):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        evaluate.semantic_retrieve(model, xd, bank, k=5)
        ts.append(1e6 * (time.perf_counter() - t0))
    say()
    say(f"4. predict_embedding + retrieval, {B} scans on the device against a {M}-row bank, k = 5, wall clock from the call to the "
        f"(B, k) numpy arrays: median {median(ts):.1f} us of 9 calls ({min(ts):.1f} .. {max(ts):.1f}); no expectation was set")
    own = [int(i) for i in rng.integers(0, M, B)]
    t0 = time.perf_counter()
    evaluate.semantic_identification(model, xd, bank, own)
    say(f"   semantic_identification (the whole (B, M) similarity matrix crosses the bus): {1e3 * (time.perf_counter() - t0):.2f} ms")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    say(MARK)
    say(f"tools/semantic_bench.py on one {torch.cuda.get_device_name(0)}, tnt_version {_lib.load().tnt_version()}.")
    say()
    only = set(sys.argv[1:])
    if not only <= {"1", "2", "3", "4"}:
        raise SystemExit(f"sections are 1 2 3 4, got {sorted(only)}")
    want = lambda k: not only or k in only
    loss_us = loss_launch() if want("1") or want("3") else 0.0
    if want("2"):
        selection()
    model = steps(loss_us) if want("3") or want("4") else None
    if want("4"):
        retrieval(model)
    if not only:
        head = open(OUT).read().split(MARK)[0] if os.path.exists(OUT) else ""       # the first section is kept
        with open(OUT, "w") as f:
            f.write(head + "\n".join(LINES) + "\n")
