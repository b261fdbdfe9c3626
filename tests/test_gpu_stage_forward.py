"""The batch staging riding in the streaming encoder forward (tnt_dense_fwd_stream_gram_stage_f32, nic.NIC ``stage_fwd``): the
entry point against the two launches it replaces, bit for bit; what it refuses; the training step with the merged launch on
against off; and the steps that keep the two launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E512, U8, T4, SPLITS = 512, 8, 4, 16
MERGED, STAGE, GRAM = ("tnt_dense_fwd_stream_gram_stage_f32", "tnt_stage_batch_map_f32", "tnt_dense_fwd_stream_gram_f32")


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def same(a, b):
    """torch.equal on the bits: the poison of an element nobody wrote is a NaN, which compares unequal to itself"""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def captions(kind, B, T, rng):
    cap = np.zeros((B, T), np.int32)
    cap[:, 0] = 1
    if kind == "full":                     # nothing merged: the identity map
        cap[:, 1:T - 1] = rng.integers(3, 40, size=(B, T - 2))
        cap[:, T - 1] = 2
    elif kind == "interior":               # random lengths; caption 0 is fed a 0 whose target (7) is not the carried one (0)
        for b in range(B):
            L = int(rng.integers(0, T - 1))
            cap[b, 1:1 + L] = rng.integers(3, 40, size=L)
            cap[b, 1 + L] = 2
        cap[0] = [1, 5, 0, 7]
    else:
        assert kind == "pad"               # all padding after the first token
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    return cap, tgt


def inputs(B, N, kind, seed):
    rng = np.random.default_rng(seed)
    cap, tgt = captions(kind, B, T4, rng)
    return dict(x=dev(rng.standard_normal((B, N))), w=dev(rng.standard_normal((N, E512)) * 0.1), cap=dev(cap, torch.int32),
                tgt=dev(tgt, torch.int32), a0=dev(rng.standard_normal((B, U8))), c0=dev(rng.standard_normal((B, U8))))


def outputs(B, N):
    """every output of the two launches, poisoned: floats NaN, ints -7"""
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    n = B * T4
    return dict(enc_part=f(SPLITS * B * E512), gx_part=f(SPLITS * 64 * 64), w2_part=f(SPLITS * (E512 // 32)), x_dst=f(B, N),
                cap_dst=i(B, T4), tgt_tmajor=i(n), h0=f(B, U8), c0_dst=f(B, U8), pos=i(n), row_weight=f(n), tgt_compact=i(n),
                live=i(1), loss_row=f(n), corr_row=f(n))


def two_launches(be, d, o, B, N):
    be.stage_batch_map(d["x"], o["x_dst"], d["cap"], o["cap_dst"], d["tgt"], o["tgt_tmajor"], d["a0"], o["h0"], d["c0"],
                       o["c0_dst"], B, T4, N, N, U8, o["pos"], o["row_weight"], o["tgt_compact"], o["live"], o["loss_row"],
                       o["corr_row"])
    be.dense_fwd_stream_gram(o["x_dst"], d["w"], o["enc_part"], o["gx_part"], o["w2_part"], B, E512, N, N, E512, SPLITS)


def merged(be, d, o, B, N, x=None):
    return be.dense_fwd_stream_gram_stage(d["x"] if x is None else x, d["w"], o["enc_part"], o["gx_part"], o["w2_part"], B, E512,
                                          N, E512, SPLITS, o["x_dst"], N, d["cap"], o["cap_dst"], d["tgt"], o["tgt_tmajor"],
                                          d["a0"], o["h0"], d["c0"], o["c0_dst"], T4, U8, o["pos"], o["row_weight"],
                                          o["tgt_compact"], o["live"], o["loss_row"], o["corr_row"])


# ------------------------------------------------------------------------------ the entry point
@pytest.mark.parametrize("kind", ["full", "pad", "interior"])
@pytest.mark.parametrize("N", [16, 592])          # one 16-k tile for 64 wave slots; 37 tiles: some slots get none
@pytest.mark.parametrize("B", [1, 5, 64])
def test_merged_launch_equals_the_two_launches(be, B, N, kind):
    d = inputs(B, N, kind, 100 * B + N)
    ref, got = outputs(B, N), outputs(B, N)
    two_launches(be, d, ref, B, N)
    assert merged(be, d, got, B, N) is True
    live = int(ref["live"].item())
    assert 0 < live <= B * T4 and (kind == "interior" or live == (B * T4 if kind == "full" else B))
    if kind == "interior":
        assert int(ref["pos"][2 * B].item()) >= 0, "the fed 0 with another target keeps its own row"
    for k in ("enc_part", "w2_part", "x_dst", "h0", "c0_dst"):
        assert bool(torch.isfinite(ref[k]).all()), (k, "the reference left elements unwritten")
    for k in ref:
        assert same(got[k], ref[k]), (k, B, N, kind)
    assert same(got["x_dst"], d["x"]) and same(got["tgt_tmajor"].view(T4, B), d["tgt"].t().contiguous())
    assert merged(be, d, got, B, N) is True       # ... and again on the same buffers
    for k in ref:
        assert same(got[k], ref[k]), (k, B, N, kind, "second launch")


# ------------------------------------------------------------------------------ refusals
def raw_rc(be, d, o, B, N, x):
    p = lambda t: t.data_ptr()
    return be.lib.tnt_dense_fwd_stream_gram_stage_f32(
        p(x), p(d["w"]), p(o["enc_part"]), p(o["gx_part"]), p(o["w2_part"]), B, E512, N, E512, SPLITS, p(o["x_dst"]), N,
        p(d["cap"]), p(o["cap_dst"]), p(d["tgt"]), p(o["tgt_tmajor"]), p(d["a0"]), p(o["h0"]), p(d["c0"]), p(o["c0_dst"]), T4,
        U8, p(o["pos"]), p(o["row_weight"]), p(o["tgt_compact"]), p(o["live"]), p(o["loss_row"]), p(o["corr_row"]), be._s())


def misaligned(x):
    """the same values one float off a 16-byte boundary"""
    buf = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    y = buf[1:1 + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == 4 and y.is_contiguous()
    return y


@pytest.mark.parametrize("case,B,N", [("misaligned", 8, 592), ("B65", 65, 592), ("N20", 8, 20)])
def test_entry_refuses_before_any_launch(be, case, B, N):
    d = inputs(B, N, "interior", 7)
    x = misaligned(d["x"]) if case == "misaligned" else d["x"]
    o, untouched = outputs(B, N), outputs(B, N)
    assert raw_rc(be, d, o, B, N, x) != 0
    rec = be._rec = []
    try:
        assert merged(be, d, o, B, N, x=x) is False
    finally:
        be._rec = None
    assert rec == [], "a refused call is not part of a launch plan"
    torch.cuda.synchronize()
    for k in o:
        assert same(o[k], untouched[k]), (k, "written by a refused call")


# ------------------------------------------------------------------------------ the training step
NV, V50, T5, B8 = 592, 50, 5, 8


def make_model(stage_fwd, N=NV, r_in=0.0, **attrs):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    m = NIC(N, E512, E512, V50, T5, r_in, 0.2, 0.2, 0.01, 0.00003, 0.00001, seed=42)         # the rates of bench.make_model
    m.stage_fwd = stage_fwd
    for k, v in attrs.items():
        setattr(m, k, v)
    m.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def host_batch(B=B8, N=NV):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, N)).astype(np.float32)
    cap = np.zeros((B, T5), np.int32)
    for b in range(B):
        L = int(rng.integers(0, T5 - 1))
        cap[b, 0] = 1
        cap[b, 1:1 + L] = rng.integers(3, V50, size=L)
        cap[b, 1 + L] = 2
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    z = np.zeros((B, E512), np.float32)
    return (x, cap, z, z.copy()), tgt


def dev_batch(h, x_dtype=torch.float32, shift=False):
    (x, cap, a0, c0), tgt = h
    xd = dev(x).to(x_dtype)
    return (misaligned(xd) if shift else xd, dev(cap, torch.int32), dev(a0), dev(c0)), dev(tgt, torch.int32)


def run(m, batch, steps):
    """``steps`` training steps, the first (eager) one with the backend recording -> (names launched in step 1, metrics,
    state)"""
    rec = m.be._rec = []
    try:
        hist = [m.train_step(batch).as_floats()]
    finally:
        m.be._rec = None
    hist += [m.train_step(batch).as_floats() for _ in range(steps - 1)]
    m.check_device_errors()
    state = dict(theta=m.arena.theta.clone(), m=m.opt_m.clone(), v=m.opt_v.clone(), mean=m.mov_mean.clone(),
                 var=m.mov_var.clone())
    assert all(np.isfinite(v) for h in hist for v in h.values()), hist
    return [name for _, name, _ in rec], hist, state


def assert_same_run(a, b):
    (_, ha, sa), (_, hb, sb) = a, b
    assert ha == hb, (ha, hb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("plan_step", [True, False])
def test_training_step_merged_on_against_off(plan_step):
    """four steps (eager, recorded / captured, two replays) from one seed: weights, Adam moments, moving statistics and every
    metric equal, and the merged launch stands for the two it replaces"""
    batch = dev_batch(host_batch())
    on, off = make_model(True, plan_step=plan_step), make_model(False, plan_step=plan_step)
    ra, rb = run(on, batch, 4), run(off, batch, 4)
    if not on._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    assert MERGED in ra[0] and STAGE not in ra[0] and GRAM not in ra[0], ra[0]
    assert MERGED not in rb[0] and STAGE in rb[0] and GRAM in rb[0], rb[0]
    assert len(ra[0]) == len(rb[0]) - 1, "one launch less"
    assert isinstance(on._graphs[("train", B8, T5, "compact")], tuple) == plan_step
    assert_same_run(ra, rb)


@pytest.mark.parametrize("case", ["misaligned", "B65", "N20"])
def test_model_falls_back_where_the_entry_refuses(case):
    """B = 65 and N = 20 never reach the entry (the model's own conditions); a misaligned x does, is refused, and the model
    issues the staging launch of the two-launch step -- which has always refused such a tensor: the same launch and the same
    error with ``stage_fwd`` on and off"""
    from masters_thesis_amd._lib import KernelLibraryError
    B, N = (65, NV) if case == "B65" else (B8, 20) if case == "N20" else (B8, NV)
    batch = dev_batch(host_batch(B, N), shift=case == "misaligned")
    if case == "misaligned":
        for stage_fwd in (True, False):
            m = make_model(stage_fwd)
            rec = m.be._rec = []
            try:
                with pytest.raises(KernelLibraryError, match=STAGE):
                    m.train_step(batch)
            finally:
                m.be._rec = None
            assert [name for _, name, _ in rec] == [STAGE], (stage_fwd, rec)
        return
    ra, rb = run(make_model(True, N=N), batch, 3), run(make_model(False, N=N), batch, 3)
    assert MERGED not in ra[0] and ra[0] == rb[0], (ra[0], rb[0])
    assert_same_run(ra, rb)


@pytest.mark.parametrize("case", ["r_in", "float16", "numpy"])
def test_other_steps_keep_the_two_launches(case):
    """input Dropout (the forward reads the masked copy), float16 betas (widened by the staging launch), host inputs (staged
    tensor by tensor)"""
    h = host_batch()
    batch = h if case == "numpy" else dev_batch(h, torch.float16 if case == "float16" else torch.float32)
    r_in = 0.1 if case == "r_in" else 0.0
    ra, rb = run(make_model(True, r_in=r_in), batch, 3), run(make_model(False, r_in=r_in), batch, 3)
    assert MERGED not in ra[0] and GRAM in ra[0] and ra[0] == rb[0], (ra[0], rb[0])
    if case == "r_in":
        assert STAGE in ra[0]
    elif case == "float16":
        assert "tnt_stage_batch_h16" in ra[0]
    assert_same_run(ra, rb)
