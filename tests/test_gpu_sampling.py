"""Top-k / nucleus sampling on the GPU: tnt_sample_topkp_f32 against the float64 restatement (tests/topkp_oracle.py) over
a grid of shapes and filters, its reduction to tnt_sample_rows_f32, top_k = 1 as the argmax, its stream, its
distribution, the sampled decode of both models at the BASELINE shapes against the float64 decode, and captured replay
against eager decoding."""
import numpy as np
import pytest
import torch

from oracle import models as M
from helpers import tiny_groups
from topkp_oracle import SampledNICDense, filter_weights, sample_topkp

pytestmark = pytest.mark.gpu

MARGIN = 1e-5


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def _rows(rng, rows, V, ld, from_logits):
    """float32 input rows (rows, ld): plain rows, rows quantised to a coarse grid (exact ties everywhere, at every
    boundary), and rows with zero-probability columns; probabilities are the float32 softmax"""
    l = rng.standard_normal((rows, V)) * 2.0
    l[1::3] = np.round(l[1::3] * 2) / 2
    zero = np.zeros((rows, V), bool)
    zero[2::3] = rng.random((len(range(2, rows, 3)), V)) < 0.3
    zero[:, 0] &= False                                  # column 0 keeps every row non-empty
    l = np.where(zero, -np.inf, l).astype(np.float32)
    if not from_logits:
        e = np.exp(l.astype(np.float64) - l.max(-1, keepdims=True))
        l = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    x = np.full((rows, ld), np.nan, np.float32)          # the padding columns must never be read
    x[:, :V] = l
    return x, zero


@pytest.mark.parametrize("V", [1, 2, 13, 257, 5001, 16384])
@pytest.mark.parametrize("from_logits", [True, False])
def test_kernel_matches_restatement(be, V, from_logits):
    rng = np.random.default_rng(V + from_logits)
    rows, ld = 48, V + 3
    x, zero = _rows(rng, rows, V, ld, from_logits)
    xd = dev(x)
    out = torch.zeros(rows, dtype=torch.int32, device="cuda")
    n = nbad = 0
    worst = 0.0
    for temp in (0.7, 1.0, 1.5):
        for k in sorted({0, 1, 5, 50, V - 1, V, V + 3}):
            for p in (0.05, 0.5, 0.9, 1.0):
                site, step = 7 + k, int(p * 100)
                be.sample_topkp(xd, out, rows, V, ld, temp, k, p, from_logits, 1234, site, step, None)
                got = out.cpu().numpy()
                assert (got >= 0).all() and (got < V).all()
                assert not zero[np.arange(rows), got].any()
                want, margin = sample_topkp(x[:, :V], temp, k, p, from_logits, 1234, site, step)
                bad = got != want
                assert np.all(margin[bad] < MARGIN), (temp, k, p, np.flatnonzero(bad), margin[bad])
                n += rows
                nbad += int(bad.sum())
                worst = max(worst, float(margin[bad].max()) if bad.any() else 0.0)
    print(f"V={V} from_logits={from_logits}: {nbad} of {n} rows differ from float64 (all within margin {MARGIN})")
    assert nbad <= 0.01 * n


@pytest.mark.parametrize("V,ld,from_logits,temp", [(1, 1, True, 1.0), (11, 12, True, 1.0), (5001, 5004, False, 1.0),
                                                   (5001, 5004, True, 0.7), (300, 300, False, 2.0),
                                                   (16384, 16385, True, 1.3)])
def test_unfiltered_equals_sample_rows(be, V, ld, from_logits, temp):
    rng = np.random.default_rng(V)
    rows = 512
    logits = rng.standard_normal((rows, ld)) * 2.0
    if from_logits:
        x = logits
    else:
        x = np.exp(logits) / np.exp(logits[:, :V]).sum(-1, keepdims=True)
    xd = dev(x)
    a = torch.zeros(rows, dtype=torch.int32, device="cuda")
    b = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
    step_dev = torch.tensor([2], dtype=torch.int32, device="cuda")
    be.sample_rows(xd, a, rows, V, ld, temp, from_logits, 99, 113, 3, step_dev)
    be.sample_topkp(xd, b, rows, V, ld, temp, 0, 1.0, from_logits, 99, 113, 3, step_dev)
    assert torch.equal(a, b)
    be.sample_topkp(xd, b, rows, V, ld, temp, V + 5, 1.0, from_logits, 99, 113, 3, step_dev)    # K >= V: no filter
    assert torch.equal(a, b)


def test_top1_is_the_argmax(be):
    rng = np.random.default_rng(5)
    rows, V = 256, 5001
    x = rng.standard_normal((rows, V)).astype(np.float32)
    tied = np.arange(rows) % 2 == 1
    for r in np.flatnonzero(tied):
        j = np.sort(rng.choice(V, 4, replace=False))
        x[r, j] = x[r].max() + 0.5
    out = torch.zeros(rows, dtype=torch.int32, device="cuda")
    for from_logits in (True, False):
        xi = x if from_logits else np.exp(x - x.max(-1, keepdims=True)) / np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)
        xi = xi.astype(np.float32)
        for p in (1.0, 0.3):
            be.sample_topkp(dev(xi), out, rows, V, V, 1.0, 1, p, from_logits, 3, 9, 1, None)
            got = out.cpu().numpy()
            want = np.array([np.flatnonzero(row == row.max())[0] for row in xi])
            assert np.array_equal(got, want)
            assert (tied[:, None] & (np.arange(V)[None, :] < got[:, None]) & (xi == xi.max(-1, keepdims=True))).sum() == 0


def test_stream(be):
    rng = np.random.default_rng(6)
    rows, V = 512, 5001
    x = dev(rng.standard_normal((rows, V)))
    o = [torch.zeros(rows, dtype=torch.int32, device="cuda") for _ in range(4)]
    be.sample_topkp(x, o[0], rows, V, V, 1.0, 50, 0.9, True, 77, 120, 5, None)
    be.sample_topkp(x, o[1], rows, V, V, 1.0, 50, 0.9, True, 77, 120, 5, None)
    be.sample_topkp(x, o[2], rows, V, V, 1.0, 50, 0.9, True, 77, 120, 2, torch.tensor([3], dtype=torch.int32, device="cuda"))
    be.sample_topkp(x, o[3], rows, V, V, 1.0, 50, 0.9, True, 77, 120, 6, None)
    assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
    assert not torch.equal(o[0], o[3])


@pytest.mark.parametrize("k,p", [(3, 1.0), (0, 0.6)])
def test_distribution(be, k, p):
    probs = np.array([0.3, 0.05, 0.25, 0.1, 0.2, 0.1])
    n = 60000
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    be.sample_topkp(dev(np.tile(probs, (n, 1))), out, n, 6, 6, 1.0, k, p, False, 21, 7, 0, None)
    keep, _ = filter_weights(probs / probs.max(), k, p)
    want = np.where(keep, probs, 0) / probs[keep].sum()
    got = np.bincount(out.cpu().numpy(), minlength=6) / n
    assert np.abs(got - want).max() < 0.01, (got, want)
    assert got[~keep].sum() == 0


def test_bad_arguments(be):
    from masters_thesis_amd._lib import KernelLibraryError
    x = dev(np.zeros((2, 20000)))
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    for args in [(0, 5, 1.0, 0, 0.5), (2, 0, 1.0, 0, 0.5), (2, 5, 0.0, 0, 0.5), (2, 5, 1.0, 0, 0.0), (2, 16385, 1.0, 0, 0.5)]:
        rows, V, t, k, p = args
        with pytest.raises(KernelLibraryError):
            be.sample_topkp(x, out, rows, V, 20000, t, k, p, True, 1, 1, 1, None)


# ---------------------------------------------------------------------------------------------------- BASELINE shapes
B0, T0, V0, U0, E0, N0 = 64, 15, 5001, 512, 512, 20000


def _prefix_compare(name, got_ids, got_probs, want_ids, want_probs, margins):
    """ids (B, T) compared up to each sample's first position whose draw has margin < MARGIN (after a near tie the
    rest of a caption legitimately diverges); probabilities (B, T, V) over the compared prefix plus that position"""
    B, T = got_ids.shape
    low = margins < MARGIN
    cut = np.where(low.any(1), low.argmax(1), T)
    for b in range(B):
        assert np.array_equal(got_ids[b, :cut[b]], want_ids[b, :cut[b]]), (name, b, cut[b])
        n = min(cut[b] + 1, T)
        assert np.abs(got_probs[b, :n] - want_probs[b, :n]).max() < 1e-4, (name, b)
    print(f"{name}: {int((T - cut).sum())} of {B * T} positions cut after a near tie ({int((cut < T).sum())} captions)")
    assert (cut > 0).mean() >= 0.5


def _sharpen(model, p0):
    """scale the output layer so that the logits spread like a trained model's (std 2.5 over the vocabulary) instead of
    the near-uniform distribution of the initial weights, where nearly every filter decision is a near tie"""
    f = 2.5 / np.log(np.maximum(p0, 1e-30)).std(-1).mean()
    for k in ("time_distributed_softmax/kernel", "time_distributed_softmax/bias"):
        model.set_weight(k, model.get_weight(k) * f)


def _recording_sampler(seed, temp, k, p, step, margins):
    def s(probs, i):
        ids, m = sample_topkp(probs, temp, k, p, False, seed, M.S_SAMPLE + i, step)
        if i == 0:
            print(f"position 0: {(m < MARGIN).sum()} of {len(m)} draws within the margin")
        margins.append(m)
        return ids
    return s


@pytest.mark.parametrize("k,p", [(0, 0.9), (40, 1.0), (200, 0.5)])
def test_attention_decode_at_config3(k, p):
    from masters_thesis_amd.lc_nic import NIC, synthetic_groups
    g = synthetic_groups(N0, 360, 32, seed=42)
    model = NIC(g, U0, 512, E0, 32, V0, T0, 0.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 3e-5, 1e-5, seed=42)
    rng = np.random.default_rng(31)
    x = rng.standard_normal((B0, N0)).astype(np.float32)
    z = np.zeros((B0, U0), np.float32)
    start = np.ones(B0, np.int64)
    _sharpen(model, model.greedy_predict(x, z, z, start, 1, return_s=False)[1][:, 0])
    orc = M.LcNIC(g, U0, 512, E0, 32, V0, T0, 0.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.01, 0.001, 3e-5, 1e-5)
    orc.p = {key: v.astype(np.float64) for key, v in model.get_weights_dict().items()}
    got = model.sample_predict(x, z, z, start, T0, temperature=1.0, top_k=k, top_p=p, sample_step=4)
    margins = []
    want = orc.greedy_predict(x, z, z, start, T0, sampler=_recording_sampler(model.seed, 1.0, k, p, 4, margins))
    _prefix_compare(f"config 3 top_k={k} top_p={p}", got[0][:, :, 0], got[1], want[0][:, :, 0], want[1],
                    np.stack(margins, 1))


@pytest.mark.parametrize("k,p", [(0, 0.9), (40, 1.0), (200, 0.5)])
def test_dense_decode_at_config2(k, p):
    from masters_thesis_amd.nic import NIC
    model = NIC(N0, U0, E0, V0, T0, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5, seed=42)
    rng = np.random.default_rng(32)
    x = rng.standard_normal((B0, N0)).astype(np.float32)
    z = np.zeros((B0, U0), np.float32)
    start = np.ones(B0, np.int64)
    _sharpen(model, model.greedy_predict(x, z, z, start, 1)[0, :, 0])
    orc = SampledNICDense(N0, U0, E0, V0, T0, 0.0, 0.2, 0.2, 0.01, 3e-5, 1e-5)
    orc.p = {key: v.astype(np.float64) for key, v in model.get_weights_dict().items()}
    ids, probs = model.sample_predict(x, z, z, start, T0, temperature=1.0, top_k=k, top_p=p, sample_step=4)
    margins = []
    wids, wprobs = orc.sample_predict(x, z, z, start, T0, _recording_sampler(model.seed, 1.0, k, p, 4, margins))
    _prefix_compare(f"config 2 top_k={k} top_p={p}", ids[:, :, 0], probs[:, :, 0].transpose(1, 0, 2), wids[:, :, 0],
                    wprobs[:, :, 0].transpose(1, 0, 2), np.stack(margins, 1))


# ---------------------------------------------------------------------------------------------------- captured replay
def _small_pair(kind):
    rng = np.random.default_rng(51)
    models = []
    if kind == "attention":
        from masters_thesis_amd.lc_nic import NIC
        g = (tiny_groups(41, 5, rng), [16] * 5)
        orc = M.LcNIC(g, 16, 512, 12, 6, 13, 5, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5).init_params(rng)
        for use_graph in (True, False):
            models.append(NIC(g, 16, 512, 12, 6, 13, 5, *(0,) * 6, 0.01, 0.001, 3e-5, 1e-5, seed=9, use_graph=use_graph))
        N = 41
    else:
        from masters_thesis_amd.nic import NIC
        orc = M.NICDense(23, 16, 10, 13, 6, 0, 0, 0, 0.01, 3e-5, 1e-5).init_params(rng)
        for use_graph in (True, False):
            models.append(NIC(23, 16, 10, 13, 6, 0, 0, 0, 0.01, 3e-5, 1e-5, seed=9, use_graph=use_graph))
        N = 23
    for m in models:
        for key, v in orc.p.items():
            m.set_weight(key, v)
    return models, N


@pytest.mark.parametrize("kind", ["attention", "dense"])
def test_captured_replay_equals_eager(kind):
    (graph, eager), N = _small_pair(kind)
    rng = np.random.default_rng(52)
    B, T, U = 8, 5, 16
    x = rng.standard_normal((B, N)).astype(np.float32)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    outs = []
    for step in (0, 1, 2):              # eager warm-up, capture, replay on the graph-using model
        a = graph.sample_predict(x, z, z, start, T, top_k=6, top_p=0.8, sample_step=step)
        b = eager.sample_predict(x, z, z, start, T, top_k=6, top_p=0.8, sample_step=step)
        for u, v in zip(a, b):
            if u is not None:
                assert np.array_equal(u, v), (kind, step)
        outs.append(a[0])
    assert any(not np.array_equal(outs[0], o) for o in outs[1:])
    assert isinstance(graph._graphs[next(k for k in graph._graphs if k[0] == "sample")], torch.cuda.CUDAGraph)
