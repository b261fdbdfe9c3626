"""Consensus decoding on the GPU, the models: nic.NIC, lc_nic.NIC and ms_nic.NIC with the weights of the tiny golden
fixtures against the float64 consensus loops of tests/consensus_oracle.py -- copies of one scan equal the plain decode,
different scans equal the restatement (greedy, beam, with constraints), the sampler reads the mixed rows, the captured
replay repeats the bits, the subject slices are the members, and consensus=None is the call without the keyword."""
import numpy as np
import pytest

import consensus_oracle as CO
from topkp_oracle import sample_topkp

pytestmark = pytest.mark.gpu

T, K, END = 4, 3, 2
# scans whose float64 consensus loops decide nothing by less than GAP (asserted on the restatement in the tests)
SEED = {"dense": 56, "lc": 20, "ms": 2}
SEED_COPIES = {"dense": 1, "lc": 5}              # the same for the plain decode of the scans that are copied
GAP = 1e-4
bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a


def device_model(kind, **kw):
    orc, ctor, mkw = CO.golden_case(kind)
    if kind == "dense":
        from masters_thesis_amd.nic import NIC
    elif kind == "lc":
        from masters_thesis_amd.lc_nic import NIC
    else:
        from masters_thesis_amd.ms_nic import NIC
    model = NIC(*ctor, seed=11, **mkw, **kw)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return orc, model


def run(kind, model, path, x, z, start, **kw):
    """-> (ids (M, T) or (M, k, T), probs (T, M, V) or scores (M, k)) of one decode path"""
    if path == "beam":
        return model.beam_search(x, z, z, start, T, beam_width=K, end_id=END, **kw)
    if path == "sample":
        kw.update(temperature=0.9, top_k=5, top_p=0.95, sample_step=3)
    if kind == "dense":
        if path == "greedy":
            p = model.greedy_predict(x, z, z, start, T, **kw)[:, :, 0, :]
            return p.argmax(-1).T, p
        ids, p = model.sample_predict(x, z, z, start, T, **kw)
        return ids[:, :, 0], p[:, :, 0, :]
    out = (model.greedy_predict if path == "greedy" else model.sample_predict)(x, z, z, start, T, **kw)
    return out[0][:, :, 0], out[1].transpose(1, 0, 2)


def members(kind):
    return 2 if kind == "ms" else 3


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_copies_of_one_scan_decode_as_the_scan_alone(kind):
    from masters_thesis_amd.model_base import Consensus
    from constrain_oracle import constrained_beam, constrained_decode
    orc, model = device_model(kind)
    for G in (2, 4):
        x, z, start = CO.scans(G, 3, SEED_COPIES[kind], identical=True)
        gap = CO.rel_gap(constrained_decode(orc, x[:3], z[:3], z[:3], start, T)[1].reshape(-1, orc.V)).min()
        margin = constrained_beam(orc, x[:3], z[:3], z[:3], start, T, k=K, end_id=END)[2].min()
        assert gap >= GAP and margin >= GAP, (gap, margin)         # the restatement alone: nothing is decided by a near tie
        for path in ("greedy", "beam"):
            plain = run(kind, model, path, x[:3], z[:3], start)
            for mode in CO.MODES:
                got = run(kind, model, path, x, z, start, consensus=Consensus(G, mode))
                assert got[0].shape == plain[0].shape and got[1].shape == plain[1].shape
                assert np.array_equal(got[0], plain[0]), (G, path, mode)
                if path == "beam":
                    assert np.abs(got[1] - plain[1]).max() <= 1e-5 * np.abs(plain[1]).max(), (G, mode)
                else:
                    assert np.abs(got[1] - plain[1]).max() <= 1e-5, (G, mode)


@pytest.mark.parametrize("kind", ["dense", "lc", "ms"])
def test_different_scans_match_the_float64_loop(kind):
    """(b) and (f): three scans per image, or the two subject slices of ms2_tiny; (d): the same with constraints"""
    from masters_thesis_amd.model_base import Consensus, DecodeConstraints
    orc, model = device_model(kind)
    G = members(kind)
    x, z, start = CO.scans(G, 3, SEED[kind])
    w = None if kind == "ms" else (0.5, 0.2, 0.3)
    con = dict(theta=1.0, n=2, m=3, end_id=END, bad_ids=())
    for mode in CO.MODES:
        for weights in (None, w) if w else (None,):
            wf = None if weights is None else np.asarray(Consensus(G, mode, weights).weights)
            for c in (None, con) if weights is None else (None,):
                ckw = {} if c is None else dict(constraints=DecodeConstraints(no_repeat_ngram_size=2, min_length=3, end_id=END))
                ids, probs, gap = CO.consensus_decode(orc, x, z, z, start, T, G, mode, wf, con=c)
                seqs, scores, margin = CO.consensus_beam(orc, x, z, z, start, T, G, K, END, mode, wf, con=c)
                if weights is None:
                    assert gap.min() >= GAP and margin.min() >= GAP, (kind, mode, gap.min(), margin.min())     # the restatement alone
                keep = slice(None) if weights is None else (gap >= GAP) & (margin >= GAP)
                cons = Consensus(G, mode, weights)
                got = run(kind, model, "greedy", x, z, start, consensus=cons, **ckw)
                assert got[0].shape == (3, T) and got[1].shape == probs.shape
                assert np.array_equal(got[0][keep], ids[keep]), (kind, mode, weights, c)
                assert np.abs(got[1][:, keep] - probs[:, keep]).max() <= 1e-5, (kind, mode)
                gb = run(kind, model, "beam", x, z, start, consensus=cons, **ckw)
                assert gb[0].shape == (3, K, T) and gb[1].shape == (3, K)
                assert np.array_equal(gb[0][keep], seqs[keep]), (kind, mode, weights, c)
                assert np.abs(gb[1][keep] - scores[keep]).max() <= 1e-5 * np.abs(scores[keep]).max(), (kind, mode)
                if c is not None:                  # the constraints bit: no <end> before position 3, no repeated bigram
                    assert not np.any(got[0][:, :3] == END) and np.all(got[1][:3, :, END] == 0.0)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_the_sampler_reads_the_mixture_and_every_member_is_fed_the_draw(kind):
    from masters_thesis_amd.model_base import Consensus
    from oracle import models as M
    _, model = device_model(kind)
    G = 3
    x, z, start = CO.scans(G, 3, 9)
    for mode in CO.MODES:
        ids, probs = run(kind, model, "sample", x, z, start, consensus=Consensus(G, mode))
        assert ids.shape == (3, T) and probs.shape[:2] == (T, 3)
        assert np.abs(probs.sum(-1) - 1).max() <= 1e-5
        ok = np.ones(3, bool)
        for i in range(T):
            want, margin = sample_topkp(probs[i].astype(np.float64), 0.9, 5, 0.95, False, model.seed, M.S_SAMPLE + i, 3)
            ok &= margin > 1e-5                    # the sampler's own decision margin (tests/test_gpu_sampling.py)
            assert np.array_equal(ids[ok, i], want[ok]), (kind, mode, i)
        assert ok.sum() >= 2
    if kind == "lc":                               # the unfiltered draw (tnt_sample_rows_f32, not captured) takes the same route
        out = model.sample_predict(x, z, z, start, T, sample_step=3, consensus=Consensus(G))
        assert out[0].shape == (3, T, 1) and out[1].shape[:2] == (3, T) and out[2].shape[1] == G * 3


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_replay_returns_the_same_bits(kind):
    import torch
    from masters_thesis_amd.model_base import Consensus
    _, model = device_model(kind)
    G = 3
    x, z, start = CO.scans(G, 3, SEED[kind])
    for path in ("greedy", "sample", "beam"):
        outs = [run(kind, model, path, x, z, start, consensus=Consensus(G, "logmean")) for _ in range(3)]
        for o in outs[1:]:                         # eager warm-up, capture + replay, replay
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(bits(o[1]), bits(outs[0][1])), path
        if not (kind == "lc" and path == "beam"):  # lc_nic's beam loop is eager
            keys = [k for k in model._graphs if k[0] == path and "consensus" in k]
            assert len(keys) == 1 and isinstance(model._graphs[keys[0]], torch.cuda.CUDAGraph), keys


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_none_is_the_call_without_the_keyword(kind):
    _, model = device_model(kind)
    x, z, start = CO.scans(1, 3, 8)
    for path in ("greedy", "sample", "beam"):
        base = run(kind, model, path, x, z, start)
        keys = set(model._graphs)
        got = run(kind, model, path, x, z, start, consensus=None)
        assert np.array_equal(got[0], base[0]) and np.array_equal(bits(got[1]), bits(base[1])), path
        assert set(model._graphs) == keys and "_cons_bufs" not in model.__dict__


def test_one_member_goes_through_the_kernel_and_equals_the_plain_decode():
    from masters_thesis_amd.model_base import Consensus
    _, model = device_model("dense")
    x, z, start = CO.scans(1, 3, 8)
    base = run("dense", model, "greedy", x, z, start)
    got = run("dense", model, "greedy", x, z, start, consensus=Consensus(1))
    assert np.array_equal(got[0], base[0]) and np.abs(got[1] - base[1]).max() <= 1e-6
    assert "_cons_bufs" in model.__dict__ and any("consensus" in k for k in model._graphs)
