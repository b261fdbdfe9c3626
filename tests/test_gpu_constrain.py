"""Constrained caption decoding on the GPU: tnt_decode_constrain_f32 bit for bit against the float32 restatement
(tests/constrain_oracle.py) over a grid of shapes, steps, parents, finished rows and rules; its refusals; -inf through
tnt_softmax_cce_f32; the six decode paths of nic.NIC and lc_nic.NIC against the constrained float64 restatements at the
tiny and mid fixture shapes; captured replay, capture reuse across bad_ids, parity without constraints; the properties
of the emitted captions at the config-2 and config-3 sizes; and evaluate.simple_eval's constrained sequential draw."""
import ctypes as C

import numpy as np
import pytest
import torch

from constrain_oracle import (as_dict, case_constraints, constrain_logits_f32, restatement_case, run_path, violations)
from test_gpu_beam import MARGIN

pytestmark = pytest.mark.gpu


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


# ---------------------------------------------------------------------------------------------------- the kernel
def _case(rng, V, ld, rows, i, with_parent, with_fin, n_bad):
    """random inputs of one launch: logits with NaN padding, histories over a small alphabet (repeats, repeated n-grams)
    or the whole vocabulary, out-of-range ids planted, parents permuting within groups of 4 rows"""
    ldh = max(i, 1) + 3
    x = np.full((rows, ld), np.nan, np.float32)
    x[:, :V] = rng.standard_normal((rows, V)).astype(np.float32) * 3
    small = rng.random(rows) < 0.7
    hist = np.where(small[:, None], rng.integers(0, min(V, 4), (rows, ldh)), rng.integers(0, V, (rows, ldh))).astype(np.int32)
    odd = rng.random((rows, ldh)) < 0.05
    hist[odd] = rng.choice([-1, V, V + 100, -2 ** 31], int(odd.sum())).astype(np.int32)
    last = hist[:, -1].copy()
    parent = None
    if with_parent:
        k = 4 if rows % 4 == 0 else 1
        parent = (np.arange(rows) // k * k + np.stack([rng.permutation(k) for _ in range(rows // k)]).reshape(-1)).astype(np.int32)
    fin = (rng.random(rows) < 0.3).astype(np.int32) if with_fin else None
    bad = rng.integers(0, V, n_bad).astype(np.int32)
    if n_bad > 2:
        bad[1] = bad[0]                                       # a duplicate
        bad[2] = V + 5                                        # out of range: ignored
    return x, hist, last, parent, fin, bad, ldh


def _expect(x, hist_in, last, parent, fin, bad, V, i, theta, n, m, end_id):
    rows = x.shape[0]
    par = np.arange(rows) if parent is None else parent
    h = np.concatenate([hist_in[par][:, :max(i - 1, 0)], last[:, None]], axis=1)[:, :i] if i > 0 else np.zeros((rows, 0), np.int32)
    out = x.copy()
    for r in range(rows):
        if fin is None or not fin[r]:
            out[r, :V] = constrain_logits_f32(x[r, :V], h[r], theta, n, m, end_id, bad.tolist(), i)
    return out, h


@pytest.mark.parametrize("V", [11, 5001])
@pytest.mark.parametrize("rows", [1, 64, 320])
def test_kernel_equals_restatement_bitwise(be, V, rows):
    rng = np.random.default_rng(V * 7 + rows)
    dev = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    # (ld, n, i, parents, fin) is a full product; theta x n_bad (9 pairs) and the 4 (m, end_id) choices are CYCLED over it
    # by the launch counter, a deterministic sample, not a product with it: every value occurs, 9 and 4 are coprime so every
    # (theta, n_bad, m, end_id) combination occurs too, but which of them meets which i and n follows from the loop order
    rest = [(th, nb) for th in (1.0, 1.2, 2.0) for nb in (0, 1, 64)]
    cases = q = 0
    for ld in (V, V + 5):
        for n in (0, 1, 2, 3):
            for i in sorted({0, 1, max(n - 1, 0), n, 14, 64}):
                for with_parent in (False, True):
                    for with_fin in (False, True):
                        theta, n_bad = rest[q % 9]
                        q += 1
                        m, end_id = ((0, -1), (3, 2), (20, V - 1), (70, 0))[q % 4]
                        x, hist, last, parent, fin, bad, ldh = _case(rng, V, ld, rows, i, with_parent, with_fin, n_bad)
                        want, h = _expect(x, hist, last, parent, fin, bad, V, i, theta, n, m, end_id)
                        xd, hin = dev(x), dev(hist)
                        hout = torch.full((rows, ldh), -9, dtype=torch.int32, device="cuda")
                        be.decode_constrain(xd, ld, V, rows, i, hin, hout, ldh, dev(last) if i > 0 else None, dev(parent),
                                            dev(fin), theta, n, m, end_id, dev(bad) if n_bad else None, n_bad)
                        torch.cuda.synchronize()
                        got, gh = xd.cpu().numpy(), hout.cpu().numpy()
                        tag = (V, ld, rows, i, n, theta, n_bad, m, end_id, with_parent, with_fin)
                        assert np.array_equal(got.view(np.int32), want.view(np.int32)), tag
                        assert np.array_equal(gh[:, :i], h) and np.all(gh[:, i:] == -9), tag
                        assert np.array_equal(hin.cpu().numpy(), hist), tag
                        cases += 1
    print(f"V={V} rows={rows}: {cases} launches bit-identical")


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    x = torch.randn(8, 16, device="cuda")
    x0 = x.clone()
    i32 = dict(dtype=torch.int32, device="cuda")
    hin, hout = torch.ones(8, 8, **i32), torch.full((8, 8), -9, **i32)
    last, bad = torch.ones(8, **i32), torch.ones(4, **i32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(logits=x, ld=16, V=12, rows=8, i=3, hist_in=hin, hist_out=hout, ldh=8, last_token=last, theta=1.5, n=2, m=0,
             end_id=-1, bad_ids=bad, n_bad=4):
        return lib.tnt_decode_constrain_f32(p(logits), ld, V, rows, i, p(hist_in), p(hist_out), ldh, p(last_token), None, None,
                                            theta, n, m, end_id, p(bad_ids), n_bad, None)
    bads = [dict(rows=0), dict(rows=-1), dict(V=0), dict(ld=11), dict(ldh=2), dict(i=0, ldh=0), dict(i=-1), dict(i=65, ldh=80),
            dict(theta=0.99), dict(theta=float("nan")), dict(theta=float("inf")), dict(n=-1), dict(m=-1), dict(m=2, end_id=-1),
            dict(logits=None), dict(hist_in=None), dict(hist_out=None), dict(bad_ids=None), dict(hist_out=hin),
            dict(last_token=None), dict(n_bad=65), dict(n_bad=-1)]
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw, rc)                   # TNT_BADARG
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and bool((hout == -9).all())     # nothing was launched
    assert call() == 0 and call(i=0, hist_in=None, last_token=None) == 0 and call(bad_ids=None, n_bad=0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x, x0)


@pytest.mark.parametrize("V,ld", [(29, 29), (501, 504), (5001, 5008)])
def test_softmax_turns_a_ban_into_probability_zero(be, V, ld):
    rng = np.random.default_rng(V)
    rows, i = 64, 9
    x = torch.from_numpy((rng.standard_normal((rows, ld)) * 4).astype(np.float32)).cuda()
    hist = torch.from_numpy(rng.integers(0, V, (rows, 12)).astype(np.int32)).cuda()
    hout = torch.zeros_like(hist)
    bad = torch.from_numpy(rng.choice(V, 5, replace=False).astype(np.int32)).cuda()
    be.decode_constrain(x, ld, V, rows, i, hist, hout, 12, hist[:, 11].contiguous(), None, None, 1.2, 1, 20, 0, bad, 5)
    banned = torch.isinf(x[:, :V]) & (x[:, :V] < 0)
    assert int(banned.sum()) >= rows * 6 and bool(banned[:, 0].all())
    be.softmax_cce(x, None, x, None, None, None, rows, V, ld, 0.0)
    torch.cuda.synchronize()
    p = x[:, :V]
    assert bool((p[banned] == 0.0).all())
    assert bool(torch.isfinite(p).all()) and torch.allclose(p.sum(-1), torch.ones(rows, device="cuda"), atol=1e-5)
    assert bool((p[~banned] > 0).any())


# ---------------------------------------------------------------------------------------------------- the models
def _device_model(kind, orc, ctor, **kw):
    if kind == "dense":
        from masters_thesis_amd.nic import NIC
    else:
        from masters_thesis_amd.lc_nic import NIC
    model = NIC(*ctor, seed=11, **kw)
    for k, v in orc.p.items():
        model.set_weight(k, v)
    return model


def _run_model(kind, model, path, x, z, start, T, c, k, end_id, explicit=False):
    """-> (ids, probs (T, B, V) or scores); c None: the call without the keyword, or with constraints=None (explicit)"""
    kw = {"constraints": c} if (c is not None or explicit) else {}
    if path == "beam":
        return model.beam_search(x, z, z, start, T, beam_width=k, end_id=end_id, **kw)
    if path == "sample":
        kw.update(temperature=0.9, top_k=8, top_p=0.95, sample_step=3)
    if kind == "dense":
        if path == "greedy":
            p = model.greedy_predict(x, z, z, start, T, **kw)[:, :, 0, :]
            return p.argmax(-1).T, p
        ids, p = model.sample_predict(x, z, z, start, T, **kw)
        return ids[:, :, 0], p[:, :, 0, :]
    out = (model.greedy_predict if path == "greedy" else model.sample_predict)(x, z, z, start, T, **kw)
    return out[0][:, :, 0], out[1].transpose(1, 0, 2)


@pytest.mark.parametrize("shape", ["tiny", "mid"])
@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_models_match_the_restatement(kind, shape):
    from masters_thesis_amd.model_base import DecodeConstraints
    orc, x, z, start, T, ctor = restatement_case(kind, shape, 7)
    model = _device_model(kind, orc, ctor)
    ckw, k, end_id = case_constraints(shape)
    for path in ("greedy", "sample", "beam"):
        c = DecodeConstraints(end_id=-1 if path == "beam" else end_id, **ckw)
        want = run_path(orc, path, x, z, start, T, as_dict(c, end_id), k, end_id, model.seed)
        for call in range(3):                      # eager warm-up, capture + replay, replay
            got = _run_model(kind, model, path, x, z, start, T, c, k, end_id)
        ok = want[2] > (1e-5 if path == "sample" else MARGIN)      # the sampler's margin is relative (test_gpu_sampling.py)
        print(f"{kind} {shape} {path}: {int((~ok).sum())} of {len(ok)} samples left out (margin)")
        assert ok.mean() >= 0.5
        assert np.array_equal(got[0][ok], want[0][ok]), (kind, shape, path)
        if path == "beam":
            assert np.abs(got[1][ok] - want[1][ok]).max() <= 1e-4 * max(1.0, np.abs(want[1][ok]).max())
        else:
            assert np.abs(got[1][:, ok] - want[1][:, ok]).max() <= 1e-4
            assert np.all(got[1][:, :, list(c.bad_ids)] == 0.0)
        for row in got[0][ok].reshape(-1, T):
            assert not violations(row, c.no_repeat_ngram_size, c.min_length, end_id, c.bad_ids)


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_replay_equals_eager_and_one_capture_serves_other_bad_ids(kind):
    from masters_thesis_amd.model_base import DecodeConstraints
    orc, x, z, start, T, ctor = restatement_case(kind, "tiny", 9)
    graph, eager = _device_model(kind, orc, ctor, use_graph=True), _device_model(kind, orc, ctor, use_graph=False)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a
    paths = ("greedy", "sample") if kind == "lc" else ("greedy", "sample", "beam")      # lc_nic's beam loop is eager
    for path in paths:
        for call, bad in enumerate([(3,), (3,), (3,), (5,), (3,)]):
            c = DecodeConstraints(1.2, 2, 2, bad, end_id=-1 if path == "beam" else 2)
            a = _run_model(kind, graph, path, x, z, start, T, c, 3, 2)
            b = _run_model(kind, eager, path, x, z, start, T, c, 3, 2)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (path, call)
            if path != "beam":
                assert np.all(a[1][:, :, bad[0]] == 0.0)
        keys = [key for key in graph._graphs if key[0] == path and "constrain" in key]
        assert len(keys) == 1 and isinstance(graph._graphs[keys[0]], torch.cuda.CUDAGraph), keys
    # a different length of bad_ids, or other parameters, is another capture
    _run_model(kind, graph, "greedy", x, z, start, T, DecodeConstraints(1.2, 2, 2, (3, 5), end_id=2), 3, 2)
    assert len([key for key in graph._graphs if key[0] == "greedy" and "constrain" in key]) == 2


@pytest.mark.parametrize("kind", ["dense", "lc"])
def test_none_and_neutral_are_the_unconstrained_decode(kind):
    from masters_thesis_amd.model_base import DecodeConstraints
    orc, x, z, start, T, ctor = restatement_case(kind, "mid", 10)
    model = _device_model(kind, orc, ctor)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a
    for path in ("greedy", "sample", "beam"):
        base = _run_model(kind, model, path, x, z, start, T, None, 5, 2)
        keys = set(model._graphs)
        for c in (None, DecodeConstraints()):
            got = _run_model(kind, model, path, x, z, start, T, c, 5, 2, explicit=True)
            assert np.array_equal(got[0], base[0]) and np.array_equal(bits(got[1]), bits(base[1])), path
        assert set(model._graphs) == keys and "_con_bufs" not in model.__dict__


def _pick(ids, V):
    """constraint arguments that the unconstrained sequences violate (as tests/test_host_constrain.py picks them)"""
    T = ids.shape[-1]
    ids = ids.reshape(-1, T)
    first = np.bincount(ids[:, :2].reshape(-1), minlength=V)
    first[0] = 0
    end_id = int(first.argmax())
    cnt = np.bincount(ids.reshape(-1), minlength=V)
    cnt[[0, end_id]] = 0
    return dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3,
                bad_ids=tuple(int(v) for v in np.argsort(-cnt, kind="stable")[:3])), end_id


@pytest.mark.parametrize("kind", ["dense", "attention"])
def test_properties_at_full_size(kind):
    """config 2 (dense) and config 3 (attention): V = 5001, B = 64, 15 tokens, width 5"""
    from masters_thesis_amd.model_base import DecodeConstraints
    from test_gpu_beam import _sharpen
    from test_gpu_fullsize import N, U, V, T, make
    B = 64
    model = make(kind, rates=(0.0,) * (3 if kind == "dense" else 6))
    rng = np.random.default_rng(12)
    x = rng.standard_normal((B, N)).astype(np.float32)
    z = np.zeros((B, U), np.float32)
    start = np.ones(B, np.int64)
    k2 = "dense" if kind == "dense" else "lc"
    p0 = _run_model(k2, model, "greedy", x, z, start, 1, None, 1, -1)[1][0]
    _sharpen(model, p0)
    obeys = lambda seqs, c, e: all(not violations(r, c.no_repeat_ngram_size, c.min_length, e, c.bad_ids) for r in seqs.reshape(-1, T))
    seen = lambda seqs, c, e: set().union(*(violations(r, c.no_repeat_ngram_size, c.min_length, e, c.bad_ids) for r in seqs.reshape(-1, T)))
    # greedy
    free = _run_model(k2, model, "greedy", x, z, start, T, None, 1, -1)[0]
    ckw, end_id = _pick(free, V)
    c = DecodeConstraints(end_id=end_id, **ckw)
    assert seen(free, c, end_id) == {"ngram", "min_length", "bad"}
    assert obeys(_run_model(k2, model, "greedy", x, z, start, T, c, 1, -1)[0], c, end_id)
    # beam, width 5, min_length against the beam's end id
    free = np.concatenate([model.beam_search(x, z, z, start, T, beam_width=5, end_id=e)[0] for e in (-1, end_id)])
    cb = DecodeConstraints(**ckw)
    assert seen(free, cb, end_id) == {"ngram", "min_length", "bad"}
    assert obeys(model.beam_search(x, z, z, start, T, beam_width=5, end_id=end_id, constraints=cb)[0], cb, end_id)
    # sampling: 14 streams x 15 positions = 210 draws per row
    draw = lambda s, cc: (model.sample_predict(x, z, z, start, T, temperature=1.0, top_k=8, sample_step=s,
                                               **({} if cc is None else {"constraints": cc}))[0][:, :, 0])
    free = np.concatenate([draw(s, None) for s in range(3)])
    ckw, end_id = _pick(free, V)
    c = DecodeConstraints(end_id=end_id, **ckw)
    assert seen(free, c, end_id) == {"ngram", "min_length", "bad"}
    for s in range(14):
        assert obeys(draw(s, c), c, end_id), s
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------- evaluate.simple_eval
def test_simple_eval_constrained_draws_follow_the_restatement():
    """evaluate.simple_eval(constraints=...): position t is drawn from its teacher-forced logits, constrained by the draws
    at positions 0 .. t-1, on the stream (seed, S_SAMPLE + t, sample_step).  Restated on the host from the device's own
    logits: constrain_logits_f32 is what the kernel writes bit for bit, so only the sampler's arithmetic differs from the
    float64 draw; a row is compared when every one of its draws keeps tests/test_gpu_sampling.py's relative margin of 1e-5
    (a row that may have taken another token continues from another history).  At least half of the rows are compared."""
    from masters_thesis_amd import think_and_tell as TT
    from masters_thesis_amd.evaluate import simple_eval
    from masters_thesis_amd.model_base import DecodeConstraints, S_SAMPLE
    from oracle.models_tt import CaptionGeneratorTT
    from topkp_oracle import sample_topkp
    rng = np.random.default_rng(116)
    B, N, E, U, V, Tt, end_id = 48, 40, 16, 32, 61, 11, 2
    orc = CaptionGeneratorTT(N, E, U, V, Tt, l2_reg=0.01, dropout=0.0, show_and_tell=False).init_params(rng)
    model = TT.CaptionGenerator(TT.Encoder(E, 0.01, "glorot_uniform", 0.0), TT.Decoder(E, U, V, 0.01, "glorot_uniform", 0.0),
                                None, Tt, seed=11)
    x = rng.standard_normal((B, N)).astype(np.float32)
    tgt = rng.integers(1, V, (B, Tt)).astype(np.int32)
    model._stage(x, tgt)
    for k, v in orc.p.items():
        model.set_weight(k, v * 4 if v.ndim == 2 else v)             # wider logits: the rules have something to decide
    logits = model((x, None, tgt), training=False).cpu().numpy()     # (B, T+1, V)
    assert logits.shape == (B, Tt + 1, V)
    kw = dict(temperature=0.9, top_k=12, top_p=0.95)
    compared = 0
    for c in (DecodeConstraints(1.2, 2, 3, (5, 6, 0), end_id=end_id), DecodeConstraints(2.0, 1, 0, (7,))):
        eid = end_id if c.min_length else -1
        for step in (0, 5):
            ids, _ = simple_eval(model, x, tgt, None, sample_step=step, constraints=c, **kw)
            again, _ = simple_eval(model, x, tgt, None, sample_step=step, constraints=c, **kw)
            assert ids.shape == (B, Tt + 1) and np.array_equal(ids, again)
            for row in ids:
                assert not violations(row, c.no_repeat_ngram_size, c.min_length, eid, c.bad_ids)
            want = np.zeros((B, Tt + 1), np.int64)
            margin = np.full(B, np.inf)
            for t in range(Tt + 1):
                xt = np.stack([constrain_logits_f32(logits[b, t], want[b, :t], c.repetition_penalty, c.no_repeat_ngram_size,
                                                    c.min_length, eid, list(c.bad_ids), t) for b in range(B)])
                want[:, t], mg = sample_topkp(xt, kw["temperature"], kw["top_k"], kw["top_p"], True, model.seed, S_SAMPLE + t, step)
                margin = np.minimum(margin, mg)
            ok = margin > 1e-5
            print(f"simple_eval {c!r} step {step}: {int((~ok).sum())} of {B} rows left out (margin)")
            assert ok.mean() >= 0.5
            assert np.array_equal(ids[ok], want[ok]), (c, step)
            compared += int(ok.sum())
    assert compared
    # None and a neutral object: the one-launch draw, bit for bit
    a, _ = simple_eval(model, x, tgt, None, sample_step=3, **kw)
    for c in (None, DecodeConstraints()):
        assert np.array_equal(simple_eval(model, x, tgt, None, sample_step=3, constraints=c, **kw)[0], a)
    with pytest.raises(ValueError):
        simple_eval(model, x, tgt, None, constraints=DecodeConstraints(bad_ids=(V,)))
