"""The self-critical step's rewards on the GPU, the kernel: tnt_caption_reward_f32 against the float64 restatement
(tests/reward_oracle.py) over scan, sample and reference counts and caption lengths, both kinds and both baselines, on a
vocabulary of nine ids with end token 2, so that early ends, zeros before the end, captions without a terminator and
repeated n-grams all occur; tables of 0, 1, 2, 37 and a few thousand entries; scans without references, end_id = -1, ids
beyond 16 bits, bit-equal repeats, evaluate.device_scores, and every refusal.

Tolerances.  score: 1e-9 absolute on the 0..10 scale -- float64 on both sides, the difference is the summation order and
a few ulp of exp / sqrt / log over at most a few hundred terms (~1e-13).  counted: exact.  adv: within one float32 ulp
of float32(the restatement's advantage); where the advantage is so small that a float32 ulp is below the float64 noise
of the two scores it is the difference of, within 2e-9 (twice the score bound) of the float64 advantage instead."""
import ctypes as C

import numpy as np
import pytest
import torch

import reward_oracle as RO
from masters_thesis_amd import evaluate

pytestmark = pytest.mark.gpu

END = 2
SHAPES = [(1, 1, 1, 1, 1), (3, 2, 5, 2, 7), (2, 16, 15, 8, 20), (5, 4, 64, 3, 64)]         # (B, K, T, M, Lr)


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def rows(rng, n, L, end_id=END):
    """n rows of L ids over {0, .., 8}: row i % 4 == 0 has no terminator, i % 4 == 1 a zero and behind it an end token
    (where L >= 3), i % 4 == 2 an early end token followed by garbage, the others random ids 0..8; words from a window of
    three, so that n-grams repeat"""
    out = np.empty((n, L), np.int32)
    for i in range(n):
        lo = int(rng.integers(3, 7))
        row = rng.integers(lo, lo + 3, L)
        if i % 4 == 1 and L >= 3:
            z = int(rng.integers(1, L - 1))
            row[z], row[int(rng.integers(z + 1, L))] = 0, 2
        elif i % 4 == 2:
            row[int(rng.integers(0, max(1, L // 2)))] = 2
        elif i % 4 == 3:
            row = rng.integers(0, 9, L)
        out[i] = row
    return out


def make_case(seed, B, K, T, M, Lr, end_id=END):
    rng = np.random.default_rng(seed)
    w = rows(rng, B * K, T, end_id)
    fed = np.concatenate([rng.integers(-5, 99, (B * K, 1)).astype(np.int32), w[:, :T - 1]], 1)     # column 0 is never read
    greedy = np.concatenate([rows(rng, B, T, end_id).T, rng.integers(-2 ** 31, 2 ** 31 - 1, (T, 2)).astype(np.int32)], 1)
    refs = rows(rng, B * M, Lr, end_id).reshape(B, M, Lr)
    n_refs = rng.integers(1, M + 1, B).astype(np.int32)
    n_refs[0] = M
    return dict(fed=np.ascontiguousarray(fed), last=np.ascontiguousarray(w[:, T - 1]), greedy=np.ascontiguousarray(greedy),
                refs=refs, n_refs=n_refs, w=w, B=B, K=K, T=T, M=M, Lr=Lr)


def data_grams(case, end_id=END):
    """every gram key of the case's captions, ascending"""
    seqs = [RO.caption(r, end_id) for r in case["w"]] + [RO.caption(case["greedy"][:, b], end_id) for b in range(case["B"])]
    seqs += [RO.caption(case["refs"][b, j], end_id) for b in range(case["B"]) for j in range(case["n_refs"][b])]
    keys = {RO.gram_key(s[i:i + k]) for s in seqs for k in range(1, 5) for i in range(len(s) - k + 1)}
    return sorted(k for k in keys if k is not None)


def make_table(seed, grams, n):
    """a table of n entries: of the data's grams never the smallest nor the largest (lookups below the first and above the
    last entry), always the second and, from n = 2, the second largest (lookups that hit the first and the last entry);
    filled up with the data's other grams and then with keys the data does not hold"""
    rng = np.random.default_rng(seed)
    ndoc = 50
    keys = set()
    if n >= 1 and len(grams) >= 3:
        keys.add(grams[1])
    if n >= 2 and len(grams) >= 4:
        keys.add(grams[-2])
    inner = [g for g in grams[2:-2]]
    rng.shuffle(inner)
    for g in inner:
        if len(keys) >= n:
            break
        keys.add(g)
    lo, hi = (grams[1], grams[-2]) if len(grams) >= 4 else (1, 2 ** 62)
    while len(keys) < n:
        k = RO.gram_key([int(v) for v in rng.integers(1, 65536, int(rng.integers(1, 5)))])
        if lo < k < hi or len(grams) < 4:
            keys.add(k)
    keys = np.array(sorted(keys), np.uint64)
    idf = np.log(ndoc) - np.log(rng.integers(1, ndoc + 1, len(keys)).astype(np.float64))
    return keys, idf, np.array([np.log(float(ndoc)), 6.0])


def launch(be, case, table, kind, baseline, end_id=END, with_score=True):
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, K, T = case["B"], case["K"], case["T"]
    ins = [up(case[k]) for k in ("fed", "last", "greedy", "refs", "n_refs")]
    keys, idf, params = table
    tk = up(keys.view(np.int64)) if len(keys) else None
    ti = up(idf) if len(keys) else None
    tp = up(params) if params is not None else None
    adv = torch.full((B * K,), -7.0, device=dev)
    score = torch.full((B, K + 1), -7.0, dtype=torch.float64, device=dev) if with_score else None
    counted = torch.full((B * K,), -9, dtype=torch.int32, device=dev)
    be.caption_reward(ins[0], T, ins[1], ins[2] if baseline == 0 else None, case["greedy"].shape[1], ins[3], ins[4], case["M"],
                      case["Lr"], tk, ti, len(keys), tp, B, K, end_id, kind, baseline, adv, score, counted)
    torch.cuda.synchronize()
    for t, k in zip(ins, ("fed", "last", "greedy", "refs", "n_refs")):
        assert np.array_equal(t.cpu().numpy(), case[k]), k                                # the inputs are read only
    return adv.cpu().numpy(), score.cpu().numpy() if with_score else None, counted.cpu().numpy()


def check(got, want, tag):
    adv, score, counted = got
    wadv, wscore, wcnt = want
    assert np.array_equal(counted, wcnt), tag
    err = float(np.abs(score - wscore).max())
    assert err <= 1e-9, (tag, err)
    w32 = wadv.astype(np.float32)
    ok = (np.abs(adv - w32) <= np.spacing(np.abs(w32))) | (np.abs(adv.astype(np.float64) - wadv) <= 2e-9)
    assert ok.all(), (tag, adv, w32)
    return err


def want_of(case, table, kind, baseline, end_id=END):
    return RO.reward(case["fed"], case["last"], case["greedy"], case["refs"], case["n_refs"], table[0], table[1], table[2],
                     end_id, kind, baseline, case["K"])


@pytest.mark.parametrize("B,K,T,M,Lr", SHAPES)
def test_kernel_matches_the_restatement(be, B, K, T, M, Lr):
    case = make_case(100 * B + K, B, K, T, M, Lr)
    caps = [RO.caption(r, END) for r in case["w"]]
    if T >= 5:                                            # what the generator is for, on this very data
        w = case["w"]
        assert any(len(c) < T and w[i][len(c)] == END for i, c in enumerate(caps)), "an early end"
        assert any(len(c) < T and w[i][len(c)] == 0 and END in w[i][len(c):] for i, c in enumerate(caps)), "a zero before the end"
        assert any(len(c) == T for c in caps), "a full-length caption without a terminator"
        assert any(max(RO.tf(c, k).values(), default=0) > 1 for c in caps for k in (1, 2)), "a repeated gram"
    grams = data_grams(case)
    table = make_table(7, grams, 37 if len(grams) > 40 else min(2, max(0, len(grams) - 2)))
    worst = 0.0
    for kind in (0, 1):
        for baseline in ((0, 1) if K >= 2 else (0,)):
            want = want_of(case, table, kind, baseline)
            got = launch(be, case, table, kind, baseline)
            worst = max(worst, check(got, want, (B, K, T, M, Lr, kind, baseline)))
            if baseline == 1:
                assert not got[1][:, K].any()
            assert np.abs(want[1]).max() > 0 or T == 1
    print(f"B={B} K={K} T={T} M={M} Lr={Lr}: worst score error {worst:.3e}")


@pytest.mark.parametrize("n_keys", [0, 1, 2, 37, 3000])
def test_tables(be, n_keys):
    case = make_case(5, 3, 4, 15, 3, 12)
    grams = data_grams(case)
    assert len(grams) > 60
    keys, idf, params = table = make_table(11 + n_keys, grams, n_keys)
    assert len(keys) == n_keys and np.all(keys[1:] > keys[:-1])
    if n_keys >= 1:                                       # the lookups the binary search has to get right
        assert int(keys[0]) == grams[1] and grams[0] < int(keys[0]) and grams[-1] > int(keys[-1])
    if n_keys >= 2:
        assert int(keys[-1]) == grams[-2]
    if n_keys >= 37:
        assert len(set(grams) & set(int(k) for k in keys)) >= 37 and len(set(grams) - set(int(k) for k in keys)) >= 2
    for baseline in (0, 1):
        check(launch(be, case, table, 0, baseline), want_of(case, table, 0, baseline), (n_keys, baseline))
    if n_keys == 0:                                       # every idf is log(ndoc): the scores do not depend on it ...
        a = launch(be, case, table, 0, 0)[1]
        b = launch(be, case, (keys, idf, np.array([np.log(7.0), 6.0])), 0, 0)[1]
        assert np.abs(a - b).max() < 1e-12 and a.max() > 0
    else:                                                 # ... and with a table they do depend on the table
        flat = (keys, np.full(len(keys), params[0]), params)
        assert np.abs(launch(be, case, table, 0, 0)[1] - launch(be, case, flat, 0, 0)[1]).max() > 1e-6


def test_no_references_scores_zero(be):
    case = make_case(21, 4, 3, 9, 2, 9)
    case["n_refs"][:] = [2, 0, 1, 0]
    table = make_table(3, data_grams(case), 20)
    for kind in (0, 1):
        for baseline in (0, 1):
            got = launch(be, case, table, kind, baseline)
            check(got, want_of(case, table, kind, baseline), (kind, baseline))
            assert not got[1][[1, 3]].any() and not got[0].reshape(4, 3)[[1, 3]].any() and got[1][[0, 2]].any()
    # n_refs outside [0, M] is clamped: -3 reads as 0, 9 as M
    clamped = dict(case, n_refs=np.array([9, -3, 1, 0], np.int32))
    a, b = launch(be, clamped, table, 0, 0), launch(be, case, table, 0, 0)
    assert np.array_equal(a[1], b[1])


def test_negative_end_id_only_zero_terminates(be):
    case = make_case(31, 3, 4, 15, 3, 12)
    assert (case["w"] == 2).any() and (case["refs"] == 2).any()
    table = make_table(5, data_grams(case, -1), 37)
    for kind in (0, 1):
        want = want_of(case, table, kind, 0, end_id=-1)
        check(launch(be, case, table, kind, 0, end_id=-1), want, ("end_id=-1", kind))
        other = want_of(case, table, kind, 0, end_id=END)
        assert not np.array_equal(want[2], other[2]) and np.abs(want[1] - other[1]).max() > 1e-3


def test_ids_beyond_16_bits_match_themselves_and_no_table_entry(be):
    # sample 0 of scan 0 is its reference, and both hold 70000 (and -4): every gram matches, none is looked up.  The table
    # holds the keys that 70000 & 0xffff = 4464 would have: a kernel that truncated the id would find them.
    B, K, T, M, Lr = 2, 2, 6, 1, 6
    case = make_case(41, B, K, T, M, Lr)
    row = np.array([70000, 3, -4, 70000, 3, 5], np.int32)
    case["fed"][0, 1:], case["last"][0] = row[:5], row[5]
    case["w"][0] = row
    case["refs"][0, 0] = row
    # scan 1: ids with the top bits of a key set (the keys compare as unsigned)
    hi = np.array([65535, 40000, 65535, 40000, 3, 65535], np.int32)
    case["fed"][2, 1:], case["last"][2] = hi[:5], hi[5]
    case["w"][2] = hi
    case["refs"][1, 0] = hi
    trunc = [RO.gram_key([4464]), RO.gram_key([4464, 3]), RO.gram_key([3, 65532]), RO.gram_key([5])]
    his = [RO.gram_key([int(v) for v in hi[i:i + k]]) for k in (1, 4) for i in range(6 - k + 1)]
    keys = np.array(sorted(set(trunc + his)), np.uint64)
    assert int(keys[-1]) >= 2 ** 63
    rng = np.random.default_rng(0)
    table = (keys, rng.uniform(0.1, 2.0, len(keys)), np.array([np.log(50.0), 6.0]))
    for kind in (0, 1):
        want = want_of(case, table, kind, 0)
        got = launch(be, case, table, kind, 0)
        check(got, want, ("wide ids", kind))
        assert abs(got[1][0, 0] - (10.0 if kind == 0 else 1.0)) < 1e-9 and abs(got[1][1, 0] - (10.0 if kind == 0 else 1.0)) < 1e-9
    # the looked-up idf matters for scan 1 (its grams are in the table), not for scan 0's wide grams
    flat = (keys, np.full(len(keys), np.log(50.0)), table[2])
    case["refs"][1, 0, 5] = 3
    case["refs"][0, 0, 5] = 3
    a, b = launch(be, case, table, 0, 0)[1], launch(be, case, flat, 0, 0)[1]
    assert abs(a[1, 0] - b[1, 0]) > 1e-6


def test_two_launches_give_the_same_bits_and_score_is_optional(be):
    case = make_case(51, 5, 4, 64, 3, 64)
    table = make_table(9, data_grams(case), 37)
    for kind in (0, 1):
        for baseline in (0, 1):
            a, b = launch(be, case, table, kind, baseline), launch(be, case, table, kind, baseline)
            c = launch(be, case, table, kind, baseline, with_score=False)
            assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[0].view(np.int32), c[0].view(np.int32)) and np.array_equal(a[2], c[2])


def test_device_scores_is_the_host_scorers(be):
    rng = np.random.default_rng(61)
    corpus = [[[int(w) for w in rng.integers(3, 12, rng.integers(1, 9))] for _ in range(rng.integers(1, 4))] for _ in range(60)]
    tab = evaluate.RewardTable(corpus)
    docs = corpus[:7] + [[]]
    cands = [[[int(w) for w in rng.integers(3, 12, rng.integers(0, 10))] for _ in range(rng.integers(1, 5))] for _ in docs]
    got = evaluate.device_scores(cands, docs, "cider-d", table=tab)
    want = evaluate.CiderD(corpus).batch_scores(cands, docs)
    assert all(len(g) == len(w) and np.abs(g - w).max() <= 1e-9 for g, w in zip(got, want)) and max(w.max() for w in want) > 1
    got = evaluate.device_scores(cands, docs, "bleu4")
    want = [[evaluate.sentence_bleu(d, c, weights=(0.25,) * 4) if d else 0.0 for c in cs] for cs, d in zip(cands, docs)]
    assert all(np.abs(g - np.array(w)).max() <= 1e-9 for g, w in zip(got, want))
    # cut at end_id; refusals before any launch
    assert evaluate.device_scores([[[3, 4, 5, 2, 9]]], [[[3, 4, 5]]], "bleu4", end_id=2)[0][0] == \
        evaluate.device_scores([[[3, 4, 5]]], [[[3, 4, 5]]], "bleu4")[0][0] > 0.5
    for bad in (lambda: evaluate.device_scores(cands, docs, "cider-d"), lambda: evaluate.device_scores(cands, docs, "meteor"),
                lambda: evaluate.device_scores([[[3]] * 17], [[[3]]], "bleu4"), lambda: evaluate.device_scores([[[3] * 65]], [[[3]]], "bleu4"),
                lambda: evaluate.device_scores([[[3]]], [[[3]] * 9], "bleu4"), lambda: evaluate.device_scores([[[3]]], [[[3] * 65]], "bleu4"),
                lambda: evaluate.device_scores(cands, docs[:-1], "bleu4")):
        with pytest.raises(ValueError):
            bad()


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    B, K, T, M, Lr, ldg, nk = 3, 2, 6, 2, 5, 4, 8
    R = B * K
    i32 = dict(dtype=torch.int32, device="cuda")
    case = make_case(71, B, K, T, M, Lr)
    n_fed = R * T
    buf = torch.zeros(n_fed + 1024, **i32)                        # fed, and behind it room an output may use
    buf[:n_fed] = torch.from_numpy(case["fed"].reshape(-1)).to("cuda")
    fed, tail = buf[:n_fed], buf[n_fed:]
    last = torch.from_numpy(case["last"]).to("cuda")
    greedy = torch.zeros(T, ldg, **i32)
    refs = torch.from_numpy(case["refs"]).to("cuda")
    n_refs = torch.from_numpy(case["n_refs"]).to("cuda")
    keys = torch.arange(3, 3 + nk, dtype=torch.int64, device="cuda")
    idf = torch.ones(nk, dtype=torch.float64, device="cuda")
    params = torch.tensor([np.log(50.0), 6.0], dtype=torch.float64, device="cuda")
    adv = torch.full((R,), -7.0, device="cuda")
    score = torch.full((B, K + 1), -7.0, dtype=torch.float64, device="cuda")
    counted = torch.full((R,), -9, **i32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(fed=fed, T=T, last=last, greedy=greedy, ldg=ldg, refs=refs, n_refs=n_refs, M=M, Lr=Lr, keys=keys, idf=idf, n_keys=nk,
             params=params, B=B, K=K, end_id=END, kind=0, baseline=0, adv=adv, score=score, counted=counted):
        return lib.tnt_caption_reward_f32(p(fed), T, p(last), p(greedy), ldg, p(refs), p(n_refs), M, Lr, p(keys), p(idf), n_keys,
                                          p(params), B, K, end_id, kind, baseline, p(adv), p(score), p(counted), None)
    f32 = lambda t: t.view(torch.float32)
    bads = [dict(fed=None), dict(T=0), dict(T=65), dict(T=-1), dict(last=None), dict(greedy=None), dict(ldg=2), dict(refs=None),
            dict(n_refs=None), dict(M=0), dict(M=9), dict(M=-1), dict(Lr=0), dict(Lr=65), dict(Lr=-1), dict(keys=None), dict(idf=None),
            dict(n_keys=-1), dict(params=None), dict(B=0), dict(B=-1), dict(K=0), dict(K=17), dict(K=-1), dict(kind=2), dict(kind=-1),
            dict(baseline=2), dict(baseline=-1), dict(K=1, baseline=1), dict(adv=None), dict(counted=None),
            # outputs that overlap an input, or each other, anywhere in their extents
            dict(adv=f32(buf)), dict(adv=f32(buf[n_fed - 1:])), dict(counted=buf[7:]), dict(score=buf[n_fed - 2:].view(torch.float64)),
            dict(counted=last), dict(adv=f32(refs.view(-1)[B * M * Lr - 1:])), dict(counted=n_refs), dict(adv=f32(greedy.view(-1)[5:])),
            dict(score=idf), dict(score=keys.view(torch.float64)[nk - 1:]), dict(score=params), dict(counted=adv.view(torch.int32)),
            dict(score=tail[:R].view(torch.float64), adv=f32(tail[2:]))]
    before = buf.clone()
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw.keys(), rc)               # TNT_BADARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((adv == -7.0).all()) and bool((score == -7.0).all()) and bool((counted == -9).all())
    # the smallest and the largest accepted values; what is nullable; outputs right behind the last element read
    assert call() == 0 and call(score=None) == 0 and call(baseline=1, greedy=None, ldg=0) == 0
    assert call(kind=1, keys=None, idf=None, params=None, n_keys=0) == 0 and call(keys=None, idf=None, n_keys=0) == 0
    assert call(adv=f32(tail), counted=tail[512:]) == 0 and call(end_id=-1) == 0
    torch.cuda.synchronize()
    assert bool((counted >= 1).all()) and bool((counted <= T).all()) and bool((score >= 0).all()) and bool((adv != -7.0).all())
