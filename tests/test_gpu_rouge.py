"""ROUGE-L on the GPU, the kernel: tnt_caption_rouge_f32 against the float64 restatement (tests/rouge_oracle.py) on the
inputs of tests/rouge_cases.py -- B in {1, 3, 5}, T and Lr in {1, 2, 15, 63, 64}, K in {1, 2, 16}, M in {1, 8}, vocabularies of
2, 3 and 50 words, and a case whose lengths and values are set by hand: lengths 0, 1 and the full 64 (a candidate equal to
its 64-word reference, and its reverse), a terminator at position 0, n_refs of 0 and above M, ldg > B, ids at INT32_MIN,
INT32_MAX and above 65535 -- with both baselines, end_id < 0, lcs and score null, bit-equal repeats,
evaluate.device_scores(kind="rouge-l"), and every refusal.  tests/test_host_rouge.py checks that these inputs tell the
definition from the longest common substring, the maximum of per-reference F-scores and beta = 1.

Tolerances.  lcs and counted: exact.  score: 1e-12 absolute -- float64 on both sides in the same operation order, six
roundings on values of at most 2.44, so three orders of magnitude of room.  adv: within one float32 ulp of float32(the
restatement's advantage); where the advantage is so small that a float32 ulp is below the float64 noise of the two scores
it is the difference of, within 2e-12 (twice the score bound) of the float64 advantage instead."""
import ctypes as C

import numpy as np
import pytest
import torch

import rouge_cases as RC
import rouge_oracle as RG
from masters_thesis_amd import evaluate

pytestmark = pytest.mark.gpu

END = RC.END
INPUTS = ("fed", "last", "greedy", "refs", "n_refs")


@pytest.fixture
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def launch(be, case, baseline, end_id=END, beta=RG.BETA, with_score=True, with_lcs=True):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    B, K, T, M = case["B"], case["K"], case["T"], case["M"]
    ins = [up(case[k]) for k in INPUTS]
    adv = torch.full((B * K,), -7.0, device="cuda")
    score = torch.full((B, K + 1), -7.0, dtype=torch.float64, device="cuda") if with_score else None
    counted = torch.full((B * K,), -9, dtype=torch.int32, device="cuda")
    lcs = torch.full((B, K + 1, M), -9, dtype=torch.int32, device="cuda") if with_lcs else None
    be.caption_rouge(ins[0], T, ins[1], ins[2] if baseline == 0 else None, case["greedy"].shape[1], ins[3], ins[4], M, case["Lr"],
                     B, K, end_id, beta, baseline, adv, score, counted, lcs)
    torch.cuda.synchronize()
    for t, k in zip(ins, INPUTS):
        assert np.array_equal(t.cpu().numpy(), case[k]), k                                # the inputs are read only
    return (adv.cpu().numpy(), score.cpu().numpy() if with_score else None, counted.cpu().numpy(),
            lcs.cpu().numpy() if with_lcs else None)


def check(got, want, tag):
    adv, score, counted, lcs = got
    wadv, wscore, wcnt, wlcs = want
    assert np.array_equal(counted, wcnt), tag
    assert np.array_equal(lcs, wlcs), tag
    err = float(np.abs(score - wscore).max())
    print(f"{tag}: worst score error {err:.3e}")
    assert err <= 1e-12, (tag, err)
    w32 = wadv.astype(np.float32)
    ok = (np.abs(adv - w32) <= np.spacing(np.abs(w32))) | (np.abs(adv.astype(np.float64) - wadv) <= 2e-12)
    assert ok.all(), (tag, adv, w32)


@pytest.mark.parametrize("name", RC.NAMES)
def test_kernel_matches_the_restatement(be, name):
    case = RC.case(name)
    for baseline in RC.baselines(name):
        want = RC.want(name, baseline)
        got = launch(be, case, baseline)
        check(got, want, (name, baseline))
        if baseline == 1:
            assert not got[1][:, case["K"]].any() and not got[3][:, case["K"]].any()
        assert want[1].max() > 0 and want[3].max() > 0


def test_forced_lengths_and_values(be):
    """what tests/test_host_rouge.py pins in the restatement, in the kernel's own output"""
    adv, score, counted, lcs = launch(be, RC.case("forced"), 0)
    assert lcs[0, 0, 0] == 64 and score[0, 0] == 1.0 and lcs[0, 1, 1] == 64 and 1 <= lcs[0, 1, 0] < 64     # the all-ones mask
    assert score[0, 2] == 0.0 and not lcs[0, 2].any()                                                    # a terminator at position 0
    assert lcs[1].tolist() == [[0, 1], [0, 0], [0, 1]] and counted[2:4].tolist() == [2, 1]
    assert lcs[2, 0, 0] == 8 and lcs[2, 2, 0] == 1 and lcs[2, 2, 1] == 2                                 # full int32 words compared
    assert not score[3].any() and not lcs[3].any() and score[4].any()                                    # n_refs 0, and 11 as 2


@pytest.mark.parametrize("name", ["2", "forced"])
def test_negative_end_id_only_zero_terminates(be, name):
    case = RC.case(name)
    assert (case["w"] == END).any() and (case["refs"] == END).any()
    want = RC.want(name, 0, end_id=-1)
    check(launch(be, case, 0, end_id=-1), want, (name, "end_id=-1"))
    other = RC.want(name, 0)
    assert not np.array_equal(want[2], other[2]) and not np.array_equal(want[3], other[3])


def test_beta(be):
    case = RC.case("2")
    for beta in (1.0, 0.5, 8.0):
        check(launch(be, case, 0, beta=beta), RC.want("2", 0, beta=beta), ("beta", beta))


@pytest.mark.parametrize("name", ["2", "forced"])
def test_two_launches_give_the_same_bits_and_score_and_lcs_are_optional(be, name):
    case = RC.case(name)
    for baseline in (0, 1):
        a, b = launch(be, case, baseline), launch(be, case, baseline)
        c = launch(be, case, baseline, with_score=False, with_lcs=False)
        d = launch(be, case, baseline, with_score=False)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert c[1] is None and c[3] is None and np.array_equal(a[0].view(np.int32), c[0].view(np.int32)) and np.array_equal(a[2], c[2])
        assert np.array_equal(a[0].view(np.int32), d[0].view(np.int32)) and np.array_equal(a[3], d[3])


def test_device_scores_is_evaluate_rouge_l(be):
    rng = np.random.default_rng(61)
    docs = [[[int(w) for w in rng.integers(3, 9, rng.integers(0, 12))] for _ in range(rng.integers(1, 5))] for _ in range(9)] + [[]]
    cands = [[[int(w) for w in rng.integers(3, 9, rng.integers(0, 12))] for _ in range(rng.integers(1, 5))] for _ in docs]
    for beta in (1.2, 2.0):
        got = evaluate.device_scores(cands, docs, "rouge-l", beta=beta)
        want = [[evaluate.rouge_l(d, c, beta=beta) for c in cs] for cs, d in zip(cands, docs)]
        assert all(len(g) == len(w) and np.abs(g - np.array(w)).max() <= 1e-12 for g, w in zip(got, want))
        assert max(max(w) for w in want) > 0.5
    # cut at end_id; the hand value; refusals before any launch
    assert evaluate.device_scores([[[3, 4, 5, 2, 9]]], [[[3, 4, 5]]], "rouge-l", end_id=2)[0][0] == 1.0
    assert abs(evaluate.device_scores([[[1, 2, 3, 4]]], [[[1, 3, 4, 5, 6]]], "rouge-l")[0][0] - 1.098 / 1.68) <= 1e-15
    for bad in (lambda: evaluate.device_scores(cands, docs, "meteor"), lambda: evaluate.device_scores([[[3]] * 17], [[[3]]], "rouge-l"),
                lambda: evaluate.device_scores([[[3] * 65]], [[[3]]], "rouge-l"), lambda: evaluate.device_scores([[[3]]], [[[3]] * 9], "rouge-l"),
                lambda: evaluate.device_scores(cands, docs[:-1], "rouge-l")):
        with pytest.raises(ValueError):
            bad()


def test_bad_arguments_return_badarg_and_launch_nothing():
    from masters_thesis_amd import _lib
    lib = _lib.load()
    assert lib.tnt_version() >= 137
    B, K, T, M, Lr, ldg = 3, 2, 6, 2, 5, 4
    R = B * K
    i32 = dict(dtype=torch.int32, device="cuda")
    case = RC.make_case(71, B, K, T, M, Lr, 3)
    n_fed = R * T
    buf = torch.zeros(n_fed + 1024, **i32)                        # fed, and behind it room an output may use
    buf[:n_fed] = torch.from_numpy(case["fed"].reshape(-1)).to("cuda")
    fed, tail = buf[:n_fed], buf[n_fed:]
    last = torch.from_numpy(case["last"]).to("cuda")
    greedy = torch.zeros(T, ldg, **i32)
    refs = torch.from_numpy(case["refs"]).to("cuda")
    n_refs = torch.from_numpy(case["n_refs"]).to("cuda")
    adv = torch.full((R,), -7.0, device="cuda")
    score = torch.full((B, K + 1), -7.0, dtype=torch.float64, device="cuda")
    counted = torch.full((R,), -9, **i32)
    lcs = torch.full((B, K + 1, M), -9, **i32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    NULL = object()

    def call(fed=fed, T=T, last=last, greedy=greedy, ldg=ldg, refs=refs, n_refs=n_refs, M=M, Lr=Lr, B=B, K=K, end_id=END, beta=1.2,
             baseline=0, adv=adv, score=score, counted=counted, lcs=lcs):
        bt = C.c_double(0.0 if beta is NULL else beta)             # a host pointer, read during the call
        return lib.tnt_caption_rouge_f32(p(fed), T, p(last), p(greedy), ldg, p(refs), p(n_refs), M, Lr, B, K, end_id,
                                         None if beta is NULL else C.addressof(bt), baseline, p(adv), p(score), p(counted), p(lcs), None)
    f32 = lambda t: t.view(torch.float32)
    bads = [dict(fed=None), dict(T=0), dict(T=65), dict(T=-1), dict(last=None), dict(greedy=None), dict(ldg=2), dict(refs=None),
            dict(n_refs=None), dict(M=0), dict(M=9), dict(M=-1), dict(Lr=0), dict(Lr=65), dict(Lr=-1), dict(B=0), dict(B=-1),
            dict(K=0), dict(K=17), dict(K=-1), dict(baseline=2), dict(baseline=-1), dict(K=1, baseline=1), dict(adv=None),
            dict(counted=None), dict(beta=NULL), dict(beta=0.0), dict(beta=-1.2), dict(beta=float("inf")), dict(beta=float("nan")),
            dict(beta=1e200),
            # outputs that overlap an input, or each other, anywhere in their extents
            dict(adv=f32(buf)), dict(adv=f32(buf[n_fed - 1:])), dict(counted=buf[7:]), dict(score=buf[n_fed - 2:].view(torch.float64)),
            dict(lcs=buf[n_fed - 1:]), dict(counted=last), dict(adv=f32(refs.view(-1)[B * M * Lr - 1:])), dict(counted=n_refs),
            dict(lcs=n_refs), dict(adv=f32(greedy.view(-1)[5:])), dict(counted=adv.view(torch.int32)), dict(lcs=counted),
            dict(lcs=score.view(torch.int32).view(-1)[2 * B * (K + 1) - 1:]), dict(score=tail[:R].view(torch.float64), adv=f32(tail[2:])),
            dict(lcs=tail[:8], counted=tail[B * (K + 1) * M - 1:])]
    before = buf.clone()
    for kw in bads:
        rc = call(**kw)
        assert -1100 < rc <= -1000, (kw.keys(), rc)               # TNT_BADARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((adv == -7.0).all()) and bool((score == -7.0).all()) and bool((counted == -9).all())
    assert bool((lcs == -9).all())
    # the smallest and the largest accepted values; what is nullable; outputs right behind the last element read
    assert call() == 0 and call(score=None) == 0 and call(lcs=None) == 0 and call(baseline=1, greedy=None, ldg=0) == 0
    assert call(adv=f32(tail), counted=tail[512:], lcs=tail[600:]) == 0 and call(end_id=-1) == 0 and call(beta=1e-3) == 0
    torch.cuda.synchronize()
    assert bool((counted >= 1).all()) and bool((counted <= T).all()) and bool((score >= 0).all()) and bool((adv != -7.0).all())
    assert bool((lcs >= 0).all()) and bool((lcs <= min(T, Lr)).all())
