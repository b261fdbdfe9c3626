"""Keeps tests/test_gpu_head.py complete: the dispatch of tnt_softmax_cce_f32 is parsed -- the nv4 bucket ladder of
tnt_row_ladder (tnt_rowhead.h), which seqops.hip and every other softmax head call, and the softmax_cce_reg_kernel<N> /
generic kernel that tnt_softmax_cce_f32 launches for the N it is handed -- and the GPU test's V_LIST must reach every bucket
on both sides of each bound and the generic kernel past the last one; its SMX_LADDER (which kernel, hence which pad
contract, it expects) must equal the source's.  A new bucket or a moved bound fails here until the GPU test covers it.
CPU-only: the files are parsed, not imported."""
import ast
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "masters-thesis_amd", "csrc")
SEQOPS = os.path.join(CSRC, "seqops.hip")
ROWHEAD = os.path.join(CSRC, "tnt_rowhead.h")
GPU_TEST = os.path.join(HERE, "test_gpu_head.py")


def _dispatch():
    src = open(ROWHEAD).read()
    start = src.index("static inline void tnt_row_ladder(")
    body = src[start:src.index("\n}\n", start)]
    per = re.search(r"const int nv4 = \(V \+ (\d+)\) / (\d+);", body)
    assert per and int(per.group(1)) + 1 == int(per.group(2)), "nv4 = ceil(V / W) not found in tnt_row_ladder"
    ladder = [(op, int(b), int(n))
              for op, b, n in re.findall(r"if \(aligned && nv4 (==|<=) (\d+)\) launch\(tnt_nv4<(\d+)>\{\}\);", body)]
    assert ladder, "register-row ladder not found in tnt_row_ladder"
    # every launch is one rung of the ladder, and the re-reading row (N = 0) is the final else
    assert body.count("launch(tnt_nv4<") - 1 == len(ladder), "a launch outside the parsed ladder"
    assert re.search(r"else launch\(tnt_nv4<0>\{\}\);\s*$", body), "the re-reading row is not the final else"
    # tnt_softmax_cce_f32 takes that ladder: register kernel <N> for N > 0, the generic kernel for N = 0, nothing else
    src = open(SEQOPS).read()
    start = src.index('extern "C" int32_t tnt_softmax_cce_f32(')
    body = src[start:src.index("\n}\n", start)]
    assert body.count("tnt_row_ladder(al, V,") == 1 and body.count("hipLaunchKernelGGL(") == 2
    assert re.search(r"if constexpr \(N > 0\)\s+hipLaunchKernelGGL\(\(softmax_cce_reg_kernel<N>\),", body)
    assert re.search(r"else\s+hipLaunchKernelGGL\(softmax_cce_kernel,", body), "generic kernel is not the final else"
    return int(per.group(2)), ladder


def _gpu_test_constants():
    tree = ast.parse(open(GPU_TEST).read(), GPU_TEST)
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            if node.targets[0].id in ("V_LIST", "SMX_LADDER"):
                out[node.targets[0].id] = ast.literal_eval(node.value)
    return out["V_LIST"], [tuple(r) for r in out["SMX_LADDER"]]


def _buckets():
    """[(lo, hi, N)]: V in (lo, hi] runs softmax_cce_reg_kernel<N> (aligned rows, ld % 4 == 0)"""
    W, ladder = _dispatch()
    out, prev = [], 0
    for op, bound, n in ladder:
        assert bound > prev, f"ladder bounds not increasing at nv4 {op} {bound}"
        assert op == "<=" or bound == prev + 1, f"'nv4 == {bound}' leaves nv4 in ({prev}, {bound}) to a later rung"
        # the kernel's window is 4 * 256 * N = W * N columns: it must hold the longest row of its bucket
        assert n >= bound, f"softmax_cce_reg_kernel<{n}> launched for nv4 up to {bound}: columns past {W * n} unread"
        out.append((W * prev, W * bound, n))
        prev = bound
    return out


def test_gpu_head_ladder_matches_source():
    _, ladder = _dispatch()
    _, smx = _gpu_test_constants()
    assert smx == [(b, n) for _, b, n in ladder], f"test_gpu_head.SMX_LADDER {smx} != source {ladder}"


def test_v_list_reaches_every_bucket_and_the_generic_kernel():
    vs, _ = _gpu_test_constants()
    vset = set(vs)
    missing = []
    for lo, hi, n in _buckets():
        for v in (lo + 1, hi):                     # both sides of each bound
            if v not in vset:
                missing.append(f"V={v} (softmax_cce_reg_kernel<{n}>, V in ({lo}, {hi}])")
        if not any(lo < v <= hi for v in vs):
            missing.append(f"softmax_cce_reg_kernel<{n}>")
    last = _buckets()[-1][1]
    if last + 1 not in vset:
        missing.append(f"V={last + 1} (first V of the generic kernel)")
    if not any(v > 2 * last for v in vs):
        missing.append(f"a V well past {last} (generic kernel, several values per thread)")
    assert not missing, f"tests/test_gpu_head.py V_LIST misses: {missing}"
