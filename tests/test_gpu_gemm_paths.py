"""Every kernel of csrc/gemm.hip and csrc/gemm3.hip on a real MI355X against plain float64 numpy, at the tile, k-stage and
K-split edges, on operands that are views into larger buffers.

Which test launches which kernel -- read against gemm_dispatch / launch_1r (csrc/gemm.hip) and tnt_gemm3_f32 (csrc/gemm3.hip):

    kernel                                   test                               arguments that select it
    gemm_kernel<BM,BN,TA,TB,VEC=true>        test_tiled[*-vec], test_tiled_split    tnt_gemm_f32_tile, bm x bn in 64x64 128x128 64x128 128x64,
                                                                                NN / TN / NT; operands 16-byte aligned, ld % 4 == 0
    gemm_kernel<BM,BN,TA,TB,VEC=false>       test_tiled[*-front1 / *-ld1],      the view starts one float into its buffer; ld % 4 == 1
                                             test_tiled_split
    splitk_reduce_kernel                     test_tiled_split                   K 200 splitk 3 and 4 (last chunk 8 long), K 100 splitk 8
                                                                                (runs as 4), K 33 splitk 2; every epilogue
    gemm1r_kernel<.., PD=1>   cfg 1          test_one_round[1-*]                tnt_gemm_fused_f32 cfg = 1: 160x128, 16 waves
                                             test_tiled_one_round_epilogues     tnt_gemm_f32_tile bm x bn = 160x128: pre / act / accumulate
    gemm1r_kernel<.., PD=3>   cfg 9          test_one_round[9-*]                cfg = 9: 1 to 6 k tiles through the 3-deep register ring
    gemm2_kernel              cfg 21 22 24   test_one_round[21-*] .. [28-*]     cfg = 21, 22, 24, 25, 26, 28: 1 to 6 k tiles, the odd
                              25 26 28                                          trailing step at 1, 3 and 5
    (cfg = 0: pick_cfg_1r)                   test_one_round_auto                1000 x 500, NN and TN; NT is refused (TNT_BADARG)
    gemm3_kernel<Cfg,LIVE=false>             test_gemm3[tile-*]                 tiles 1 .. 11, NN / TN / NT, 1 to 4 K stages
                                             test_gemm3_split[tile-*]           splitk 2, 3, 8 (clamped), with A2 / C2, with a bias
                                             test_gemm3_split_without_owner     tile 7, splitk 12: splits 8 to 11 own no row
                                             test_gemm3_embedded                tiles 7 and 9, NN / NT, row stride roundup4(K) + 8, 1e6
                                                                                between the rows, NaN behind the last one
    gemm3_kernel<Cfg,LIVE=true>              test_gemm3_live_rows_with_a_k_tail the same product with a device-side row count
    gemm3_pair_kernel<C1,C2,LIVE>            test_gemm3_embedded_pair           TN + NT in one grid, the NT product's K = BK + 5; every
                                                                                other pair: test_gemm3_pair (tests/test_gpu_ops.py)
    g3_arm_kernel                            test_gemm3_split                   tnt_gemm3_work_arm before every split launch

Protocol (as tests/test_gpu_rowop_paths.py).  Inputs are rounded to float32 before the float64 reference sees them.  Every
operand is a view into a larger buffer (gemm_oracle.embed): floats in front of it, a row stride above its width, floats behind
it, all NaN (0x7FC00000) wherever include/tnt_hip.h does not require data -- everything around an operand of the tiled and
one-round kernels (their loaders mask by element) and around an M/N-contiguous operand of gemm3.  A K-contiguous operand of
gemm3 has what the header asks for: zeros in the pad columns [K, roundup4(K)), finite floats (GAP = 1e6, which no result could
hide) in the rest of the row stride, where a row's last K stage reads on and multiplies by zeros; only behind its last row,
which is not read, stands NaN.  C, pre, C2 and colsum start as NaN inside POISON bands (Guards); their pad columns
must still hold those bits afterwards; every launch runs twice on fresh outputs and must give the same bits.

Two kinds of data per case.  exact: integers in [-3, 3] -- every float32 partial sum is exact in any order, so C, pre, C2 and
colsum must equal the float64 result bit for bit: a dropped or doubled k term of any size cannot hide.  random: standard
normals against gemm_oracle.fp32_dot_bound, (K + 2) 2^-24 (|op(A)| |op(B)| + |bias|) per element -- the bound of a float32
dot product in any order, so it needs no measurement; gemm3 keeps its own tighter bound, 1e-6 max(1, sqrt(K / 256)) of the
largest magnitude.  Activations: none, relu and leaky (float32(x * float32(slope))) are exact given the device's own pre; tanh
is held to float64 tanh of the device's pre within ETOL = 1e-5.  Where a launch returns no pre, exact data gives it anyway
(the float64 pre is the float32 one); random data allows the dot bound (the activations are 1-Lipschitz) plus one rounding of
the result, plus ETOL for tanh.  Every test prints its worst error / bound ratios (Report).

gemm_oracle.py holds the sizes; tests/test_host_gemm_edges.py pins each to the edge it is named for, and every split case to
tiles * S * batch <= 256 workgroups (one round: the splits of a tile wait for each other)."""
import numpy as np
import pytest
import torch

import gemm_oracle as G
from test_gpu_encoder_paths import refuse, twice, untouched
from test_gpu_lstm_paths import Guards, r32      # noqa: F401  (Guards: through twice)
from test_gpu_ops import close, dev              # noqa: F401
from test_gpu_rowop_paths import Report, bits, host

pytestmark = pytest.mark.gpu

NAN = float("nan")
ETOL = 1e-5
SLOPE = 0.2
SENTINEL = 0x7FC5EED5           # what tnt_gemm3_work_arm writes (checked, never used as a fill)
KINDS = ("exact", "random")
GAP = 1e6                       # between the rows of a K-contiguous gemm3 operand: finite by contract, and not small


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def data(rng, kind, *shape):
    return G.ints(rng, *shape) if kind == "exact" else r32(rng.standard_normal(shape))


def put(e):
    """an embedded operand on the device: the view that starts `front` floats into its buffer"""
    d = dev(e.buf)
    return d[len(e.buf) - len(e.view):]


def pads_kept(out, N):
    """the pad columns of a NaN-initialised output kept their bits"""
    if out.shape[-1] > N:
        pad = out[..., N:]
        assert torch.equal(bits(pad.contiguous()), bits(torch.full_like(pad, NAN).contiguous())), "a pad column of an output was written"


def preset(view, N, a):
    """the live columns of a guarded output set to `a` (accumulate): the pad columns stay NaN"""
    view[:, :N] = dev(a)
    return view


def compare(rep, kind, name, got, want, bound=None):
    """exact data: bit for bit; random data: every element within its bound"""
    if kind == "exact":
        rep.exact(name, got, want)
    else:
        got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
        err = np.abs(got.astype(np.float64) - want)
        rep.within(name, float((err / (bound + 1e-300)).max()), 1.0)


def check_activation(rep, kind, name, C, pre_dev, pre_ref, epi_act, cold, bound):
    """C = act(pre) (+ cold) from the device's own pre where the launch returned one, else from the reference"""
    Ch = host(C)
    if pre_dev is not None or kind == "exact":
        p32 = host(pre_dev) if pre_dev is not None else pre_ref.astype(np.float32)
        if epi_act == "tanh":
            want = np.tanh(p32.astype(np.float64)) + (0 if cold is None else cold)
            rep.within(name + "/tanh", float(np.abs(Ch - want).max()), ETOL * (np.abs(want).max() + 1e-30))
        else:
            a32 = G.act(p32, epi_act, SLOPE)
            rep.exact(name, Ch, a32 if cold is None else a32 + cold.astype(np.float32))
    else:
        want = G.act(pre_ref, epi_act, SLOPE) + (0 if cold is None else cold)
        slack = bound + G.U24 * np.abs(want) + (ETOL if epi_act == "tanh" else 0.0)
        rep.within(name, float((np.abs(Ch - want) / (slack + 1e-300)).max()), 1.0)


# ------------------------------------------------------------------------------------------------ (a) the tiled kernel
def epilogue_args(epi):
    """(activation, bias?, pre?, accumulate?) of a named epilogue"""
    if epi in ("none", "leaky", "relu", "tanh"):
        return epi, True, False, False
    return {"pre": ("leaky", True, True, False), "acc": ("none", False, False, True), "pre+acc": ("none", False, True, True)}[epi]


def run_tiled(be, rep, tag, bm, bn, lay, M, N, K, form, epi, splitk=1):
    tA, tB = G.LAYOUTS[lay]
    front, ld_extra = G.TILED_FORMS[form]
    actname, has_bias, has_pre, acc = epilogue_args(epi)
    ldc = N + 3
    for kind in KINDS:
        rng = np.random.default_rng([bm, bn, M, N, K, splitk, len(epi), KINDS.index(kind)])
        opA, opB = data(rng, kind, M, K), data(rng, kind, K, N)
        bias = data(rng, kind, N) if has_bias else None
        cold = data(rng, kind, M, N) if acc else None
        eA, eB = G.embed(opA, tA, ld_extra, front), G.embed(opB, tB, ld_extra, front)
        Ad, Bd, bd = put(eA), put(eB), None if bias is None else dev(bias)
        assert (Ad.data_ptr() % 16 == 0 and eA.ld % 4 == 0) == (form == "vec")

        def launch(gs):
            C = gs.new("C", M, ldc)
            if acc:
                preset(C, N, cold)
            P = gs.new("pre", M, ldc) if has_pre else None
            W = gs.new("work", splitk * M * N) if splitk > 1 else None
            be.gemm_tile(Ad, Bd, C, M, N, K, eA.ld, eB.ld, ldc, bm, bn, transA=tA, transB=tB, bias=bd, pre=P,
                         act=G.ACTS[actname], slope=SLOPE, accumulate=acc, splitk=splitk, work=W)
            return (C, P) if has_pre else (C,)
        out = twice(launch)
        C, P = out[0], (out[1] if has_pre else None)
        pads_kept(C, N)
        pre_ref = G.product(opA, opB, bias)
        bound = G.fp32_dot_bound(opA, opB, (0 if bias is None else np.abs(bias)) + (0 if cold is None else np.abs(cold)))
        name = f"{tag} {M}x{N}x{K} {form} {epi} {kind}"
        if has_pre:
            pads_kept(P, N)
            compare(rep, kind, name + " pre", P[:, :N], pre_ref, bound)
        check_activation(rep, kind, name + " C", C[:, :N], None if P is None else P[:, :N], pre_ref, actname, cold, bound)


@pytest.mark.parametrize("form", G.TILED_FORMS)
@pytest.mark.parametrize("lay", G.LAYOUTS)
@pytest.mark.parametrize("bm,bn", G.TILED, ids=lambda v: str(v))
def test_tiled(be, bm, bn, lay, form):
    """tnt_gemm_f32_tile, one forced tile on one layout in one loader form: M in 1, BM - 1, BM + 1, N in 3, BN + 1, K in 1, 31,
    32, 33, 67, the seven epilogues dealt over the thirty shapes (each meets at least four of them)"""
    rep = Report(f"tiled {bm}x{bn} {lay} {form}")
    for i, (M, N, K) in enumerate(G.tiled_shapes(bm, bn)):
        run_tiled(be, rep, lay, bm, bn, lay, M, N, K, form, G.TILED_EPILOGUES[i % len(G.TILED_EPILOGUES)])
    rep.check()


@pytest.mark.parametrize("lay", G.LAYOUTS)
@pytest.mark.parametrize("bm,bn", G.TILED, ids=lambda v: str(v))
def test_tiled_split(be, bm, bn, lay):
    """tnt_gemm_f32_tile with splitk > 1 (gemm_kernel's partials + splitk_reduce_kernel's epilogue) at (BM + 1) x (BN + 1): a last
    chunk of 8, of 4 (a split of 8 that runs as 4, the work buffer sized for 8 and guarded) and of 1; the full epilogue list on
    the 64x64 tile, one epilogue per layout and split on the others; the loader forms dealt over the cases"""
    rep = Report(f"tiled split {bm}x{bn} {lay}")
    forms = list(G.TILED_FORMS)
    li = list(G.LAYOUTS).index(lay)
    for j, (K, S) in enumerate(G.TILED_SPLITS):
        epis = G.TILED_EPILOGUES if (bm, bn) == (64, 64) else (G.TILED_EPILOGUES[(2 * li + j + 3) % 7],)
        for i, epi in enumerate(epis):
            run_tiled(be, rep, f"{lay} S{S}", bm, bn, lay, bm + 1, bn + 1, K, forms[(i + j + li) % 3], epi, splitk=S)
    rep.check()


@pytest.mark.parametrize("epi", G.TILED_EPILOGUES)
def test_tiled_one_round_epilogues(be, epi):
    """tnt_gemm_f32_tile with bm x bn = 160 x 128: gemm1r_kernel (cfg 1) with the epilogues only this entry point gives it, at
    161 x 129 and K of 1, 2 and 3 k tiles (NN, float4 loads: the only form it takes)"""
    rep = Report(f"one-round epilogue {epi}")
    for K in (31, 33, 67):
        run_tiled(be, rep, "NN", 160, 128, "NN", 161, 129, K, "vec", epi)
    rep.check()


# ------------------------------------------------------------------------------------------------ (b) the one-round family
def run_fused(be, rep, cfg, lay, M, N, K, rider, ld_extra, tag=""):
    tA, tB = G.LAYOUTS[lay]
    has_bias, has_cs, has_a2 = "bias" in rider, "colsum" in rider, "A2" in rider
    ldc = N + 3
    for kind in KINDS:
        rng = np.random.default_rng([cfg, M, N, K, len(rider), KINDS.index(kind)])
        opA, opA2, opB = data(rng, kind, M, K), data(rng, kind, M, K), data(rng, kind, K, N)
        bias = data(rng, kind, N) if has_bias else None
        eA, eA2, eB = G.embed(opA, tA, ld_extra, 8), G.embed(opA2, tA, ld_extra, 8), G.embed(opB, tB, ld_extra, 8)
        Ad, A2d, Bd, bd = put(eA), put(eA2), put(eB), None if bias is None else dev(bias)

        def launch(gs):
            C = gs.new("C", M, ldc)
            C2 = gs.new("C2", M, ldc) if has_a2 else None
            col = gs.new("colsum", ldc) if has_cs else None
            be.gemm_fused(Ad, Bd, C, M, N, K, eA.ld, eB.ld, ldc, transA=tA, transB=tB, bias=bd, colsum=col,
                          A2=A2d if has_a2 else None, C2=C2, cfg=cfg)
            return tuple(t for t in (C, C2, col) if t is not None)
        out = list(twice(launch))
        name = f"{tag}{M}x{N}x{K} {rider} {kind}"
        C = out.pop(0)
        pads_kept(C, N)
        compare(rep, kind, name + " C", C[:, :N], G.product(opA, opB, bias), G.fp32_dot_bound(opA, opB, bias))
        if has_a2:
            C2 = out.pop(0)
            pads_kept(C2, N)
            compare(rep, kind, name + " C2", C2[:, :N], G.product(opA2, opB, bias), G.fp32_dot_bound(opA2, opB, bias))
        if has_cs:
            col = out.pop(0)
            pads_kept(col, N)
            compare(rep, kind, name + " colsum", col[:N], G.colsum(opB), (K + 2) * G.U24 * np.abs(opB).sum(0))


@pytest.mark.parametrize("lay", G.LAYOUTS)
@pytest.mark.parametrize("cfg", G.CFG_1R)
def test_one_round(be, cfg, lay):
    """tnt_gemm_fused_f32, one configuration on one layout: K of 1 to 6 k tiles (5, 32, 33, 64, 96, 97, 130, 161), M = BM + 1 (a
    second row of workgroups, which must leave colsum alone), N in 7, BN + 1; the riders -- bias, colsum (TN), A2 / C2,
    colsum + A2 (TN) or bias + A2 -- dealt so that every rider meets both N and every K meets two riders"""
    _, BM, BN = G.CFG_1R[cfg][:3]
    riders = ("bias", "colsum", "A2", "colsum+A2") if lay == "TN" else ("bias", "none", "A2", "bias+A2")
    rep = Report(f"one-round cfg {cfg} {lay}")
    for ki, K in enumerate(G.FUSED_K):
        for ni, N in enumerate((7, BN + 1)):
            run_fused(be, rep, cfg, lay, BM + 1, N, K, riders[(ki + 2 * ni) % 4], 4 * ((ki >> 1) & 1))
    rep.check()


def test_one_round_auto(be):
    """cfg = 0: the configuration tnt_gemm_fused_cfg names, on one shape per layout it serves; NT, which it does not serve, is
    refused before anything is written"""
    rep = Report("one-round auto")
    for lay, (M, N, K) in G.FUSED_AUTO.items():
        tA, tB = G.LAYOUTS[lay]
        assert be.gemm_fused_cfg(M, N, K, tA, tB) in G.CFG_1R
        run_fused(be, rep, 0, lay, M, N, K, "colsum" if lay == "TN" else "bias", 4, tag=lay + " ")
    rep.check()
    M, N, K = 64, 64, 64
    assert be.gemm_fused_cfg(M, N, K, False, True) == 0
    A, C = torch.zeros(64, 64, device="cuda"), torch.full((64, 64), 7.0, device="cuda")
    refuse(lambda: be.gemm_fused(A, A, C, M, N, K, 64, 64, 64, transB=True))
    untouched(C)


# ------------------------------------------------------------------------------------------------ (c) gemm3
def g3_operands(rng, kind, lay, M, N, K, ld_extra, front=8, two=False):
    """embedded operands of a gemm3 launch.  K-contiguous: zeros in the pad columns, GAP in the rest of the row stride and in
    front, NaN behind the last row; M/N-contiguous: NaN everywhere"""
    tA, tB = G.LAYOUTS[lay]
    ops = [data(rng, kind, M, K), data(rng, kind, K, N)] + ([data(rng, kind, M, K)] if two else [])

    def lay_out(op, trans, kc):
        e = G.embed(op, trans, ld_extra, front, fill=GAP if kc else G.NAN, zero_pad=kc)
        if kc:
            e.buf[-G.TAIL:] = G.NAN
        return e
    es = [lay_out(ops[0], tA, not tA), lay_out(ops[1], tB, tB)] + ([lay_out(ops[2], tA, not tA)] if two else [])
    return ops, es


def run_gemm3(be, rep, tile, lay, M, N, K, rider, ld_extra, S=1, live=None, name=""):
    tA, tB = G.LAYOUTS[lay]
    has_bias, has_cs, has_a2 = "bias" in rider, "colsum" in rider, "A2" in rider
    ldc = G.roundup4(N) + 4
    wf = G.g3_work_floats(tile, M, N, S, 2 if has_a2 else 1)
    if S > 1:
        assert wf == be.gemm3_work_floats(M, N, tile, S, 2 if has_a2 else 1) and wf % 4 == 0
        assert G.g3_units(tile, M, N, S, 2 if has_a2 else 1) <= G.G3_UNITS
    for kind in KINDS:
        rng = np.random.default_rng([tile, M, N, K, S, len(rider), KINDS.index(kind)])
        (opA, opB, *rest), es = g3_operands(rng, kind, lay, M, N, K, ld_extra, two=has_a2)
        bias = data(rng, kind, N) if has_bias else None
        ds = [put(e) for e in es]
        bd = None if bias is None else dev(bias)

        def launch(gs):
            C = gs.new("C", M, ldc)
            C2 = gs.new("C2", M, ldc) if has_a2 else None
            col = gs.new("colsum", ldc) if has_cs else None
            work = sync = None
            if S > 1:
                work, sync = gs.new("work", wf), torch.zeros(1, dtype=torch.int32, device="cuda")
                be.gemm3_work_arm(work)
            be.gemm3(ds[0], ds[1], C, M, N, K, es[0].ld, es[1].ld, ldc, transA=tA, transB=tB, bias=bd, colsum=col,
                     A2=ds[2] if has_a2 else None, C2=C2, tile=tile, splitk=S, work=work, sync=sync,
                     live=live, live_mode=1 if live is not None else 0)
            if S > 1:
                torch.cuda.synchronize()
                assert bool((work.view(torch.int32) == SENTINEL).all()), "the exchange buffer is not re-armed"
                assert int(sync.sum()) == 0, "the error word is set"
            return tuple(t for t in (C, C2, col) if t is not None)
        out = list(twice(launch))
        tag = f"{name}{M}x{N}x{K} {rider} {kind}"
        for o, a in zip(out[:2 if has_a2 else 1], [opA] + rest):
            pads_kept(o, N)
            want = G.product(a, opB, bias)
            compare(rep, kind, tag + " C", o[:, :N], want, G.g3_bound(want, K))
        if has_cs:
            pads_kept(out[-1], N)
            compare(rep, kind, tag + " colsum", out[-1][:N], G.colsum(opB), (K + 2) * G.U24 * np.abs(opB).sum(0))


@pytest.mark.parametrize("lay", G.LAYOUTS)
@pytest.mark.parametrize("tile", G.G3)
def test_gemm3(be, tile, lay):
    """tnt_gemm3_f32 unsplit, one tile on one layout: K of 1, 2, 3 and 4 stages of that tile's BK (fewer stages than the ring is
    deep, tails inside a 4-chunk, a 16-block, a stage), M = BM + 1, N in 3, BN + 5, row strides roundup4(width) and + 4; a bias on
    every layout, colsum on TN"""
    BM, BN, bk = G.g3_tile(tile)
    rep = Report(f"gemm3 tile {tile} {lay}")
    for ki, K in enumerate(G.g3_ks(bk)):
        for ni, N in enumerate((3, BN + 5)):
            rider = ("bias", "colsum" if lay == "TN" else "none")[(ki + ni) % 2]
            run_gemm3(be, rep, tile, lay, BM + 1, N, K, rider, 4 * ((ki + 1) % 2))
    rep.check()


@pytest.mark.parametrize("lay", G.LAYOUTS)
@pytest.mark.parametrize("tile", G.G3)
def test_gemm3_split(be, tile, lay):
    """tnt_gemm3_f32 with the K split reduced inside the launch, every tile on every layout: S = 2 and 3 with a shorter last
    split, S = 8 on two stages (clamped to 2, the work buffer sized for 8), a second product on the second half of the work
    buffer, a bias; after every launch the work buffer is all "not written yet" and the error word 0"""
    BM, BN, _ = G.g3_tile(tile)
    rep = Report(f"gemm3 split tile {tile} {lay}")
    for i, (name, K, S, batch, bias) in enumerate(G.g3_split_cases(tile)):
        rider = "A2" if batch == 2 else ("bias" if bias else "none")
        run_gemm3(be, rep, tile, lay, BM + 1, (BN + 5, 3)[i == 1], K, rider, 4 * (i % 2), S=S, name=name + " ")
    rep.check()


def test_gemm3_split_without_owner(be):
    """tile 7 has 8 accumulator tile rows per workgroup: with S = 12 (K = 1536: 48 stages, 4 each) splits 8 to 11 own none --
    they only send"""
    tile, M, N, K, S = G.G3_OWNERLESS
    rep = Report("gemm3 owner-less splits")
    for lay in G.LAYOUTS:
        run_gemm3(be, rep, tile, lay, M, N, K, "none", 0, S=S, name=lay + " ")
    rep.check()


def embedded_case(tile, lay, kind):
    """tnt_gemm3_f32's operands the way a model hands them over: K = BK + 5 at a row stride of roundup4(K) + 8, GAP between the
    rows, NaN behind the last row"""
    c = G.G3_EMBEDDED
    M, N, K = c["M"], c["N"], G.g3_tile(tile)[2] + 5
    rng = np.random.default_rng([tile, len(lay), KINDS.index(kind), 77])
    (opA, opB), es = g3_operands(rng, kind, lay, M, N, K, c["ld_extra"])
    return M, N, K, opA, opB, es


@pytest.mark.parametrize("lay", ["NN", "NT"])
@pytest.mark.parametrize("tile", G.G3_EMBEDDED["tiles"])
def test_gemm3_embedded(be, tile, lay):
    """A K-contiguous operand embedded in a larger buffer (unsplit NN and NT, tiles 7 and 9, 70 x 40, K = BK + 5, row stride
    roundup4(K) + 8): the second stage of a row runs over the gap into the next row.  The contract of include/tnt_hip.h: those
    floats are finite (GAP = 1e6 here, and the next row's data), the floats behind the last row are not read (NaN here) -- then
    none of it may show in C: exact on integer data.  With NaN in the gap C is NaN throughout (the kernel multiplies the gap by
    zeros; measured, and why the header asks for finite floats: masking them cost 0.45 % of the training step,
    profiles/gemm_paths_bench.txt)."""
    tA, tB = G.LAYOUTS[lay]
    rep = Report(f"gemm3 embedded tile {tile} {lay}")
    for kind in KINDS:
        M, N, K, opA, opB, es = embedded_case(tile, lay, kind)
        ldc = G.roundup4(N) + 4
        Ad, Bd = put(es[0]), put(es[1])

        def launch(gs):
            C = gs.new("C", M, ldc)
            be.gemm3(Ad, Bd, C, M, N, K, es[0].ld, es[1].ld, ldc, transA=tA, transB=tB, tile=tile)
            return (C,)
        C, = twice(launch)
        pads_kept(C, N)
        want = G.product(opA, opB)
        got = host(C)[:, :N]
        assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite elements of C"
        compare(rep, kind, f"{kind} C", got, want, G.g3_bound(want, K))
    rep.check()


@pytest.mark.parametrize("tile", G.G3_EMBEDDED["tiles"])
def test_gemm3_live_rows_with_a_k_tail(be, tile):
    """the embedded NN case with a device-side row count (live_mode 1, 41 of 70 rows): rows [0, 41) exact, the rest not written"""
    M, N, K, opA, opB, es = embedded_case(tile, "NN", "exact")
    ldc, lv = G.roundup4(N) + 4, 41
    Ad, Bd, live = put(es[0]), put(es[1]), torch.tensor([lv], dtype=torch.int32, device="cuda")

    def launch(gs):
        C = gs.new("C", M, ldc)
        be.gemm3(Ad, Bd, C, M, N, K, es[0].ld, es[1].ld, ldc, tile=tile, live=live, live_mode=1)
        return (C,)
    C, = twice(launch)
    pads_kept(C, N)
    rep = Report(f"gemm3 live rows tile {tile}")
    rep.exact("C", C[:lv, :N], G.product(opA, opB)[:lv])
    assert bool(torch.isnan(C[lv:]).all()), "a row past the live extent was written"


def test_gemm3_embedded_pair(be):
    """tnt_gemm3_pair_f32, TN (tile 7) + NT (tile 7) in one grid, the NT product being the embedded case (K = BK + 5, GAP between
    the rows): both outputs exact, and bit-identical to the single launches"""
    M, N, K, opA, opB, es = embedded_case(7, "NT", "exact")
    rng = np.random.default_rng(5)
    M1, N1, K1 = 37, 50, 45
    (pA, pB), ps = g3_operands(rng, "exact", "TN", M1, N1, K1, 4)
    ldc, ldc1 = G.roundup4(N) + 4, G.roundup4(N1) + 4
    Ad, Bd, Pd, Qd = put(es[0]), put(es[1]), put(ps[0]), put(ps[1])
    assert be.gemm3_pair_supported(7, True, False, 7, False, True)

    def single(gs):
        C1, C = gs.new("C1", M1, ldc1), gs.new("C", M, ldc)
        be.gemm3(Pd, Qd, C1, M1, N1, K1, ps[0].ld, ps[1].ld, ldc1, transA=True, tile=7)
        be.gemm3(Ad, Bd, C, M, N, K, es[0].ld, es[1].ld, ldc, transB=True, tile=7)
        return C1, C

    def pair(gs):
        C1, C = gs.new("C1", M1, ldc1), gs.new("C", M, ldc)
        d1 = be.gemm3_desc(Pd, Qd, C1, M1, N1, K1, ps[0].ld, ps[1].ld, ldc1, transA=True, tile=7)
        d2 = be.gemm3_desc(Ad, Bd, C, M, N, K, es[0].ld, es[1].ld, ldc, transB=True, tile=7)
        be.gemm3_pair(d1, d2)
        return C1, C
    s1, s = twice(single)
    p1, p = twice(pair)
    rep = Report("gemm3 embedded pair")
    rep.exact("TN C", p1[:, :N1], G.product(pA, pB))
    rep.exact("NT C", p[:, :N], G.product(opA, opB))
    assert torch.equal(bits(p1.contiguous()), bits(s1.contiguous())) and torch.equal(bits(p.contiguous()), bits(s.contiguous()))
