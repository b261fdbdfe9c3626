"""Every kernel of csrc/encoder.hip on a real MI355X against plain float64 numpy, at ragged sizes and on every launch path.

Which test launches which kernel -- read against the dispatch in tnt_dense_fwd_stream_*_f32, tnt_dense_dw_*_f32,
tnt_dense_gram_norm_f32, tnt_locally_dense_*_f32 and tnt_block_dense_dx_f32:

    kernel                                   test                            arguments that select it
    dense_fwd_stream_kernel<4,4,false>       test_fwd_stream                 gx_part null; (K, nsplit) below, B in 1 17 64 65 130, E in 32 96
    dense_fwd_stream_kernel<4,4,true>        test_fwd_stream_gram            gx_part given: GRAM_CASES
    dense_dw_skinny_kernel<1,false>          test_dw_skinny[1-*]             E <= 128: (4149, 128, 64) (8200, 48, 1) (1, 16, 1)
    dense_dw_skinny_kernel<2,true>           test_dw_skinny[2v-*]            128 < E <= 256, E % 256 == 0, dw aligned: (4149, 256, 63)
    dense_dw_skinny_kernel<2,false>          test_dw_skinny[2-*]             128 < E < 256: (4149, 144, 37) (4149, 240, 17); dw misaligned: (4149, 256, 63)
    dense_dw_skinny_kernel<4,true>           test_dw_skinny[4v-*]            E > 256, E % 512 == 0, dw aligned: (4149, 1024, 3); and the
                                             test_dw_sqnorm_slots / test_dw_adam     float32 product the fused epilogues are checked with
    dense_dw_skinny_kernel<4,false>          test_dw_skinny[4-*]             E > 256, E % 512 != 0: (4149, 304, 33) (4149, 768, 4) (15, 304, 64);
                                                                             dw misaligned: (1000, 512, 64)
    dense_dw_skinny_kernel<4,true,1>         test_dw_sqnorm_slots            tnt_dense_dw_sqnorm_f32: FUSED_CASES
    dense_dw_skinny_kernel<4,true,2>         test_dw_adam                    tnt_dense_dw_adam_f32 (mode sq) and tnt_dense_dw_adam_fin_f32 (modes clip,
                                                                             override, noclip): FUSED_CASES.  (<4,true,2,true>, the non-temporal
                                                                             moments, is chosen per process: model-level child test in test_gpu_nic.py)
    dense_gram_norm_kernel                   test_gram_norm_slots            GN_CASES, synthetic gx_part / w2_part
    locally_dense_fwd_kernel                 test_locally_dense              plain (vreg null), split batch-major, split voxel-major; D in 16 48 64
    locally_dense_combine_kernel             test_locally_dense              the split forward's second launch
    locally_dense_bwd_kernel                 test_locally_dense              plain, split batch-major, split voxel-major
    block_dense_dx_kernel                    test_block_dense_dx             (B, R, Din, Dout) in DX_CASES

Forward ring (DEPTH = 4, NW = 4): tile i of the K / 16 full tiles belongs to wave slot i % (4 nsplit), slot q = 4 split + wave; a
slot enters the main loop with 4 or more tiles and drains (tiles % 4) behind it; a K % 16 remainder is one masked tile on slot
(K / 16) % (4 nsplit).  Tiles per slot (FWD_TILES, asserted against the kernel's formula in test_fwd_stream):

    (K, nsplit)   tiles per slot                      reaches
    (256, 1)      4 4 4 4                             main loop, empty drain
    (272, 1)      5 4 4 4                             drain 1
    (352, 1)      6 6 5 5                             drain 2 and 1
    (444, 1)      7 7 7 6                             drain 3 and 2; the masked tile on slot 3, behind a main loop and a drain of 2
    (880, 3)      5 on slots 0..6, 4 on 7..11         nsplit % 8 != 0: workgroup -> (column group, split) without the XCD mapping
    (2136, 8)     5 on slots 0..4, 4 on 5..31         XCD mapping with one split per XCD; the masked tile on slot 5 behind a main loop
    (36, 16)      1 1 0 0 ... (64 slots)              fewer tiles than slots; the masked tile on slot 2, which has no full tile
    (8, 1)        0 0 0 0                             no full tile at all (K < 16): the prologue's loads are clamped to the K columns
The Gram form runs (256, 1): 4 4 4 4, (352, 1): 6 6 5 5, (880, 3) and (2128, 8): 5 / 4 as above, (64, 16): 1 1 1 1 0 ... with two
splits per XCD; gram() trails mac() by one region, so gx_part and w2_part are checked split by split as well as summed.  The STAGE
rider (<4,4,true,true>, tnt_dense_fwd_stream_gram_stage_f32) has its own file, test_gpu_stage_forward.py.

Skinny dW: a workgroup (blockIdx.x) runs the strips s = blockIdx.x, += gridDim.x of 16 voxel rows, gridDim.x = min(strips, 256);
N = 4149 is 260 strips (workgroups 0..3 run two, the last strip holds 5 rows), N = 8200 is 513 (workgroup 0 runs three, the last
strip holds 8 rows).  E = 144 / 304 leave a wave with 1 of 2 / 3 of 4 tiles, E = 768 and 1024 have a second column group
(blockIdx.y = 1), whose upper four waves own nothing at E = 768, E = 48 leaves five of the eight waves idle.

Pad columns (ldx > K, ldw > E, ldx > N) hold PAD = 1e6, not zero: a kernel that reads them fails its comparison.  Outputs are NaN
inside POISON bands (Guards of test_gpu_lstm_paths.py); every launch runs twice on fresh buffers and must give the same bits.
Inputs are rounded to float32 before the float64 reference sees them.

Tolerances are the existing ones: forward 2e-5 (`close`: of the reference's largest magnitude), gx / w2 1e-5, dW RTOL = 1e-4 and
2e-6 against be.gemm, fused update as test_gpu_optim_tail.test_dense_dw_adam_fin (moments 1e-5, theta 1e-6, g taken from the kernel's
own float32 product), split against plain 1e-5.  For the record, the same operation in float32 numpy against float64 on the CPU at
the largest sizes used here: x @ w at K = 2136 5.7e-7 (6.5e-7 at K = 2128, E = 512), x x^T at K = 2128 4.4e-7, sum w^2 5e-9,
x^T dpre at Bk = 64 2.8e-7 -- factors of 35, 23 and 360 inside the bounds.  Two bounds are per slot and derived here:
  * dense_dw_sqnorm, slot by slot: 1e-5 of the slot's value.  All terms are squares; a lane adds at most 3 strips x 16 of them, then 6
    shuffle steps and 8 wave sums follow: under 65 roundings of 2^-24 each = 3.9e-6, plus 3 per term.
  * dense_gram_norm, slot by slot: 1e-6 of the sum of the absolute values of the slot's terms (the kernel accumulates in double and
    rounds once to float: 6e-8 of the value, which may cancel against its terms).  The sum over slots keeps the 2e-5 bound."""
import functools

import numpy as np
import pytest
import torch

from oracle import ops as O
from test_gpu_lstm_paths import Guards, r32
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

PAD = 1e6                       # pad columns of the inputs: finite (the kernels mask by multiplying with 0), never zero
F32 = lambda x: float(np.float32(x))
B1, B2, EPS = F32(0.9), F32(0.98), 1e-8


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def padded(a, ld):
    """the rows of `a` at row stride ld, the pad columns filled with PAD"""
    out = np.full(a.shape[:-1] + (ld,), PAD)
    out[..., :a.shape[-1]] = a
    return out


def bits(t):
    return t.view(torch.int32)


def twice(launch):
    """launch(gs) -> tuple of guarded outputs, run twice on fresh Guards: bands intact, both runs bit-equal; returns the first"""
    runs = []
    for _ in range(2):
        gs = Guards()
        out = launch(gs)
        torch.cuda.synchronize()
        gs.check()
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(bits(a), bits(b)), f"output {k}: a second launch gave other bits"
    return runs[0]


def refuse(call):
    from masters_thesis_amd._lib import KernelLibraryError
    with pytest.raises(KernelLibraryError):
        call()


def untouched(*tensors):
    torch.cuda.synchronize()
    assert all(float(t.min()) == 7.0 == float(t.max()) for t in tensors), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ (a) streaming forward
FWD_TILES = {(256, 1): [4, 4, 4, 4], (272, 1): [5, 4, 4, 4], (352, 1): [6, 6, 5, 5], (444, 1): [7, 7, 7, 6],
             (880, 3): [5] * 7 + [4] * 5, (2136, 8): [5] * 5 + [4] * 27, (36, 16): [1, 1] + [0] * 62, (8, 1): [0, 0, 0, 0]}
FWD_B = (1, 17, 64, 65, 130)            # 65 and 130 leave a last row block of 1 and 2 rows
FWD_CASES = [pytest.param(K, ns, B, (32, 96)[(i + j) % 2], id=f"K{K}-s{ns}-B{B}-E{(32, 96)[(i + j) % 2]}")
             for i, (K, ns) in enumerate(FWD_TILES) for j, B in enumerate(FWD_B)]


def slot_tiles(K, ns):
    """full tiles of every wave slot: `nt` of dense_fwd_stream_kernel"""
    T, n = K // 16, 4 * ns
    return [(T - q + n - 1) // n if q < T else 0 for q in range(n)]


def split_columns(K, ns):
    """the k indices that split s multiplies: its wave slots' full tiles, and the masked tile on slot (K / 16) % (4 ns)"""
    T, n = K // 16, 4 * ns
    cols = [[] for _ in range(ns)]
    for i in range(T):
        cols[(i % n) // 4] += range(16 * i, 16 * i + 16)
    if K % 16:
        cols[(T % n) // 4] += range(16 * T, K)
    assert sorted(k for c in cols for k in c) == list(range(K))
    return [np.asarray(c, np.int64) for c in cols]


@functools.lru_cache(maxsize=None)
def fwd_case(B, K, E):
    """inputs (float32-rounded) of one forward case, never modified"""
    rng = np.random.default_rng([B, K, E])
    return r32(rng.standard_normal((B, K))), r32(rng.standard_normal((K, E)) / np.sqrt(K))


def check_parts(part, x, w, K, ns):
    """the K-split partials summed against x @ w, and every split against the product over its own tiles"""
    close(part.sum(0), x @ w, rtol=2e-5)
    for s, c in enumerate(split_columns(K, ns)):
        close(part[s], x[:, c] @ w[c], rtol=2e-5)


@pytest.mark.parametrize("K,ns,B,E", FWD_CASES)
def test_fwd_stream(be, K, ns, B, E):
    """tnt_dense_fwd_stream_f32: every ring path of FWD_TILES at every B of FWD_B, both E, ldx = K + 4, ldw = E + 6 with the pad
    columns of x and w holding PAD; a split without a tile is exactly 0"""
    assert slot_tiles(K, ns) == FWD_TILES[(K, ns)]
    x, w = fwd_case(B, K, E)
    ldx, ldw = K + 4, E + 6
    xd, wd = dev(padded(x, ldx)), dev(padded(w, ldw))

    def launch(gs):
        part = gs.new("part", ns, B, E)
        be.dense_fwd_stream(xd, wd, part, B, E, K, ldx, ldw, ns)
        return (part,)
    part, = twice(launch)
    check_parts(part, x, w, K, ns)


def test_fwd_stream_refuses_bad_arguments(be):
    """K % 4 != 0, ldx % 4 != 0, E % 32 != 0, odd ldw, nsplit 0 and 65, x off 16-byte alignment: an error code, nothing written"""
    B, K, E = 5, 32, 64
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    x, w, part = f(B * 40 + 4), f(40 * 100), f(65 * B * 96)
    for K_, E_, ldx, ldw, ns, x_ in ((30, E, 32, E, 1, x), (K, E, 34, E, 1, x), (K, 48, K, 48, 1, x), (K, E, K, 65, 1, x),
                                     (K, E, K, E, 0, x), (K, E, K, E, 65, x), (K, E, K, E, 1, x[1:])):
        refuse(lambda: be.dense_fwd_stream(x_, w, part, B, E_, K_, ldx, ldw, ns))
    untouched(x, w, part)


# ------------------------------------------------------------------------------------------------ (b) Gram form
GRAM_CASES = [(5, 256, 512, 1, 256, 512), (33, 352, 544, 1, 356, 546), (17, 880, 512, 3, 880, 518), (64, 2128, 512, 8, 2132, 512),
              (1, 64, 1024, 16, 64, 1024)]


@pytest.mark.parametrize("B,K,E,ns,ldx,ldw", GRAM_CASES)
def test_fwd_stream_gram(be, B, K, E, ns, ldx, ldw):
    """tnt_dense_fwd_stream_gram_f32: part as in (a); gx_part summed over the splits against x x^T (rows and columns < B) and
    w2_part summed against sum w^2 over the real columns, then both split by split (a tile that gram() counted twice or not at all
    sits in one split); w2_part has exactly nsplit * E / 32 entries, all written.  E = 544: the 17th column group repeats Gram
    tile (0, 0) and must not store it."""
    x, w = fwd_case(B, K, E)
    xd, wd = dev(padded(x, ldx)), dev(padded(w, ldw))
    nct = E // 32

    def launch(gs):
        part, gx, w2 = gs.new("part", ns, B, E), gs.new("gx_part", ns, 64, 64), gs.new("w2_part", ns, nct)
        be.dense_fwd_stream_gram(xd, wd, part, gx, w2, B, E, K, ldx, ldw, ns)
        return part, gx, w2
    part, gx, w2 = twice(launch)
    check_parts(part, x, w, K, ns)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(w2).all()), "an entry of gx_part / w2_part was not written"
    close(gx.sum(0)[:B, :B], x @ x.T, rtol=1e-5)
    close(w2.double().sum().reshape(1), [(w * w).sum()], rtol=1e-5)
    for s, c in enumerate(split_columns(K, ns)):
        close(gx[s, :B, :B], x[:, c] @ x[:, c].T, rtol=1e-5)
        close(w2[s], (w[c] ** 2).reshape(len(c), nct, 32).sum((0, 2)), rtol=1e-5)


def test_fwd_stream_gram_refuses_bad_arguments(be):
    """E = 480 (15 column groups), K % 16 != 0, B = 65, null gx_part: an error code, nothing written"""
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    x, w, part, gx, w2 = f(65 * 80), f(80 * 512), f(65 * 512), f(64 * 64), f(16)
    for B, K, E, gx_ in ((5, 64, 480, gx), (5, 72, 512, gx), (65, 64, 512, gx), (5, 64, 512, None)):
        refuse(lambda: be.dense_fwd_stream_gram(x, w, part, gx_, w2, B, E, K, K, E, 1))
    untouched(x, w, part, gx, w2)


# ------------------------------------------------------------------------------------------------ (c) skinny dW
# (N, E, Bk, dw one float off 16-byte alignment, kernel: tiles per wave, v = vector row layout)
DW_CASES = [(4149, 128, 64, False, "1"), (8200, 48, 1, False, "1"), (4149, 144, 37, False, "2"), (4149, 240, 17, False, "2"),
            (4149, 256, 63, False, "2v"), (4149, 256, 63, True, "2"), (4149, 304, 33, False, "4"), (4149, 768, 4, False, "4"),
            (1000, 512, 64, True, "4"), (4149, 1024, 3, False, "4v"), (1, 16, 1, False, "1"), (15, 304, 64, False, "4")]


def dw_kernel(E, misaligned):
    """the instantiation tnt_dense_dw_skinny_f32 picks"""
    tpw = 4 if E > 256 else (2 if E > 128 else 1)
    return f"{tpw}{'v' if tpw > 1 and E % (128 * tpw) == 0 and not misaligned else ''}"


@pytest.mark.parametrize("N,E,Bk,off,kernel", [pytest.param(*c, id=f"{c[4]}-{c[0]}x{c[1]}x{c[2]}{'-off' if c[3] else ''}") for c in DW_CASES])
def test_dw_skinny(be, N, E, Bk, off, kernel):
    """tnt_dense_dw_skinny_f32, all five kernels: dW against float64 x[:, :N]^T dpre and against be.gemm, ldx = N + 3 with PAD in
    the pad columns; rows >= N (the band behind the view) and, with dw one float off alignment, the floats around it untouched"""
    assert dw_kernel(E, off) == kernel
    rng = np.random.default_rng([N, E, Bk])
    x, dpre = r32(rng.standard_normal((Bk, N))), r32(rng.standard_normal((Bk, E)) * 0.01)
    ldx = N + 3
    xd, dd = dev(padded(x, ldx)), dev(dpre)

    def launch(gs):
        flat = gs.new("dw", N * E + 4)
        dw = flat[1:1 + N * E] if off else flat[:N * E]
        assert dw.data_ptr() % 16 == (4 if off else 0)
        be.dense_dw_skinny(xd, dd, dw.view(N, E), N, E, Bk, ldx)
        return (flat,)
    flat, = twice(launch)
    lo = 1 if off else 0
    assert bool(torch.isnan(flat[:lo]).all()) and bool(torch.isnan(flat[lo + N * E:]).all()), "written outside dw"
    dw = flat[lo:lo + N * E].view(N, E)
    close(dw, x.T @ dpre)
    ref = torch.zeros(N, E, device="cuda")
    be.gemm(xd, dd, ref, N, E, Bk, ldx, E, E, transA=True)
    close(dw, ref.cpu().numpy(), rtol=2e-6)


def test_dw_skinny_refuses_bad_arguments(be):
    """Bk = 65, E = 40, ldx < N: an error code, nothing written"""
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    x, dpre, dw = f(65 * 40), f(65 * 48), f(40 * 48)
    for N, E, Bk, ldx in ((32, 32, 65, 32), (32, 40, 8, 32), (32, 32, 8, 31)):
        refuse(lambda: be.dense_dw_skinny(x, dpre, dw, N, E, Bk, ldx))
    untouched(x, dpre, dw)


# ------------------------------------------------------------------------------------------------ (d) fused epilogues
FUSED_CASES = [(4149, 1024, 33), (8200, 512, 64), (5, 512, 1)]
LAM = F32(0.01)


class FusedCase:
    """inputs of one fused-epilogue case on the host and the device, the kernel's own float32 product X^T D (as float64), and the
    float64 product; never modified"""
    def __init__(self, be, N, E, Bk):
        rng = np.random.default_rng([N, E, Bk])
        self.N, self.E, self.Bk, self.ldx = N, E, Bk, N + 3
        self.x, self.dpre = r32(rng.standard_normal((Bk, N))), r32(rng.standard_normal((Bk, E)) * 0.01)
        self.theta, self.m0 = r32(rng.standard_normal((N, E)) * 0.05), r32(rng.standard_normal((N, E)) * 1e-3)
        self.v0 = r32(rng.random((N, E)) * 1e-6)
        self.xd, self.dd = dev(padded(self.x, self.ldx)), dev(self.dpre)
        self.thd, self.md, self.vd = dev(self.theta), dev(self.m0), dev(self.v0)
        gk = torch.zeros(N, E, device="cuda")
        be.dense_dw_skinny(self.xd, self.dd, gk, N, E, Bk, self.ldx)
        self.g64 = self.x.T @ self.dpre
        close(gk, self.g64)
        self.gk = gk.cpu().double().numpy()
        self.q64 = ((self.g64 + 2 * LAM * self.theta) ** 2).sum()
        nstrip = (N + 15) // 16
        self.grid, self.ny = min(nstrip, 256), E // 512
        self.nwg = self.grid * self.ny


@functools.lru_cache(maxsize=None)
def fused_case(be, N, E, Bk):
    return FusedCase(be, N, E, Bk)


@pytest.mark.parametrize("N,E,Bk", FUSED_CASES)
def test_dw_sqnorm_slots(be, N, E, Bk):
    """tnt_dense_dw_sqnorm_f32 slot by slot: slot blockIdx.y * gridDim.x + blockIdx.x holds sum (g + 2 lambda theta)^2 and
    sum theta^2 over its workgroup's strips (s = blockIdx.x, += gridDim.x) and 512 columns, with g the kernel's own float32
    product; the slots behind the workgroups up to nslot are exactly 0 (each workgroup zeroes slot + k * workgroups: nslot spans
    two rounds and a bit), nothing behind nslot is written; the sums over the slots against float64 within 1e-5"""
    c = fused_case(be, N, E, Bk)
    nslot = 2 * c.nwg + 3

    def launch(gs):
        partial = gs.new("partial", nslot, 2)
        be.dense_dw_sqnorm(c.xd, c.dd, c.thd, LAM, partial, nslot, N, E, Bk, c.ldx)
        return (partial,)
    p = twice(launch)[0].cpu().double().numpy()
    owner = (np.arange(N) // 16) % c.grid                       # blockIdx.x of the workgroup that runs a row's strip
    for name, col, elems in (("q", 0, (c.gk + 2 * LAM * c.theta) ** 2), ("wq", 1, c.theta ** 2)):
        rows = elems.reshape(N, c.ny, 512).sum(2)
        want = np.stack([np.bincount(owner, weights=rows[:, by], minlength=c.grid) for by in range(c.ny)]).reshape(-1)
        err = np.abs(p[:c.nwg, col] - want)
        print(f"{name}: worst slot error / slot value {np.max(err / want):.3e}")
        assert (err <= 1e-5 * want).all(), (name, int(np.argmax(err / want)), float(np.max(err / want)))
    assert (p[c.nwg:] == 0).all(), "a slot behind the workgroups' is not 0"
    assert abs(p[:, 0].sum() - c.q64) <= 1e-5 * c.q64 and abs(p[:, 1].sum() - (c.theta ** 2).sum()) <= 1e-5 * (c.theta ** 2).sum()


@pytest.mark.parametrize("N,E,Bk", FUSED_CASES)
def test_dw_adam(be, N, E, Bk):
    """tnt_dense_dw_adam_fin_f32 (clip from the span partials partial[k0:k1]: sq_override < 0; sq_override >= 0; clipnorm = 0)
    and tnt_dense_dw_adam_f32 (clip from sq): theta, m, v of N rows inside guard bands against float64 by the scheme and bounds
    of test_gpu_optim_tail.test_dense_dw_adam_fin (g = the kernel's own float32 product, everything behind it float64); a tripped
    guard leaves all three bit-identical"""
    c = fused_case(be, N, E, Bk)
    k0, nslot = 3, c.nwg + 2
    partial = torch.full((2 * (k0 + nslot + 5),), 7.0, device="cuda")
    be.dense_dw_sqnorm(c.xd, c.dd, c.thd, LAM, partial[2 * k0:], nslot, N, E, Bk, c.ldx)
    torch.cuda.synchronize()
    assert float(partial[:2 * k0].max()) == 7.0 and float(partial[2 * (k0 + nslot):].min()) == 7.0
    sq32 = F32(partial[2 * k0:2 * (k0 + nslot):2].double().sum().item())
    sq, lr_t = dev([sq32]), dev([3e-4])
    for mode in ("clip", "override", "noclip", "sq"):
        clip = 0.0 if mode == "noclip" else 0.1
        ovr = dev([4.0 if mode == "override" else -1.0])

        def run(tripped):
            gs = Guards()
            th, m, v = gs.new("theta", N, E), gs.new("m", N, E), gs.new("v", N, E)
            th.copy_(c.thd); m.copy_(c.md); v.copy_(c.vd)
            guard = torch.full((1,), int(tripped), dtype=torch.int32, device="cuda")
            if mode == "sq":
                be.dense_dw_adam(c.xd, c.dd, th, m, v, LAM, sq, None, lr_t, B1, B2, EPS, clip, N, E, Bk, c.ldx, guard=guard)
            else:
                be.dense_dw_adam_fin(c.xd, c.dd, th, m, v, LAM, partial, k0, k0 + nslot, ovr, lr_t, B1, B2, EPS, clip, N, E, Bk,
                                     c.ldx, guard=guard)
            torch.cuda.synchronize()
            gs.check()
            return th, m, v
        for got, before in zip(run(True), (c.thd, c.md, c.vd)):
            assert torch.equal(bits(got), bits(before)), (mode, "a tripped guard did not hold the state")
        th, m, v = run(False)
        for a, b in zip((th, m, v), run(False)):
            assert torch.equal(bits(a), bits(b)), (mode, "a second launch gave other bits")
        ge = c.gk + 2 * LAM * c.theta
        q = {"override": 4.0, "sq": sq32}.get(mode, c.q64)
        if clip > 0:
            ge = ge * clip / max(np.sqrt(q), clip)
        _, mw, vw = O.adam_update(c.theta, c.m0, c.v0, ge, 1, 1.0, B1, B2, EPS)
        tw = c.theta - F32(3e-4) * mw / (np.sqrt(vw) + EPS)              # lr_t is given (3e-4), not derived from t
        close(m, mw, rtol=1e-5); close(v, vw, rtol=1e-5); close(th, tw, rtol=1e-6)


def test_dw_fused_refuses_bad_arguments(be):
    """E = 768, theta off 16-byte alignment, k1 <= k0, nslot smaller than the workgroup count: an error code, nothing written"""
    N, Bk = 40, 4
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    x, dpre, th, m, v, partial, one = f(Bk * N), f(Bk * 768), f(N * 768 + 4), f(N * 768), f(N * 768), f(64), f(1)
    adam = lambda E, th_: be.dense_dw_adam(x, dpre, th_, m, v, LAM, one, None, one, B1, B2, EPS, 0.1, N, E, Bk, N)
    fin = lambda E, th_, k0, k1: be.dense_dw_adam_fin(x, dpre, th_, m, v, LAM, partial, k0, k1, None, one, B1, B2, EPS, 0.1, N, E,
                                                      Bk, N)
    sqn = lambda E, th_, nslot: be.dense_dw_sqnorm(x, dpre, th_, LAM, partial, nslot, N, E, Bk, N)
    for call in (lambda: adam(768, th), lambda: fin(768, th, 0, 3), lambda: sqn(768, th, 3),
                 lambda: adam(512, th[1:]), lambda: fin(512, th[1:], 0, 3), lambda: sqn(512, th[1:], 3),
                 lambda: fin(512, th, 3, 3), lambda: fin(512, th, 3, 2), lambda: sqn(512, th, 2)):      # 40 rows: 3 workgroups
        refuse(call)
    untouched(x, dpre, th, m, v, partial, one)


# ------------------------------------------------------------------------------------------------ (e) Gram norm
GN_CASES = [(1, 64, 1, 2), (15, 64, 3, 6), (17, 192, 16, 96), (64, 128, 8, 32)]


@pytest.mark.parametrize("Bk,E,ns,nw2", GN_CASES)
def test_gram_norm_slots(be, Bk, E, ns, nw2):
    """tnt_dense_gram_norm_f32 alone, slot by slot, on host-built by-products of a K = 16 nsplit forward (gx_part entries of rows and
    columns >= Bk hold PAD): slot 4 b + qd = (sum over b' in [16 qd, 16 qd + 16), b' < Bk of (sum_s gx[s, b, b']) (D D^T)[b, b'],
    plus 4 l2 sum_e D[b, e] (pre - bias)[b, e] when qd == 0; 0), slot 4 Bk + k = (4 l2^2 w2[k], w2[k]), the slots behind up to
    nslot = 4 Bk + nw2 + 5 exactly 0, nothing behind nslot written"""
    assert nw2 == ns * (E // 32)
    rng = np.random.default_rng([Bk, E, ns])
    K, l2, nslot = 16 * ns, LAM, 4 * Bk + nw2 + 5
    x, w = rng.standard_normal((Bk, K)), rng.standard_normal((K, E)) / np.sqrt(K)
    D, bias = r32(rng.standard_normal((Bk, E)) * 0.01), r32(0.1 * rng.standard_normal(E))
    pre = r32(x @ w + bias)
    gx = np.full((ns, 64, 64), PAD)
    for s in range(ns):
        gx[s, :Bk, :Bk] = r32(x[:, 16 * s:16 * s + 16] @ x[:, 16 * s:16 * s + 16].T)
    w2 = r32((w ** 2).reshape(ns, 16, E // 32, 32).sum((1, 3)).reshape(-1))
    ins = (dev(D), dev(pre), dev(bias), dev(gx), ns, dev(w2), nw2, l2)

    def launch(gs):
        partial = gs.new("partial", nslot, 2)
        be.dense_gram_norm(*ins, partial, nslot, Bk, E)
        return (partial,)
    p32 = twice(launch)[0].cpu().numpy()
    p = p32.astype(np.float64)
    T = gx[:, :Bk, :Bk].sum(0) * (D @ D.T)
    mid = 4 * l2 * (D * (pre - bias)).sum(1)
    want = np.zeros(nslot)
    for b in range(Bk):
        for qd in range(4):
            terms = np.append(T[b, 16 * qd:min(16 * qd + 16, Bk)], mid[b] if qd == 0 else 0.0)
            want[4 * b + qd] = terms.sum()
            assert abs(p[4 * b + qd, 0] - terms.sum()) <= 1e-6 * np.abs(terms).sum(), (b, qd, p[4 * b + qd, 0], terms.sum())
    assert (p[:4 * Bk, 1] == 0).all()
    want[4 * Bk:4 * Bk + nw2] = 4 * l2 * l2 * w2
    assert (np.abs(p[4 * Bk:4 * Bk + nw2, 0] - 4 * l2 * l2 * w2) <= 1e-6 * 4 * l2 * l2 * w2).all()
    assert (p32[4 * Bk:4 * Bk + nw2, 1] == w2.astype(np.float32)).all()
    assert (p[4 * Bk + nw2:] == 0).all(), "the slots behind the w2 slots are not 0"
    assert abs(p[:, 0].sum() - want.sum()) <= 2e-5 * want.sum()
    assert abs(p[:, 1].sum() - w2.sum()) <= 1e-5 * w2.sum()


def test_gram_norm_refuses_bad_arguments(be):
    """Bk = 65, E = 96, nslot = 4 Bk + nw2 - 1: an error code, nothing written"""
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    D, pre, bias, gx, w2, partial = f(65 * 128), f(65 * 128), f(128), f(64 * 64), f(4), f(2 * 300)
    for Bk, E, nslot in ((65, 128, 300), (8, 96, 300), (8, 128, 4 * 8 + 4 - 1)):
        refuse(lambda: be.dense_gram_norm(D, pre, bias, gx, 1, w2, 4, LAM, partial, nslot, Bk, E))
    untouched(D, pre, bias, gx, w2, partial)


# ------------------------------------------------------------------------------------------------ (f) locally dense
LD_SIZES = (1, 2, 3, 127, 128, 129, 257)          # the kc4 zero padding (1, 2, 3) and the edges of the KC = 128 chunks
LD_NVOX = 700


@functools.lru_cache(maxsize=None)
def ld_groups():
    """explicit region lists: the sizes of LD_SIZES, one voxel shared by two regions, one voxel listed twice inside a region"""
    rng = np.random.default_rng(5)
    perm = rng.permutation(LD_NVOX)
    cuts = np.cumsum((0,) + LD_SIZES)
    groups = [perm[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    groups[4][0] = groups[3][0]
    groups[5][7] = groups[5][3]
    assert [len(g) for g in groups] == list(LD_SIZES) and len(set(groups[5])) == 128 and groups[3][0] in groups[4]
    return groups


def split_tables(goff, piece):
    """(vgoff, vreg, vfirst, rfirst) of the split launches: every region cut into pieces of at most `piece` voxels"""
    vg, vr, vf, rf = [0], [], [], [0]
    for r in range(len(goff) - 1):
        k = int(goff[r])
        while k < goff[r + 1]:
            k2 = min(int(goff[r + 1]), k + piece)
            vg.append(k2); vr.append(r); vf.append(int(k == goff[r])); k = k2
        rf.append(len(vr))
    return vg, vr, vf, rf


@pytest.mark.parametrize("D", [16, 48, 64])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_locally_dense(be, B, D):
    """tnt_locally_dense_{fwd,bwd}_f32 and their split forms (pieces of 50 and of 128; x batch-major [B][N + 5] and voxel-major
    [N][ldt], pads holding PAD) at DT = 1, 3, 4 column tiles and one to three row blocks (65, 129: a last block of one row):
    pre / y against O.locally_dense_fwd, dW / db against x[:, g]^T dpre[:, r] and dpre.sum(0); all outputs start as NaN, so a
    first row block that accumulated would fail; split against plain within 1e-5, voxel-major bit-equal to batch-major"""
    groups = ld_groups()
    R, N = len(groups), LD_NVOX
    rng = np.random.default_rng([B, D])
    x, dpre = r32(rng.standard_normal((B, N))), r32(rng.standard_normal((B, R, D)))
    Ws = [r32(rng.standard_normal((len(g), D)) / np.sqrt(len(g))) for g in groups]
    bs = [r32(rng.standard_normal(D) * 0.1) for _ in groups]
    goff = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    nidx = int(goff[-1])
    ti = lambda a: dev(np.asarray(a), torch.int32)
    ldx, ldt = N + 5, (B + 3) // 4 * 4 + 4
    xd, xT = dev(padded(x, ldx)), dev(padded(x.T, ldt))
    idx, gd, Wd, bd, dd = ti(np.concatenate(groups)), ti(goff), dev(np.concatenate(Ws)), dev(np.stack(bs)), dev(dpre)
    want_y, want_pre = O.locally_dense_fwd(x, groups, Ws, bs)
    want_dW, want_db = np.concatenate([x[:, g].T @ dpre[:, r] for r, g in enumerate(groups)]), dpre.sum(0)

    def fwd(gs):
        pre, y = gs.new("pre", B, R, D), gs.new("y", B, R, D)
        be.locally_dense_fwd(xd, ldx, idx, gd, Wd, bd, pre, y, B, R, D, 0.2)
        return pre, y

    def bwd(gs):
        dW, db = gs.new("dW", nidx, D), gs.new("db", R, D)
        be.locally_dense_bwd(xd, ldx, idx, gd, dd, dW, db, B, R, D)
        return dW, db
    pre, y = twice(fwd)
    dW, db = twice(bwd)
    close(pre, want_pre); close(y, want_y); close(dW, want_dW); close(db, want_db)
    for piece in (50, 128):
        vg, vr, vf, rf = split_tables(goff, piece)
        NV = len(vr)
        assert NV > R
        vgd, vrd, vfd, rfd = ti(vg), ti(vr), ti(vf), ti(rf)
        got = {}
        for major, xin, ld in ((False, xd, ldx), (True, xT, ldt)):
            def fwd_split(gs):
                pre_s, y_s, part = gs.new("pre", B, R, D), gs.new("y", B, R, D), gs.new("partial", NV, 64, D)
                be.locally_dense_fwd_split(xin, ld, idx, vgd, vrd, rfd, NV, Wd, bd, pre_s, y_s, part, B, R, D, 0.2, voxel_major=major)
                return pre_s, y_s

            def bwd_split(gs):
                dW_s, db_s = gs.new("dW", nidx, D), gs.new("db", R, D)
                be.locally_dense_bwd_split(xin, ld, idx, vgd, vrd, vfd, NV, dd, dW_s, db_s, B, R, D, voxel_major=major)
                return dW_s, db_s
            got[major] = twice(fwd_split) + twice(bwd_split)
        for a, b in zip(got[False], got[True]):
            assert torch.equal(bits(a), bits(b)), (piece, "voxel-major differs from batch-major")
        pre_s, y_s, dW_s, db_s = got[False]
        close(pre_s, want_pre); close(y_s, want_y); close(dW_s, want_dW); close(db_s, want_db)
        close(pre_s, pre.cpu().numpy(), rtol=1e-5); close(dW_s, dW.cpu().numpy(), rtol=1e-5); close(db_s, db.cpu().numpy(), rtol=1e-5)


def test_locally_dense_refuses_bad_arguments(be):
    """D = 24, D = 80, NV < R (split), voxel-major with ldx % 4 != 0: an error code from all four entry points, nothing written"""
    B, N, R = 5, 16, 2
    f = lambda n: torch.full((n,), 7.0, device="cuda")
    x, W, bias, dpre = f(N * 8), f(N * 80), f(R * 80), f(B * R * 80)
    pre, y, dW, db, part = f(B * R * 80), f(B * R * 80), f(N * 80), f(R * 80), f(3 * 64 * 80)
    ti = lambda a: dev(np.asarray(a), torch.int32)
    idx, goff, vg, vr, vf, rf = ti(np.arange(N)), ti([0, 8, 16]), ti([0, 4, 8, 16]), ti([0, 0, 1]), ti([1, 0, 1]), ti([0, 2, 3])
    fwd_s = lambda ld, NV, D, major: be.locally_dense_fwd_split(x, ld, idx, vg, vr, rf, NV, W, bias, pre, y, part, B, R, D, 0.2,
                                                                voxel_major=major)
    bwd_s = lambda ld, NV, D, major: be.locally_dense_bwd_split(x, ld, idx, vg, vr, vf, NV, dpre, dW, db, B, R, D, voxel_major=major)
    for D in (24, 80):
        refuse(lambda: be.locally_dense_fwd(x, N, idx, goff, W, bias, pre, y, B, R, D, 0.2))
        refuse(lambda: be.locally_dense_bwd(x, N, idx, goff, dpre, dW, db, B, R, D))
        refuse(lambda: fwd_s(N, 3, D, False))
        refuse(lambda: bwd_s(N, 3, D, False))
    for call in (fwd_s, bwd_s):
        refuse(lambda: call(N, 1, 16, False))
        refuse(lambda: call(6, 3, 16, True))
    untouched(x, W, bias, dpre, pre, y, dW, db, part)


# ------------------------------------------------------------------------------------------------ block dense dx
DX_CASES = [(5, 3, 17, 64), (66, 2, 64, 64), (7, 4, 1, 17), (3, 2, 48, 33)]


@pytest.mark.parametrize("B,R,Din,Dout", DX_CASES)
def test_block_dense_dx(be, B, R, Din, Dout):
    """tnt_block_dense_dx_f32: dx[b, r] = W[r] @ dpre[b, r] against float64 at batch sizes that are no multiple of its 4 rows per
    pass, the widest layer and ragged ones"""
    rng = np.random.default_rng([B, R, Din, Dout])
    W, dpre = r32(rng.standard_normal((R, Din, Dout))), r32(rng.standard_normal((B, R, Dout)))
    Wd, dd = dev(W), dev(dpre)

    def launch(gs):
        dx = gs.new("dx", B, R, Din)
        be.block_dense_dx(dd, Wd, dx, B, R, Din, Dout)
        return (dx,)
    close(twice(launch)[0], np.einsum("rkn,brn->brk", W, dpre))
