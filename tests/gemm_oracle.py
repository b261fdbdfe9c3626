"""Operand builder, float64 references and launch arithmetic of the three hand-written GEMM families (csrc/gemm.hip: the tiled
kernel with its split-K reduce, the one-round gemm1r / gemm2 family; csrc/gemm3.hip: the LDS-DMA family), shared by
tests/test_gpu_gemm_paths.py (which compares the kernels with them) and tests/test_host_gemm_edges.py (which checks the
references against oracle.ops, the mirrors against the constants in the sources, and every named size against the edge it is
named for).  numpy only.

An operand is handed to a kernel the way the models hand theirs over: as a view into a larger buffer (`embed`), `front` floats
behind its start, at a row stride above its width, with something unpleasant (`fill`, NaN by default) in every float the
interface does not promise to read as data."""
import collections

import numpy as np

from oracle import ops as O

NAN = np.float32(np.nan)                  # 0x7FC00000: the quiet NaN, never the split-K exchange's "not written yet" pattern
U24 = 2.0 ** -24                          # unit roundoff of float32
TAIL = 64                                 # floats behind the last row of an embedded operand

# ---- mirrors of the sources (test_host_gemm_edges.py reads the originals)
BK = 32                                                                  # csrc/gemm.hip: k depth of a tile, both families
TILED = ((64, 64), (128, 128), (64, 128), (128, 64))                     # launch_layout: the forced tiles of tnt_gemm_f32_tile
# launch_1r: cfg -> (kernel, BM, BN, WGM, WGN, register prefetch depth PD; gemm2 has two named stages)
CFG_1R = {1: ("gemm1r", 160, 128, 2, 8, 1), 9: ("gemm1r", 64, 64, 4, 2, 3), 21: ("gemm2", 64, 64, 2, 2, 2),
          22: ("gemm2", 64, 64, 4, 2, 2), 24: ("gemm2", 128, 64, 4, 2, 2), 25: ("gemm2", 64, 32, 2, 2, 2),
          26: ("gemm2", 64, 160, 2, 5, 2), 28: ("gemm2", 160, 128, 2, 8, 2)}
# tnt_gemm3_f32: tile -> (TM, TN, WGM, WGN, BK, NS); the workgroup tile is 16 TM WGM x 16 TN WGN (g3_tile repeats it)
G3 = {1: (5, 4, 2, 2, 32, 3), 2: (4, 5, 2, 2, 32, 3), 3: (4, 4, 2, 2, 32, 3), 4: (2, 5, 4, 1, 32, 3), 5: (2, 4, 2, 2, 32, 3),
      6: (4, 2, 2, 2, 32, 3), 7: (2, 2, 2, 2, 32, 3), 8: (4, 5, 4, 1, 32, 3), 9: (2, 2, 2, 2, 64, 3), 10: (2, 4, 2, 2, 64, 3),
      11: (4, 2, 2, 2, 64, 3)}
NS = 3                                                                   # depth of gemm3's LDS ring
G3_UNITS = 256                                                           # g3_cost: workgroups of a split launch, one round
LAYOUTS = {"NN": (False, False), "TN": (True, False), "NT": (False, True)}


def roundup4(n):
    return (n + 3) // 4 * 4


def g3_tile(tile):
    """(BM, BN, BK) of gemm3 configuration `tile`"""
    tm, tn, wgm, wgn, bk, _ = G3[tile]
    return 16 * tm * wgm, 16 * tn * wgn, bk


def g3_acc_rows(tile):
    """accumulator tile rows of a workgroup (NW * TM): the units of ownership in the in-launch reduction"""
    tm, _, wgm, wgn, _, _ = G3[tile]
    return wgm * wgn * tm


# ---- launch arithmetic
def tiled_split(K, splitk):
    """gemm_dispatch: (kchunk, the split count that really runs, length of the last chunk)"""
    kchunk = -(-(-(-K // max(splitk, 1))) // BK) * BK
    s = -(-K // kchunk)
    return kchunk, s, K - (s - 1) * kchunk


def g3_split(tile, K, S):
    """g3_prepare: (K stages in all, stages per split, the split count that really runs, stages of the last split)"""
    bk = g3_tile(tile)[2]
    nst = -(-K // bk)
    s = min(max(S, 1), nst)
    per = -(-nst // s)
    s = -(-nst // per)
    return nst, per, s, nst - (s - 1) * per


def g3_units(tile, M, N, S, batch=1):
    bm, bn, _ = g3_tile(tile)
    return -(-M // bm) * -(-N // bn) * S * batch


def g3_work_floats(tile, M, N, S, batch=1):
    """tnt_gemm3_work_floats: sized by the REQUESTED split"""
    bm, bn, _ = g3_tile(tile)
    return 0 if S <= 1 else g3_units(tile, M, N, S, 2 if batch > 1 else 1) * bm * bn


def g3_ownerless(tile, S):
    """the splits that own no accumulator tile row: owner of row i is i mod S"""
    return sorted(set(range(S)) - {i % S for i in range(g3_acc_rows(tile))})


def k_tiles(K):
    return -(-K // BK)


# ---- operands
Embedded = collections.namedtuple("Embedded", "buf view ld logical")


def embed(op, trans, ld_extra=0, front=0, fill=NAN, zero_pad=False):
    """Lay the logical operand `op` (op(A) [M][K] or op(B) [K][N]), stored transposed if `trans`, into a larger float32 buffer:
    `front` floats before its first element (a sub-view; front % 4 != 0: one that is not 16-byte aligned), row stride
    ld = roundup4(width) + ld_extra, TAIL floats behind the last row.  zero_pad: the pad columns [width, roundup4(width)) hold
    zeros (what gemm3 requires of a K-contiguous operand); every other float that is not an element is `fill`.
    Returns (buffer, the view to pass = buffer[front:], ld, the float64 logical matrix of the float32-rounded values)."""
    stored = np.asarray(op, np.float64).T if trans else np.asarray(op, np.float64)
    rows, width = stored.shape
    ld = roundup4(width) + ld_extra
    buf = np.full(front + rows * ld + TAIL, fill, np.float32)
    body = buf[front:front + rows * ld].reshape(rows, ld)
    if zero_pad:
        body[:, width:roundup4(width)] = 0.0
    body[:, :width] = stored
    logical = body[:, :width].astype(np.float64)
    return Embedded(buf, buf[front:], ld, logical.T if trans else logical)


def extract(e, shape, trans):
    """the logical matrix back out of an embedded operand's view (the inverse of embed)"""
    rows, width = (shape[1], shape[0]) if trans else shape
    body = e.view[:rows * e.ld].reshape(rows, e.ld)[:, :width].astype(np.float64)
    return body.T if trans else body


def ints(rng, *shape):
    """integer-valued data in [-3, 3]: every float32 partial sum of products of it is exact in any order (up to K = 2^24 / 9)"""
    return rng.integers(-3, 4, shape).astype(np.float64)


# ---- references
def product(opA, opB, bias=None):
    """op(A) op(B) (+ bias, [N] or [M][N]) in float64"""
    pre = np.asarray(opA, np.float64) @ np.asarray(opB, np.float64)
    return pre if bias is None else pre + np.asarray(bias, np.float64)


def colsum(opB):
    return np.asarray(opB, np.float64).sum(0)


ACTS = {"none": O.ACT_NONE, "leaky": O.ACT_LEAKY, "relu": O.ACT_RELU, "tanh": O.ACT_TANH}


def act(pre, kind, slope=0.2):
    """the activation of a pre-activation.  A float32 `pre` (the device's own) gives what tnt_act must produce from it bit for
    bit where the arithmetic is exact: none, relu, and leaky as float32(x * float32(slope)); tanh, and any float64 `pre`, give
    the float64 value."""
    pre = np.asarray(pre)
    if pre.dtype == np.float32 and kind != "tanh":
        if kind == "none":
            return pre
        if kind == "relu":
            return np.where(pre > 0, pre, np.float32(0))
        assert kind == "leaky"
        return np.where(pre > 0, pre, pre * np.float32(slope)).astype(np.float32)
    pre = pre.astype(np.float64)
    if kind == "leaky":
        return np.where(pre > 0, pre, pre * float(np.float32(slope)))
    return O.act_fwd(pre, ACTS[kind], slope)


def fp32_dot_bound(opA, opB, bias=None):
    """(K + 2) u (|op(A)| |op(B)| + |bias|), u = 2^-24: the bound of a float32 dot product of K terms plus one addend summed in
    any order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_n with n roundings per term, to first
    order) with one rounding to spare -- the one an epilogue spends.  `bias` is whatever else is added: [N] or [M][N]."""
    opA, opB = np.abs(np.asarray(opA, np.float64)), np.abs(np.asarray(opB, np.float64))
    mag = opA @ opB
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, np.float64))
    return (opA.shape[1] + 2) * U24 * mag


def g3_bound(want, K):
    """gemm3's own bound (tests/test_gpu_ops.py: test_gemm3): 1e-6 max(1, sqrt(K / 256)) of the largest magnitude"""
    return 1e-6 * max(1.0, (K / 256) ** 0.5) * (np.abs(want).max() + 1e-30)


# ---- the sizes of tests/test_gpu_gemm_paths.py, each named for one edge (test_host_gemm_edges.py asserts the edge)
TILED_K = (1, 31, 32, 33, 67)                     # one k, a tile less one, a whole tile, one more, two tiles and a ragged third
TILED_FORMS = {"vec": (8, 4), "front1": (1, 0), "ld1": (0, 1)}     # (front, ld_extra): float4 loads; unaligned; ld % 4 != 0
TILED_EPILOGUES = ("none", "leaky", "relu", "tanh", "pre", "acc", "pre+acc")
TILED_SPLITS = ((200, 3), (200, 4), (100, 8), (33, 2))              # (K, requested splitk)
FUSED_K = (5, 32, 33, 64, 96, 97, 130, 161)       # 1 to 6 k tiles, odd and even counts, tails that are no multiple of 4
FUSED_AUTO = {"NN": (1000, 500, 33), "TN": (1000, 500, 70)}          # shapes tnt_gemm_fused_cfg serves (cfg = 0)
G3_OWNERLESS = (7, 65, 69, 1536, 12)              # tile, M, N, K, S: splits 8 to 11 own no accumulator row
G3_EMBEDDED = dict(tiles=(7, 9), M=70, N=40, ld_extra=8)


def tiled_shapes(bm, bn):
    """every (M, N, K) of a forced tile: M in 1, BM - 1, BM + 1; N in 3, BN + 1; K over TILED_K"""
    return [(M, N, K) for M in (1, bm - 1, bm + 1) for N in (3, bn + 1) for K in TILED_K]


def g3_ks(bk):
    """K of 1, 2, 3 and 4 stages: the tail ends inside a 4-chunk, inside a 16-block, inside a stage, nowhere"""
    return (bk - 3, bk + 1, 2 * bk + 17, 4 * bk)


def g3_split_cases(tile):
    """(name, K, requested S, batch, bias) of the split launches of one tile"""
    bk = g3_tile(tile)[2]
    return [("S2", 2 * bk + 17, 2, 1, False), ("S3", 4 * bk + 9, 3, 1, False), ("S8 clamped", bk + 1, 8, 1, False),
            ("S2 A2", 2 * bk + 17, 2, 2, False), ("S2 bias", 3 * bk + 5, 2, 1, True)]
