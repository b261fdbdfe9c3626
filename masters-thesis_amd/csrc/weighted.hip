// Softmax + CategoricalCrossentropy(from_logits=False) with per-class token weights, the focal factor (Lin et al. 2017) and
// an optional normalisation by the weight sum, in one launch (tnt_softmax_cce_weighted_f32; definition in
// include/tnt_hip.h, restated by tests/weighted_oracle.py).
//
// One 256-thread workgroup per row; the row walk (load + max, first-maximum index, exp-sum), the block reductions and the
// kernel ladder come from tnt_rowhead.h, and the one kernel template below holds what is the weighted head's own.
// Two barriers, as in the plain head (seqops.hip).  What the weights and the focal factor add:
//   * every quantity they bring is a scalar of the row: w_r = class_weight[y], and behind the Z barrier pc, ce, f, g
//     (one logf, one powf per thread on wave-uniform values; gamma == 0 branches around both powers, gamma == 1 and
//     gamma == 2 around the powf).  Every element is then written as coef p_v with coef = gscale k w_r m_y g, and the
//     owner of column y patches it to coef (p_y - 1) behind its own store (same thread, same address: program order).
//     No per-element logf / powf, no third reduction.
//   * normalise = 1 needs W = sum_r w_r over ALL rows before any row can be written.  Every workgroup forms it itself:
//     thread t gathers class_weight[target[r]] for r = t, t + 256, ... (ceil(rows / 256) dependent-load pairs, issued in
//     front of the row load so that their latency overlaps it), the wave sums are posted to LDS and combined behind the
//     barrier of the row maximum.  No second launch, no atomics, no host sync; every workgroup computes the same bits
//     because the order is fixed (header).  normalise = 0, or no class_weight (W = rows exactly), gathers nothing.
//   * a row with w_r == 0 writes zeros whatever its logits hold.  Where none of its outputs needs the logits (probs null,
//     and correct_row null or scaled by w_r, i.e. normalise = 1) the workgroup leaves in front of the row walk, as the rows
//     behind the terminator do in tnt_scst_cce_f32.
// Pad columns [V, ld): as in seqops.hip (masked to -inf as they are read; written as zero inside the register window,
// neither read nor written otherwise).
#include "tnt_rowhead.h"

namespace {

constexpr float WT_LO = 1e-7f;
constexpr float WT_HI = 1.f - 1e-7f;

struct WtRow {
  float coef;   // gscale k w_r m_y g: what multiplies (p_v - [v == y])
  float py;
};

// behind the Z barrier: the row's scalars, and its loss / correct outputs by thread 0.  kw = k w_r (0 where w_r == 0).
__device__ __forceinline__ WtRow wt_row_tail(int row, int y, bool has_y, float xy, float m, float invZ, int am, float kw,
                                             float gamma, int normalise, float gs, bool has_target, float* loss_row,
                                             float* correct_row) {
  WtRow r;
  r.py = has_y ? expf(xy - m) * invZ : 0.f;
  const float my = (r.py >= WT_LO && r.py <= WT_HI) ? 1.f : 0.f;      // keras: zero gradient where the clip of ce is active
  const float pc = fminf(fmaxf(r.py, WT_LO), WT_HI);
  const float ce = -logf(pc);
  float f = 1.f, g = 1.f;
  if (gamma != 0.f) {                                                 // uniform over the grid
    const float omp = 1.f - pc;                                       // >= 1.19e-7: the powers stay finite
    const float e = gamma - 1.f;                                      // gamma 1 and 2 (keras's default) need no powf either
    const float q = e == 0.f ? 1.f : (e == 1.f ? omp : powf(omp, e));
    f = q * omp;
    g = f + gamma * pc * q * ce;
  }
  r.coef = (kw * (my * g)) * gs;
  if (threadIdx.x == 0 && has_target) {
    if (loss_row) loss_row[row] = kw * (f * ce);
    if (correct_row) correct_row[row] = (am == y) ? (normalise ? kw : 1.f) : 0.f;
  }
  return r;
}

// NV4 >= 1: register-resident row (V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned rows), which also zeroes the pad columns
// inside its window; NV4 == 0: re-reading row (any V, ld, alignment), which neither reads nor writes a pad column.
// Column c belongs to the thread that stores it: (c >> 2) & 255 on the register row, c & 255 on the re-reading row.
template <int NV4>
__global__ __launch_bounds__(256) void softmax_cce_weighted_kernel(const float* logits, const int* target, const float* cw,
                                                                   float* probs, float* loss_row, float* correct_row,
                                                                   float* dlogits, int rows, int V, int ld, float gscale,
                                                                   float gamma, int normalise) {
  __shared__ float shm[4], shz[4], shw[4];
  __shared__ int shi[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  const int y = target ? target[row] : -1;
  const bool has_y = y >= 0 && y < V;
  const float wr = (cw && has_y) ? cw[y] : 1.f;
  float* drow = dlogits ? dlogits + (long)row * ld : nullptr;
  if (target && wr == 0.f && !probs && (normalise || !correct_row)) {  // uniform: nothing of this row needs its logits
    if (tid == 0) {
      if (loss_row) loss_row[row] = 0.f;
      if (correct_row) correct_row[row] = 0.f;
    }
    if (drow) {
      if constexpr (NV4 > 0) {
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
          const int j = 4 * (tid + 256 * i);
          if (j < ld) *reinterpret_cast<float4*>(drow + j) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      } else {
        for (int j = tid; j < V; j += 256) drow[j] = 0.f;
      }
    }
    return;
  }
  // W, this thread's part: rows tid, tid + 256, ... in ascending order.  An id outside [0, V) weighs 1, as w_r does.
  const bool gather = normalise && cw && target;
  if (gather) {
    float ws = 0.f;
    for (int r = tid; r < rows; r += 256) {
      const int t = target[r];
      ws += (t >= 0 && t < V) ? cw[t] : 1.f;
    }
    tnt_wave_post(tnt_wave_sum(ws), shw);                     // rides on the barrier of the maximum
  }
  TntRow<NV4> w{x, V};
  int am;
  const float m = w.max_first(shm, shi, am);                  // the first barrier
  float k = 1.f;
  if (gather) {
    const float W = (shw[0] + shw[1]) + (shw[2] + shw[3]);
    k = (W == 0.f) ? 0.f : (float)rows / W;
  }
  const float kw = (wr == 0.f) ? 0.f : k * wr;
  const float xy = has_y ? x[y] : -INFINITY;                  // before any thread overwrites the row (aliasing)
  // the second barrier; also: every read of the row above precedes every write below
  const float Z = tnt_block_sum4(w.exp_sum(m), shz);
  am = w.first(shi, am);
  const float invZ = 1.f / Z;
  const float gs = target ? gscale : 0.f;                     // no target: no loss to differentiate, zero rows
  const WtRow r = wt_row_tail(row, y, has_y, xy, m, invZ, am, kw, gamma, normalise, gs, target != nullptr, loss_row,
                              correct_row);
  float* prow = (probs && probs != dlogits) ? probs + (long)row * ld : nullptr;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      if (j >= ld) continue;
      const float4 e = w.d[i];
      const float4 p = make_float4(e.x * invZ, e.y * invZ, e.z * invZ, e.w * invZ);
      if (drow) *reinterpret_cast<float4*>(drow + j) = make_float4(r.coef * p.x, r.coef * p.y, r.coef * p.z, r.coef * p.w);
      if (prow) *reinterpret_cast<float4*>(prow + j) = p;
    }
  } else {
    if (!drow && !prow) return;
    // logits may alias probs/dlogits: every thread reads its own elements before overwriting them
    for (int j = tid; j < V; j += 256) {
      const float p = expf(x[j] - m) * invZ;
      if (drow) drow[j] = r.coef * p;
      if (prow) prow[j] = p;
    }
  }
  // the thread that owns column y patches it after its own store (same thread, same address: program order)
  const auto owner = [](int c) { return NV4 > 0 ? (c >> 2) & 255 : c & 255; };
  if (drow && has_y && owner(y) == tid) drow[y] = r.coef * (r.py - 1.f);
}

}  // namespace

extern "C" int32_t tnt_softmax_cce_weighted_f32(const float* logits, const int32_t* target, const float* class_weight,
                                                float* probs, float* loss_row, float* correct_row, float* dlogits,
                                                int32_t rows, int32_t V, int32_t ld, float gscale, float gamma,
                                                int32_t normalise, void* stream) {
  if (rows == 0) return 0;
  if (rows < 0) return TNT_BADARG(7);
  if (V <= 0) return TNT_BADARG(8);
  if (ld < V) return TNT_BADARG(9);
  if (!logits) return TNT_BADARG(0);
  if (!(gamma >= 0.f && gamma <= 3.402823466e38f)) return TNT_BADARG(11);       // NaN fails both compares
  if (normalise != 0 && normalise != 1) return TNT_BADARG(12);
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits) && (!probs || tnt_aligned16(probs)) &&
                  (!dlogits || tnt_aligned16(dlogits));
  tnt_row_ladder(al, V, [&](auto n) {
    hipLaunchKernelGGL((softmax_cce_weighted_kernel<decltype(n)::value>), dim3(rows), dim3(256), 0, s, logits, target,
                       class_weight, probs, loss_row, correct_row, dlogits, rows, V, ld, gscale, gamma, normalise);
  });
  TNT_LAUNCH_CHECK();
  return 0;
}
