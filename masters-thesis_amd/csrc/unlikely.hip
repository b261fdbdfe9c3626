// Softmax + CategoricalCrossentropy(from_logits=False) + token-level unlikelihood (Welleck et al. 2020) in one launch
// (tnt_softmax_cce_unlikely_f32; definition in include/tnt_hip.h, restated by tests/unlikelihood_oracle.py).
//
// One 256-thread workgroup per row; the row walk (load + max, first-maximum index, exp-sum), the block reductions and the
// kernel ladder come from tnt_rowhead.h, and the one kernel template below holds what is the unlikelihood term's own.
// Two barriers, as in the plain head (seqops.hip): tnt_rowhead.h's reductions carry one each and none behind the combine.
// What the unlikelihood term adds:
//   * the candidate set C of row (t, b), the distinct ids of target[0 .. t-1][b] without y, 0 and ids outside [0, V).
//     Wave 0 forms it between the two barriers: lane j < t holds target[j * B + b] (loaded at the top of the kernel, so
//     that load's latency hides behind the row load), duplicates go by wave shuffles (first occurrence wins), the
//     survivors are compacted with a ballot into LDS together with their logits x_c -- fetched here, in front of the
//     second barrier, so in front of every write of the row (outputs may alias the logits).  Wave 0 has its own quarter
//     of the exp-sum behind this, so the up to 62 shuffles, the ballot and the dependent x_c load are NOT hidden: they
//     lengthen the workgroup's path to the second barrier.  tools/unlikelihood_bench.py separates that time (its
//     alpha = 0 arm against its all-zero-targets arm).
//   * behind the second barrier every wave computes p_c, q_c = m_c p_c / (1 - p_c) of candidate `lane` and their wave sum
//     Q: four identical copies of the same operations in the same order, which costs no third barrier.  Wave 0 also sums
//     the loss terms -log1p(-p_c).
//   * every element is written as gscale (m_y - alpha Q) p_v; the owner of column y and the owners of the at most 63
//     candidate columns then patch their element behind their own store (same thread, same address: program order).
//     A membership test per element would cost |C| compares on each of the V elements; the patch costs |C| LDS
//     broadcasts per thread.  No atomics, every address written by one thread, no scratch.
// A row without candidates (t = 0, or alpha = 0: C is not formed) writes the bits of tnt_softmax_cce_f32.
// Pad columns [V, ld): as in seqops.hip (masked to -inf as they are read; written as zero inside the register window,
// neither read nor written otherwise).
#include "tnt_rowhead.h"

namespace {

constexpr float UL_LO = 1e-7f;
constexpr float UL_HI = 1.f - 1e-7f;

struct UlCand {
  int id[64];
  float x[64];
  int n;
};

// wave 0 (tid < 64): the candidate set of the row into LDS.  cid: lane j's target[j * B + b] (anything for j >= t).
__device__ __forceinline__ void ul_form_candidates(UlCand& c, const float* x, int cid, int t, int y, int V, int lane) {
  bool keep = lane < t && cid > 0 && cid < V && cid != y;
  for (int k = 0; k + 1 < t; ++k) {                          // t is uniform: every lane takes part in every shuffle
    const int o = __shfl(cid, k, 64);
    if (k < lane && o == cid) keep = false;                  // an earlier position holds the same id
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
    c.id[pos] = cid;
    c.x[pos] = x[cid];                                       // before any thread overwrites the row (aliasing)
  }
  if (lane == 0) c.n = __popcll(mask);
}

struct UlRow {
  float coef;   // m_y - alpha Q: what multiplies p_v in every class
  float my;     // m_y
  float py;
};

__device__ __forceinline__ float ul_q(float pc) {
  const float omp = 1.f - pc;
  return omp >= UL_LO ? pc / omp : 0.f;
}

// behind the Z barrier: Q (every wave, the same bits), the row's loss / correct outputs by thread 0
__device__ __forceinline__ UlRow ul_row_tail(const UlCand& c, int row, int y, bool has_y, float xy, float m, float invZ, int am,
                                             float alpha, bool has_target, float* loss_row, float* correct_row) {
  const int lane = threadIdx.x & 63;
  const int nc = c.n;
  float Q = 0.f, ul = 0.f;
  if (nc > 0) {                                              // uniform over the workgroup
    float q = 0.f, l = 0.f;
    if (lane < nc) {
      const float pc = expf(c.x[lane] - m) * invZ;
      q = ul_q(pc);
      if (threadIdx.x < 64 && loss_row) l = (1.f - pc >= UL_LO) ? -log1pf(-pc) : -logf(UL_LO);
    }
    Q = tnt_wave_sum(q);
    if (threadIdx.x < 64 && loss_row) ul = tnt_wave_sum(l);
  }
  UlRow r;
  r.py = has_y ? expf(xy - m) * invZ : 0.f;
  r.my = (r.py >= UL_LO && r.py <= UL_HI) ? 1.f : 0.f;       // keras: zero gradient where the clip of ce is active
  r.coef = r.my - alpha * Q;
  if (threadIdx.x == 0 && has_target) {
    if (loss_row) loss_row[row] = -logf(fminf(fmaxf(r.py, UL_LO), UL_HI)) + alpha * ul;
    if (correct_row) correct_row[row] = (am == y) ? 1.f : 0.f;
  }
  return r;
}

// the gradient of candidate k's column, by the thread that owns it.  p_c and q_c are recomputed here by the very operations
// ul_row_tail uses for the terms of Q (the same expf, product and ul_q on the same LDS value), so the patched column
// holds the bits Q was summed from: the two places must stay in lock-step.
__device__ __forceinline__ float ul_cand_grad(const UlCand& c, int k, const UlRow& r, float m, float invZ, float alpha, float gs) {
  const float pc = expf(c.x[k] - m) * invZ;
  return (r.coef * pc + alpha * ul_q(pc)) * gs;
}

// NV4 >= 1: register-resident row (V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned rows), which also zeroes the pad columns
// inside its window; NV4 == 0: re-reading row (any V, ld, alignment), which neither reads nor writes a pad column.
// Column c belongs to the thread that stores it: (c >> 2) & 255 on the register row, c & 255 on the re-reading row.
template <int NV4>
__global__ __launch_bounds__(256) void softmax_cce_unlikely_kernel(const float* logits, const int* target, float* probs,
                                                                   float* loss_row, float* correct_row, float* dlogits,
                                                                   int B, int V, int ld, float gscale, float alpha) {
  __shared__ float shm[4], shz[4];
  __shared__ int shi[4];
  __shared__ UlCand cand;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  const int t = row / B, b = row - t * B;
  const bool form = target != nullptr && alpha > 0.f && t > 0;
  const int y = target ? target[row] : -1;
  int cid = 0;
  if (form && tid < t) cid = target[tid * B + b];            // t <= 63: lanes of wave 0
  if (tid == 0 && !form) cand.n = 0;
  TntRow<NV4> w{x, V};
  int am;
  const float m = w.max_first(shm, shi, am);                 // the first barrier
  const bool has_y = y >= 0 && y < V;
  const float xy = has_y ? x[y] : -INFINITY;                 // before any thread overwrites the row (aliasing)
  if (form && tid < 64) ul_form_candidates(cand, x, cid, t, y, V, tid);
  // the second barrier; also: the candidates and their logits are in LDS, and every read of the row above precedes every
  // write below
  const float Z = tnt_block_sum4(w.exp_sum(m), shz);
  am = w.first(shi, am);
  const float invZ = 1.f / Z;
  const UlRow r = ul_row_tail(cand, row, y, has_y, xy, m, invZ, am, alpha, target != nullptr, loss_row, correct_row);
  const float gs = target ? gscale : 0.f;                    // no target: no loss to differentiate, zero rows
  float* drow = dlogits ? dlogits + (long)row * ld : nullptr;
  float* prow = (probs && probs != dlogits) ? probs + (long)row * ld : nullptr;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      if (j >= ld) continue;
      const float4 e = w.d[i];
      const float4 p = make_float4(e.x * invZ, e.y * invZ, e.z * invZ, e.w * invZ);
      if (drow)
        *reinterpret_cast<float4*>(drow + j) = make_float4(r.coef * p.x * gs, r.coef * p.y * gs, r.coef * p.z * gs, r.coef * p.w * gs);
      if (prow) *reinterpret_cast<float4*>(prow + j) = p;
    }
  } else {
    if (!drow && !prow) return;
    // logits may alias probs/dlogits: every thread reads its own elements before overwriting them
    for (int j = tid; j < V; j += 256) {
      const float p = expf(x[j] - m) * invZ;
      if (drow) drow[j] = r.coef * p * gs;
      if (prow) prow[j] = p;
    }
  }
  if (!drow) return;
  // the threads that own column y and the candidate columns patch them after their own store (same thread, same address:
  // program order)
  const auto owner = [](int c) { return NV4 > 0 ? (c >> 2) & 255 : c & 255; };
  if (has_y && owner(y) == tid) drow[y] = (r.coef * r.py - r.my) * gs;
  const int nc = cand.n;
  for (int k = 0; k < nc; ++k) {
    const int c = cand.id[k];
    if (owner(c) == tid) drow[c] = ul_cand_grad(cand, k, r, m, invZ, alpha, gs);
  }
}

}  // namespace

extern "C" int32_t tnt_softmax_cce_unlikely_f32(const float* logits, const int32_t* target, float* probs, float* loss_row,
                                                float* correct_row, float* dlogits, int32_t B, int32_t T, int32_t V,
                                                int32_t ld, float gscale, float alpha, void* stream) {
  if (B < 0) return TNT_BADARG(6);
  if (T < 1 || T > 64) return TNT_BADARG(7);
  if (B == 0) return 0;
  if (V <= 0) return TNT_BADARG(8);
  if (ld < V) return TNT_BADARG(9);
  if (!logits) return TNT_BADARG(0);
  if (!(alpha >= 0.f && alpha <= 3.402823466e38f)) return TNT_BADARG(11);       // NaN fails both compares
  if ((long)B * T > 0x7fffffffL) return TNT_BADARG(6);
  const int rows = B * T;
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits) && (!probs || tnt_aligned16(probs)) &&
                  (!dlogits || tnt_aligned16(dlogits));
  tnt_row_ladder(al, V, [&](auto n) {
    hipLaunchKernelGGL((softmax_cce_unlikely_kernel<decltype(n)::value>), dim3(rows), dim3(256), 0, s, logits, target, probs,
                       loss_row, correct_row, dlogits, B, V, ld, gscale, alpha);
  });
  TNT_LAUNCH_CHECK();
  return 0;
}
