// Label-smoothed softmax + CategoricalCrossentropy(from_logits=False, label_smoothing=eps) in one launch
// (tnt_softmax_cce_smooth_f32; definition in include/tnt_hip.h, restated by tests/smooth_oracle.py).
//
// One 256-thread workgroup per row; the row walk (load + max, first-maximum index, exp-sum), the block reductions and the
// kernel ladder come from tnt_rowhead.h, and the one kernel template below holds what is smoothing's own: its second
// reduction, its row tail and its write.  What smoothing adds to the plain head (seqops.hip): the smoothed target ys_v = (1 - eps) [v == y] + eps / V
// is nonzero in every class, so keras's element-wise clip(p, 1e-7, 1 - 1e-7) acts per class, not per row.  With
// m_v = [1e-7 <= p_v <= 1 - 1e-7]:
//   loss      = -((1 - eps) L_y + (eps / V) sum_v L_v),   L_v = log clip(p_v) = m_v ? (x_v - max) - log Z : log(bound)
//   dlogits_v = gscale (c p_v - m_v ys_v),                c = sum_v m_v ys_v = (1 - eps) m_y + (eps / V) n_u
// so there is no per-element logf: after Z the row needs one more block reduction of two values, n_u = #{v : m_v} and
// S = sum_{m_v} (x_v - max).  A class can only sit above the upper bound if it is the row maximum with Z < 1 + 1.2e-7,
// i.e. p = 1 / Z and every other class is far below 1/2: n_hi = [1 / Z > 1 - 1e-7], n_lo = V - n_u - n_hi.
// The register row (NV4 >= 1) keeps x - max and exp(x - max) of the row in VGPRs (2 x 4 NV4 values per thread), so the row
// is read once and written once; the re-reading row (NV4 == 0) reads it (from the L2) in each of its four passes.
// Pad columns [V, ld): as in seqops.hip (masked to -inf as they are read; written as zero inside the register window,
// neither read nor written otherwise).
#include "tnt_rowhead.h"

namespace {

constexpr float SM_LO = 1e-7f;
constexpr float SM_HI = 1.f - 1e-7f;

struct SmoothRow {
  float c;      // sum_v m_v ys_v
  float ysy;    // m_y ys_y: what the target's own class subtracts (0 if its clip is active or there is no such class)
  float py;
};

// the row's scalars from its reductions, and its loss / correct outputs by thread 0.  y outside [0, V): the one-hot
// matches no class (ys_v = eps / V everywhere).
__device__ __forceinline__ SmoothRow smooth_row_tail(int row, int V, int y, bool has_y, float xy, float m, float Z, float invZ,
                                                     int n_u, float S, int am, float eps, bool has_target, float* loss_row,
                                                     float* correct_row) {
  const float eV = eps / (float)V;
  const float dy = xy - m;
  const float py = has_y ? expf(dy) * invZ : 0.f;
  const bool my = has_y && py >= SM_LO && py <= SM_HI;
  SmoothRow r;
  r.py = py;
  r.c = (my ? 1.f - eps : 0.f) + eV * (float)n_u;
  r.ysy = my ? (1.f - eps) + eV : 0.f;
  if (threadIdx.x == 0 && has_target) {
    if (loss_row) {
      const float logZ = logf(Z);
      const float log_lo = logf(SM_LO), log_hi = logf(SM_HI);
      const int n_hi = (invZ > SM_HI) ? 1 : 0;
      const int n_lo = V - n_u - n_hi;
      const float sumL = (S - (float)n_u * logZ) + ((float)n_lo * log_lo + (float)n_hi * log_hi);
      const float Ly = !has_y ? 0.f : (my ? dy - logZ : (py < SM_LO ? log_lo : log_hi));
      loss_row[row] = -((1.f - eps) * Ly + eV * sumL);
    }
    if (correct_row) correct_row[row] = (am == y) ? 1.f : 0.f;
  }
  return r;
}

__device__ __forceinline__ float smooth_grad(float p, float c, float eV, float gs) {
  const bool mv = p >= SM_LO && p <= SM_HI;
  return (c * p - (mv ? eV : 0.f)) * gs;
}

// NV4 >= 1: register-resident row (V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned rows), which also zeroes the pad columns
// inside its window; NV4 == 0: re-reading row (any V, ld, alignment), which neither reads nor writes a pad column.
// Three barriers: the maximum, Z (the first-maximum index rides on it), and S (n_u rides on it).
template <int NV4>
__global__ __launch_bounds__(256) void softmax_cce_smooth_kernel(const float* logits, const int* target, float* probs,
                                                                 float* loss_row, float* correct_row, float* dlogits,
                                                                 int rows, int V, int ld, float gscale, float eps) {
  __shared__ float shm[4], shz[4], shs[4];
  __shared__ int shi[4], shc[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  TntRow<NV4> w{x, V};
  int am;
  const float m = w.max_first(shm, shi, am);
  const int y = target ? target[row] : -1;
  const bool has_y = y >= 0 && y < V;
  const float xy = has_y ? x[y] : -INFINITY;                 // before any thread overwrites the row (aliasing)
  float4 dm[NV4 > 0 ? NV4 : 1];                              // register row: x - max, kept beside exp(x - max)
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) dm[i] = make_float4(w.d[i].x - m, w.d[i].y - m, w.d[i].z - m, w.d[i].w - m);
  }
  const float Z = tnt_block_sum4(w.exp_sum(m), shz);
  am = w.first(shi, am);
  const float invZ = 1.f / Z;
  // p_v, and the two reductions over the classes whose clip is inactive
  int n_u = 0;
  float S = 0.f;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      float4& e = w.d[i];
      e.x *= invZ; e.y *= invZ; e.z *= invZ; e.w *= invZ;
      const bool mx = e.x >= SM_LO && e.x <= SM_HI, my = e.y >= SM_LO && e.y <= SM_HI;
      const bool mz = e.z >= SM_LO && e.z <= SM_HI, mw = e.w >= SM_LO && e.w <= SM_HI;
      n_u += (int)mx + (int)my + (int)mz + (int)mw;
      S += ((mx ? dm[i].x : 0.f) + (my ? dm[i].y : 0.f)) + ((mz ? dm[i].z : 0.f) + (mw ? dm[i].w : 0.f));
    }
  } else {
    for (int j = tid; j < V; j += 256) {
      const float dj = x[j] - m;
      const float p = expf(dj) * invZ;
      const bool mv = p >= SM_LO && p <= SM_HI;
      n_u += (int)mv;
      S += mv ? dj : 0.f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_u += __shfl_xor(n_u, o, 64);
  tnt_wave_post(n_u, shc);
  S = tnt_block_sum4(S, shs);                                // its barrier: every read of the row above precedes every write below
  n_u = (shc[0] + shc[1]) + (shc[2] + shc[3]);
  const SmoothRow r = smooth_row_tail(row, V, y, has_y, xy, m, Z, invZ, n_u, S, am, eps, target != nullptr, loss_row,
                                      correct_row);
  const float gs = target ? gscale : 0.f;                    // no target: no loss to differentiate, zero rows
  const float eV = eps / (float)V;
  float* drow = dlogits ? dlogits + (long)row * ld : nullptr;
  float* prow = (probs && probs != dlogits) ? probs + (long)row * ld : nullptr;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      if (j >= ld) continue;
      const float4 e = w.d[i];
      if (drow)
        *reinterpret_cast<float4*>(drow + j) = make_float4(smooth_grad(e.x, r.c, eV, gs), smooth_grad(e.y, r.c, eV, gs),
                                                           smooth_grad(e.z, r.c, eV, gs), smooth_grad(e.w, r.c, eV, gs));
      if (prow) *reinterpret_cast<float4*>(prow + j) = e;
    }
    // the thread that owns column y patches it after its own vector store (same thread, same address: program order)
    if (drow && has_y && ((y >> 2) & 255) == tid) drow[y] = (r.c * r.py - r.ysy) * gs;
  } else {
    if (!drow && !prow) return;
    // logits may alias probs/dlogits: every thread reads its own elements before overwriting them
    for (int j = tid; j < V; j += 256) {
      const float p = expf(x[j] - m) * invZ;
      if (drow) drow[j] = (j == y) ? (r.c * r.py - r.ysy) * gs : smooth_grad(p, r.c, eV, gs);
      if (prow) prow[j] = p;
    }
  }
}

}  // namespace

extern "C" int32_t tnt_softmax_cce_smooth_f32(const float* logits, const int32_t* target, float* probs, float* loss_row,
                                              float* correct_row, float* dlogits, int32_t rows, int32_t V, int32_t ld,
                                              float gscale, float label_smoothing, void* stream) {
  if (rows == 0) return 0;
  if (rows < 0) return TNT_BADARG(6);
  if (V <= 0) return TNT_BADARG(7);
  if (ld < V) return TNT_BADARG(8);
  if (!logits) return TNT_BADARG(0);
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return TNT_BADARG(10);      // NaN fails both compares
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits) && (!probs || tnt_aligned16(probs)) &&
                  (!dlogits || tnt_aligned16(dlogits));
  tnt_row_ladder(al, V, [&](auto n) {
    hipLaunchKernelGGL((softmax_cce_smooth_kernel<decltype(n)::value>), dim3(rows), dim3(256), 0, s, logits, target, probs,
                       loss_row, correct_row, dlogits, rows, V, ld, gscale, label_smoothing);
  });
  TNT_LAUNCH_CHECK();
  return 0;
}
