// Consensus decoding (tnt_consensus_mix_f32, tnt_consensus_spread_i32; the definitions are in include/tnt_hip.h): the G
// member rows of one mixed row -- several scans of the same image, or the subjects of the multi-subject model -- are
// combined into one next-word distribution, in the place where softmax + argmax sit in a plain decode.
//
// Mix: one workgroup of 16 waves per mixed row r; member g is logits row g*Rm + r.
//   1. member statistics: member g gets W = 16 / G waves (G = 3: 5 waves, G = 16: one).  Each wave scans its strided share
//      of the member row for the max, the W wave results meet in LDS (one barrier), then the same waves sum exp(x - m_g)
//      and meet again (second barrier).  m_g, and c_g = w_g / s_g (mean) or log s_g (logmean), stay in LDS.
//   2. mix: thread t owns columns t, t + 1024, ...; per column it walks the G members in ascending g (fixed order) and
//      keeps the running first-max.  logmean parks l_v in the mix row itself (every thread re-reads only the columns it
//      wrote: program order, no barrier needed for that), reduces L = max l_v and Z = sum exp(l_v - L) over the block,
//      then rewrites the columns as exp(l_v - L) / Z.
// The member rows are read three times (max, sum, mix); at V = 5001 and G <= 16 they sit in L2 behind the head GEMM that
// wrote them, and the launch is bound by its latency, not by that traffic.  Deterministic; no atomics; no scratch memory.
#include "tnt_common.h"

namespace {

constexpr int CM_THREADS = 1024;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_MAXG = 16;
constexpr int CM_NONE = 0x7fffffff;
constexpr int CM_UNROLL = 4;

struct CmBest { float v; int i; };

// larger value wins; ties -> the smaller index (argmax_combine of seqops.hip: the first-max rule of tnt_argmax_rows_f32)
__device__ __forceinline__ CmBest cm_combine(CmBest a, CmBest b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

__device__ __forceinline__ CmBest cm_block_best(CmBest a, CmBest* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    CmBest b; b.v = __shfl_xor(a.v, o, 64); b.i = __shfl_xor(a.i, o, 64);
    a = cm_combine(a, b);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  CmBest r = sh[0];
  for (int q = 1; q < CM_WAVES; ++q) r = cm_combine(r, sh[q]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ float cm_block_max(float v, float* sh) {
  v = tnt_wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int q = 1; q < CM_WAVES; ++q) r = fmaxf(r, sh[q]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ float cm_block_sum(float v, float* sh) {
  v = tnt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int q = 0; q < CM_WAVES; ++q) r += sh[q];
  __syncthreads();
  return r;
}

template <int MODE>
__global__ __launch_bounds__(CM_THREADS) void consensus_mix_kernel(const float* __restrict__ logits, int ld, int V, int Rm,
                                                                   int G, const float* __restrict__ w,
                                                                   float* __restrict__ mix, int ldm,
                                                                   int* __restrict__ token) {
  __shared__ float part[CM_WAVES];      // per-wave partial of pass 1 (max, then exp-sum); block reductions of pass 2
  __shared__ float mg[CM_MAXG];         // m_g
  __shared__ float cg[CM_MAXG];         // mean: w_g / s_g     logmean: log s_g
  __shared__ float wg[CM_MAXG];         // w_g
  __shared__ CmBest shb[CM_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  // ---- 1. member statistics
  const int W = CM_WAVES / G;
  const int g = wave / W;                          // g >= G: an idle wave (it still meets every barrier)
  const bool act = g < G;
  const float* x = logits + ((long)(act ? g : 0) * Rm + r) * (long)ld;
  const int t0 = (wave - g * W) * 64 + lane, stride = W * 64;
  const int vend = act ? V : 0;
  float m = -INFINITY;
  for (int v0 = t0; v0 < vend; v0 += CM_UNROLL * stride) {
    float xv[CM_UNROLL];
#pragma unroll
    for (int u = 0; u < CM_UNROLL; ++u) {
      const int v = v0 + u * stride;
      xv[u] = v < vend ? x[v] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < CM_UNROLL; ++u) m = fmaxf(m, xv[u]);
  }
  m = tnt_wave_max(m);
  if (lane == 0) part[wave] = m;
  __syncthreads();
  if (act) {
    m = part[g * W];
    for (int q = 1; q < W; ++q) m = fmaxf(m, part[g * W + q]);
  }
  // a member row with nothing above -inf: m_g = 0 and s_g = 1 below, so that each of its columns stays -inf (no NaN)
  const bool empty = !(m > -INFINITY);
  if (empty) m = 0.f;
  __syncthreads();                                 // every wave has read the maxima before part is reused for the sums
  float s = 0.f;
  for (int v0 = t0; v0 < vend; v0 += CM_UNROLL * stride) {
    float xv[CM_UNROLL];
#pragma unroll
    for (int u = 0; u < CM_UNROLL; ++u) {
      const int v = v0 + u * stride;
      xv[u] = v < vend ? x[v] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < CM_UNROLL; ++u) s += expf(xv[u] - m);
  }
  s = tnt_wave_sum(s);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (act && wave == g * W && lane == 0) {
    float sg = part[g * W];
    for (int q = 1; q < W; ++q) sg += part[g * W + q];
    if (empty) sg = 1.f;
    const float wv = w ? w[g] : 1.f / (float)G;
    mg[g] = m;
    wg[g] = wv;
    cg[g] = MODE == 0 ? wv / sg : logf(sg);
  }
  __syncthreads();

  // ---- 2. mix + first-max
  float* out = mix + (long)r * ldm;
  const float* x0 = logits + (long)r * ld;
  const long gstep = (long)Rm * ld;                // member g of column v: x0[g * gstep + v]
  CmBest best; best.v = -INFINITY; best.i = CM_NONE;
  if (MODE == 0) {
    for (int v = tid; v < V; v += CM_THREADS) {
      float p = 0.f;
      for (int q = 0; q < G; ++q) p += expf(x0[q * gstep + v] - mg[q]) * cg[q];
      out[v] = p;
      if (p > best.v) { best.v = p; best.i = v; }
    }
  } else {
    float L = -INFINITY;
    for (int v = tid; v < V; v += CM_THREADS) {
      float l = 0.f;
      for (int q = 0; q < G; ++q) l += wg[q] * ((x0[q * gstep + v] - mg[q]) - cg[q]);
      out[v] = l;
      L = fmaxf(L, l);
    }
    L = cm_block_max(L, part);
    const bool none = !(L > -INFINITY);            // every l_v is -inf (or NaN): the row is all zero, token 0
    float z = 0.f;
    if (!none)
      for (int v = tid; v < V; v += CM_THREADS) z += expf(out[v] - L);
    const float Z = cm_block_sum(z, part);
    const float invZ = 1.f / Z;
    for (int v = tid; v < V; v += CM_THREADS) {
      const float p = none ? 0.f : expf(out[v] - L) * invZ;
      out[v] = p;
      if (p > best.v) { best.v = p; best.i = v; }
    }
  }
  if (!token) return;                              // uniform over the block
  best = cm_block_best(best, shb);
  const int id = best.i == CM_NONE ? 0 : best.i;
  if (tid < G) token[(long)tid * Rm + r] = id;
}

__global__ __launch_bounds__(256) void consensus_spread_kernel(const int* __restrict__ token, const int* __restrict__ parent,
                                                               const int* __restrict__ fin, int Rm, int G,
                                                               int* __restrict__ token_out, int* __restrict__ parent_out,
                                                               int* __restrict__ fin_out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= G * Rm) return;
  const int g = row / Rm, r = row - g * Rm;
  if (token) token_out[row] = token[r];
  if (parent) parent_out[row] = parent[r] + g * Rm;
  if (fin) fin_out[row] = fin[r];
}

}  // namespace

extern "C" int32_t tnt_consensus_mix_f32(const float* logits, int32_t ld, int32_t V, int32_t Rm, int32_t G, const float* w,
                                         int32_t mode, float* mix, int32_t ldm, int32_t* token, void* stream) {
  if (!logits) return TNT_BADARG(0);
  if (V <= 0) return TNT_BADARG(2);
  if (ld < V) return TNT_BADARG(1);
  if (Rm <= 0) return TNT_BADARG(3);
  if (G < 1 || G > CM_MAXG) return TNT_BADARG(4);
  if (mode != 0 && mode != 1) return TNT_BADARG(6);
  if (!mix) return TNT_BADARG(7);
  if (ldm < V) return TNT_BADARG(8);
  if ((long)G * Rm > 0x7fffffffL) return TNT_BADARG(3);
  {                                                    // the mix rows are written while member rows are still being read
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)mix;
    const uintptr_t na = (((uintptr_t)G * (uintptr_t)Rm - 1) * (uintptr_t)ld + (uintptr_t)V) * sizeof(float);
    const uintptr_t nb = (((uintptr_t)Rm - 1) * (uintptr_t)ldm + (uintptr_t)V) * sizeof(float);
    if (a < b + nb && b < a + na) return TNT_BADARG(7);
  }
  if (mode == 0)
    hipLaunchKernelGGL(consensus_mix_kernel<0>, dim3(Rm), dim3(CM_THREADS), 0, tnt_stream(stream), logits, ld, V, Rm, G, w,
                       mix, ldm, token);
  else
    hipLaunchKernelGGL(consensus_mix_kernel<1>, dim3(Rm), dim3(CM_THREADS), 0, tnt_stream(stream), logits, ld, V, Rm, G, w,
                       mix, ldm, token);
  TNT_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t tnt_consensus_spread_i32(const int32_t* token, const int32_t* parent, const int32_t* fin, int32_t Rm,
                                            int32_t G, int32_t* token_out, int32_t* parent_out, int32_t* fin_out,
                                            void* stream) {
  if (Rm <= 0) return TNT_BADARG(3);
  if (G < 1 || G > CM_MAXG) return TNT_BADARG(4);
  if ((long)G * Rm > 0x7fffffffL) return TNT_BADARG(3);
  if (token && !token_out) return TNT_BADARG(5);
  if (parent && !parent_out) return TNT_BADARG(6);
  if (fin && !fin_out) return TNT_BADARG(7);
  if (!token && !parent && !fin) return 0;             // nothing to spread: no launch
  const int rows = G * Rm;
  hipLaunchKernelGGL(consensus_spread_kernel, dim3((rows + 255) / 256), dim3(256), 0, tnt_stream(stream), token, parent, fin,
                     Rm, G, token_out, parent_out, fin_out);
  TNT_LAUNCH_CHECK();
  return 0;
}
