// Classifier-free guidance for caption decoding (tnt_guidance_mix_f32; the definition is in include/tnt_hip.h): the
// next-word distribution given the scan contrasted with the one the same model gives for a null scan, in the place where
// softmax + argmax sit in a plain decode.  The layout is the consensus one with two members: conditional row r, null row
// Rm + r.
//
// One workgroup of 16 waves per mixed row; thread t owns columns t, t + 1024, ... of BOTH member rows.
//   1. the two rows are read ONCE, into registers (NC = ceil(V / 1024) <= 8 columns per thread and row: V = 5001 is 5); the
//      maxima of both rows meet in LDS in one barrier, the two exp-sums in a second.
//   2. lc, ln and the guided logit g per column, from the registers; g takes the conditional logit's register.  The
//      plausibility threshold needs no reduction: (x - m) - log s is monotone in x, so max_v lc_v is (0 - log s_c).
//      Gm = max g meets in a third barrier, Z = sum exp(g - Gm) in a fourth, the first-max argmax of p in a fifth.
// Every block reduction has LDS words of its own, so each costs one barrier.  V > 8192 (NC = 0) re-reads the logits from
// memory in every pass and parks g in the mix row itself (a thread re-reads only the columns it wrote: program order).
// Fixed summation orders (a thread's columns ascending, the wave butterfly of tnt_wave_sum, the 16 waves ascending);
// no atomics; no scratch memory (the register arrays are indexed by unrolled constants only).
#include <cmath>
#include "tnt_common.h"

namespace {

constexpr int GM_THREADS = 1024;
constexpr int GM_WAVES = GM_THREADS / 64;
constexpr int GM_MAXNC = 8;
constexpr int GM_NONE = 0x7fffffff;

struct GmBest { float v; int i; };

// larger value wins; ties -> the smaller index (the first-max rule of tnt_argmax_rows_f32, as cm_combine of consensus.hip)
__device__ __forceinline__ GmBest gm_combine(GmBest a, GmBest b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// block reductions over sh[GM_WAVES], each call on LDS words no other reduction uses: one barrier
__device__ __forceinline__ float gm_block_max(float v, float* sh) {
  v = tnt_wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int q = 1; q < GM_WAVES; ++q) r = fmaxf(r, sh[q]);
  return r;
}

__device__ __forceinline__ float gm_block_sum(float v, float* sh) {
  v = tnt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int q = 0; q < GM_WAVES; ++q) r += sh[q];
  return r;
}

__device__ __forceinline__ GmBest gm_block_best(GmBest a, GmBest* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    GmBest b; b.v = __shfl_xor(a.v, o, 64); b.i = __shfl_xor(a.i, o, 64);
    a = gm_combine(a, b);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  GmBest r = sh[0];
  for (int q = 1; q < GM_WAVES; ++q) r = gm_combine(r, sh[q]);
  return r;
}

// NC > 0: both rows in NC registers per thread (V <= NC * 1024); NC = 0: any V, the rows re-read from memory
template <int NC>
__global__ __launch_bounds__(GM_THREADS) void guidance_mix_kernel(const float* __restrict__ logits, int ld, int V, int Rm,
                                                                  float scale, float plaus, float* __restrict__ mix, int ldm,
                                                                  int* __restrict__ token) {
  constexpr bool REG = NC > 0;
  __shared__ float sh_mc[GM_WAVES], sh_mn[GM_WAVES], sh_sc[GM_WAVES], sh_sn[GM_WAVES], sh_g[GM_WAVES], sh_z[GM_WAVES];
  __shared__ GmBest sh_b[GM_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* xc = logits + (long)r * ld;              // the conditional row
  const float* xn = logits + ((long)Rm + r) * ld;       // its null row
  float* out = mix + (long)r * ldm;
  const int nc = REG ? NC : (V + GM_THREADS - 1) / GM_THREADS;
  float a[REG ? NC : 1], b[REG ? NC : 1];               // REG: the thread's conditional / null logits; a becomes g, then p

  // ---- 1. row statistics of both members
  float mc = -INFINITY, mn = -INFINITY;
#pragma unroll
  for (int u = 0; u < nc; ++u) {
    const int v = tid + u * GM_THREADS;
    const float c = v < V ? xc[v] : -INFINITY, n = v < V ? xn[v] : -INFINITY;
    if constexpr (REG) { a[u] = c; b[u] = n; }
    mc = fmaxf(mc, c);
    mn = fmaxf(mn, n);
  }
  mc = tnt_wave_max(mc);
  mn = tnt_wave_max(mn);
  if ((tid & 63) == 0) { sh_mc[tid >> 6] = mc; sh_mn[tid >> 6] = mn; }
  __syncthreads();
  mc = sh_mc[0]; mn = sh_mn[0];
  for (int q = 1; q < GM_WAVES; ++q) { mc = fmaxf(mc, sh_mc[q]); mn = fmaxf(mn, sh_mn[q]); }
  // a row with nothing above -inf: m = 0 and s = 1, so that each of its columns stays -inf (no NaN)
  const bool empty_c = !(mc > -INFINITY), empty_n = !(mn > -INFINITY);
  if (empty_c) mc = 0.f;
  if (empty_n) mn = 0.f;
  float sc = 0.f, sn = 0.f;
#pragma unroll
  for (int u = 0; u < nc; ++u) {
    const int v = tid + u * GM_THREADS;
    float c, n;
    if constexpr (REG) { c = a[u]; n = b[u]; }
    else { c = v < V ? xc[v] : -INFINITY; n = v < V ? xn[v] : -INFINITY; }
    sc += expf(c - mc);
    sn += expf(n - mn);
  }
  sc = tnt_wave_sum(sc);
  sn = tnt_wave_sum(sn);
  if ((tid & 63) == 0) { sh_sc[tid >> 6] = sc; sh_sn[tid >> 6] = sn; }
  __syncthreads();
  sc = 0.f; sn = 0.f;
  for (int q = 0; q < GM_WAVES; ++q) { sc += sh_sc[q]; sn += sh_sn[q]; }
  if (empty_c) sc = 1.f;
  if (empty_n) sn = 1.f;
  const float lsc = logf(sc), lsn = logf(sn);

  // ---- 2. the guided logits, their maximum
  // max_v lc_v is the conditional maximum's own lc = (m - m) - log s; an empty conditional row has no finite lc at all
  const bool masked = plaus > 0.f;
  const float thr = masked ? logf(plaus) + (empty_c ? -INFINITY : 0.f - lsc) : -INFINITY;
  float Gm = -INFINITY;
#pragma unroll
  for (int u = 0; u < nc; ++u) {
    const int v = tid + u * GM_THREADS;
    float c, n;
    if constexpr (REG) { c = a[u]; n = b[u]; }
    else { c = v < V ? xc[v] : -INFINITY; n = v < V ? xn[v] : -INFINITY; }
    const float lc = (c - mc) - lsc, ln = (n - mn) - lsn;
    float g = -INFINITY;                                  // a ban stays a ban: inf - inf is never formed
    if (lc > -INFINITY && !(masked && lc < thr)) g = ln > -INFINITY ? fmaf(scale, lc - ln, lc) : lc;
    if constexpr (REG) a[u] = g;
    else if (v < V) out[v] = g;
    Gm = fmaxf(Gm, g);
  }
  Gm = gm_block_max(Gm, sh_g);
  const bool none = !(Gm > -INFINITY);                    // every g_v is -inf: the row is all zero, token 0

  // ---- 3. p = exp(g - Gm) / Z, its first maximum
  float z = 0.f;
#pragma unroll
  for (int u = 0; u < nc; ++u) {
    const int v = tid + u * GM_THREADS;
    float e = 0.f;
    if constexpr (REG) { e = none ? 0.f : expf(a[u] - Gm); a[u] = e; }
    else if (v < V) { e = none ? 0.f : expf(out[v] - Gm); out[v] = e; }
    z += e;
  }
  const float Z = gm_block_sum(z, sh_z);
  GmBest best; best.v = -INFINITY; best.i = GM_NONE;
#pragma unroll
  for (int u = 0; u < nc; ++u) {
    const int v = tid + u * GM_THREADS;
    if (v < V) {
      float e;
      if constexpr (REG) e = a[u];
      else e = out[v];
      const float p = none ? 0.f : e / Z;
      out[v] = p;
      if (p > best.v) { best.v = p; best.i = v; }
    }
  }
  if (!token) return;                                     // uniform over the block
  best = gm_block_best(best, sh_b);
  const int id = best.i == GM_NONE ? 0 : best.i;
  if (tid < 2) token[(long)tid * Rm + r] = id;
}

template <int NC>
void gm_launch(const float* logits, int ld, int V, int Rm, float scale, float plaus, float* mix, int ldm, int* token,
               hipStream_t s) {
  hipLaunchKernelGGL(guidance_mix_kernel<NC>, dim3(Rm), dim3(GM_THREADS), 0, s, logits, ld, V, Rm, scale, plaus, mix, ldm,
                     token);
}

}  // namespace

extern "C" int32_t tnt_guidance_mix_f32(const float* logits, int32_t ld, int32_t V, int32_t Rm, float scale, float plaus,
                                        float* mix, int32_t ldm, int32_t* token, void* stream) {
  if (!logits) return TNT_BADARG(0);
  if (V <= 0) return TNT_BADARG(2);
  if (ld < V) return TNT_BADARG(1);
  if (Rm <= 0 || 2L * Rm > 0x7fffffffL) return TNT_BADARG(3);
  if (!std::isfinite(scale) || scale < 0.f) return TNT_BADARG(4);
  if (!std::isfinite(plaus) || plaus < 0.f || !(plaus < 1.f)) return TNT_BADARG(5);
  if (!mix) return TNT_BADARG(6);
  if (ldm < V) return TNT_BADARG(7);
  {                                                    // the mix rows are written while member rows are still being read
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)mix;
    const uintptr_t na = ((2 * (uintptr_t)Rm - 1) * (uintptr_t)ld + (uintptr_t)V) * sizeof(float);
    const uintptr_t nb = (((uintptr_t)Rm - 1) * (uintptr_t)ldm + (uintptr_t)V) * sizeof(float);
    if (a < b + nb && b < a + na) return TNT_BADARG(6);
  }
  hipStream_t s = tnt_stream(stream);
  const int nc = (V + GM_THREADS - 1) / GM_THREADS;
  switch (nc <= GM_MAXNC ? nc : 0) {
    case 1: gm_launch<1>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 2: gm_launch<2>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 3: gm_launch<3>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 4: gm_launch<4>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 5: gm_launch<5>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 6: gm_launch<6>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 7: gm_launch<7>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    case 8: gm_launch<8>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
    default: gm_launch<0>(logits, ld, V, Rm, scale, plaus, mix, ldm, token, s); break;
  }
  TNT_LAUNCH_CHECK();
  return 0;
}
