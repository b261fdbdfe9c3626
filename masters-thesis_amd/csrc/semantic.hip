// The sentence-embedding target of nic.NIC (the reference's fifth input, the "GUSE" vector of the caption; its loss is
// lc_NIC.py:488-502, cosine_loss = 1 - cos) and nearest-neighbour retrieval in that space.  Definitions: include/tnt_hip.h.
//   tnt_cosine_loss_f32     per row: cos of the l2-normalised prediction and target, loss = 1 - cos, its gradient, the mean
//   tnt_row_inv_norm_f32    per row: 1 / sqrt(max(sum x^2, 1e-12))
//   tnt_cosine_topk_f32     per row of raw dot products: the k largest cosine similarities and their indices
// Everything is float32 with a fixed summation order and no float atomics: two runs give the same bits, and a row's bits
// depend on that row alone (one wave, or one workgroup, owns a row and walks it the same way whatever B is).
#include "tnt_common.h"

namespace {
constexpr float SEM_EPS = 1e-12f;    // keras l2_normalize: x * rsqrt(max(sum x^2, epsilon))
constexpr int CL_T = 1024;           // cosine loss: 16 waves, wave w owns the rows w, w + 16, ... of the workgroup's 256
constexpr int CL_ROWS = 256;
constexpr int RN_T = 256;            // inverse norms: 4 waves, one row each
constexpr int TK_T = 1024;           // selection: one workgroup per row
constexpr int TK_W = TK_T / 64;

// One wave's sums over a row of G floats: lane l takes the float4 l, l + 64, ... (x, y, z, w in order, fused multiply-add)
// and then the G % 4 tail elements (lanes 0 .. 2); VEC = false: the floats l, l + 64, ...; then the 64-lane butterfly.
template <bool VEC, bool PAIR>
__device__ __forceinline__ void sem_row_sums(const float* z, const float* g, int G, int lane, float& szz, float& sgg,
                                             float& szg) {
  float a = 0.f, b = 0.f, c = 0.f;
  int j0 = 0;
  if (VEC) {
    const int G4 = G >> 2;
    for (int q = lane; q < G4; q += 64) {
      const float4 x = *reinterpret_cast<const float4*>(z + 4 * q);
      a = fmaf(x.x, x.x, a); a = fmaf(x.y, x.y, a); a = fmaf(x.z, x.z, a); a = fmaf(x.w, x.w, a);
      if (PAIR) {
        const float4 y = *reinterpret_cast<const float4*>(g + 4 * q);
        b = fmaf(y.x, y.x, b); b = fmaf(y.y, y.y, b); b = fmaf(y.z, y.z, b); b = fmaf(y.w, y.w, b);
        c = fmaf(x.x, y.x, c); c = fmaf(x.y, y.y, c); c = fmaf(x.z, y.z, c); c = fmaf(x.w, y.w, c);
      }
    }
    j0 = G4 << 2;
  }
  for (int j = j0 + lane; j < G; j += 64) {
    const float x = z[j];
    a = fmaf(x, x, a);
    if (PAIR) {
      const float y = g[j];
      b = fmaf(y, y, b);
      c = fmaf(x, y, c);
    }
  }
  szz = tnt_wave_sum(a);
  if (PAIR) { sgg = tnt_wave_sum(b); szg = tnt_wave_sum(c); }
}

// ---------------------------------------------------------------------------------------------------
// Cosine loss.  Workgroup x owns the rows [256 x, 256 x + 256); wave w walks its rows in ascending order.  Per row: the
// three sums, cos, loss, then (dz given) the gradient, every lane rewriting exactly the elements it read -- so dz may be z.
// z and dz are not __restrict__ for that reason.  The losses of the workgroup's rows wait in LDS; with one workgroup
// (B <= 256) thread 0 adds them in ascending row order and writes the mean, otherwise cosine_mean_kernel does.
template <bool VEC>
__global__ __launch_bounds__(CL_T) void cosine_loss_kernel(const float* z, int ldz, const float* __restrict__ g, int ldg,
                                                           float* dz, float* __restrict__ loss_row,
                                                           float* __restrict__ cos_row, float* __restrict__ out, int B,
                                                           int G, float gscale) {
  __shared__ float lrow[CL_ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = blockIdx.x * CL_ROWS;
  const int nr = min(CL_ROWS, B - r0);
  for (int rr = w; rr < nr; rr += CL_T / 64) {
    const int r = r0 + rr;
    const float* zr = z + (long)r * ldz;
    const float* gr = g + (long)r * ldg;
    float szz, sgg, szg;
    sem_row_sums<VEC, true>(zr, gr, G, lane, szz, sgg, szg);
    const float inz = 1.f / sqrtf(fmaxf(szz, SEM_EPS));
    const float ing = 1.f / sqrtf(fmaxf(sgg, SEM_EPS));
    const float cs = (szg * inz) * ing;
    const float loss = 1.f - cs;
    if (lane == 0) {
      loss_row[r] = loss;
      cos_row[r] = cs;
      lrow[rr] = loss;
    }
    if (dz != nullptr) {
      // d cos / d z = (gn - cos zn) / nz; below the epsilon the normaliser is the constant 1e-6: gn / nz
      const float k = szz > SEM_EPS ? cs * inz : 0.f;
      const float s = -gscale * inz;
      float* dr = dz + (long)r * ldz;
      int j0 = 0;
      if (VEC) {
        const int G4 = G >> 2;
        for (int q = lane; q < G4; q += 64) {
          const float4 x = *reinterpret_cast<const float4*>(zr + 4 * q);
          const float4 y = *reinterpret_cast<const float4*>(gr + 4 * q);
          float4 d;
          d.x = s * (y.x * ing - k * x.x); d.y = s * (y.y * ing - k * x.y);
          d.z = s * (y.z * ing - k * x.z); d.w = s * (y.w * ing - k * x.w);
          *reinterpret_cast<float4*>(dr + 4 * q) = d;
        }
        j0 = G4 << 2;
      }
      for (int j = j0 + lane; j < G; j += 64) dr[j] = s * (gr[j] * ing - k * zr[j]);
    }
  }
  if (out == nullptr || gridDim.x != 1) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < nr; ++i) s += lrow[i];
    out[0] = s / (float)B;
  }
}

// B > 256: the mean of loss_row in ascending row order, one thread
__global__ void cosine_mean_kernel(const float* __restrict__ loss_row, float* __restrict__ out, int B) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = 0.f;
  for (int i = 0; i < B; ++i) s += loss_row[i];
  out[0] = s / (float)B;
}

// ---------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(RN_T) void row_inv_norm_kernel(const float* __restrict__ X, long ldx, float* __restrict__ inv,
                                                            long rows, int G) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (RN_T / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                      // (wave-uniform)
  float s, u0, u1;
  sem_row_sums<VEC, false>(X + r * ldx, nullptr, G, lane, s, u0, u1);
  if (lane == 0) inv[r] = 1.f / sqrtf(fmaxf(s, SEM_EPS));
}

// ---------------------------------------------------------------------------------------------------
// Selection.  The order is total: larger similarity first, equal similarities (-0 == +0) by ascending index, NaN below
// -inf and among themselves by ascending index.  One 64-bit key holds it: the high word is the similarity's bits made
// monotone (0 for NaN, which lies below -inf's 0x007fffff), the low word is ~index, so a larger key is an earlier rank and
// no two columns share a key.  Pass p finds the largest key strictly below the key of pass p - 1: k passes over a row that
// stays in the L2 (256 KB at M = 65 536), nothing kept between passes but that one key.  Why passes and not per-thread
// candidate lists: DESIGN.md.
__device__ __forceinline__ unsigned long long sem_key(float v, int m) {
  unsigned int hi;
  if (v != v) {
    hi = 0u;
  } else {
    const unsigned int u = __float_as_uint(v + 0.f);          // -0 -> +0: the two compare equal
    hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((unsigned long long)hi << 32) | (unsigned long long)(~(unsigned int)m);
}

__device__ __forceinline__ unsigned long long sem_wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned int lo = __shfl_xor((unsigned int)v, o, 64);
    const unsigned int hi = __shfl_xor((unsigned int)(v >> 32), o, 64);
    const unsigned long long t = ((unsigned long long)hi << 32) | lo;
    v = t > v ? t : v;
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(TK_T) void cosine_topk_kernel(const float* __restrict__ S, long lds,
                                                           const float* __restrict__ qinv, const float* __restrict__ binv,
                                                           int* __restrict__ idx, float* __restrict__ sim, int M, int k) {
  __shared__ unsigned long long sh[2][TK_W];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* row = S + (long)b * lds;
  const float qi = qinv[b];
  unsigned long long prev = ~0ull;            // above every key: ~index is never 0xffffffff with the high word at its maximum
  for (int p = 0; p < k; ++p) {
    unsigned long long best = 0ull;           // below every key: ~index >= 0x80000000 for index < 2^31
    int j0 = 0;
    if (VEC) {
      const int M4 = M >> 2;
      for (int q = t; q < M4; q += TK_T) {
        const float4 s = *reinterpret_cast<const float4*>(row + 4 * q);
        const float4 n = *reinterpret_cast<const float4*>(binv + 4 * q);
        const unsigned long long k0 = sem_key((s.x * qi) * n.x, 4 * q), k1 = sem_key((s.y * qi) * n.y, 4 * q + 1),
                                 k2 = sem_key((s.z * qi) * n.z, 4 * q + 2), k3 = sem_key((s.w * qi) * n.w, 4 * q + 3);
        if (k0 < prev && k0 > best) best = k0;
        if (k1 < prev && k1 > best) best = k1;
        if (k2 < prev && k2 > best) best = k2;
        if (k3 < prev && k3 > best) best = k3;
      }
      j0 = M4 << 2;
    }
    for (int j = j0 + t; j < M; j += TK_T) {
      const unsigned long long kk = sem_key((row[j] * qi) * binv[j], j);
      if (kk < prev && kk > best) best = kk;
    }
    best = sem_wave_max_u64(best);
    unsigned long long* s = sh[p & 1];        // alternating: a slow wave may still be combining the pass before
    if ((t & 63) == 0) s[t >> 6] = best;
    __syncthreads();
    best = s[0];
#pragma unroll
    for (int i = 1; i < TK_W; ++i) best = s[i] > best ? s[i] : best;
    if (t == 0) {
      const int m = (int)(~(unsigned int)best);           // k <= M: every pass finds a column
      idx[(long)b * k + p] = m;
      sim[(long)b * k + p] = (row[m] * qi) * binv[m];
    }
    prev = best;
  }
}
}  // namespace

extern "C" int32_t tnt_cosine_loss_f32(const float* z, int32_t ldz, const float* g, int32_t ldg, float* dz, float* loss_row,
                                       float* cos_row, float* out, int32_t B, int32_t G, float gscale, void* stream) {
  if (z == nullptr || g == nullptr || loss_row == nullptr || cos_row == nullptr) return TNT_BADARG(1);
  if (B <= 0) return TNT_BADARG(9);
  if (G <= 0 || G > 2048) return TNT_BADARG(10);
  if (ldz < G) return TNT_BADARG(2);
  if (ldg < G) return TNT_BADARG(4);
  const bool vec = tnt_aligned16(z) && tnt_aligned16(g) && (dz == nullptr || tnt_aligned16(dz)) && ldz % 4 == 0 && ldg % 4 == 0;
  const int nb = (B + CL_ROWS - 1) / CL_ROWS;
  hipLaunchKernelGGL(vec ? cosine_loss_kernel<true> : cosine_loss_kernel<false>, dim3(nb), dim3(CL_T), 0, tnt_stream(stream),
                     z, ldz, g, ldg, dz, loss_row, cos_row, out, B, G, gscale);
  TNT_LAUNCH_CHECK();
  if (out != nullptr && nb > 1) {
    hipLaunchKernelGGL(cosine_mean_kernel, dim3(1), dim3(64), 0, tnt_stream(stream), loss_row, out, B);
    TNT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int32_t tnt_row_inv_norm_f32(const float* X, int64_t ldx, float* inv, int64_t rows, int32_t G, void* stream) {
  if (X == nullptr || inv == nullptr) return TNT_BADARG(1);
  if (rows <= 0 || rows > (int64_t)0x7fffffff * (RN_T / 64)) return TNT_BADARG(4);
  if (G <= 0) return TNT_BADARG(5);
  if (ldx < G) return TNT_BADARG(2);
  const bool vec = tnt_aligned16(X) && ldx % 4 == 0;
  const unsigned nb = (unsigned)((rows + RN_T / 64 - 1) / (RN_T / 64));
  hipLaunchKernelGGL(vec ? row_inv_norm_kernel<true> : row_inv_norm_kernel<false>, dim3(nb), dim3(RN_T), 0, tnt_stream(stream),
                     X, (long)ldx, inv, (long)rows, G);
  TNT_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t tnt_cosine_topk_f32(const float* S, int64_t lds, const float* qinv, const float* binv, int32_t* idx,
                                       float* sim, int32_t B, int32_t M, int32_t k, void* stream) {
  if (S == nullptr || qinv == nullptr || binv == nullptr || idx == nullptr || sim == nullptr) return TNT_BADARG(1);
  if (B <= 0) return TNT_BADARG(7);
  if (M <= 0) return TNT_BADARG(8);
  if (k <= 0 || k > 64 || k > M) return TNT_BADARG(9);
  if (lds < M) return TNT_BADARG(2);
  const bool vec = tnt_aligned16(S) && tnt_aligned16(binv) && lds % 4 == 0;
  hipLaunchKernelGGL(vec ? cosine_topk_kernel<true> : cosine_topk_kernel<false>, dim3(B), dim3(TK_T), 0, tnt_stream(stream), S,
                     (long)lds, qinv, binv, idx, sim, M, k);
  TNT_LAUNCH_CHECK();
  return 0;
}
