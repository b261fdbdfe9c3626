// The contrastive (CLIP-style, in-batch negatives) form of nic.NIC's sentence-embedding target: tnt_contrastive_loss_f32.
// Definition: include/tnt_hip.h.  Phases, each its own launch on the one stream (a phase that needs another's result is
// another launch; no workgroup waits for another):
//   ct_logits_kernel   16 x 16 tiles of L = (zn . gn) / temperature and, soft, of the target Gram S; the squared norms
//   ct_stats_kernel    one wave per row: row / column / target log-sum-exp, the row's loss and hit
//   ct_grad_kernel     one workgroup per row: dL's row into LDS, the dL-weighted sum of target rows, the l2 backward
//   ct_mean_kernel     the two means in ascending row order
// Everything is float32 with a fixed summation order that does not depend on the grid, and no float atomics: two runs
// give the same bits.  Plain FMAs and not the MFMA 16x16x4 f32: why is in DESIGN.md.
#include "tnt_common.h"

namespace {
constexpr float CT_EPS = 1e-12f;     // as SEM_EPS of semantic.hip
constexpr int CT_TILE = 16;          // logits: a workgroup of 256 threads owns a 16 x 16 tile, one element per thread
constexpr int CT_KC = 64;            // ... and walks G in chunks of 64 columns staged in LDS
constexpr int CT_LD = CT_KC + 4;     // 68 floats a row: 16-byte aligned, and 16 rows fall on 16 different 4-bank slots
constexpr int CT_T = 256;
constexpr int CT_MAXB = 1024;

__device__ __forceinline__ float ct_inv_norm(float ss) { return 1.f / sqrtf(fmaxf(ss, CT_EPS)); }

// ---------------------------------------------------------------------------------------------------
// Logits.  blockIdx = (column tile, row tile, plane).  Plane 0: A = z, L[i][j] = ((z_i . g_j) iz_i) ig_j inv_t.  Plane 1
// (soft targets): A = g, S[i][j] = ((g_i . g_j) (ig_i ig_j)) soft_inv_t, the same bits as S[j][i].  Every thread adds its
// products in ascending column order with one accumulator, and beside them sum a^2 of its row and sum g^2 of its column
// the same way: the norms of a row are the same bits in every tile, and the tiles of column tile 0 / row tile 0 write them
// out (szz from plane 0, sgg from plane 0).  Rows >= B and columns >= G are staged as 0 and never read from memory (the
// load's row and column are clamped into the matrix).
__global__ __launch_bounds__(CT_T) void ct_logits_kernel(const float* z, int ldz, const float* __restrict__ g, int ldg,
                                                         float* __restrict__ szz, float* __restrict__ sgg,
                                                         float* __restrict__ L, float* __restrict__ S, int B, int G,
                                                         float inv_t, float soft_inv_t) {
  __shared__ __attribute__((aligned(16))) float as[CT_TILE][CT_LD];
  __shared__ __attribute__((aligned(16))) float bs[CT_TILE][CT_LD];
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
  const int i0 = blockIdx.y * CT_TILE, j0 = blockIdx.x * CT_TILE;
  const bool soft = blockIdx.z == 1;
  const float* A = soft ? g : z;
  const int lda = soft ? ldg : ldz;
  float acc = 0.f, saa = 0.f, sbb = 0.f;
  // thread t stages the elements t, t + 256, ... of the 16 x 64 chunk: row e >> 6, column e & 63.  The next chunk's loads
  // are issued into registers before the current chunk's products, so their latency hides behind the FMAs.
  constexpr int NE = CT_TILE * CT_KC / CT_T;
  float ra[NE], rb[NE];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = t + u * CT_T, r = e >> 6, k = e & 63;
      const bool kin = k0 + k < G;                      // unconditional loads from clamped (row, column), then the select
      const int kc = min(k0 + k, G - 1);
      const float a = A[(long)min(i0 + r, B - 1) * lda + kc];
      const float b = g[(long)min(j0 + r, B - 1) * ldg + kc];
      ra[u] = (kin && i0 + r < B) ? a : 0.f;
      rb[u] = (kin && j0 + r < B) ? b : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < G; k0 += CT_KC) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = t + u * CT_T;
      as[e >> 6][e & 63] = ra[u];
      bs[e >> 6][e & 63] = rb[u];
    }
    __syncthreads();
    if (k0 + CT_KC < G) fetch(k0 + CT_KC);
#pragma unroll
    for (int k = 0; k < CT_KC; k += 4) {
      const float4 a = *reinterpret_cast<const float4*>(&as[ti][k]);
      const float4 b = *reinterpret_cast<const float4*>(&bs[tj][k]);
      acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
      saa = fmaf(a.x, a.x, saa); saa = fmaf(a.y, a.y, saa); saa = fmaf(a.z, a.z, saa); saa = fmaf(a.w, a.w, saa);
      sbb = fmaf(b.x, b.x, sbb); sbb = fmaf(b.y, b.y, sbb); sbb = fmaf(b.z, b.z, sbb); sbb = fmaf(b.w, b.w, sbb);
    }
    __syncthreads();
  }
  const int i = i0 + ti, j = j0 + tj;
  if (i >= B || j >= B) return;
  if (soft) {
    S[i * B + j] = (acc * (ct_inv_norm(saa) * ct_inv_norm(sbb))) * soft_inv_t;
    return;
  }
  L[i * B + j] = ((acc * ct_inv_norm(saa)) * ct_inv_norm(sbb)) * inv_t;
  if (blockIdx.x == 0 && tj == 0) szz[i] = saa;
  if (blockIdx.y == 0 && ti == 0) sgg[j] = sbb;
}

// ---------------------------------------------------------------------------------------------------
// Row statistics.  One wave per row i; lane l takes the columns l, l + 64, ... in ascending order, then the 64-lane
// butterfly.  Only valid columns (sum g_j^2 > eps) take part; an invalid row writes zeros.  lse_c is formed only for the
// symmetric loss, lse_q only with soft targets.
__global__ __launch_bounds__(CT_T) void ct_stats_kernel(const float* __restrict__ sgg, const float* __restrict__ L,
                                                        const float* __restrict__ S, float* __restrict__ lse_r,
                                                        float* __restrict__ lse_c, float* __restrict__ lse_q,
                                                        float* __restrict__ loss_row, int* __restrict__ hit_row, int B,
                                                        int soft, int symmetric) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (CT_T / 64) + (threadIdx.x >> 6);
  if (i >= B) return;                                   // (wave-uniform)
  if (!(sgg[i] > CT_EPS)) {
    if (lane == 0) { lse_r[i] = 0.f; lse_c[i] = 0.f; lse_q[i] = 0.f; loss_row[i] = 0.f; hit_row[i] = 0; }
    return;
  }
  const float* Lr = L + i * B;
  const float* Sr = S + i * B;                          // (read only when soft)
  float mr = -INFINITY, mc = -INFINITY, mq = -INFINITY;
  int arg = 0x7fffffff;
  for (int j = lane; j < B; j += 64) {
    if (!(sgg[j] > CT_EPS)) continue;
    const float l = Lr[j];
    if (l > mr || arg == 0x7fffffff) { mr = l; arg = j; }         // the first maximum of the lane's ascending columns
    if (symmetric) mc = fmaxf(mc, L[j * B + i]);
    if (soft) mq = fmaxf(mq, Sr[j]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                    // the first maximum over the wave: larger value, then smaller column
    const float v = __shfl_xor(mr, o, 64);
    const int a = __shfl_xor(arg, o, 64);
    if (a != 0x7fffffff && (arg == 0x7fffffff || v > mr || (v == mr && a < arg))) { mr = v; arg = a; }
  }
  if (symmetric) mc = tnt_wave_max(mc);
  if (soft) mq = tnt_wave_max(mq);
  float sr = 0.f, sc = 0.f, sq = 0.f, qa = 0.f, qb = 0.f;
  for (int j = lane; j < B; j += 64) {
    if (!(sgg[j] > CT_EPS)) continue;
    const float l = Lr[j];
    const float c = symmetric ? L[j * B + i] : 0.f;
    sr += expf(l - mr);
    if (symmetric) sc += expf(c - mc);
    if (soft) {
      const float e = expf(Sr[j] - mq);
      sq += e;
      qa = fmaf(e, l, qa);
      qb = fmaf(e, c, qb);
    }
  }
  sr = tnt_wave_sum(sr);
  const float lr_ = mr + logf(sr);
  float lc_ = 0.f, lq_ = 0.f, tr = Lr[i], tc = Lr[i];   // hard targets: Q = [i == j]
  if (symmetric) lc_ = mc + logf(tnt_wave_sum(sc));
  if (soft) {
    sq = tnt_wave_sum(sq); qa = tnt_wave_sum(qa); qb = tnt_wave_sum(qb);
    lq_ = mq + logf(sq);
    tr = qa / sq; tc = qb / sq;                         // sum_j Q_ij L_ij and sum_j Q_ij L_ji
  }
  if (lane == 0) {
    lse_r[i] = lr_; lse_c[i] = lc_; lse_q[i] = lq_;
    loss_row[i] = symmetric ? 0.5f * ((lr_ - tr) + (lc_ - tc)) : lr_ - tr;
    hit_row[i] = arg == i ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------
// Gradient.  Workgroup i owns row i of dz.  Thread t forms coef[j] = dL_ij ig_j inv_t for j = t, t + 256, ... into LDS
// (0 for an invalid j), then owns the columns t, t + 256, ... (NQ of them) and adds coef[j] g_j over ascending j, one
// accumulator per column; zn . dzn by the wave butterfly and the four waves in order; then the l2 backward.  Each
// element of z is read, then the same element of dz written, by the same thread, and no other workgroup reads row i of
// z: dz may be z.
template <int NQ>
__global__ __launch_bounds__(CT_T) void ct_grad_kernel(const float* z, int ldz, const float* __restrict__ g, int ldg,
                                                       float* dz, const float* __restrict__ szz,
                                                       const float* __restrict__ sgg, const float* __restrict__ L,
                                                       const float* __restrict__ S, const float* __restrict__ lse_r,
                                                       const float* __restrict__ lse_c, const float* __restrict__ lse_q,
                                                       int B, int G, float inv_t, int soft, int symmetric, float weight) {
  __shared__ float coef[CT_MAXB];
  __shared__ int cnt[CT_T / 64];
  __shared__ float red[CT_T / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = blockIdx.x;
  float* dr = dz + (long)i * ldz;
  if (!(sgg[i] > CT_EPS)) {                             // an invalid row: no gradient  (workgroup-uniform)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (q * CT_T + t < G) dr[q * CT_T + t] = 0.f;
    return;
  }
  int n = 0;
  for (int j = t; j < B; j += CT_T) n += sgg[j] > CT_EPS ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) cnt[w] = n;
  __syncthreads();
  const int Bv = cnt[0] + cnt[1] + cnt[2] + cnt[3];     // >= 1: row i is valid
  const float scale = weight / (float)Bv;
  const float bcol = symmetric ? 0.5f : 0.f, brow = 1.f - bcol;
  const float lri = lse_r[i], lqi = lse_q[i];
  for (int j = t; j < B; j += CT_T) {
    float c = 0.f;
    const float sg = sgg[j];
    if (sg > CT_EPS) {
      const float l = L[i * B + j];
      float d = brow * expf(l - lri);
      if (symmetric) d = fmaf(bcol, expf(l - lse_c[j]), d);
      if (soft) {
        const float s = S[i * B + j];                   // (= S[j][i], bit for bit)
        float qq = brow * expf(s - lqi);
        if (symmetric) qq = fmaf(bcol, expf(s - lse_q[j]), qq);
        d -= qq;
      } else if (j == i) {
        d -= 1.f;
      }
      c = ((d * scale) * inv_t) * ct_inv_norm(sg);
    }
    coef[j] = c;
  }
  __syncthreads();
  float acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
  // No branch in the loop, so that the loads of several rows are in flight together: a column past G is clamped to
  // G - 1 (read again, its sum never stored), and a row with coef 0 (an invalid target, whose values may be anything)
  // contributes an exact 0.
  int col[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) col[q] = min(q * CT_T + t, G - 1);
#pragma unroll 8
  for (int j = 0; j < B; ++j) {
    const float c = coef[j];
    const float* gr = g + (long)j * ldg;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float x = gr[col[q]];
      acc[q] = fmaf(c, c != 0.f ? x : 0.f, acc[q]);
    }
  }
  const float sz = szz[i];
  const float iz = ct_inv_norm(sz);
  const float* zr = z + (long)i * ldz;
  float zn[NQ];
  float dot = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    zn[q] = q * CT_T + t < G ? zr[q * CT_T + t] * iz : 0.f;
    dot = fmaf(zn[q], acc[q], dot);
  }
  dot = tnt_wave_sum(dot);
  if (lane == 0) red[w] = dot;
  __syncthreads();
  // below the epsilon the normaliser is the constant 1e-6: dz = iz dzn
  const float k = sz > CT_EPS ? ((red[0] + red[1]) + red[2]) + red[3] : 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q * CT_T + t < G) dr[q * CT_T + t] = iz * (acc[q] - zn[q] * k);
}

// ---------------------------------------------------------------------------------------------------
// out[0] = (sum_i loss_row[i]) / max(Bv, 1), out[1] = (sum_i hit_row[i]) / max(Bv, 1): the rows through LDS, then one
// thread adds them in ascending order.
__global__ __launch_bounds__(CT_T) void ct_mean_kernel(const float* __restrict__ sgg, const float* __restrict__ loss_row,
                                                       const int* __restrict__ hit_row, float* __restrict__ out, int B) {
  __shared__ float ls[CT_MAXB];
  __shared__ short hs[CT_MAXB], vs[CT_MAXB];
  for (int i = threadIdx.x; i < B; i += CT_T) {
    ls[i] = loss_row[i];
    hs[i] = (short)hit_row[i];
    vs[i] = sgg[i] > CT_EPS ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float s = 0.f, h = 0.f;
  int bv = 0;
  for (int i = 0; i < B; ++i) { s += ls[i]; h += (float)hs[i]; bv += vs[i]; }
  const float den = (float)max(bv, 1);
  out[0] = s / den;
  out[1] = h / den;
}
}  // namespace

extern "C" int32_t tnt_contrastive_loss_f32(const float* z, int32_t ldz, const float* g, int32_t ldg, float* dz, float* work,
                                            float* loss_row, int32_t* hit_row, float* out, int32_t B, int32_t G,
                                            float inv_temperature, float soft_inv_temperature, int32_t symmetric, float weight,
                                            void* stream) {
  if (z == nullptr || g == nullptr || work == nullptr || loss_row == nullptr || hit_row == nullptr) return TNT_BADARG(1);
  if (B <= 0 || B > CT_MAXB) return TNT_BADARG(10);
  if (G <= 0 || G > 2048) return TNT_BADARG(11);
  if (ldz < G) return TNT_BADARG(2);
  if (ldg < G) return TNT_BADARG(4);
  if (!(inv_temperature > 0.f) || inv_temperature > 3.0e38f) return TNT_BADARG(12);
  if (!(soft_inv_temperature >= 0.f) || soft_inv_temperature > 3.0e38f) return TNT_BADARG(13);
  if (symmetric != 0 && symmetric != 1) return TNT_BADARG(14);
  if (!(weight >= 0.f) || weight > 3.0e38f) return TNT_BADARG(15);
  const int soft = soft_inv_temperature > 0.f ? 1 : 0;
  // work: szz [B], sgg [B], lse_r [B], lse_c [B], lse_q [B], L [B][B], (soft) S [B][B] -- TNT_CONTRASTIVE_WORK_FLOATS
  float* szz = work;
  float* sgg = szz + B;
  float* lse_r = sgg + B;
  float* lse_c = lse_r + B;
  float* lse_q = lse_c + B;
  float* L = lse_q + B;
  float* S = soft ? L + (size_t)B * B : L;              // (hard targets: never read)
  hipStream_t st = tnt_stream(stream);
  const int nt = (B + CT_TILE - 1) / CT_TILE;
  hipLaunchKernelGGL(ct_logits_kernel, dim3(nt, nt, soft ? 2 : 1), dim3(CT_T), 0, st, z, ldz, g, ldg, szz, sgg, L, S, B, G,
                     inv_temperature, soft_inv_temperature);
  TNT_LAUNCH_CHECK();
  hipLaunchKernelGGL(ct_stats_kernel, dim3((B + CT_T / 64 - 1) / (CT_T / 64)), dim3(CT_T), 0, st, sgg, L, S, lse_r, lse_c,
                     lse_q, loss_row, hit_row, B, soft, symmetric);
  TNT_LAUNCH_CHECK();
  if (dz != nullptr) {
    const int nq = (G + CT_T - 1) / CT_T;
    auto kern = nq <= 1 ? ct_grad_kernel<1> : nq <= 2 ? ct_grad_kernel<2> : nq <= 4 ? ct_grad_kernel<4> : ct_grad_kernel<8>;
    hipLaunchKernelGGL(kern, dim3(B), dim3(CT_T), 0, st, z, ldz, g, ldg, dz, szz, sgg, L, S, lse_r, lse_c, lse_q, B, G,
                       inv_temperature, soft, symmetric, weight);
    TNT_LAUNCH_CHECK();
  }
  if (out != nullptr) {
    hipLaunchKernelGGL(ct_mean_kernel, dim3(1), dim3(CT_T), 0, st, sgg, loss_row, hit_row, out, B);
    TNT_LAUNCH_CHECK();
  }
  return 0;
}
