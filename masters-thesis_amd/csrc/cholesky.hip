// Dense symmetric positive-definite solves for ridge decoding (masters_thesis_amd/ridge.py): the dual form of ridge
// regression from n scans to the sentence embedding needs (K + alpha I) A = Y with K the n x n Gram matrix of the scans.
// Definitions: include/tnt_hip.h.
//   tnt_cholesky_f32         L L^T = K + shift I, blocked left-looking at NB = 64: per block column one product on the
//                            library's own GEMM family (gemm3, no split) and one panel launch
//   tnt_cholesky_solve_f32   X <- L^-T L^-1 X in place: a forward and a backward sweep over the block rows, per step one
//                            product and one 64-row triangular launch
//   tnt_gram_center_f32      K <- H K H, H = I - 11^T/n, the row means kept for the caller
// No workgroup waits for another inside a launch (the launch boundary is the only synchronisation), no float atomics, every
// sum in a fixed order: the same input gives the same bits.  The 64 x 64 triangular work is done in float64 in LDS and
// rounded once; `status` (one int32 in device memory) carries the first bad pivot, and a launch that finds it nonzero returns
// before it touches anything else.
#include "tnt_common.h"

#include <math.h>

namespace {
constexpr int CH_NB = 64;            // block edge
constexpr int CH_T = 256;            // 4 waves: thread t owns column t & 63 of the 64 x 64 block, every 4th row from t >> 6
constexpr int CH_LD = CH_NB + 1;     // LDS row stride (in elements): a column walk touches every bank once
constexpr int GC_T = 256;            // gram_center: 4 waves
constexpr int GC_ROWS = 16;          // gram_center apply: rows per workgroup

// the one status read of a launch: thread 0 fetches the word, every thread of the workgroup takes the same answer
__device__ __forceinline__ bool ch_dead(const int* status, int* slot) {
  if (threadIdx.x == 0) *slot = *status;
  __syncthreads();
  return *slot != 0;
}

// Solves T Z = B in place for the 64 right-hand sides held as the COLUMNS of Bm ([i][c], stride CH_LD, float64); T = Lm
// (TRANS = false, forward substitution) or Lm^T (TRANS = true, backward), Lm the float32 lower factor, nb its order.  Step k
// leaves row k of Bm alone -- it is scaled by 1 / T_kk when it is used and, for the result, by ch_tri_scale afterwards -- so
// no thread writes what another reads inside a step; one barrier per step.  Rows i of a column go to its four threads as
// i = first + q, + 4, ...: a fixed order.
template <bool TRANS>
__device__ __forceinline__ void ch_tri_solve(double* Bm, const float* Lm, int nb, int t) {
  const int c = t & 63, q = t >> 6;
  for (int s = 0; s < nb; ++s) {
    const int k = TRANS ? nb - 1 - s : s;
    __syncthreads();
    const double x = Bm[k * CH_LD + c] / (double)Lm[k * CH_LD + k];
    if (TRANS) {
      for (int i = q; i < k; i += 4) Bm[i * CH_LD + c] -= (double)Lm[k * CH_LD + i] * x;
    } else {
      for (int i = k + 1 + q; i < nb; i += 4) Bm[i * CH_LD + c] -= (double)Lm[i * CH_LD + k] * x;
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// Panel of block column j0.  EVERY workgroup factors the diagonal block D = K[j0.., j0..] + shift I - P[0..] itself (the same
// arithmetic in the same order: the same bits everywhere), so that none has to wait for another; workgroup 0 stores L11,
// workgroup b >= 1 solves its 64 rows of L21 = (K21 - P21) L11^-T against the ROUNDED L11 (the factor that is stored).
// P (hasP) is the product L[j0:, :j0] L[j0:j0+64, :j0]^T, row r - j0, stride 64.
// The factorisation is right-looking inside the block, unscaled: step k subtracts a_ik a_jk / d_k, d_k = a_kk, from the
// trailing lower triangle and leaves column k as it is, so a step needs one barrier; L_ik = a_ik / sqrt(d_k) at the end.
__global__ __launch_bounds__(CH_T) void chol_panel_kernel(const float* __restrict__ K, long ldk, float* __restrict__ L,
                                                          long ldl, const float* __restrict__ P, int n, int j0, float shift,
                                                          int hasP, int* status) {
  __shared__ double Am[CH_NB * CH_LD];       // the diagonal block, then (b >= 1) the right-hand sides, transposed
  __shared__ float Lm[CH_NB * CH_LD];
  __shared__ int dead;
  if (ch_dead(status, &dead)) return;
  const int t = threadIdx.x;
  const int nb = min(CH_NB, n - j0);
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int i = e >> 6, j = e & 63;
    double v = i == j ? 1.0 : 0.0;
    if (i < nb && j <= i) {                  // the lower triangle only: K's strict upper triangle is never read
      v = (double)K[(long)(j0 + i) * ldk + j0 + j];
      if (i == j) v += (double)shift;
      if (hasP) v -= (double)P[i * CH_NB + j];
    }
    Am[i * CH_LD + j] = v;
  }
  int bad = -1;
  {
    const int i = t & 63, q = t >> 6;
    for (int k = 0; k < nb; ++k) {
      __syncthreads();
      const double d = Am[k * CH_LD + k];    // the same word for every thread: the branch is uniform
      const float lf = (float)sqrt(d);
      if (!(d > 0.0) || !(lf > 0.f) || isinf(lf)) { bad = k; break; }
      if (i > k && i < nb) {
        const double f = Am[i * CH_LD + k] / d;
        for (int j = k + 1 + q; j <= i; j += 4) Am[i * CH_LD + j] -= f * Am[j * CH_LD + k];
      }
    }
  }
  if (bad >= 0) {                            // every workgroup of the launch finds the same pivot; one of them files it
    if (blockIdx.x == 0 && t == 0) *status = 1 + j0 + bad;
    return;
  }
  __syncthreads();
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int i = e >> 6, k = e & 63;
    float v = i == k ? 1.f : 0.f;
    if (i < nb && k <= i) {
      const double s = sqrt(Am[k * CH_LD + k]);
      v = (float)(i == k ? s : Am[i * CH_LD + k] / s);
    }
    Lm[i * CH_LD + k] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
      const int i = e >> 6, k = e & 63;
      if (i < nb && k <= i) L[(long)(j0 + i) * ldl + j0 + k] = Lm[i * CH_LD + k];
    }
    return;
  }
  const int r0 = j0 + CH_NB * (int)blockIdx.x;          // nb == 64 here: there are rows below the block
  const int nr = min(CH_NB, n - r0);
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int r = e >> 6, c = e & 63;
    double v = 0.0;
    if (r < nr) {
      v = (double)K[(long)(r0 + r) * ldk + j0 + c];
      if (hasP) v -= (double)P[(long)(r0 - j0 + r) * CH_NB + c];
    }
    Am[c * CH_LD + r] = v;                   // transposed: row r of L21 is right-hand side r of L11 z = b
  }
  ch_tri_solve<false>(Am, Lm, CH_NB, t);
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int r = e >> 6, c = e & 63;
    if (r < nr) L[(long)(r0 + r) * ldl + j0 + c] = (float)(Am[c * CH_LD + r] / (double)Lm[c * CH_LD + c]);
  }
}

// ---------------------------------------------------------------------------------------------------
// One block row of a sweep: X[j0.., c0..] <- T^-1 (X[j0.., c0..] - P), T = L_jj (forward) or L_jj^T (backward), 64 columns
// of X per workgroup.  P (hasP): [nb][ldp], the product of the sweep's earlier block rows.
template <bool TRANS>
__global__ __launch_bounds__(CH_T) void chol_tri_kernel(const float* __restrict__ L, long ldl, float* __restrict__ X, long ldx,
                                                        const float* __restrict__ P, long ldp, int n, int j0, int G, int hasP,
                                                        const int* status) {
  __shared__ double Bm[CH_NB * CH_LD];
  __shared__ float Lm[CH_NB * CH_LD];
  __shared__ int dead;
  if (ch_dead(status, &dead)) return;
  const int t = threadIdx.x;
  const int nb = min(CH_NB, n - j0);
  const int c0 = CH_NB * (int)blockIdx.x;
  const int nc = min(CH_NB, G - c0);
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int i = e >> 6, k = e & 63;
    float l = i == k ? 1.f : 0.f;
    if (i < nb && k <= i) l = L[(long)(j0 + i) * ldl + j0 + k];        // the lower triangle only
    Lm[i * CH_LD + k] = l;
    double v = 0.0;                          // (here k is the column of X)
    if (i < nb && k < nc) {
      v = (double)X[(long)(j0 + i) * ldx + c0 + k];
      if (hasP) v -= (double)P[(long)i * ldp + c0 + k];
    }
    Bm[i * CH_LD + k] = v;
  }
  ch_tri_solve<TRANS>(Bm, Lm, nb, t);
  for (int e = t; e < CH_NB * CH_NB; e += CH_T) {
    const int i = e >> 6, c = e & 63;
    if (i < nb && c < nc) X[(long)(j0 + i) * ldx + c0 + c] = (float)(Bm[i * CH_LD + c] / (double)Lm[i * CH_LD + i]);
  }
}

// ---------------------------------------------------------------------------------------------------
// Gram centring.  Launch 1: one wave per row, lane l adds the float4 l, l + 64, ... (x, y, z, w in order) in float64, then the
// 64-lane butterfly; mean[i] = (float)(sum / n).  Launch 2: every workgroup forms the grand mean from mean[0..n) itself --
// thread t adds the entries t, t + 256, ... in float64, then a fixed tree over LDS: the same bits in every workgroup, nobody
// waits -- and rewrites its 16 rows: K_ij <- (float)((double)K_ij - m_i - m_j + g).  Workgroup 0 files g in mean[n].
__device__ __forceinline__ double gc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(GC_T) void gram_rowmean_kernel(const float* __restrict__ K, long ldk, int n, float* __restrict__ mean) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * (GC_T / 64) + (threadIdx.x >> 6);
  if (r >= n) return;                        // (wave-uniform)
  const float* row = K + (long)r * ldk;
  double s = 0.0;
  const int n4 = n >> 2;
  for (int q = lane; q < n4; q += 64) {
    const float4 x = *reinterpret_cast<const float4*>(row + 4 * q);
    s += (double)x.x; s += (double)x.y; s += (double)x.z; s += (double)x.w;
  }
  for (int j = (n4 << 2) + lane; j < n; j += 64) s += (double)row[j];
  s = gc_wave_sum(s);
  if (lane == 0) mean[r] = (float)(s / (double)n);
}

__global__ __launch_bounds__(GC_T) void gram_center_kernel(float* __restrict__ K, long ldk, int n, float* __restrict__ mean) {
  __shared__ double part[GC_T];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += GC_T) s += (double)mean[i];
  part[t] = s;
  __syncthreads();
  for (int o = GC_T / 2; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  const double g = part[0] / (double)n;
  if (blockIdx.x == 0 && t == 0) mean[n] = (float)g;      // nobody reads mean[n] in this launch
  const int r0 = (int)blockIdx.x * GC_ROWS;
  const int nr = min(GC_ROWS, n - r0);
  for (int rr = 0; rr < nr; ++rr) {
    float* row = K + (long)(r0 + rr) * ldk;
    const double mi = (double)mean[r0 + rr];
    for (int j = t; j < n; j += GC_T) row[j] = (float)((double)row[j] - mi - (double)mean[j] + g);
  }
}

// The product of a block step on the library's own family: gemm3 at the tile its cost model picks with the split
// forbidden (no exchange buffer, no workgroup waiting for a peer), or -- where gemm3's 32-bit operand offsets do not reach
// (rows x stride >= 2^29 floats) -- tnt_gemm_f32.  The choice depends on the shapes alone.
int32_t ch_product(bool g3, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int tA,
                   int tB, void* stream) {
  if (g3) {
    int32_t tile = 0, sk = 1;
    if (int32_t rc = tnt_gemm3_plan(M, N, K, tA, tB, 1, 0, &tile, &sk)) return rc;
    return tnt_gemm3_f32(A, B, C, nullptr, nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc, tA, tB, tile, 1, nullptr, nullptr,
                         nullptr, 0, stream);
  }
  return tnt_gemm_f32(A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, tA, tB, TNT_ACT_NONE, 0.f, 0, 1, nullptr, stream);
}

constexpr int CH_NMAX = 32768;
bool ch_g3_reach(long rows, long ld) { return rows * ld < (1L << 29); }
}  // namespace

extern "C" int32_t tnt_cholesky_f32(const float* K, int32_t ldk, float* L, int32_t ldl, int32_t n, float shift, float* work,
                                    int32_t* status, void* stream) {
  if (K == nullptr || !tnt_aligned16(K)) return TNT_BADARG(1);
  if (L == nullptr || !tnt_aligned16(L) || L == K) return TNT_BADARG(3);
  if (n < 1 || n > CH_NMAX) return TNT_BADARG(5);
  if (ldk < n || ldk % 4) return TNT_BADARG(2);
  if (ldl < n || ldl % 4) return TNT_BADARG(4);
  if (work == nullptr || !tnt_aligned16(work)) return TNT_BADARG(7);
  if (status == nullptr) return TNT_BADARG(8);
  hipStream_t s = tnt_stream(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return -(int32_t)hipGetLastError();
  const bool g3 = ch_g3_reach(n, ldl);
  for (int j0 = 0; j0 < n; j0 += CH_NB) {
    const int nb = n - j0 < CH_NB ? n - j0 : CH_NB;
    if (j0 > 0) {
      // P = L[j0:, :j0] L[j0:j0+nb, :j0]^T; both operands K-contiguous with K = j0, a multiple of 64: no stage reaches past K
      if (int32_t rc = ch_product(g3, L + (long)j0 * ldl, L + (long)j0 * ldl, work, n - j0, nb, j0, ldl, ldl, CH_NB, 0, 1, stream))
        return rc;
    }
    hipLaunchKernelGGL(chol_panel_kernel, dim3((n - j0 + CH_NB - 1) / CH_NB), dim3(CH_T), 0, s, K, (long)ldk, L, (long)ldl, work, n,
                       j0, shift, j0 > 0 ? 1 : 0, status);
    TNT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int32_t tnt_cholesky_solve_f32(const float* L, int32_t ldl, int32_t n, float* X, int32_t ldx, int32_t G, float* work,
                                          const int32_t* status, void* stream) {
  if (L == nullptr || !tnt_aligned16(L)) return TNT_BADARG(1);
  if (n < 1 || n > CH_NMAX) return TNT_BADARG(3);
  if (ldl < n || ldl % 4) return TNT_BADARG(2);
  if (X == nullptr || !tnt_aligned16(X)) return TNT_BADARG(4);
  if (G < 1) return TNT_BADARG(6);
  if (ldx < G || ldx % 4) return TNT_BADARG(5);
  if (work == nullptr || !tnt_aligned16(work)) return TNT_BADARG(7);
  if (status == nullptr) return TNT_BADARG(8);
  hipStream_t s = tnt_stream(stream);
  const bool g3 = ch_g3_reach(n, ldl) && ch_g3_reach(n, ldx);
  const dim3 grid((G + CH_NB - 1) / CH_NB);
  const int jlast = (n - 1) / CH_NB * CH_NB;
  for (int j0 = 0; j0 < n; j0 += CH_NB) {                 // L z = x, block rows ascending
    const int nb = n - j0 < CH_NB ? n - j0 : CH_NB;
    if (j0 > 0) {
      // P = L[j0:j0+nb, :j0] X[:j0]: A is K-contiguous with K = j0, a multiple of 64; X is N-contiguous
      if (int32_t rc = ch_product(g3, L + (long)j0 * ldl, X, work, nb, G, j0, ldl, ldx, ldx, 0, 0, stream)) return rc;
    }
    hipLaunchKernelGGL(chol_tri_kernel<false>, grid, dim3(CH_T), 0, s, L, (long)ldl, X, (long)ldx, work, (long)ldx, n, j0, G,
                       j0 > 0 ? 1 : 0, status);
    TNT_LAUNCH_CHECK();
  }
  for (int j0 = jlast; j0 >= 0; j0 -= CH_NB) {            // L^T a = z, block rows descending
    const int below = n - j0 - CH_NB;                     // rows under block row j0 (<= 0: the last one)
    if (below > 0) {
      // P = L[j0+64:, j0:j0+64]^T X[j0+64:]: A stored [K][ldl], M-contiguous; X N-contiguous: no K-contiguous operand at all
      if (int32_t rc = ch_product(g3, L + (long)(j0 + CH_NB) * ldl + j0, X + (long)(j0 + CH_NB) * ldx, work, CH_NB, G, below, ldl,
                                  ldx, ldx, 1, 0, stream))
        return rc;
    }
    hipLaunchKernelGGL(chol_tri_kernel<true>, grid, dim3(CH_T), 0, s, L, (long)ldl, X, (long)ldx, work, (long)ldx, n, j0, G,
                       below > 0 ? 1 : 0, status);
    TNT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int32_t tnt_gram_center_f32(float* K, int32_t ldk, int32_t n, float* mean, void* stream) {
  if (K == nullptr || !tnt_aligned16(K)) return TNT_BADARG(1);
  if (n < 1 || n > CH_NMAX) return TNT_BADARG(3);
  if (ldk < n || ldk % 4) return TNT_BADARG(2);
  if (mean == nullptr) return TNT_BADARG(4);
  hipStream_t s = tnt_stream(stream);
  hipLaunchKernelGGL(gram_rowmean_kernel, dim3((n + GC_T / 64 - 1) / (GC_T / 64)), dim3(GC_T), 0, s, K, (long)ldk, n, mean);
  TNT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_center_kernel, dim3((n + GC_ROWS - 1) / GC_ROWS), dim3(GC_T), 0, s, K, (long)ldk, n, mean);
  TNT_LAUNCH_CHECK();
  return 0;
}
