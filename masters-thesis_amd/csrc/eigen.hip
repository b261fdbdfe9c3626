// Symmetric eigensolver of order <= 128 for PCA of the scans (masters_thesis_amd/pca.py): block subspace iteration on the
// n x n Gram matrix needs, per iteration, the eigenvectors of an m x m Ritz matrix and the matrix that orthonormalises a
// block of m columns from their Gram matrix.  Definitions: include/tnt_hip.h.
//   tnt_syev_jacobi_f32   all eigenvalues and eigenvectors of a symmetric float32 matrix, cyclic Jacobi
//   tnt_gram_whiten_f32   M with (Z M)^T (Z M) = I from S = Z^T Z: the same kernel, S scaled to unit diagonal on load and the
//                         eigenvectors scaled by diag(r) . diag(w^-1/2) on store
// One launch of ONE workgroup of 16 waves.  A and V live in LDS in float32 at a row stride of 129 floats, so that a walk down
// a column (lanes over rows: bank = (row + column) mod 32) and a walk along a row (lanes over columns) both touch every bank
// once per 32 lanes.  A round of the round-robin ordering has floor(m / 2) disjoint pairs and three barriers:
//   1. wave 0, lane k: pair k of the round, its rotate / skip decision, (c, s) and the two new diagonal entries in float64,
//      rounded once; the ballot of the decisions tells every wave whether the round has any work      -- barrier
//   2. A <- A J: wave w takes the pairs w, w + 16, ...; its lanes walk down the two columns           -- barrier
//   3. A <- J^T A: the lanes walk along the two rows; the 2 x 2 block gets (a_pp', 0; 0, a_qq') as computed in phase 1;
//      V <- V J by the same wave, down the two columns of V                                            -- barrier
// A round in which no pair rotates costs the first barrier alone.  Both triangles of A are kept and updated; decisions read
// the lower one.  No atomics, no scratch, every sum in a fixed order: the same input gives the same bits.
#include "tnt_common.h"

#include <math.h>

namespace {
constexpr int EJ_M = 128;             // largest order
constexpr int EJ_LD = EJ_M + 1;       // LDS row stride in floats
constexpr int EJ_T = 1024;            // 16 waves
constexpr int EJ_W = EJ_T / 64;
constexpr int EJ_P = EJ_M / 2;        // pairs per round at the most
constexpr double EJ_U = 5.9604644775390625e-08;      // 2^-24

// the dynamic LDS of the one workgroup, carved in this order (doubles first where alignment asks for it)
struct EjLds {
  float A[EJ_M * EJ_LD];
  float V[EJ_M * EJ_LD];
  double part[EJ_M];                  // row sums of squares at load; the column factors (sign x scale) at store
  double r[EJ_M];                     // whiten: 1 / sqrt(S_jj), 0 for a dropped column
  double thr;                         // 2^-24 ||A||_F / sqrt(m)
  float c[EJ_P], s[EJ_P], dp[EJ_P], dq[EJ_P];
  int p[EJ_P], q[EJ_P];               // p < 0: the pair is skipped
  float w[EJ_M], wsort[EJ_M];
  int perm[EJ_M];
  int bad, rank;
  int round_any[2], sweep_any[2];
};
static_assert(sizeof(EjLds) <= 160 * 1024, "one CU's LDS");

__device__ __forceinline__ void ej_rotate(float* x, float* y, float c, float s) {
  const float a = *x, b = *y;
  *x = fmaf(c, a, -(s * b));
  *y = fmaf(s, a, c * b);
}

__global__ __launch_bounds__(EJ_T) void jacobi_kernel(const float* __restrict__ Ain, long lda, int m, float* __restrict__ wout,
                                                      float* __restrict__ Vout, long ldv, int max_sweeps, int whiten, float tau,
                                                      int* __restrict__ info) {
  extern __shared__ __align__(16) unsigned char ej_raw[];
  EjLds& L = *reinterpret_cast<EjLds*>(ej_raw);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // ---- load: the lower triangle, mirrored; whiten scales it to unit diagonal in float64, rounded once
  if (t == 0) L.bad = 0;
  if (t < m) {
    double r = 1.0;
    if (whiten) {
      const float d = Ain[(long)t * lda + t];
      r = (isfinite(d) && d > 0.f) ? 1.0 / sqrt((double)d) : 0.0;
    }
    L.r[t] = r;
  }
  __syncthreads();
  bool bad = false;
  for (int i = wave; i < m; i += EJ_W) {
    const double ri = L.r[i];
    for (int j = lane; j < m; j += 64) {
      L.V[i * EJ_LD + j] = i == j ? 1.f : 0.f;
      if (j <= i) {
        float v = Ain[(long)i * lda + j];
        bad |= !isfinite(v);
        if (whiten) v = (float)((double)v * ri * L.r[j]);
        L.A[i * EJ_LD + j] = v;
        L.A[j * EJ_LD + i] = v;
      }
    }
  }
  if (bad) L.bad = 1;                        // every writer stores the same word
  __syncthreads();
  if (L.bad) {                               // (uniform) w and V are not touched
    if (t == 0) { info[0] = 2; info[1] = 0; info[2] = whiten ? 0 : m; }
    return;
  }
  if (t < m) {                               // ||A||_F: row t left to right in float64, then the rows top to bottom
    double s = 0.0;
    for (int j = 0; j < m; ++j) { const double v = (double)L.A[t * EJ_LD + j]; s += v * v; }
    L.part[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += L.part[i];
    L.thr = EJ_U * sqrt(s) / sqrt((double)m);
  }
  __syncthreads();

  // ---- sweeps.  The circle method over n2 = m rounded up to even: player n1 = n2 - 1 stays, the others turn; for odd m
  // that player is the bye, so a round has floor(m / 2) pairs and a sweep has m rounds (m - 1 for even m).
  const int n2 = m + (m & 1), n1 = n2 - 1, nslots = n2 >> 1, nrounds = m > 1 ? n1 : 0;
  int sweeps = 0, converged = 0, g = 0;      // g: rounds since the start, the parity of the flag slots
  while (sweeps < max_sweeps) {
    ++sweeps;
    if (nrounds == 0) { converged = 1; break; }
    unsigned long long swept = 0;            // (wave 0) the ballots of this sweep
    for (int r = 0; r < nrounds; ++r, ++g) {
      if (wave == 0) {
        bool go = false;
        int lo = 0, hi = 0;
        float c = 1.f, s = 0.f, dp = 0.f, dq = 0.f;
        if (lane < nslots) {
          int a = r, b = n1;
          if (lane > 0) {
            a = r + lane; if (a >= n1) a -= n1;
            b = r - lane; if (b < 0) b += n1;
          }
          lo = min(a, b); hi = max(a, b);
          if (hi < m) {
            const double app = (double)L.A[lo * EJ_LD + lo], aqq = (double)L.A[hi * EJ_LD + hi];
            const double apq = (double)L.A[hi * EJ_LD + lo];
            const double mag = fabs(apq);
            go = mag > EJ_U * sqrt(fabs(app * aqq)) && mag > L.thr;
            if (go) {
              const double th = (aqq - app) / (2.0 * apq);
              const double tn = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
              const double cd = 1.0 / sqrt(1.0 + tn * tn);
              c = (float)cd; s = (float)(tn * cd);
              dp = (float)(app - tn * apq); dq = (float)(aqq + tn * apq);
            }
          }
        }
        L.p[lane] = go ? lo : -1; L.q[lane] = hi;      // (64 lanes, EJ_P slots)
        L.c[lane] = c; L.s[lane] = s; L.dp[lane] = dp; L.dq[lane] = dq;
        const unsigned long long any = __ballot(go);
        swept |= any;
        if (lane == 0) {
          L.round_any[g & 1] = any != 0;
          if (r == nrounds - 1) L.sweep_any[sweeps & 1] = swept != 0;
        }
      }
      __syncthreads();
      if (!L.round_any[g & 1]) continue;     // (uniform) nothing rotates in this round
      for (int k = wave; k < nslots; k += EJ_W) {
        const int p = L.p[k];
        if (p < 0) continue;                 // (wave-uniform)
        const int q = L.q[k];
        const float c = L.c[k], s = L.s[k];
        for (int i = lane; i < m; i += 64) ej_rotate(&L.A[i * EJ_LD + p], &L.A[i * EJ_LD + q], c, s);
      }
      __syncthreads();
      for (int k = wave; k < nslots; k += EJ_W) {
        const int p = L.p[k];
        if (p < 0) continue;
        const int q = L.q[k];
        const float c = L.c[k], s = L.s[k], dp = L.dp[k], dq = L.dq[k];
        for (int j = lane; j < m; j += 64) {
          const float a = L.A[p * EJ_LD + j], b = L.A[q * EJ_LD + j];
          float x = fmaf(c, a, -(s * b)), y = fmaf(s, a, c * b);
          if (j == p) { x = dp; y = 0.f; }
          if (j == q) { x = 0.f; y = dq; }
          L.A[p * EJ_LD + j] = x;
          L.A[q * EJ_LD + j] = y;
        }
        for (int i = lane; i < m; i += 64) ej_rotate(&L.V[i * EJ_LD + p], &L.V[i * EJ_LD + q], c, s);
      }
      __syncthreads();
    }
    if (!L.sweep_any[sweeps & 1]) { converged = 1; break; }
  }

  // ---- descending order, ties by the column they came from; the sign rule; the store
  __syncthreads();
  if (t < m) { L.w[t] = L.A[t * EJ_LD + t]; L.perm[t] = t; }      // (a NaN of an overflow leaves ranks unassigned: stay in range)
  __syncthreads();
  if (t < m) {
    const float wi = L.w[t];
    int rank = 0;
    for (int j = 0; j < m; ++j) {
      const float wj = L.w[j];
      rank += (wj > wi || (wj == wi && j < t)) ? 1 : 0;
    }
    L.perm[rank] = t;
    L.wsort[rank] = wi;
  }
  __syncthreads();
  if (t < m) {
    const int col = L.perm[t];
    float best = -1.f, at = 0.f;
    for (int i = 0; i < m; ++i) {
      const float v = L.V[i * EJ_LD + col];
      if (fabsf(v) > best) { best = fabsf(v); at = v; }
    }
    double f = at < 0.f ? -1.0 : 1.0;
    if (whiten) {
      const double den = fmax((double)L.wsort[t], (double)tau * (double)L.wsort[0]);
      f *= den > 0.0 ? 1.0 / sqrt(den) : 0.0;
    }
    L.part[t] = f;
    wout[t] = L.wsort[t];
  }
  if (t == 0 && whiten) {
    int rank = 0;
    const double cut = (double)tau * (double)L.wsort[0];
    for (int i = 0; i < m; ++i) rank += (double)L.wsort[i] > cut ? 1 : 0;
    L.rank = rank;
  }
  __syncthreads();
  for (int i = wave; i < m; i += EJ_W) {
    const double ri = whiten ? L.r[i] : 1.0;
    for (int j = lane; j < m; j += 64)
      Vout[(long)i * ldv + j] = (float)((double)L.V[i * EJ_LD + L.perm[j]] * L.part[j] * ri);
  }
  if (t == 0) { info[0] = converged ? 0 : 1; info[1] = sweeps; info[2] = whiten ? L.rank : m; }
}

int32_t ej_launch(const float* A, int lda, int m, float* w, float* V, int ldv, int max_sweeps, int whiten, float tau, int32_t* info,
                  void* stream) {
  // asked for at every launch: the attribute belongs to the current device, and a call costs microseconds beside a solve
  if (hipFuncSetAttribute((const void*)jacobi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(EjLds)) != hipSuccess)
    return TNT_BADARG(90);
  hipLaunchKernelGGL(jacobi_kernel, dim3(1), dim3(EJ_T), sizeof(EjLds), tnt_stream(stream), A, (long)lda, m, w, V, (long)ldv,
                     max_sweeps, whiten, tau, info);
  TNT_LAUNCH_CHECK();
  return 0;
}

constexpr int EJ_SWEEPS_MAX = 64;
bool ej_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
}  // namespace

extern "C" int32_t tnt_syev_jacobi_f32(const float* A, int32_t lda, int32_t m, float* w, float* V, int32_t ldv, int32_t max_sweeps,
                                       int32_t* info, void* stream) {
  if (A == nullptr || !tnt_aligned16(A)) return TNT_BADARG(1);
  if (m < 1 || m > EJ_M) return TNT_BADARG(3);
  if (lda < m || lda % 4) return TNT_BADARG(2);
  if (w == nullptr || !ej_aligned4(w)) return TNT_BADARG(4);
  if (V == nullptr || !tnt_aligned16(V)) return TNT_BADARG(5);
  if (ldv < m || ldv % 4) return TNT_BADARG(6);
  if (max_sweeps < 1 || max_sweeps > EJ_SWEEPS_MAX) return TNT_BADARG(7);
  if (info == nullptr || !ej_aligned4(info)) return TNT_BADARG(8);
  if (V == A) return TNT_BADARG(9);
  return ej_launch(A, lda, m, w, V, ldv, max_sweeps, 0, 0.f, info, stream);
}

extern "C" int32_t tnt_gram_whiten_f32(const float* S, int32_t lds, int32_t m, float* M, int32_t ldm, float tau, float* w,
                                       int32_t* info, void* stream) {
  if (S == nullptr || !tnt_aligned16(S)) return TNT_BADARG(1);
  if (m < 1 || m > EJ_M) return TNT_BADARG(3);
  if (lds < m || lds % 4) return TNT_BADARG(2);
  if (M == nullptr || !tnt_aligned16(M)) return TNT_BADARG(4);
  if (ldm < m || ldm % 4) return TNT_BADARG(5);
  if (!(tau > 0.f && tau < 1.f)) return TNT_BADARG(6);
  if (w == nullptr || !ej_aligned4(w)) return TNT_BADARG(7);
  if (info == nullptr || !ej_aligned4(info)) return TNT_BADARG(8);
  if (M == S) return TNT_BADARG(9);
  return ej_launch(S, lds, m, w, M, ldm, EJ_SWEEPS_MAX, 1, tau, info, stream);
}
