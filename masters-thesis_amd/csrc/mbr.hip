// Minimum Bayes risk caption selection (tnt_mbr_select_f32; the definition is in include/tnt_hip.h): of the Nc candidate
// captions of a scan the one with the highest expected n-gram utility against the first Nr of them.
//
// One workgroup of 256 threads per scan b:
//   0. stage: the scan's Nc x L tokens go to LDS once (row stride L_MAX + 1 words: the rows of different candidates start
//      in different banks), then thread c scans candidate c for its length.
//   1. hypothesis counts, dealt over the (candidate i, position a) pairs: for every order k the number of times the
//      k-gram at a occurs in i -- or 0 when it occurred before a (it is counted at its first position) or runs past the
//      caption's end.  Four counts <= 64 are packed into one word hc[i][a].  They depend on i alone, so the Nr pairs of a
//      hypothesis share them.
//   2. pairs, dealt over the threads (pair p = i * Nr + j: the threads of a wave share i, whose tokens and counts are LDS
//      broadcasts, and walk different reference rows): per first position a of i the reference j is scanned once; the
//      length m <= order of the common prefix of the grams at a and at b counts one occurrence for every k <= m.  Then
//      c_k += min(count in i, count in j).  Integer compares only.  The utility goes to LDS (and to util / match).
//   3. thread i sums its row of utilities in ascending j; wave 0 reduces the first maximum; the chosen tokens are copied
//      out of LDS.
// Tokens are compared and never index anything.  No atomics, no scratch memory, fixed summation orders: deterministic.
#include "tnt_common.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_MAXC = 64;                // candidates per scan
constexpr int MB_MAXL = 64;                // tokens per candidate
constexpr int MB_MAXO = 4;                 // n-gram order
constexpr int MB_LDT = MB_MAXL + 1;        // LDS row stride of the tokens and the counts
constexpr float MB_EPS = 0.1f;             // evaluate.sentence_bleu's method-1 epsilon

struct MbrArgs {
  const int* ids; int ld;
  int B, Nc, Nr, L, end_id, order, kind;
  float* expected; int* best; int* out_ids; int ldo; int* match; float* util;
};

// the length m <= lim of the common prefix of the window x0..x3 and the gram g0..g3: branch-free, on registers
__device__ __forceinline__ int mb_prefix(int x0, int x1, int x2, int x3, int g0, int g1, int g2, int g3, int lim) {
  int m = x0 == g0;
  m += (m == 1) & (x1 == g1);
  m += (m == 2) & (x2 == g2);
  m += (m == 3) & (x3 == g3);
  return min(m, lim);
}

// one in the bytes [0, m) of a word, 0 <= m <= 4: an occurrence of the k-gram for every k <= m
__device__ __forceinline__ unsigned mb_ones(int m) { return m == 0 ? 0u : (0x01010101u >> (8 * (MB_MAXO - m))); }

__global__ __launch_bounds__(MB_THREADS) void mbr_select_kernel(MbrArgs a) {
  __shared__ int tok[MB_MAXC * MB_LDT + MB_MAXO];       // the tail words: grams and windows are loaded unguarded, up to
                                                        // word L + 3 of a row (compared under lim only)
  __shared__ unsigned hc[MB_MAXC * MB_LDT];
  __shared__ float us[MB_MAXC * MB_MAXC];               // u(i, j) at i * Nr + j
  __shared__ float es[MB_MAXC];
  __shared__ int len[MB_MAXC];
  __shared__ int sbest;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Nc = a.Nc, Nr = a.Nr, L = a.L, order = a.order;

  // ---- 0. stage
  for (int x = tid; x < Nc * L; x += MB_THREADS) {
    const int c = x / L, t = x - c * L;
    tok[c * MB_LDT + t] = a.ids[((long)c * L + t) * a.ld + b];
  }
  if (tid < MB_MAXO) tok[MB_MAXC * MB_LDT + tid] = 0;
  __syncthreads();
  if (tid < Nc) {
    const int* h = tok + tid * MB_LDT;
    int n = 0;
    while (n < L && h[n] != 0 && !(a.end_id >= 0 && h[n] == a.end_id)) ++n;
    len[tid] = n;
  }
  __syncthreads();

  // ---- 1. per (candidate, position): the gram's count in the candidate at its first position, per order
  for (int x = tid; x < Nc * L; x += MB_THREADS) {
    const int i = x / L, p = x - i * L;
    const int n = len[i];
    unsigned w = 0;
    if (p < n) {
      const int* h = tok + i * MB_LDT;
      const int kmax = min(order, n - p);
      const int g0 = h[p], g1 = h[p + 1], g2 = h[p + 2], g3 = h[p + 3];
      unsigned cnt = 0, seen = 0;                       // cnt: a byte per order; seen: bit k-1, the k-gram occurs before p
      int x0 = h[0], x1 = h[1], x2 = h[2], x3 = h[3];   // the window slides: one LDS read per position, off the compare chain
      for (int q = 0; q < n; ++q) {
        const int m = mb_prefix(x0, x1, x2, x3, g0, g1, g2, g3, min(kmax, n - q));      // q == p: kmax
        if (q < p) seen |= (1u << m) - 1u;
        else cnt += mb_ones(m);
        x0 = x1; x1 = x2; x2 = x3; x3 = h[q + 4];
      }
#pragma unroll
      for (int k = 0; k < MB_MAXO; ++k)
        if (!((seen >> k) & 1u)) w |= cnt & (0xffu << (8 * k));
    }
    hc[i * MB_LDT + p] = w;
  }
  __syncthreads();

  // ---- 2. the pairs
  const float inv_order = 1.f / (float)order;
  for (int x = tid; x < Nc * Nr; x += MB_THREADS) {
    const int i = x / Nr, j = x - i * Nr;
    const int nh = len[i], nr = len[j];
    const int* h = tok + i * MB_LDT;
    const int* r = tok + j * MB_LDT;
    int c[MB_MAXO] = {0, 0, 0, 0};
    for (int p = 0; p < nh; ++p) {
      const unsigned w = hc[i * MB_LDT + p];
      if (w == 0) continue;                             // every gram at p occurred before
      const int kmax = min(order, nh - p);
      const int g0 = h[p], g1 = h[p + 1], g2 = h[p + 2], g3 = h[p + 3];
      unsigned cnt = 0;
      int x0 = r[0], x1 = r[1], x2 = r[2], x3 = r[3];
      for (int q = 0; q < nr; ++q) {
        cnt += mb_ones(mb_prefix(x0, x1, x2, x3, g0, g1, g2, g3, min(kmax, nr - q)));
        x0 = x1; x1 = x2; x2 = x3; x3 = r[q + 4];
      }
#pragma unroll
      for (int k = 0; k < MB_MAXO; ++k) c[k] += (int)min((w >> (8 * k)) & 0xffu, (cnt >> (8 * k)) & 0xffu);
    }
    float u = 0.f;
    if (a.kind == 0) {
#pragma unroll
      for (int k = 0; k < MB_MAXO; ++k)
        if (k < order) {
          const int den = max(nh - k, 0) + max(nr - k, 0);
          u += den > 0 ? (float)(2 * c[k]) / (float)den : 0.f;
        }
      u = u / (float)order;
    } else if (nh > 0 && c[0] > 0) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < MB_MAXO; ++k)
        if (k < order) {
          const float num = c[k] > 0 ? (float)c[k] : MB_EPS;
          s += inv_order * logf(num / (float)max(1, nh - k));
        }
      const float bp = nh > nr ? 1.f : expf(1.f - (float)nr / (float)nh);
      u = bp * expf(s);
    }
    us[x] = u;
    const long pair = ((long)b * Nc + i) * Nr + j;
    if (a.util) a.util[pair] = u;
    if (a.match)
#pragma unroll
      for (int k = 0; k < MB_MAXO; ++k)
        if (k < order) a.match[pair * order + k] = c[k];
  }
  __syncthreads();

  // ---- 3. expected utility, first maximum, the chosen caption
  if (tid < Nc) {
    double s = 0.0;
    for (int j = 0; j < Nr; ++j) s += (double)us[tid * Nr + j];
    const float e = (float)(s / (double)Nr);
    es[tid] = e;
    a.expected[(long)b * Nc + tid] = e;
  }
  __syncthreads();
  if (tid < 64) {
    float v = tid < Nc ? es[tid] : -INFINITY;
    int ix = tid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(ix, o, 64);
      if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
    }
    if (tid == 0) { sbest = ix; a.best[b] = ix; }
  }
  __syncthreads();
  if (a.out_ids && tid < L) a.out_ids[(long)tid * a.ldo + b] = tok[sbest * MB_LDT + tid];
}

bool mb_overlap(const void* p, uintptr_t np, const void* q, uintptr_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p != nullptr && q != nullptr && a < b + nq && b < a + np;
}

}  // namespace

extern "C" int32_t tnt_mbr_select_f32(const int32_t* ids, int32_t ld, int32_t B, int32_t Nc, int32_t Nr, int32_t L,
                                      int32_t end_id, int32_t order, int32_t kind, float* expected, int32_t* best,
                                      int32_t* out_ids, int32_t ldo, int32_t* match, float* util, void* stream) {
  if (!ids) return TNT_BADARG(0);
  if (B <= 0) return TNT_BADARG(2);
  if (ld < B) return TNT_BADARG(1);
  if (Nc < 1 || Nc > MB_MAXC) return TNT_BADARG(3);
  if (Nr < 1 || Nr > Nc) return TNT_BADARG(4);
  if (L < 1 || L > MB_MAXL) return TNT_BADARG(5);
  if (order < 1 || order > MB_MAXO) return TNT_BADARG(7);
  if (kind != 0 && kind != 1) return TNT_BADARG(8);
  if (!expected) return TNT_BADARG(9);
  if (!best) return TNT_BADARG(10);
  if (out_ids && ldo < B) return TNT_BADARG(12);
  {                                                    // ids is read while the outputs are written
    const uintptr_t uB = (uintptr_t)B, pairs = uB * (uintptr_t)Nc * (uintptr_t)Nr;
    const uintptr_t nids = (((uintptr_t)Nc * (uintptr_t)L - 1) * (uintptr_t)ld + uB) * sizeof(int32_t);
    if (mb_overlap(ids, nids, expected, uB * (uintptr_t)Nc * sizeof(float))) return TNT_BADARG(9);
    if (mb_overlap(ids, nids, best, uB * sizeof(int32_t))) return TNT_BADARG(10);
    if (mb_overlap(ids, nids, out_ids, (((uintptr_t)L - 1) * (uintptr_t)(out_ids ? ldo : 0) + uB) * sizeof(int32_t)))
      return TNT_BADARG(11);
    if (mb_overlap(ids, nids, match, pairs * (uintptr_t)order * sizeof(int32_t))) return TNT_BADARG(13);
    if (mb_overlap(ids, nids, util, pairs * sizeof(float))) return TNT_BADARG(14);
  }
  MbrArgs a;
  a.ids = ids; a.ld = ld;
  a.B = B; a.Nc = Nc; a.Nr = Nr; a.L = L; a.end_id = end_id; a.order = order; a.kind = kind;
  a.expected = expected; a.best = best; a.out_ids = out_ids; a.ldo = ldo; a.match = match; a.util = util;
  hipLaunchKernelGGL(mbr_select_kernel, dim3(B), dim3(MB_THREADS), 0, tnt_stream(stream), a);
  TNT_LAUNCH_CHECK();
  return 0;
}
