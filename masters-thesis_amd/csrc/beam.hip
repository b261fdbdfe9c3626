// One beam-search step, one launch per decoded token (tnt_beam_step_f32; the definition is in include/tnt_hip.h): the
// expansion of tnt_beam_topk_f32 (seqops.hip), bit for bit, and the reorder of the LSTM state by parent beam.
//
// One workgroup of 16 waves per sample.  Beam row j of the sample gets W = 16 / k waves (k = 5: 3 waves, k = 1: all 16):
//   1. per-row selection: k rounds; round r takes the best candidate of the row strictly after round r-1's winner in
//      the order (value desc, token asc).  Each lane scans its strided tokens for that, 8 loads in flight at a time
//      (a strict `>` keeps the lowest token among equal values), the wave reduces with ties to the lower token, and
//      the W wave winners of the row meet in LDS (double-buffered slots, one barrier per round).  No taken-list, no dynamically indexed per-lane arrays.
//      Within one row the global order is the row's own order, so the sample's k best are among the union of the
//      rows' k best.  The value ranked is the float32 candidate score_in[j] + logf(fmaxf(p, 1e-30f)), the same
//      expression as tnt_beam_topk_f32, so values that logf and the addition merge still tie and resolve by index.
//      A finished row has one candidate, token 0 at its own score: its scan is the single token 0.
//   2. merge: the <= k*k row winners are ranked in LDS by (value desc, flat index j*V + v asc); rank < k is the output
//      slot.  A slot with no eligible candidate (only possible for non-finite score_in) gets what tnt_beam_topk_f32
//      writes then: score -inf, candidate 0.
//   3. reorder: every thread copies the k parent rows of h and c (float4 when ldh, U and the pointers allow it).
// Each workgroup reads and writes only its own sample's rows.  Deterministic; no atomics; no scratch memory.
#include "tnt_common.h"

namespace {

constexpr int BS_THREADS = 1024;
constexpr int BS_WAVES = BS_THREADS / 64;
constexpr int BS_MAXK = 16;
constexpr int BS_NONE = 0x7fffffff;
constexpr int BS_UNROLL = 8;

struct BsCand { float v; int i; };

// larger value wins; ties -> the smaller index (argmax_combine of seqops.hip)
__device__ __forceinline__ BsCand bs_combine(BsCand a, BsCand b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

__device__ __forceinline__ BsCand bs_wave_best(BsCand a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    BsCand b; b.v = __shfl_xor(a.v, o, 64); b.i = __shfl_xor(a.i, o, 64);
    a = bs_combine(a, b);
  }
  return a;
}

__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(const float* __restrict__ probs, int ld,
                                                               const float* __restrict__ score_in,
                                                               const int* __restrict__ fin_in, int V, int k, int end_id,
                                                               float* __restrict__ score_out, int* __restrict__ parent,
                                                               int* __restrict__ token, int* __restrict__ fin_out,
                                                               const float* __restrict__ h_in,
                                                               const float* __restrict__ c_in, int ldh, int U,
                                                               float* __restrict__ h_out, float* __restrict__ c_out,
                                                               int vec4) {
  __shared__ float sc[BS_MAXK];
  __shared__ int fn[BS_MAXK];
  __shared__ BsCand slot[2][BS_WAVES];
  __shared__ BsCand win[BS_MAXK * BS_MAXK];     // [row j][round r]: the row's r-th best (i = BS_NONE: none)
  __shared__ int par[BS_MAXK];                  // output slot -> local parent row
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long row0 = (long)b * k;
  if (tid < k) { sc[tid] = score_in[row0 + tid]; fn[tid] = fin_in[row0 + tid]; }
  __syncthreads();

  // ---- 1. per-row selection
  const int W = BS_WAVES / k;
  const int j = wave / W;                        // j >= k: an idle wave (it still meets every barrier)
  const bool act = j < k;
  const int t0 = (wave - j * W) * 64 + lane, stride = W * 64;
  const float s = act ? sc[j] : 0.f;
  const bool fj = act && fn[j] != 0;
  const int vend = act ? (fj ? min(V, 1) : V) : 0;   // a finished row: only token 0 can be eligible
  const float* pr = probs + (row0 + (act ? j : 0)) * (long)ld;
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    BsCand best; best.v = -INFINITY; best.i = BS_NONE;
    for (int v0 = t0; v0 < vend; v0 += BS_UNROLL * stride) {
      float p[BS_UNROLL];               // BS_UNROLL loads issued before the first is used (static indices: registers)
#pragma unroll
      for (int u = 0; u < BS_UNROLL; ++u) {
        const int v = v0 + u * stride;
        p[u] = (!fj && v < vend) ? pr[v] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < BS_UNROLL; ++u) {   // ascending v within the lane: the strict > keeps the lowest tied token
        const int v = v0 + u * stride;
        const float val = fj ? s : s + logf(fmaxf(p[u], 1e-30f));
        const bool after = val < pv || (val == pv && v > pi);
        if (v < vend && after && val > best.v) { best.v = val; best.i = v; }
      }
    }
    best = bs_wave_best(best);
    if (lane == 0) slot[r & 1][wave] = best;
    __syncthreads();
    if (act) {
      BsCand w = slot[r & 1][j * W];
      for (int q = 1; q < W; ++q) w = bs_combine(w, slot[r & 1][j * W + q]);
      pv = w.v; pi = w.i;                        // none: (-inf, BS_NONE), after which nothing is eligible
      if (t0 == 0) win[j * k + r] = w;
    }
  }
  __syncthreads();

  // ---- 2. merge the row winners: rank by (value desc, j asc, v asc)
  const int n = k * k;
  if (tid < n) {
    const BsCand e = win[tid];
    if (e.i != BS_NONE) {
      const int je = tid / k;
      int rank = 0;
      for (int q = 0; q < n; ++q) {
        const BsCand o = win[q];
        const int jo = q / k;
        rank += (o.i != BS_NONE) && (o.v > e.v || (o.v == e.v && (jo < je || (jo == je && o.i < e.i))));
      }
      if (rank < k) {
        score_out[row0 + rank] = e.v;
        parent[row0 + rank] = (int)(row0 + je);
        token[row0 + rank] = e.i;
        fin_out[row0 + rank] = (fn[je] || e.i == end_id) ? 1 : 0;
        par[rank] = je;
      }
    }
  }
  if (tid == 0) {
    int nvalid = 0;
    for (int q = 0; q < n; ++q) nvalid += win[q].i != BS_NONE;
    for (int r = nvalid; r < k; ++r) {
      score_out[row0 + r] = -INFINITY;
      parent[row0 + r] = (int)row0;
      token[row0 + r] = 0;
      fin_out[row0 + r] = (fn[0] || end_id == 0) ? 1 : 0;
      par[r] = 0;
    }
  }
  if (U == 0) return;
  __syncthreads();

  // ---- 3. reorder the state: h_out[b*k + r] = h_in[b*k + par[r]], likewise c
  if (vec4) {
    const int n4 = U >> 2, per = k * n4;
    for (int it = tid; it < 2 * per; it += BS_THREADS) {
      const int which = it >= per, rem = it - which * per, r = rem / n4, q = rem - r * n4;
      const float* src = (which ? c_in : h_in) + (row0 + par[r]) * (long)ldh;
      float* dst = (which ? c_out : h_out) + (row0 + r) * (long)ldh;
      reinterpret_cast<floatx4*>(dst)[q] = reinterpret_cast<const floatx4*>(src)[q];
    }
  } else {
    const int per = k * U;
    for (int it = tid; it < 2 * per; it += BS_THREADS) {
      const int which = it >= per, rem = it - which * per, r = rem / U, q = rem - r * U;
      const float* src = (which ? c_in : h_in) + (row0 + par[r]) * (long)ldh;
      float* dst = (which ? c_out : h_out) + (row0 + r) * (long)ldh;
      dst[q] = src[q];
    }
  }
}

// byte ranges of two row-strided state buffers of `rows` rows overlap
bool bs_overlap(const float* a, const float* b, long rows, int ldh, int U) {
  const long span = ((rows - 1) * (long)ldh + U) * (long)sizeof(float);
  const char *pa = reinterpret_cast<const char*>(a), *pb = reinterpret_cast<const char*>(b);
  return pa < pb + span && pb < pa + span;
}

}  // namespace

extern "C" int32_t tnt_beam_step_f32(const float* probs, int32_t ld, const float* score_in, const int32_t* fin_in,
                                     int32_t B, int32_t V, int32_t k, int32_t end_id, float* score_out,
                                     int32_t* parent, int32_t* token, int32_t* fin_out, const float* h_in,
                                     const float* c_in, int32_t ldh, int32_t U, float* h_out, float* c_out,
                                     void* stream) {
  if (B <= 0) return TNT_BADARG(4);
  if (V <= 0) return TNT_BADARG(5);
  if (k < 1 || k > BS_MAXK) return TNT_BADARG(6);
  if (ld < V) return TNT_BADARG(1);
  if (U < 0) return TNT_BADARG(15);
  if (ldh < U) return TNT_BADARG(14);
  if (score_out == score_in || fin_out == fin_in) return TNT_BADARG(8);
  int vec4 = 0;
  if (U > 0) {
    if (!h_in || !c_in || !h_out || !c_out) return TNT_BADARG(12);
    const long rows = (long)B * k;
    if (bs_overlap(h_out, h_in, rows, ldh, U) || bs_overlap(h_out, c_in, rows, ldh, U) ||
        bs_overlap(c_out, h_in, rows, ldh, U) || bs_overlap(c_out, c_in, rows, ldh, U))
      return TNT_BADARG(16);
    vec4 = (U % 4 == 0 && ldh % 4 == 0 && tnt_aligned16(h_in) && tnt_aligned16(c_in) && tnt_aligned16(h_out) &&
            tnt_aligned16(c_out)) ? 1 : 0;
  }
  hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(BS_THREADS), 0, tnt_stream(stream), probs, ld, score_in, fin_in,
                     V, k, end_id, score_out, parent, token, fin_out, h_in, c_in, ldh, U, h_out, c_out, vec4);
  TNT_LAUNCH_CHECK();
  return 0;
}
