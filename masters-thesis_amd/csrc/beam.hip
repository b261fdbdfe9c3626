// The beam-search steps, one launch per decoded token (the definitions are in include/tnt_hip.h):
//   tnt_beam_step_f32          the expansion of tnt_beam_topk_f32 (seqops.hip), bit for bit, and the reorder of the
//                              LSTM state by parent beam;
//   tnt_beam_step_diverse_f32  the same step for diverse (group) beam search with Hamming diversity.  The k beams of a
//                              sample are Gd groups of kp = k / Gd; the groups choose in ascending order, and a
//                              candidate's selection key is its score minus lambda times the number of beams the
//                              earlier groups of the sample have chosen at this step with the same token.
// Both are instantiations of one kernel, beam_step_kernel<DIVERSE>, and differ in phase 2 only; the plain instantiation
// carries nothing of the diverse one (a compile-time switch: a run-time groups == 1 branch costs a wave of occupancy).
//
// One workgroup of 16 waves per sample.  Beam row j of the sample gets W = 16 / k waves (k = 5: 3 waves, k = 1: all 16):
//   1. per-row selection: k rounds; round r takes the best candidate of the row strictly after round r-1's winner in
//      the order (value desc, token asc).  Each lane scans its strided tokens for that, 8 loads in flight at a time
//      (a strict `>` keeps the lowest token among equal values), the wave reduces with ties to the lower token, and
//      the W wave winners of the row meet in LDS (double-buffered slots, one barrier per round).  No taken-list, no
//      dynamically indexed per-lane arrays.
//      Within one row the global order is the row's own order, so the sample's k best are among the union of the
//      rows' k best.  The value ranked is the float32 candidate score_in[j] + logf(fmaxf(p, 1e-30f)), the same
//      expression as tnt_beam_topk_f32, so values that logf and the addition merge still tie and resolve by index.
//      A finished row has one candidate, token 0 at its own score: its scan is the single token 0.
//   2. merge: the <= k*k row winners are ranked in LDS by (value desc, flat index j*V + v asc); rank < k is the output
//      slot.  A slot with no eligible candidate (only possible for non-finite score_in) gets what tnt_beam_topk_f32
//      writes then: score -inf, candidate 0.
//   3. reorder: every thread copies the k parent rows of h and c (float4 when ldh, U and the pointers allow it).
// The diverse step:
//   1. the same selection, once, for all groups at the same time.  The penalty only lowers keys, and the groups before g
//      have chosen g*kp tokens at the most, so the kp best keys of group g are among each of its rows' (g+1)*kp <= k
//      best VALUES: at least kp of those carry no penalty, and every token behind them in the row's order (value desc,
//      token asc) has a key no better than theirs and comes later in the tie order.  Rows of group g therefore run
//      (g+1)*kp of the k rounds and sit out the rest.
//   2. the groups in ascending order, on the <= kp*k prepared candidates of the group in LDS: key = value - lambda * n_v
//      (two separately rounded float32 operations) with n_v counted over the <= k tokens chosen so far, which live in
//      LDS; rank by (key desc, flat index j*V + v asc); rank < kp is the output slot.  Two barriers per group; this is
//      the only part that runs Gd times, and it never touches the probabilities again.
//   3. the same reorder.
// lambda = 0 or Gd = 1 leaves key = value: the diverse launch is then tnt_beam_step_f32's on (B*Gd, kp), bit for bit.
// Each workgroup reads and writes only its own sample's rows.  Deterministic; no atomics; no scratch memory.
#include <cmath>

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

// DIVERSE = false: tnt_beam_step_f32's kernel; groups and lambda are not read, and the cut-off of the rounds, key[],
// ctok[] and the group loop are not in it.  DIVERSE = true: tnt_beam_step_diverse_f32's.
template <bool DIVERSE>
__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(
    const float* __restrict__ probs, int ld, const float* __restrict__ score_in, const int* __restrict__ fin_in, int V,
    int k, int end_id, float* __restrict__ score_out, int* __restrict__ parent, int* __restrict__ token,
    int* __restrict__ fin_out, const float* __restrict__ h_in, const float* __restrict__ c_in, int ldh, int U,
    float* __restrict__ h_out, float* __restrict__ c_out, int vec4, int groups, float lambda) {
  __shared__ float sc[BS_MAXK];
  __shared__ int fn[BS_MAXK];
  __shared__ BsCand slot[2][BS_WAVES];
  __shared__ BsCand win[BS_MAXK * BS_MAXK];     // [row j][round r]: the row's r-th best value (i = BS_NONE: none)
  __shared__ float key[BS_MAXK * BS_MAXK];      // diverse: the selection keys of the group in turn
  __shared__ int par[BS_MAXK];                  // output slot -> local parent row
  __shared__ int ctok[BS_MAXK];                 // diverse: output slot -> its token, or -1 where it adds to no n_v
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long row0 = (long)b * k;
  const int kp = DIVERSE ? k / groups : k;
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
  const int rounds = !DIVERSE ? k : act ? (j / kp + 1) * kp : 0;   // diverse: what the row's group can need
  const float* pr = probs + (row0 + (act ? j : 0)) * (long)ld;
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    BsCand best; best.v = -INFINITY; best.i = BS_NONE;
    const int ve = r < rounds ? vend : 0;
    for (int v0 = t0; v0 < ve; v0 += BS_UNROLL * stride) {
      float p[BS_UNROLL];               // BS_UNROLL loads issued before the first is used (static indices: registers)
#pragma unroll
      for (int u = 0; u < BS_UNROLL; ++u) {
        const int v = v0 + u * stride;
        p[u] = (!fj && v < ve) ? pr[v] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < BS_UNROLL; ++u) {   // ascending v within the lane: the strict > keeps the lowest tied token
        const int v = v0 + u * stride;
        const float val = fj ? s : s + logf(fmaxf(p[u], 1e-30f));
        const bool after = val < pv || (val == pv && v > pi);
        if (v < ve && after && val > best.v) { best.v = val; best.i = v; }
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

  if constexpr (!DIVERSE) {
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
  } else {
    // ---- 2. the groups in turn: penalise, rank by (key desc, j asc, v asc), emit
    const int n = kp * k;                          // candidates of one group: its kp rows x k rounds
    for (int g = 0; g < groups; ++g) {
      const int base = g * n, slot0 = g * kp;
      BsCand e; e.v = 0.f; e.i = BS_NONE;
      const int je = slot0 + tid / k;              // local row of the candidate
      if (tid < n) {
        e = win[base + tid];
        float kv = -INFINITY;
        if (e.i != BS_NONE) {
          int nv = 0;
          if (!fn[je])
            for (int q = 0; q < slot0; ++q) nv += ctok[q] == e.i;
          kv = __fsub_rn(e.v, __fmul_rn(lambda, (float)nv));
        }
        key[tid] = kv;
      }
      __syncthreads();
      if (tid < n && e.i != BS_NONE) {
        const float ke = key[tid];
        int rank = 0;
        for (int q = 0; q < n; ++q) {
          const int oi = win[base + q].i;
          const float ko = key[q];
          const int jo = slot0 + q / k;
          rank += (oi != BS_NONE) && (ko > ke || (ko == ke && (jo < je || (jo == je && oi < e.i))));
        }
        if (rank < kp) {
          const long r = row0 + slot0 + rank;
          score_out[r] = e.v;                      // the unpenalised score
          parent[r] = (int)(row0 + je);
          token[r] = e.i;
          fin_out[r] = (fn[je] || e.i == end_id) ? 1 : 0;
          par[slot0 + rank] = je;
          ctok[slot0 + rank] = fn[je] ? -1 : e.i;
        }
      }
      if (tid == 0) {                              // slots without a candidate (only for non-finite score_in)
        int nvalid = 0;
        for (int q = 0; q < n; ++q) nvalid += win[base + q].i != BS_NONE;
        for (int r = nvalid; r < kp; ++r) {
          score_out[row0 + slot0 + r] = -INFINITY;
          parent[row0 + slot0 + r] = (int)(row0 + slot0);
          token[row0 + slot0 + r] = 0;
          fin_out[row0 + slot0 + r] = (fn[slot0] || end_id == 0) ? 1 : 0;
          par[slot0 + r] = slot0;
          ctok[slot0 + r] = -1;
        }
      }
      __syncthreads();
    }
    if (U == 0) return;
  }

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

// The argument checks of both entry points, in the order they are reported, and the float4 decision of the reorder.
// `own` is what the diverse entry found about its own two arguments (0: nothing, and always for the plain entry); it is
// reported after the expansion's checks and in front of the state's.
int bs_check(const float* score_in, const int32_t* fin_in, int32_t B, int32_t V, int32_t k, int32_t ld,
             const float* score_out, const int32_t* fin_out, const float* h_in, const float* c_in, int32_t ldh,
             int32_t U, const float* h_out, const float* c_out, int own, int* vec4) {
  if (B <= 0) return TNT_BADARG(4);
  if (V <= 0) return TNT_BADARG(5);
  if (k < 1 || k > BS_MAXK) return TNT_BADARG(6);
  if (ld < V) return TNT_BADARG(1);
  if (U < 0) return TNT_BADARG(15);
  if (ldh < U) return TNT_BADARG(14);
  if (score_out == score_in || fin_out == fin_in) return TNT_BADARG(8);
  if (own) return own;
  *vec4 = 0;
  if (U > 0) {
    if (!h_in || !c_in || !h_out || !c_out) return TNT_BADARG(12);
    const long rows = (long)B * k;
    if (bs_overlap(h_out, h_in, rows, ldh, U) || bs_overlap(h_out, c_in, rows, ldh, U) ||
        bs_overlap(c_out, h_in, rows, ldh, U) || bs_overlap(c_out, c_in, rows, ldh, U))
      return TNT_BADARG(16);
    *vec4 = (U % 4 == 0 && ldh % 4 == 0 && tnt_aligned16(h_in) && tnt_aligned16(c_in) && tnt_aligned16(h_out) &&
             tnt_aligned16(c_out)) ? 1 : 0;
  }
  return 0;
}

}  // namespace

extern "C" int32_t tnt_beam_step_f32(const float* probs, int32_t ld, const float* score_in, const int32_t* fin_in,
                                     int32_t B, int32_t V, int32_t k, int32_t end_id, float* score_out,
                                     int32_t* parent, int32_t* token, int32_t* fin_out, const float* h_in,
                                     const float* c_in, int32_t ldh, int32_t U, float* h_out, float* c_out,
                                     void* stream) {
  int vec4;
  const int rc = bs_check(score_in, fin_in, B, V, k, ld, score_out, fin_out, h_in, c_in, ldh, U, h_out, c_out, 0, &vec4);
  if (rc) return rc;
  hipLaunchKernelGGL(beam_step_kernel<false>, dim3(B), dim3(BS_THREADS), 0, tnt_stream(stream), probs, ld, score_in,
                     fin_in, V, k, end_id, score_out, parent, token, fin_out, h_in, c_in, ldh, U, h_out, c_out, vec4, 1,
                     0.f);
  TNT_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t tnt_beam_step_diverse_f32(const float* probs, int32_t ld, const float* score_in,
                                             const int32_t* fin_in, int32_t B, int32_t V, int32_t k, int32_t end_id,
                                             float* score_out, int32_t* parent, int32_t* token, int32_t* fin_out,
                                             const float* h_in, const float* c_in, int32_t ldh, int32_t U, float* h_out,
                                             float* c_out, int32_t groups, float lambda, void* stream) {
  int own = 0;
  if (groups < 1 || k % groups != 0) own = TNT_BADARG(18);
  else if (!std::isfinite(lambda) || lambda < 0.f) own = TNT_BADARG(19);
  int vec4;
  const int rc = bs_check(score_in, fin_in, B, V, k, ld, score_out, fin_out, h_in, c_in, ldh, U, h_out, c_out, own, &vec4);
  if (rc) return rc;
  hipLaunchKernelGGL(beam_step_kernel<true>, dim3(B), dim3(BS_THREADS), 0, tnt_stream(stream), probs, ld, score_in,
                     fin_in, V, k, end_id, score_out, parent, token, fin_out, h_in, c_in, ldh, U, h_out, c_out, vec4,
                     groups, lambda);
  TNT_LAUNCH_CHECK();
  return 0;
}
