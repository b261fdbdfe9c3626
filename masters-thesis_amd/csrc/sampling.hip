// Top-k / nucleus (top-p) filtered categorical sampling, one workgroup per row (tnt_sample_topkp_f32; the definition is
// in include/tnt_hip.h).  The filters of lc_NIC's select_nucleus2 and img_NIC's select_topk / select_nucleus, defined
// in rank order (the reference's helpers accumulate from the least likely token).
//
// Per row, 256 threads:
//   1. the row goes to LDS (coalesced) as l, its max m is reduced, and l is replaced by w = exp((l - m) / temperature)
//      (a NaN weight counts as 0);
//   2. top-k (K < V): radix select of the K-th largest weight over the float bit patterns (w >= 0, so the pattern
//      orders like the value), four 8-bit passes of LDS count histograms; the tokens equal to it are taken lowest
//      index first through a prefix count over the threads' contiguous chunks;
//   3. nucleus (top_p < 1): the same radix walk over the candidates with mass histograms, the masses in 38-bit fixed
//      point (w <= 1; integer LDS atomics, so the sums do not depend on the order of the atomics and the kernel is
//      deterministic; the rounding is below 2^-39 per token, S_K >= 1 because the max weight is exp(0) = 1).  It finds
//      the weight of the last kept rank and the mass above it; equal weights at the cutoff are kept lowest index first
//      while mass_before < top_p * S_K;
//   4. the draw of tnt_sample_rows_f32 (seqops.hip) over the kept weights: 256 contiguous chunks, a serial prefix over
//      the chunk sums, one Philox uniform per row.  With no filter the kept set is the whole row and every float
//      operation of the draw is that kernel's, so the two return the same ids.
// The only global memory traffic is one read of the row and the id written.  No scratch memory.
#include "tnt_common.h"
#include "tnt_rng.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_MAX_V = 16384;                    // LDS: 64 KiB of weights + 16 KiB of keep flags
constexpr double TK_FIX = 274877906944.0;          // 2^38: fixed-point scale of the nucleus masses

// wave 0 only: the digit b (visited from 255 down) at which the running total of h first reaches `need`:
// above(b) < need <= above(b) + h[b], above(b) = sum of h over the digits > b.  Writes b and above(b).  Exactly one
// digit qualifies when 0 < need <= sum(h) (a zero bucket never does).
template <typename T>
__device__ __forceinline__ void tk_find_digit(const T* h, unsigned long long need, int lane, int* s_b,
                                              unsigned long long* s_above) {
  unsigned long long v[4], tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q] = (unsigned long long)h[255 - 4 * lane - q]; tot += v[q]; }
  unsigned long long inc = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  unsigned long long run = inc - tot;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (run < need && need <= run + v[q]) { *s_b = 255 - 4 * lane - q; *s_above = run; }
    run += v[q];
  }
}

// exclusive prefix of c over the 256 threads in thread order; s4: 4 words of LDS (ends with a barrier)
__device__ __forceinline__ uint32_t tk_excl_scan(uint32_t c, uint32_t* s4) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s4[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < wave; ++w) base += s4[w];
  __syncthreads();
  return base + inc - c;
}

__device__ __forceinline__ unsigned long long tk_mass(float w) { return __double2ull_rn((double)w * TK_FIX); }

__global__ __launch_bounds__(TK_THREADS) void sample_topkp_kernel(const float* x, int* out, int V, int ld,
                                                                  float inv_temp, int K, float top_p, int from_logits,
                                                                  uint64_t seed, uint32_t site, uint32_t step,
                                                                  const uint32_t* step_dev) {
  __shared__ float s_w[TK_MAX_V];
  __shared__ unsigned char s_keep[TK_MAX_V];
  __shared__ uint32_t s_cnt[256];
  __shared__ unsigned long long s_mass[256];
  __shared__ float part[257];
  __shared__ float shm[4];
  __shared__ uint32_t s_scan[4];
  __shared__ int s_b, s_pick;
  __shared__ unsigned long long s_above, s_total;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* xr = x + (long)row * ld;
  const int C = (V + 255) / 256;
  const int j0 = tid * C, j1 = min(V, j0 + C);

  // ---- 1. weights
  float mx = -INFINITY;
  for (int j = tid; j < V; j += TK_THREADS) {
    const float l = from_logits ? xr[j] : logf(xr[j]);
    s_w[j] = l;
    mx = fmaxf(mx, l);
  }
  mx = tnt_wave_max(mx);
  if (lane == 0) shm[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
  for (int j = tid; j < V; j += TK_THREADS) {
    const float w = expf((s_w[j] - mx) * inv_temp);
    s_w[j] = w >= 0.f ? w : 0.f;                 // NaN -> 0
    s_keep[j] = 1;
  }
  __syncthreads();

  // ---- 2. top-k: the K-th largest key t (rank K - 1) and how many of the tokens equal to it are candidates
  if (K < V) {
    uint32_t prefix = 0;
    unsigned long long krem = (unsigned long long)K;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const uint32_t hi = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      s_cnt[tid] = 0;
      __syncthreads();
      for (int j = tid; j < V; j += TK_THREADS) {
        const uint32_t key = __float_as_uint(s_w[j]);
        if ((key & hi) == prefix) atomicAdd(&s_cnt[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64) tk_find_digit(s_cnt, krem, lane, &s_b, &s_above);
      __syncthreads();
      prefix |= (uint32_t)s_b << shift;
      krem -= s_above;
    }
    // tokens > t are candidates; of the tokens == t the krem lowest indices
    uint32_t c = 0;
    for (int j = j0; j < j1; ++j) c += __float_as_uint(s_w[j]) == prefix;
    uint32_t tie = tk_excl_scan(c, s_scan);
    for (int j = j0; j < j1; ++j) {
      const uint32_t key = __float_as_uint(s_w[j]);
      if (key == prefix) s_keep[j] = tie++ < krem;
      else s_keep[j] = key > prefix;
    }
    __syncthreads();
  }

  // ---- 3. nucleus over the candidates
  if (top_p < 1.f) {
    if (tid == 0) s_total = 0;
    __syncthreads();
    unsigned long long loc = 0;
    for (int j = j0; j < j1; ++j)
      if (s_keep[j]) loc += tk_mass(s_w[j]);
    atomicAdd(&s_total, loc);
    __syncthreads();
    const unsigned long long total = s_total;
    if (total > 0) {
      // a rank is kept iff the mass before it is < top_p * S_K, i.e. < thr = ceil(top_p * S_K) (integer masses)
      const unsigned long long thr = (unsigned long long)ceil((double)top_p * (double)total);
      uint32_t prefix = 0;
      unsigned long long above = 0;            // candidate mass with keys above the current prefix range
      for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t hi = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        s_mass[tid] = 0;
        __syncthreads();
        for (int j = tid; j < V; j += TK_THREADS) {
          const uint32_t key = __float_as_uint(s_w[j]);
          if (s_keep[j] && (key & hi) == prefix) atomicAdd(&s_mass[(key >> shift) & 255u], tk_mass(s_w[j]));
        }
        __syncthreads();
        if (tid < 64) tk_find_digit(s_mass, thr - above, lane, &s_b, &s_above);
        __syncthreads();
        prefix |= (uint32_t)s_b << shift;
        above += s_above;
      }
      // prefix: the weight of the last kept rank; above: the candidate mass of the larger weights.  Candidates equal to
      // it are kept in index order while above + (their tie index) * mass < thr
      const unsigned long long m = tk_mass(__uint_as_float(prefix));
      uint32_t c = 0;
      for (int j = j0; j < j1; ++j) c += s_keep[j] && __float_as_uint(s_w[j]) == prefix;
      unsigned long long tie = tk_excl_scan(c, s_scan);
      for (int j = j0; j < j1; ++j) {
        if (!s_keep[j]) continue;
        const uint32_t key = __float_as_uint(s_w[j]);
        if (key == prefix) s_keep[j] = above + (tie++) * m < thr;
        else s_keep[j] = key > prefix;
      }
      __syncthreads();
    }
  }

  // ---- 4. the draw: tnt_sample_rows_f32's chunk order over the kept weights
  float loc = 0.f;
  for (int j = j0; j < j1; ++j)
    if (s_keep[j]) loc += s_w[j];
  part[tid + 1] = loc;
  if (tid == 0) s_pick = -1;
  __syncthreads();
  if (tid == 0) {                      // fixed-order prefix over the 256 chunk sums
    part[0] = 0.f;
    float run = 0.f;
    for (int t = 1; t <= 256; ++t) { run += part[t]; part[t] = run; }
  }
  __syncthreads();
  if (step_dev) step += step_dev[0];
  const uint64_t e = (uint64_t)row, g = e >> 2;
  const TntPhilox4 r = tnt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t sel = (uint32_t)e & 3u;      // select chain: a runtime index would put r.v in scratch memory
  const uint32_t rw = sel == 0u ? r.v[0] : (sel == 1u ? r.v[1] : (sel == 2u ? r.v[2] : r.v[3]));
  const float u = (float)(rw >> 8) * 5.9604644775390625e-08f;
  const float target = u * part[256];
  const int tlast = (V - 1) / C;       // last thread that owns elements (takes the u*sum == sum rounding case)
  if (part[tid] <= target && (target < part[tid + 1] || tid == tlast)) {
    float run = part[tid];
    int pick = -1, lastpos = -1;
    for (int j = j0; j < j1; ++j) {
      if (!s_keep[j]) continue;
      const float w = s_w[j];
      run += w;
      if (run > target) { pick = j; break; }
      if (w > 0.f) lastpos = j;
    }
    s_pick = pick >= 0 ? pick : lastpos;
  }
  __syncthreads();
  if (tid == 0) {
    int pick = s_pick;
    if (pick < 0) {                    // rounding past the chunk's end, or no kept weight is positive
      pick = 0;
      for (int j = V - 1; j >= 0; --j)
        if (s_keep[j] && s_w[j] > 0.f) { pick = j; break; }
    }
    out[row] = pick;
  }
}

}  // namespace

extern "C" int32_t tnt_sample_topkp_f32(const float* x, int32_t* out, int32_t rows, int32_t V, int32_t ld,
                                        float temperature, int32_t top_k, float top_p, int32_t from_logits,
                                        uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                        void* stream) {
  if (rows <= 0 || V <= 0) return TNT_BADARG(3);
  if (!(temperature > 0.f)) return TNT_BADARG(5);
  if (!(top_p > 0.f)) return TNT_BADARG(7);
  if (V > TK_MAX_V) return TNT_BADARG(4);
  const int K = top_k >= 1 ? min(top_k, V) : V;
  hipLaunchKernelGGL(sample_topkp_kernel, dim3(rows), dim3(TK_THREADS), 0, tnt_stream(stream), x, out, V, ld,
                     1.f / temperature, K, top_p, from_logits, seed, site, step, step_dev);
  TNT_LAUNCH_CHECK();
  return 0;
}
