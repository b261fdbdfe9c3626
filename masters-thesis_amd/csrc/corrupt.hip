// Training-time input corruption on the staged batch (tnt_input_corrupt_f32; the definition is in include/tnt_hip.h,
// restated by tests/corrupt_oracle.py): scan dropout, the condition dropout of classifier-free guidance -- a fired sample's
// whole scan row becomes the null scan --, and word dropout (Bowman et al. 2016) -- a fired fed caption token becomes the
// unknown-word id.  Both are Bernoulli decisions on the Philox stream of tnt_rng.h, at the step word read on the device.
//
// One launch, in place, behind whichever staging route ran (ModelBase._stage_batch): the scan workgroups, one per piece of
// SCAN_CHUNK columns of a row, and behind them the word workgroups.  A scan workgroup makes ONE Philox call for its row
// -- every thread evaluates the same uniform call once, which costs what one lane plus a broadcast would without the LDS
// round trip; nothing is evaluated per element -- and returns at once when the row did not fire, so the traffic is that
// of the fired rows.  The pieces are there for the voxel-major copy: its stores are one float per 4 * ldt bytes, every
// lane of a store instruction in a cache line of its own, and one workgroup per row spent 27 us on the 20 000 of them
// where twenty workgroups per row, on twenty CUs, spend 5.  A word thread makes one
// Philox call for four consecutive caption positions.  Every address is stored by one thread; no atomics, LDS or scratch,
// plain vector stores.
#include "tnt_common.h"
#include "tnt_rng.h"

namespace {

constexpr int SCAN_CHUNK = 1024;     // columns of a row per scan workgroup: one float4 per thread

struct CorruptArgs {
  float* x; float* xT; int32_t* cap; const float* null_scan; const uint32_t* step_dev;
  int ldx, ldt, B, T, N, nscan, nchunk, unk_id;
  long n_tok;
  float scan_rate, word_rate;
  uint64_t seed; uint32_t site_scan, site_word;
};

// "fires" = u < rate = !tnt_keep
__device__ __forceinline__ bool fires(uint64_t e, float rate, uint64_t seed, uint32_t site, uint32_t step) {
  return !tnt_keep(e, rate, seed, site, step);
}

template <bool VEC>
__global__ __launch_bounds__(256) void input_corrupt_kernel(CorruptArgs a) {
  const uint32_t step = a.step_dev[0];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.nscan) {
    // ---- scan part: columns [c0, c1) of row b, decided by element b of site_scan
    const int b = (int)blockIdx.x / a.nchunk;
    if (!fires((uint64_t)b, a.scan_rate, a.seed, a.site_scan, step)) return;
    const int c0 = ((int)blockIdx.x % a.nchunk) * SCAN_CHUNK;
    const int c1 = a.N - c0 < SCAN_CHUNK ? a.N : c0 + SCAN_CHUNK;
    float* row = a.x + (long)b * a.ldx;
    const float* nul = a.null_scan;
    if (VEC) {
      const int c = c0 + tid * 4;        // (N % 4 == 0: a float4 that starts below c1 ends below it)
      if (c < c1) {
        const float4 v = nul ? *reinterpret_cast<const float4*>(nul + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(row + c) = v;
      }
    } else {
      for (int c = c0 + tid; c < c1; c += 256) row[c] = nul ? nul[c] : 0.f;
    }
    if (a.xT != nullptr)       // the voxel-major copy: column b, one float per voxel row
      for (int c = c0 + tid; c < c1; c += 256) a.xT[(long)c * a.ldt + b] = nul ? nul[c] : 0.f;
    return;
  }
  // ---- word part: positions e = b*T + t, four per thread (one Philox call)
  const long g = (long)((int)blockIdx.x - a.nscan) * 256 + tid;
  const long e0 = g * 4;
  if (e0 >= a.n_tok) return;
  bool keep[4];
  tnt_keep4((uint64_t)e0, a.word_rate, a.seed, a.site_word, step, keep);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long e = e0 + j;
    if (e >= a.n_tok || keep[j]) continue;
    if (e % a.T == 0) continue;             // column 0: the start token
    if (a.cap[e] == 0) continue;            // id 0: padding, the mask id
    a.cap[e] = a.unk_id;
  }
}

}  // namespace

/* see include/tnt_hip.h */
extern "C" int32_t tnt_input_corrupt_f32(float* x, int32_t ldx, float* xT, int32_t ldt, int32_t* cap, int32_t B, int32_t T,
                                         int32_t N, int32_t V, float scan_rate, const float* null_scan, float word_rate,
                                         int32_t unk_id, uint64_t seed, uint32_t site_scan, uint32_t site_word,
                                         const uint32_t* step_dev, void* stream) {
  if (!(scan_rate >= 0.f && scan_rate <= 1.f)) return TNT_BADARG(9);       // (NaN fails both comparisons)
  if (!(word_rate >= 0.f && word_rate <= 1.f)) return TNT_BADARG(11);
  if (word_rate > 0.f && (unk_id < 1 || unk_id >= V)) return TNT_BADARG(12);
  if (B < 0 || T < 0 || N < 0) return TNT_BADARG(5);
  if (ldx < N) return TNT_BADARG(1);
  if (xT != nullptr && ldt < B) return TNT_BADARG(3);
  if (step_dev == nullptr) return TNT_BADARG(16);
  if (scan_rate > 0.f && x == nullptr) return TNT_BADARG(0);
  if (word_rate > 0.f && cap == nullptr) return TNT_BADARG(4);
  CorruptArgs a{};
  a.x = x; a.xT = scan_rate > 0.f ? xT : nullptr; a.cap = cap; a.null_scan = null_scan; a.step_dev = step_dev;
  a.ldx = ldx; a.ldt = ldt; a.B = B; a.T = T; a.N = N; a.unk_id = unk_id;
  a.scan_rate = scan_rate; a.word_rate = word_rate; a.seed = seed; a.site_scan = site_scan; a.site_word = site_word;
  a.nchunk = (N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  const long nscan = (scan_rate > 0.f && N > 0) ? (long)B * a.nchunk : 0;
  a.n_tok = word_rate > 0.f ? (long)B * T : 0;
  const long nword = (a.n_tok + 1023) / 1024;      // 256 threads x 4 positions
  const long grid = nscan + nword;
  if (grid == 0) return 0;
  if (grid > 0x7fffffffL) return TNT_BADARG(5);
  a.nscan = (int)nscan;
  const bool vec = (N % 4 == 0) && (ldx % 4 == 0) && tnt_aligned16(x) && tnt_aligned16(null_scan);
  if (vec)
    hipLaunchKernelGGL(input_corrupt_kernel<true>, dim3((unsigned)grid), dim3(256), 0, tnt_stream(stream), a);
  else
    hipLaunchKernelGGL(input_corrupt_kernel<false>, dim3((unsigned)grid), dim3(256), 0, tnt_stream(stream), a);
  TNT_LAUNCH_CHECK();
  return 0;
}
