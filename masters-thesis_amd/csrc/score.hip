// Caption log-likelihood scoring (nic.NIC.score_captions / lc_nic.NIC.score_captions): log p(caption | scan) per caption
// from the teacher-forced logits, read-only.  Definition in include/tnt_hip.h (tnt_caption_score_f32); restated by
// tests/score_oracle.py.
//
// Per logits row: max, exp-sum (the row walk and the block reductions of tnt_rowhead.h), lp = x_w - (m + log Z); nothing
// is written to the row.  The register-resident row keeps the row in VGPRs between the two passes (V <= 1024 * NV4,
// 16-byte aligned rows, ld % 4 == 0), so a counted row is read from HBM once; the re-reading row (NV4 = 0) reads it twice.  In front of it the terminator scan of
// the caption's ids w_1..w_{j-1} decides whether the row counts; a row that does not never reads its logits.
//
// The per-caption sum, two forms, both in ascending position order in float32, so their results are the same bits and
// the same bits run to run (no floating-point atomics):
//  - tok_lp given (what the models pass): one workgroup per logits row writes tok_lp, and a second small launch (one thread
//    per caption) walks the caption's ids again, adds its tok_lp entries and counts them.  The row grid has steps * R
//    workgroups: R = 64 captions of 14 positions are 896 workgroups on 256 CUs, where one workgroup per caption would
//    leave three quarters of the chip idle through 14 dependent row passes.  tok_lp is steps * R floats against
//    steps * R * V logits, so the second launch moves nothing that matters; it costs one launch.
//  - tok_lp null: there is nowhere to stage the row values, so one workgroup per caption walks its counted rows one
//    after the other and keeps the sum in a register.  Fine for many captions (R >= a few hundred); the caller that
//    has few passes tok_lp.
#include "tnt_rowhead.h"

namespace {

struct ScoreArgs {
  const float* logits;
  const int* cap;
  float* tok_lp;
  float* cap_lp;
  int* cap_len;
  int ld, V, T, steps, R, end_id;
};

// lp of one counted row with a valid id w, by the whole 256-thread workgroup; NV4 = 0: the generic re-reading path.  shm and
// shz: the two arrays the row's two reductions alternate between (tnt_rowhead.h), also from row to row.
template <int NV4>
__device__ __forceinline__ float score_row_lp(const float* x, int V, int w, float* shm, float* shz) {
  TntRow<NV4> row{x, V};
  const float m = row.max(shm);
  const float Z = tnt_block_sum4(row.exp_sum(m), shz);
  return x[w] - (m + logf(Z));
}

// one workgroup per logits row (j - 1) * R + r: tok_lp
template <int NV4>
__global__ __launch_bounds__(256) void caption_score_row_kernel(ScoreArgs a) {
  __shared__ float shm[4], shz[4];
  const int row = blockIdx.x;
  const int r = row % a.R, j = row / a.R + 1;            // 1 <= j <= steps <= T - 1
  const int* c = a.cap + (long)r * a.T;
  int hit = 0;
  for (int q = 1 + (int)threadIdx.x; q < j; q += 256) {
    const int id = c[q];
    hit |= (id == 0 || id == a.end_id);
  }
  const bool ended = __syncthreads_or(hit) != 0;
  const int w = c[j];
  float lp = 0.f;
  if (!ended && w != 0) {
    if (w < 0 || w >= a.V) lp = NAN;
    else lp = score_row_lp<NV4>(a.logits + (long)row * a.ld, a.V, w, shm, shz);
  }
  if (threadIdx.x == 0) a.tok_lp[row] = lp;
}

// one thread per caption: the sum of its tok_lp entries in ascending position order, and their number
__global__ __launch_bounds__(256) void caption_score_sum_kernel(ScoreArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const int* c = a.cap + (long)r * a.T;
  float sum = 0.f;
  int len = 0;
  bool ended = false;
  for (int j = 1; j <= a.steps && !ended; ++j) {
    const int w = c[j];
    if (w != 0) {
      sum += a.tok_lp[(long)(j - 1) * a.R + r];
      ++len;
    }
    ended = (w == 0 || w == a.end_id);
  }
  a.cap_lp[r] = sum;
  if (a.cap_len) a.cap_len[r] = len;
}

// one workgroup per caption (no tok_lp): its counted rows one after the other
template <int NV4>
__global__ __launch_bounds__(256) void caption_score_cap_kernel(ScoreArgs a) {
  __shared__ float shm[4], shz[4];
  const int r = blockIdx.x;
  const int* c = a.cap + (long)r * a.T;
  float sum = 0.f;
  int len = 0;
  bool ended = false;
  for (int j = 1; j <= a.steps && !ended; ++j) {         // uniform over the workgroup: every thread reads the same ids
    const int w = c[j];
    if (w != 0) {
      const long row = (long)(j - 1) * a.R + r;
      sum += (w < 0 || w >= a.V) ? NAN : score_row_lp<NV4>(a.logits + row * a.ld, a.V, w, shm, shz);
      ++len;
    }
    ended = (w == 0 || w == a.end_id);
  }
  if (threadIdx.x == 0) {
    a.cap_lp[r] = sum;
    if (a.cap_len) a.cap_len[r] = len;
  }
}

}  // namespace

extern "C" int32_t tnt_caption_score_f32(const float* logits, int32_t ld, int32_t V, const int32_t* cap, int32_t T,
                                         int32_t steps, int32_t R, int32_t end_id, float* tok_lp, float* cap_lp,
                                         int32_t* cap_len, void* stream) {
  if (!logits || !cap || !cap_lp) return TNT_BADARG(0);
  if (V < 1 || ld < V || T < 2 || R < 1 || end_id >= V) return TNT_BADARG(1);
  if (steps < 1 || steps > T - 1) return TNT_BADARG(2);
  if ((long)steps * R > 0x7fffffffL) return TNT_BADARG(3);
  ScoreArgs a{logits, cap, tok_lp, cap_lp, cap_len, ld, V, T, steps, R, end_id};
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits);
  if (tok_lp) {
    tnt_row_ladder(al, V, [&](auto n) {
      hipLaunchKernelGGL((caption_score_row_kernel<decltype(n)::value>), dim3(steps * R), dim3(256), 0, s, a);
    });
    TNT_LAUNCH_CHECK();
    hipLaunchKernelGGL(caption_score_sum_kernel, dim3((R + 255) / 256), dim3(256), 0, s, a);
  } else {
    tnt_row_ladder(al, V, [&](auto n) {
      hipLaunchKernelGGL((caption_score_cap_kernel<decltype(n)::value>), dim3(R), dim3(256), 0, s, a);
    });
  }
  TNT_LAUNCH_CHECK();
  return 0;
}
