// Caption log-likelihood scoring (nic.NIC.score_captions / lc_nic.NIC.score_captions): log p(caption | scan) per caption
// from the teacher-forced logits, read-only.  Definition in include/tnt_hip.h (tnt_caption_score_f32); restated by
// tests/score_oracle.py.
//
// Per logits row the structure of softmax_cce (seqops.hip) without its write: max, exp-sum, lp = x_w - (m + log Z).  The
// register-resident variant keeps the row in VGPRs between the two passes (V <= 1024 * NV4, 16-byte aligned rows,
// ld % 4 == 0), so a counted row is read from HBM once; the generic one re-reads it.  In front of it the terminator scan of
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
#include "tnt_common.h"

namespace {

struct ScoreArgs {
  const float* logits;
  const int* cap;
  float* tok_lp;
  float* cap_lp;
  int* cap_len;
  int ld, V, T, steps, R, end_id;
};

__device__ __forceinline__ float score_block_max4(float v, float* sh) {
  v = tnt_wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return r;
}

__device__ __forceinline__ float score_block_sum4(float v, float* sh) {
  v = tnt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}

// lp of one counted row with a valid id w, by the whole 256-thread workgroup; NV4 = 0: the generic re-reading path
template <int NV4>
__device__ __forceinline__ float score_row_lp(const float* x, int V, int w, float* sh) {
  const int tid = threadIdx.x;
  float m = -INFINITY, s = 0.f;
  if constexpr (NV4 > 0) {
    float4 v[NV4];
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      v[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (j + 3 < V) {
        v[i] = *reinterpret_cast<const float4*>(x + j);
      } else if (j < V) {                      // the row's last quad: the pad columns V .. ld-1 are not read
        v[i].x = x[j];
        if (j + 1 < V) v[i].y = x[j + 1];
        if (j + 2 < V) v[i].z = x[j + 2];
      }
      m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    }
    m = score_block_max4(m, sh);
#pragma unroll
    for (int i = 0; i < NV4; ++i)
      s += (expf(v[i].x - m) + expf(v[i].y - m)) + (expf(v[i].z - m) + expf(v[i].w - m));
  } else {
    for (int j = tid; j < V; j += 256) m = fmaxf(m, x[j]);
    m = score_block_max4(m, sh);
    for (int j = tid; j < V; j += 256) s += expf(x[j] - m);
  }
  const float Z = score_block_sum4(s, sh);
  return x[w] - (m + logf(Z));
}

// one workgroup per logits row (j - 1) * R + r: tok_lp
template <int NV4>
__global__ __launch_bounds__(256) void caption_score_row_kernel(ScoreArgs a) {
  __shared__ float sh[4];
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
    else lp = score_row_lp<NV4>(a.logits + (long)row * a.ld, a.V, w, sh);
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
  __shared__ float sh[4];
  const int r = blockIdx.x;
  const int* c = a.cap + (long)r * a.T;
  float sum = 0.f;
  int len = 0;
  bool ended = false;
  for (int j = 1; j <= a.steps && !ended; ++j) {         // uniform over the workgroup: every thread reads the same ids
    const int w = c[j];
    if (w != 0) {
      const long row = (long)(j - 1) * a.R + r;
      sum += (w < 0 || w >= a.V) ? NAN : score_row_lp<NV4>(a.logits + row * a.ld, a.V, w, sh);
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
  const int nv4 = al ? (V + 1023) / 1024 : 99;
#define TNT_SCORE(K, G) \
  do { \
    if (nv4 == 1) hipLaunchKernelGGL((K<1>), dim3(G), dim3(256), 0, s, a); \
    else if (nv4 == 2) hipLaunchKernelGGL((K<2>), dim3(G), dim3(256), 0, s, a); \
    else if (nv4 <= 4) hipLaunchKernelGGL((K<4>), dim3(G), dim3(256), 0, s, a); \
    else if (nv4 <= 5) hipLaunchKernelGGL((K<5>), dim3(G), dim3(256), 0, s, a); \
    else if (nv4 <= 8) hipLaunchKernelGGL((K<8>), dim3(G), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((K<0>), dim3(G), dim3(256), 0, s, a); \
  } while (0)
  if (tok_lp) {
    TNT_SCORE(caption_score_row_kernel, steps * R);
    TNT_LAUNCH_CHECK();
    hipLaunchKernelGGL(caption_score_sum_kernel, dim3((R + 255) / 256), dim3(256), 0, s, a);
  } else {
    TNT_SCORE(caption_score_cap_kernel, R);
  }
#undef TNT_SCORE
  TNT_LAUNCH_CHECK();
  return 0;
}
