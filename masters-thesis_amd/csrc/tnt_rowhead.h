// How a 256-thread workgroup walks one logits row of a softmax head: loading the row, its maximum, the FIRST index holding
// it (np.argmax / tf.argmax rule), the exp-sum, the four-wave block reductions, and the host-side ladder that picks the
// row kind from V and the alignment.  Used by smooth.hip, unlikely.hip, weighted.hip, scst.hip and score.hip, whose kernels
// exist once as a template over the row kind and keep only their own write phase.  seqops.hip takes the ladder alone: the
// kernels of tnt_softmax_cce_f32 / tnt_softmax_cce_live_f32 run on the benchmarked training step and keep their own text,
// so that a change here can never move them.
#pragma once
#include <type_traits>
#include "tnt_common.h"

// ---- the ladder.  launch(tnt_nv4<N>{}) with N the row kind: the smallest window 1024 N of {1, 2, 4, 5, 8} that holds V
// if the caller's rows allow float4 access (ld % 4 == 0 and every row pointer 16-byte aligned), N = 0 (the re-reading row)
// otherwise and for V > 8192.  tests/test_host_softmax_dispatch.py parses these rungs.
template <int N> using tnt_nv4 = std::integral_constant<int, N>;

template <class F>
static inline void tnt_row_ladder(bool aligned, int V, F&& launch) {
  const int nv4 = (V + 1023) / 1024;
  if (aligned && nv4 == 1) launch(tnt_nv4<1>{});
  else if (aligned && nv4 == 2) launch(tnt_nv4<2>{});
  else if (aligned && nv4 <= 4) launch(tnt_nv4<4>{});
  else if (aligned && nv4 <= 5) launch(tnt_nv4<5>{});
  else if (aligned && nv4 <= 8) launch(tnt_nv4<8>{});
  else launch(tnt_nv4<0>{});
}

// ---- four-wave block reductions: ONE barrier each, none behind the combine.  So sh must not be the array of the reduction
// in front of this one, which slower waves may still be combining: consecutive reductions alternate between two arrays.
// An array is free again behind the barrier of the reduction that follows its own (a loop over rows may reuse the pair).
__device__ __forceinline__ float tnt_block_max4(float v, float* sh) {
  v = tnt_wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__device__ __forceinline__ float tnt_block_sum4(float v, float* sh) {
  v = tnt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// a wave-uniform value that rides on the barrier of the next block reduction instead of paying for its own: posted here,
// combined by the caller from sh[0 .. 3] behind that barrier
template <class T>
__device__ __forceinline__ void tnt_wave_post(T v, T* sh) {
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}

// ---- the row.  NV4 >= 1: register-resident (V <= 1024 NV4, ld % 4 == 0, 16-byte aligned): thread tid holds float4 i of
// columns 4 (tid + 256 i) .. + 3, read once.  NV4 == 0: re-reading (any V, ld, alignment): thread tid walks columns tid,
// tid + 256, ... again in every phase (from the L2).  Neither kind knows what its caller computes or writes.
template <int NV4>
struct TntRow {
  const float* x;
  int V;
  float4 d[NV4 > 0 ? NV4 : 1];               // NV4 == 0: unused

  // load + maximum: the row's maximum, one barrier.  Columns >= V read as -inf whatever the pad holds; a quad is fetched
  // only if its first column is < V, so (V <= ld, ld % 4 == 0) nothing at or past ld is ever read.
  __device__ __forceinline__ float max(float* shm) {
    const int tid = threadIdx.x;
    float m = -INFINITY;
    if constexpr (NV4 > 0) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        const int j = 4 * (tid + 256 * i);
        d[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (j < V) {
          d[i] = *reinterpret_cast<const float4*>(x + j);
          if (j + 1 >= V) d[i].y = -INFINITY;
          if (j + 2 >= V) d[i].z = -INFINITY;
          if (j + 3 >= V) d[i].w = -INFINITY;
        }
        m = fmaxf(m, fmaxf(fmaxf(d[i].x, d[i].y), fmaxf(d[i].z, d[i].w)));
      }
    } else {
      for (int j = tid; j < V; j += 256) m = fmaxf(m, x[j]);
    }
    return tnt_block_max4(m, shm);
  }

  // load + maximum + first index holding it, one barrier.  Register row: the index is found by an equality pass over the
  // registers behind the barrier and only POSTED to shi per wave; first() combines it behind the caller's next barrier.
  // Re-reading row: one scan tracks (value, index), larger value wins, ties go to the smaller index; final on return.
  __device__ __forceinline__ float max_first(float* shm, int* shi, int& am) {
    const int tid = threadIdx.x;
    float m;
    am = 0x7fffffff;
    if constexpr (NV4 > 0) {
      m = max(shm);
#pragma unroll
      for (int i = NV4 - 1; i >= 0; --i) {
        const int j = 4 * (tid + 256 * i);
        if (d[i].w == m) am = j + 3;
        if (d[i].z == m) am = j + 2;
        if (d[i].y == m) am = j + 1;
        if (d[i].x == m) am = j;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
      tnt_wave_post(am, shi);
    } else {
      m = -INFINITY;
      for (int j = tid; j < V; j += 256) {
        const float v = x[j];
        if (v > m) { m = v; am = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float bv = __shfl_xor(m, o, 64);
        const int bi = __shfl_xor(am, o, 64);
        if (bv > m || (bv == m && bi < am)) { m = bv; am = bi; }
      }
      tnt_wave_post(m, shm);
      tnt_wave_post(am, shi);
      __syncthreads();
      m = shm[0]; am = shi[0];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (shm[k] > m || (shm[k] == m && shi[k] < am)) { m = shm[k]; am = shi[k]; }
    }
    return m;
  }

  // the row's first maximum index, behind the first barrier after max_first()
  __device__ __forceinline__ int first(const int* shi, int am) const {
    if constexpr (NV4 > 0) return min(min(shi[0], shi[1]), min(shi[2], shi[3]));
    else return am;
  }

  // the thread's part of sum_v exp(x_v - m).  Register row: d becomes exp(d - m) (0 in the columns >= V); the pairs of a
  // float4 are added first, then the quads in order of i.  Re-reading row: one accumulator at stride 256.  The order is
  // part of every caller's result.
  __device__ __forceinline__ float exp_sum(float m) {
    float s = 0.f;
    if constexpr (NV4 > 0) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        d[i].x = expf(d[i].x - m); d[i].y = expf(d[i].y - m); d[i].z = expf(d[i].z - m); d[i].w = expf(d[i].w - m);
        s += (d[i].x + d[i].y) + (d[i].z + d[i].w);
      }
    } else {
      for (int j = threadIdx.x; j < V; j += 256) s += expf(x[j] - m);
    }
    return s;
  }
};
