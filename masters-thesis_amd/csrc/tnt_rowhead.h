// The front of a one-workgroup-per-row softmax head (256 threads): loading the row, its maximum and the FIRST index
// holding it (np.argmax / tf.argmax rule).  Shared by smooth.hip and unlikely.hip; the kernels of tnt_softmax_cce_f32
// (seqops.hip) keep their own text.
#pragma once
#include "tnt_common.h"

// register-resident row (V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned): thread tid loads its float4 i from column
// 4 (tid + 256 i); pad columns [V, ld) and everything past ld read as -inf.  Returns the thread's own maximum.
template <int NV4>
__device__ __forceinline__ float tnt_row_load_max(const float* x, int tid, int V, int ld, float4 (&d)[NV4]) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int j = 4 * (tid + 256 * i);
    d[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (j < ld) {
      d[i] = *reinterpret_cast<const float4*>(x + j);
      if (j + 1 >= V) d[i].y = -INFINITY;
      if (j + 2 >= V) d[i].z = -INFINITY;
      if (j + 3 >= V) d[i].w = -INFINITY;
      if (j >= V) d[i].x = -INFINITY;
    }
    m = fmaxf(m, fmaxf(fmaxf(d[i].x, d[i].y), fmaxf(d[i].z, d[i].w)));
  }
  return m;
}

// the wave's smallest column whose value equals the row maximum m (0x7fffffff if the wave holds none)
template <int NV4>
__device__ __forceinline__ int tnt_row_first_max(const float4 (&d)[NV4], float m, int tid) {
  int am = 0x7fffffff;
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
  return am;
}

// re-reading row (any V, ld, alignment): the wave's maximum over columns tid, tid + 256, ... and its first index
__device__ __forceinline__ void tnt_row_scan_argmax(const float* x, int V, int tid, float& m, int& am) {
  m = -INFINITY;
  am = 0x7fffffff;
  for (int j = tid; j < V; j += 256) {
    const float v = x[j];
    if (v > m) { m = v; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                         // larger value wins; ties -> smaller index
    const float bv = __shfl_xor(m, o, 64);
    const int bi = __shfl_xor(am, o, 64);
    if (bv > m || (bv == m && bi < am)) { m = bv; am = bi; }
  }
}

// the four waves' (maximum, first index) pairs, left in LDS behind a barrier, combined by every thread
__device__ __forceinline__ void tnt_row_combine_argmax(const float* shm, const int* shi, float& m, int& am) {
  m = shm[0]; am = shi[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (shm[k] > m || (shm[k] == m && shi[k] < am)) { m = shm[k]; am = shi[k]; }
}
