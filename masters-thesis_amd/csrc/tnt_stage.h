// Device code of the per-step batch staging, shared by the staging kernel (rowops.hip) and the streaming encoder forward
// that carries the staging as rider workgroups (encoder.hip): one copy of the row map and of the copy loop.
// Every function here expects a workgroup of 256 threads.
#pragma once
#include "tnt_common.h"
#include <hip/hip_fp16.h>

namespace {

// One launch for the per-step input staging of a batch that is already on the device
// (data_generator_guse.py:156-171 tuple -> the static buffers of the captured step).
// XT = float, or __half when the betas crossed PCIe as IEEE half ("fp16 on-wire", SURVEY 8f rank 1: at full-cortex
// width the 84 MB float batch is what bounds the step); the widening to float happens here, in the same pass.
template <typename XT>
struct StageArgs {
  const XT* x; float* xd; const int* cap; int* capd; const int* tgt; int* tgtd;
  const float* a0; float* h0; const float* c0; float* c0d;
  int B, T, N, ldx, U;
  float* xT; int ldt; int ncopy;      // optional voxel-major copy xT[N][ldt] (blocks >= ncopy transpose 64x64 tiles)
  // optional riding job (blocks >= nstage): the keep masks of tnt_dropout_mask4_u8 for the step that this batch feeds
  uint8_t* mk_out; long mk_n4, mk_total; float mk_rate; uint64_t mk_seed; uint32_t mk_site0; const uint32_t* mk_step_dev;
  int nstage;
  // optional riding job (the LAST block): the row map of the vocabulary head (tnt_stage_batch_map_f32)
  int* map_pos; float* map_w; int* map_tgt; int* map_live; float* map_loss; float* map_corr;
};
// Row map of the vocabulary head, one workgroup.  The text LSTM carries its output through a step that is fed id 0, so position
// (t, b) with cap[b][t] == 0, t >= 1, holds the SAME output row as the nearest earlier position of caption b that has a row;
// where its target is the same too, logits, loss and dlogits repeat and the position is merged into that row (pos = -1, the
// row's multiplicity + 1).  Every other position gets a row of its own, numbered in time-major order (stable: deterministic).
// A fed 0 whose target differs keeps its own row (the chain writes the carried output there): correct for any input.
constexpr int STAGE_MAP_LDS = 1024;      // positions the map holds in LDS (3 arrays + the scan counts inside the 64 x 65 tile)
// ... with caption ids, targets and the map itself in LDS: every global access is one coalesced pass (B * T <= STAGE_MAP_LDS)
template <typename SA>
__device__ __forceinline__ void stage_rowmap_lds(const SA& a, int* lds) {
  int* s_cap = lds; int* s_tgt = lds + STAGE_MAP_LDS; int* s_pos = lds + 2 * STAGE_MAP_LDS; int* s_cnt = lds + 3 * STAGE_MAP_LDS;
  const int B = a.B, T = a.T, n = B * T, tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) { s_cap[i] = a.cap[i]; s_tgt[i] = a.tgt[i]; }
  __syncthreads();
  for (int b = tid; b < B; b += 256) {
    int rep_y = 0;
    for (int t = 0; t < T; ++t) {
      const int id = s_cap[b * T + t], y = s_tgt[b * T + t];
      const bool merged = t > 0 && id == 0 && y == rep_y;
      s_pos[t * B + b] = merged ? -1 : 1;
      if (!merged) rep_y = y;
    }
  }
  __syncthreads();
  const int per = (n + 255) / 256, lo = min(tid * per, n), hi = min(lo + per, n);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += s_pos[i] > 0 ? 1 : 0;
  s_cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < 256; ++k) { const int v = s_cnt[k]; s_cnt[k] = run; run += v; }
    s_cnt[256] = run;
    a.map_live[0] = run;
  }
  __syncthreads();
  int idx = s_cnt[tid];
  const int live = s_cnt[256];
  for (int i = lo; i < hi; ++i)
    if (s_pos[i] > 0) s_pos[i] = idx++;
  __syncthreads();
  for (int b = tid; b < B; b += 256) {
    int rep = -1, cnt = 0;
    for (int t = 0; t < T; ++t) {
      const int p = s_pos[t * B + b];
      if (p >= 0) {
        if (rep >= 0) a.map_w[rep] = (float)cnt;
        rep = p; cnt = 1;
        a.map_tgt[p] = s_tgt[b * T + t];
      } else {
        ++cnt;
      }
    }
    if (rep >= 0) a.map_w[rep] = (float)cnt;
  }
  for (int i = tid; i < n; i += 256) a.map_pos[i] = s_pos[i];
  for (int i = live + tid; i < n; i += 256) {
    a.map_w[i] = 0.f; a.map_tgt[i] = 0;
    if (a.map_loss) a.map_loss[i] = 0.f;
    if (a.map_corr) a.map_corr[i] = 0.f;
  }
}
// ... any size: the map is worked on in place in global memory (a workgroup barrier orders the passes)
template <typename SA>
__device__ __forceinline__ void stage_rowmap(const SA& a, int* s_cnt) {
  const int B = a.B, T = a.T, n = B * T, tid = threadIdx.x;
  for (int b = tid; b < B; b += 256) {                    // 1: which positions have a row (1) or are merged (-1)
    int rep_y = 0;
    for (int t = 0; t < T; ++t) {
      const int id = a.cap[b * T + t], y = a.tgt[b * T + t];
      const bool merged = t > 0 && id == 0 && y == rep_y;
      a.map_pos[t * B + b] = merged ? -1 : 1;
      if (!merged) rep_y = y;
    }
  }
  __syncthreads();
  const int per = (n + 255) / 256, lo = min(tid * per, n), hi = min(lo + per, n);
  int c = 0;                                             // 2: number the rows, time-major
  for (int i = lo; i < hi; ++i) c += a.map_pos[i] > 0 ? 1 : 0;
  s_cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < 256; ++k) { const int v = s_cnt[k]; s_cnt[k] = run; run += v; }
    s_cnt[256] = run;
    a.map_live[0] = run;
  }
  __syncthreads();
  int idx = s_cnt[tid];
  const int live = s_cnt[256];
  for (int i = lo; i < hi; ++i)
    if (a.map_pos[i] > 0) a.map_pos[i] = idx++;
  __syncthreads();
  for (int b = tid; b < B; b += 256) {                    // 3: multiplicities and targets of the rows
    int rep = -1, cnt = 0;
    for (int t = 0; t < T; ++t) {
      const int p = a.map_pos[t * B + b];
      if (p >= 0) {
        if (rep >= 0) a.map_w[rep] = (float)cnt;
        rep = p; cnt = 1;
        a.map_tgt[p] = a.tgt[b * T + t];
      } else {
        ++cnt;
      }
    }
    if (rep >= 0) a.map_w[rep] = (float)cnt;
  }
  for (int i = live + tid; i < n; i += 256) {             // rows past the live extent: nothing, and they sum to nothing
    a.map_w[i] = 0.f; a.map_tgt[i] = 0;
    if (a.map_loss) a.map_loss[i] = 0.f;
    if (a.map_corr) a.map_corr[i] = 0.f;
  }
}
__device__ __forceinline__ float stage_ld(const float* p) { return *p; }
__device__ __forceinline__ float stage_ld(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float4 stage_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 stage_ld4(const __half* p) {          // 8-byte aligned: 4 halves
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  const __half2 lo = *reinterpret_cast<const __half2*>(&u.x), hi = *reinterpret_cast<const __half2*>(&u.y);
  const float2 a = __half22float2(lo), b = __half22float2(hi);
  return make_float4(a.x, a.y, b.x, b.y);
}
// the row-map workgroup: `lds` holds (3 * STAGE_MAP_LDS + 257) ints
template <typename SA>
__device__ __forceinline__ void stage_rowmap_block(const SA& a, int* lds) {
  if (a.B * a.T <= STAGE_MAP_LDS) stage_rowmap_lds(a, lds);
  else stage_rowmap(a, lds);
}
// copy workgroup `blk` of a.ncopy: the betas (widened to float) into the padded rows of xd, ids, time-major targets, states
template <typename SA>
__device__ __forceinline__ void stage_copy(const SA& a, int blk) {
  const long gid = (long)blk * 256 + threadIdx.x, gsz = (long)a.ncopy * 256;
  if (a.N % 4 == 0 && a.ldx % 4 == 0) {
    const int n4 = a.N / 4;
    for (long e = gid; e < (long)a.B * n4; e += gsz) {
      const int r = (int)(e / n4), c = (int)(e % n4) * 4;
      *reinterpret_cast<float4*>(a.xd + (long)r * a.ldx + c) = stage_ld4(a.x + (long)r * a.N + c);
    }
  } else {
    for (long e = gid; e < (long)a.B * a.N; e += gsz) {
      const int r = (int)(e / a.N), c = (int)(e % a.N);
      a.xd[(long)r * a.ldx + c] = stage_ld(a.x + e);
    }
  }
  const int bt = a.B * a.T, bu = a.B * a.U;
  for (long e = gid; e < bt; e += gsz) {
    a.capd[e] = a.cap[e];
    if (a.tgt) { const int b = (int)(e / a.T), t = (int)(e % a.T); a.tgtd[t * a.B + b] = a.tgt[e]; }
  }
  for (long e = gid; e < bu; e += gsz) { a.h0[e] = a.a0[e]; a.c0d[e] = a.c0[e]; }
}

}  // namespace
