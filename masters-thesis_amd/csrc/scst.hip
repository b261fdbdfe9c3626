// Self-critical sequence training loss (Rennie et al. 2017) for the dense caption model's SCST step
// (nic.NIC(self_critical=...)): the REINFORCE loss of the sampled captions and its logits gradient, one launch.
// Definition in include/tnt_hip.h (tnt_scst_cce_f32); restated by tests/scst_oracle.py.
//
// One 256-thread workgroup per logits row: max, exp-sum (the row walk and the block reductions of tnt_rowhead.h), write.
// In front of it, the terminator scan of the row's sampled ids w_1..w_{t-1} (at most T ids, one block-wide OR) decides whether the
// row counts at all; a row past the caption's end (and a row whose advantage is 0 when nobody wants its log-probability)
// never reads its logits and writes a zero gradient row.  One kernel template: the register-resident row (NV4 >= 1) keeps
// the row in VGPRs between the passes (V <= 1024 * NV4, 16-byte aligned rows, ld % 4 == 0); the re-reading row (NV4 == 0)
// reads it again in each.
#include "tnt_rowhead.h"

namespace {

struct ScstArgs {
  const float* logits;
  const int* fed;
  const int* last;
  const float* adv;
  float* loss_row;
  float* lp_row;
  float* dlogits;
  int ld, V, T, R, end_id;
  float gscale;
};

// what a row does: 0 = zero row (past the terminator, or adv = 0 with no lp_row), 1 = compute, 2 = bad id
struct RowHead { int kind; int w; float adv; };

__device__ __forceinline__ RowHead scst_head(const ScstArgs& a, int row) {
  const int r = row % a.R, t = row / a.R + 1;
  const int* f = a.fed + (long)r * a.T;
  int hit = 0;
  for (int j = 1 + (int)threadIdx.x; j < t; j += 256) {
    const int id = f[j];
    hit |= (id == 0 || id == a.end_id);
  }
  const bool ended = __syncthreads_or(hit) != 0;
  RowHead h;
  h.w = t < a.T ? f[t] : a.last[r];
  h.adv = a.adv[r];
  h.kind = (ended || (h.adv == 0.f && !a.lp_row)) ? 0 : ((h.w < 0 || h.w >= a.V) ? 2 : 1);
  return h;
}

__device__ __forceinline__ void scst_zero_grad(const ScstArgs& a, int row, bool vec) {
  float* d = a.dlogits + (long)row * a.ld;
  if (vec) {
    const int n4 = a.V >> 2;
    for (int q = threadIdx.x; q < n4; q += 256) *reinterpret_cast<float4*>(d + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 4 * n4 + threadIdx.x; j < a.V; j += 256) d[j] = 0.f;
  } else {
    for (int j = threadIdx.x; j < a.V; j += 256) d[j] = 0.f;
  }
}

// a row that does not count (val 0) or holds a bad id (val NaN): zero gradient, loss_row = lp_row = val
__device__ __forceinline__ void scst_zero(const ScstArgs& a, int row, bool vec, float val) {
  scst_zero_grad(a, row, vec);
  if (threadIdx.x == 0) {
    if (a.loss_row) a.loss_row[row] = val;
    if (a.lp_row) a.lp_row[row] = val;
  }
}

// loss_row / lp_row of a counted row, and the per-element gradient scale; lse = m + log Z
__device__ __forceinline__ float scst_finish(const ScstArgs& a, int row, const RowHead& h, float xw, float m, float Z) {
  const float lp = xw - (m + logf(Z));
  if (threadIdx.x == 0) {
    if (a.loss_row) a.loss_row[row] = h.adv == 0.f ? 0.f : -h.adv * lp;
    if (a.lp_row) a.lp_row[row] = lp;
  }
  return a.gscale * h.adv;
}

// NV4 >= 1: register-resident row (V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned rows); NV4 == 0: re-reading row (any V,
// ld, alignment).  Neither writes a pad column.
template <int NV4>
__global__ __launch_bounds__(256) void scst_cce_kernel(ScstArgs a) {
  __shared__ float shm[4], shz[4];
  constexpr bool vec = NV4 > 0;
  const int row = blockIdx.x, tid = threadIdx.x;
  const RowHead h = scst_head(a, row);
  if (h.kind != 1) { scst_zero(a, row, vec, h.kind == 0 ? 0.f : NAN); return; }
  const float* x = a.logits + (long)row * a.ld;
  const int V = a.V;
  TntRow<NV4> w{x, V};
  const float xw = x[h.w];                 // before the barriers: the gradient may overwrite the row (dlogits == logits)
  const float m = w.max(shm);
  const float Z = tnt_block_sum4(w.exp_sum(m), shz);         // its barrier: every read of the row precedes every write below
  const float g = scst_finish(a, row, h, xw, m, Z);
  float* d = a.dlogits + (long)row * a.ld;
  if (g == 0.f) {                          // adv = 0 with lp_row wanted: the log-probability only
    scst_zero_grad(a, row, vec);
    return;
  }
  const float gz = g / Z;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      if (j >= V) continue;
      float4 o = make_float4(w.d[i].x * gz, w.d[i].y * gz, w.d[i].z * gz, w.d[i].w * gz);
      if (j == h.w) o.x -= g;
      if (j + 1 == h.w) o.y -= g;
      if (j + 2 == h.w) o.z -= g;
      if (j + 3 == h.w) o.w -= g;
      if (j + 3 < V) {
        *reinterpret_cast<float4*>(d + j) = o;
      } else {
        d[j] = o.x;
        if (j + 1 < V) d[j + 1] = o.y;
        if (j + 2 < V) d[j + 2] = o.z;
      }
    }
  } else {
    // every thread reads its own elements before overwriting them (dlogits may alias logits)
    for (int j = tid; j < V; j += 256) d[j] = expf(x[j] - m) * gz - (j == h.w ? g : 0.f);
  }
}

}  // namespace

extern "C" int32_t tnt_scst_cce_f32(const float* logits, int32_t ld, int32_t V, const int32_t* fed, int32_t T,
                                    const int32_t* last, const float* adv, int32_t end_id, float* loss_row, float* lp_row,
                                    float* dlogits, int32_t R, float gscale, void* stream) {
  if (!logits || !fed || !last || !adv || !dlogits) return TNT_BADARG(0);
  if (V < 1 || ld < V || T < 1 || R < 1 || end_id >= V) return TNT_BADARG(1);
  if ((long)T * R > 0x7fffffffL) return TNT_BADARG(2);
  ScstArgs a{logits, fed, last, adv, loss_row, lp_row, dlogits, ld, V, T, R, end_id, gscale};
  hipStream_t s = tnt_stream(stream);
  const int rows = T * R;
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits) && tnt_aligned16(dlogits);
  tnt_row_ladder(al, V, [&](auto n) {
    hipLaunchKernelGGL((scst_cce_kernel<decltype(n)::value>), dim3(rows), dim3(256), 0, s, a);
  });
  TNT_LAUNCH_CHECK();
  return 0;
}
