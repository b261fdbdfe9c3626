// Self-critical sequence training loss (Rennie et al. 2017) for the dense caption model's SCST step
// (nic.NIC(self_critical=...)): the REINFORCE loss of the sampled captions and its logits gradient, one launch.
// Definition in include/tnt_hip.h (tnt_scst_cce_f32); restated by tests/scst_oracle.py.
//
// One 256-thread workgroup per logits row, the row structure of softmax_cce (seqops.hip): max, exp-sum, write.  In front
// of it, the terminator scan of the row's sampled ids w_1..w_{t-1} (at most T ids, one block-wide OR) decides whether the
// row counts at all; a row past the caption's end (and a row whose advantage is 0 when nobody wants its log-probability)
// never reads its logits and writes a zero gradient row.  The register-resident variant keeps the row in VGPRs between
// the passes (V <= 1024 * NV4, 16-byte aligned rows, ld % 4 == 0); the generic one re-reads it.
#include "tnt_common.h"

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

__device__ __forceinline__ float block_max4(float v, float* sh) {
  v = tnt_wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_sum4(float v, float* sh) {
  v = tnt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
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

template <int NV4>
__global__ __launch_bounds__(256) void scst_cce_reg_kernel(ScstArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const RowHead h = scst_head(a, row);
  if (h.kind != 1) { scst_zero(a, row, true, h.kind == 0 ? 0.f : NAN); return; }
  const float* x = a.logits + (long)row * a.ld;
  const int V = a.V;
  float4 v[NV4];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int j = 4 * (tid + 256 * i);
    v[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (j < V) {
      v[i] = *reinterpret_cast<const float4*>(x + j);          // j < V <= ld, ld % 4 == 0: the quad is inside the row
      if (j + 1 >= V) v[i].y = -INFINITY;
      if (j + 2 >= V) v[i].z = -INFINITY;
      if (j + 3 >= V) v[i].w = -INFINITY;
    }
    m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
  }
  const float xw = x[h.w];                 // before the barrier: the gradient may overwrite the row (dlogits == logits)
  m = block_max4(m, sh);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    v[i].x = expf(v[i].x - m); v[i].y = expf(v[i].y - m); v[i].z = expf(v[i].z - m); v[i].w = expf(v[i].w - m);
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float Z = block_sum4(s, sh);
  const float g = scst_finish(a, row, h, xw, m, Z);
  float* d = a.dlogits + (long)row * a.ld;
  if (g == 0.f) {                          // adv = 0 with lp_row wanted: the log-probability only
    scst_zero_grad(a, row, true);
    return;
  }
  const float gz = g / Z;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int j = 4 * (tid + 256 * i);
    if (j >= V) continue;
    float4 o = make_float4(v[i].x * gz, v[i].y * gz, v[i].z * gz, v[i].w * gz);
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
}

__global__ __launch_bounds__(256) void scst_cce_kernel(ScstArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const RowHead h = scst_head(a, row);
  if (h.kind != 1) { scst_zero(a, row, false, h.kind == 0 ? 0.f : NAN); return; }
  const float* x = a.logits + (long)row * a.ld;
  const int V = a.V;
  float m = -INFINITY;
  for (int j = tid; j < V; j += 256) m = fmaxf(m, x[j]);
  const float xw = x[h.w];
  m = block_max4(m, sh);
  float s = 0.f;
  for (int j = tid; j < V; j += 256) s += expf(x[j] - m);
  const float Z = block_sum4(s, sh);
  const float g = scst_finish(a, row, h, xw, m, Z);
  float* d = a.dlogits + (long)row * a.ld;
  if (g == 0.f) {
    scst_zero_grad(a, row, false);
    return;
  }
  const float gz = g / Z;
  // every thread reads its own elements before overwriting them (dlogits may alias logits)
  for (int j = tid; j < V; j += 256) d[j] = expf(x[j] - m) * gz - (j == h.w ? g : 0.f);
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
  const int nv4 = (V + 1023) / 1024;
#define TNT_SCST(N) hipLaunchKernelGGL((scst_cce_reg_kernel<N>), dim3(rows), dim3(256), 0, s, a)
  if (al && nv4 == 1) TNT_SCST(1);
  else if (al && nv4 == 2) TNT_SCST(2);
  else if (al && nv4 <= 4) TNT_SCST(4);
  else if (al && nv4 <= 5) TNT_SCST(5);
  else if (al && nv4 <= 8) TNT_SCST(8);
  else hipLaunchKernelGGL(scst_cce_kernel, dim3(rows), dim3(256), 0, s, a);
#undef TNT_SCST
  TNT_LAUNCH_CHECK();
  return 0;
}
