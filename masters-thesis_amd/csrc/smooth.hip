// Label-smoothed softmax + CategoricalCrossentropy(from_logits=False, label_smoothing=eps) in one launch
// (tnt_softmax_cce_smooth_f32; definition in include/tnt_hip.h, restated by tests/smooth_oracle.py).
//
// Same structure as softmax_cce_reg_kernel / softmax_cce_kernel (seqops.hip): one 256-thread workgroup per row, max and
// first-maximum index, exp-sum, one write.  What smoothing adds: the smoothed target ys_v = (1 - eps) [v == y] + eps / V
// is nonzero in every class, so keras's element-wise clip(p, 1e-7, 1 - 1e-7) acts per class, not per row.  With
// m_v = [1e-7 <= p_v <= 1 - 1e-7]:
//   loss      = -((1 - eps) L_y + (eps / V) sum_v L_v),   L_v = log clip(p_v) = m_v ? (x_v - max) - log Z : log(bound)
//   dlogits_v = gscale (c p_v - m_v ys_v),                c = sum_v m_v ys_v = (1 - eps) m_y + (eps / V) n_u
// so there is no per-element logf: after Z the row needs one more block reduction of two values, n_u = #{v : m_v} and
// S = sum_{m_v} (x_v - max).  A class can only sit above the upper bound if it is the row maximum with Z < 1 + 1.2e-7,
// i.e. p = 1 / Z and every other class is far below 1/2: n_hi = [1 / Z > 1 - 1e-7], n_lo = V - n_u - n_hi.
// The register kernel keeps x - max and exp(x - max) of the row in VGPRs (2 x 4 NV4 values per thread), so the row is
// read once and written once; the generic kernel re-reads it (from the L2) for each of its four passes.
// Pad columns [V, ld): as in seqops.hip (masked to -inf as they are read; written as zero inside the register window,
// neither read nor written otherwise).
#include "tnt_rowhead.h"

namespace {

constexpr float SM_LO = 1e-7f;
constexpr float SM_HI = 1.f - 1e-7f;

struct SmoothRow {
  float c;      // sum_v m_v ys_v
  float ysy;    // m_y ys_y: what the target's own class subtracts (0 if its clip is active or there is no such class)
  float py;
};

// the row's scalars from its reductions, and its loss / correct outputs by thread 0.  y outside [0, V): the one-hot
// matches no class (ys_v = eps / V everywhere).
__device__ __forceinline__ SmoothRow smooth_row_tail(int row, int V, int y, bool has_y, float xy, float m, float Z, float invZ,
                                                     int n_u, float S, int am, float eps, bool has_target, float* loss_row,
                                                     float* correct_row) {
  const float eV = eps / (float)V;
  const float dy = xy - m;
  const float py = has_y ? expf(dy) * invZ : 0.f;
  const bool my = has_y && py >= SM_LO && py <= SM_HI;
  SmoothRow r;
  r.py = py;
  r.c = (my ? 1.f - eps : 0.f) + eV * (float)n_u;
  r.ysy = my ? (1.f - eps) + eV : 0.f;
  if (threadIdx.x == 0 && has_target) {
    if (loss_row) {
      const float logZ = logf(Z);
      const float log_lo = logf(SM_LO), log_hi = logf(SM_HI);
      const int n_hi = (invZ > SM_HI) ? 1 : 0;
      const int n_lo = V - n_u - n_hi;
      const float sumL = (S - (float)n_u * logZ) + ((float)n_lo * log_lo + (float)n_hi * log_hi);
      const float Ly = !has_y ? 0.f : (my ? dy - logZ : (py < SM_LO ? log_lo : log_hi));
      loss_row[row] = -((1.f - eps) * Ly + eV * sumL);
    }
    if (correct_row) correct_row[row] = (am == y) ? 1.f : 0.f;
  }
  return r;
}

__device__ __forceinline__ float smooth_grad(float p, float c, float eV, float gs) {
  const bool mv = p >= SM_LO && p <= SM_HI;
  return (c * p - (mv ? eV : 0.f)) * gs;
}

// register-resident: V <= 1024 * NV4, ld % 4 == 0, 16-byte aligned rows
template <int NV4>
__global__ __launch_bounds__(256) void softmax_cce_smooth_reg_kernel(const float* logits, const int* target, float* probs,
                                                                     float* loss_row, float* correct_row, float* dlogits,
                                                                     int rows, int V, int ld, float gscale, float eps) {
  __shared__ float shm[4], shz[4], shs[4];
  __shared__ int shi[4], shc[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  float4 d[NV4], e[NV4];
  float m = tnt_row_load_max<NV4>(x, tid, V, ld, d);
  m = tnt_wave_max(m);
  if ((tid & 63) == 0) shm[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
  int am = tnt_row_first_max<NV4>(d, m, tid);      // first index holding the maximum (np.argmax / tf.argmax rule)
  if ((tid & 63) == 0) shi[tid >> 6] = am;
  const int y = target ? target[row] : -1;
  const bool has_y = y >= 0 && y < V;
  const float xy = has_y ? x[y] : -INFINITY;                 // before any thread overwrites the row (aliasing)
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    d[i].x -= m; d[i].y -= m; d[i].z -= m; d[i].w -= m;
    e[i] = make_float4(expf(d[i].x), expf(d[i].y), expf(d[i].z), expf(d[i].w));
    s += (e[i].x + e[i].y) + (e[i].z + e[i].w);
  }
  s = tnt_wave_sum(s);
  if ((tid & 63) == 0) shz[tid >> 6] = s;
  __syncthreads();
  const float Z = (shz[0] + shz[1]) + (shz[2] + shz[3]);
  am = min(min(shi[0], shi[1]), min(shi[2], shi[3]));
  const float invZ = 1.f / Z;
  // p_v, and the two reductions over the classes whose clip is inactive
  int n_u = 0;
  float S = 0.f;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    e[i].x *= invZ; e[i].y *= invZ; e[i].z *= invZ; e[i].w *= invZ;
    const bool mx = e[i].x >= SM_LO && e[i].x <= SM_HI, my = e[i].y >= SM_LO && e[i].y <= SM_HI;
    const bool mz = e[i].z >= SM_LO && e[i].z <= SM_HI, mw = e[i].w >= SM_LO && e[i].w <= SM_HI;
    n_u += (int)mx + (int)my + (int)mz + (int)mw;
    S += ((mx ? d[i].x : 0.f) + (my ? d[i].y : 0.f)) + ((mz ? d[i].z : 0.f) + (mw ? d[i].w : 0.f));
  }
  S = tnt_wave_sum(S);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_u += __shfl_xor(n_u, o, 64);
  if ((tid & 63) == 0) { shs[tid >> 6] = S; shc[tid >> 6] = n_u; }
  __syncthreads();
  S = (shs[0] + shs[1]) + (shs[2] + shs[3]);
  n_u = (shc[0] + shc[1]) + (shc[2] + shc[3]);
  const SmoothRow r = smooth_row_tail(row, V, y, has_y, xy, m, Z, invZ, n_u, S, am, eps, target != nullptr, loss_row,
                                      correct_row);
  const float gs = target ? gscale : 0.f;                    // no target: no loss to differentiate, zero rows
  const float eV = eps / (float)V;
  float* drow = dlogits ? dlogits + (long)row * ld : nullptr;
  float* prow = (probs && probs != dlogits) ? probs + (long)row * ld : nullptr;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int j = 4 * (tid + 256 * i);
    if (j >= ld) continue;
    if (drow)
      *reinterpret_cast<float4*>(drow + j) = make_float4(smooth_grad(e[i].x, r.c, eV, gs), smooth_grad(e[i].y, r.c, eV, gs),
                                                         smooth_grad(e[i].z, r.c, eV, gs), smooth_grad(e[i].w, r.c, eV, gs));
    if (prow) *reinterpret_cast<float4*>(prow + j) = e[i];
  }
  // the thread that owns column y patches it after its own vector store (same thread, same address: program order)
  if (drow && has_y && ((y >> 2) & 255) == tid) drow[y] = (r.c * r.py - r.ysy) * gs;
}

// generic: any V, ld, alignment.  Neither reads nor writes a pad column.
__global__ __launch_bounds__(256) void softmax_cce_smooth_kernel(const float* logits, const int* target, float* probs,
                                                                 float* loss_row, float* correct_row, float* dlogits,
                                                                 int rows, int V, int ld, float gscale, float eps) {
  __shared__ float shm[4], shz[4], shs[4];
  __shared__ int shi[4], shc[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  float m;
  int am;
  tnt_row_scan_argmax(x, V, tid, m, am);
  if ((tid & 63) == 0) { shm[tid >> 6] = m; shi[tid >> 6] = am; }
  __syncthreads();
  tnt_row_combine_argmax(shm, shi, m, am);
  const int y = target ? target[row] : -1;
  const bool has_y = y >= 0 && y < V;
  const float xy = has_y ? x[y] : -INFINITY;                 // before any thread overwrites the row (aliasing)
  float s = 0.f;
  for (int j = tid; j < V; j += 256) s += expf(x[j] - m);
  s = tnt_wave_sum(s);
  if ((tid & 63) == 0) shz[tid >> 6] = s;
  __syncthreads();
  const float Z = (shz[0] + shz[1]) + (shz[2] + shz[3]);
  const float invZ = 1.f / Z;
  int n_u = 0;
  float S = 0.f;
  for (int j = tid; j < V; j += 256) {
    const float dj = x[j] - m;
    const float p = expf(dj) * invZ;
    const bool mv = p >= SM_LO && p <= SM_HI;
    n_u += (int)mv;
    S += mv ? dj : 0.f;
  }
  S = tnt_wave_sum(S);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_u += __shfl_xor(n_u, o, 64);
  if ((tid & 63) == 0) { shs[tid >> 6] = S; shc[tid >> 6] = n_u; }
  __syncthreads();                                           // also: every read of the row above precedes every write below
  S = (shs[0] + shs[1]) + (shs[2] + shs[3]);
  n_u = (shc[0] + shc[1]) + (shc[2] + shc[3]);
  const SmoothRow r = smooth_row_tail(row, V, y, has_y, xy, m, Z, invZ, n_u, S, am, eps, target != nullptr, loss_row,
                                      correct_row);
  const float gs = target ? gscale : 0.f;
  const float eV = eps / (float)V;
  if (!dlogits && !probs) return;
  // logits may alias probs/dlogits: every thread reads its own elements before overwriting them
  for (int j = tid; j < V; j += 256) {
    const float p = expf(x[j] - m) * invZ;
    if (dlogits) dlogits[(long)row * ld + j] = (j == y) ? (r.c * r.py - r.ysy) * gs : smooth_grad(p, r.c, eV, gs);
    if (probs && probs != dlogits) probs[(long)row * ld + j] = p;
  }
}

}  // namespace

extern "C" int32_t tnt_softmax_cce_smooth_f32(const float* logits, const int32_t* target, float* probs, float* loss_row,
                                              float* correct_row, float* dlogits, int32_t rows, int32_t V, int32_t ld,
                                              float gscale, float label_smoothing, void* stream) {
  if (rows == 0) return 0;
  if (rows < 0) return TNT_BADARG(6);
  if (V <= 0) return TNT_BADARG(7);
  if (ld < V) return TNT_BADARG(8);
  if (!logits) return TNT_BADARG(0);
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return TNT_BADARG(10);      // NaN fails both compares
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && tnt_aligned16(logits) && (!probs || tnt_aligned16(probs)) &&
                  (!dlogits || tnt_aligned16(dlogits));
  const int nv4 = (V + 1023) / 1024;
#define TNT_SMOOTH(N)                                                                                                  \
  hipLaunchKernelGGL((softmax_cce_smooth_reg_kernel<N>), dim3(rows), dim3(256), 0, s, logits, target, probs, loss_row, \
                     correct_row, dlogits, rows, V, ld, gscale, label_smoothing)
  if (al && nv4 == 1) TNT_SMOOTH(1);
  else if (al && nv4 == 2) TNT_SMOOTH(2);
  else if (al && nv4 <= 4) TNT_SMOOTH(4);
  else if (al && nv4 <= 5) TNT_SMOOTH(5);
  else if (al && nv4 <= 8) TNT_SMOOTH(8);
  else
    hipLaunchKernelGGL(softmax_cce_smooth_kernel, dim3(rows), dim3(256), 0, s, logits, target, probs, loss_row,
                       correct_row, dlogits, rows, V, ld, gscale, label_smoothing);
#undef TNT_SMOOTH
  TNT_LAUNCH_CHECK();
  return 0;
}
