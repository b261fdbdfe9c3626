// Softmax + CategoricalCrossentropy(from_logits=False) mixed with knowledge distillation (Hinton et al. 2015, "Distilling
// the Knowledge in a Neural Network") in one launch (tnt_softmax_cce_distill_f32; definition in include/tnt_hip.h, restated
// by tests/distill_oracle.py): beside the ground-truth word, every row is pulled towards a frozen teacher's
// temperature-softened next-word distribution.  It reads two logits rows (student x, teacher u) and writes one.
//
// One 256-thread workgroup per row; the row walk of the student (load + max, first-maximum index), the block reductions
// and the kernel ladder come from tnt_rowhead.h, and the one kernel template below holds what is distillation's own.
//
// The kl term without a per-element logf.  With dx_v = x_v - max x, du_v = u_v - max u, temperature t and
//   Zt = sum_v exp(dx_v / t),  Zu = sum_v exp(du_v / t),  pt_v = exp(dx_v / t) / Zt,  qt_v = exp(du_v / t) / Zu
// the logs come from the logits: log pt_v = dx_v / t - log Zt, log qt_v = du_v / t - log Zu, so
//   kl = sum_v qt_v (log qt_v - log pt_v)
//      = sum_v qt_v ((du_v - dx_v) / t - log Zu + log Zt)
//      = (1 / (t Zu)) sum_v exp(du_v / t) (du_v - dx_v)  -  log Zu + log Zt            (sum_v qt_v = 1)
//      = D / (t Zu) - log Zu + log Zt,        D = sum_v exp(du_v / t) (du_v - dx_v).
// A class whose exp(du_v / t) underflows to 0 adds exactly 0 to D (a select, not a product: du_v - dx_v may be huge, and
// is NaN in a masked pad column).  One pass over the kept differences forms Z1 = sum_v exp(dx_v) (the plain head's Z),
// Zt, Zu and D; they share ONE barrier.  t == 1 (uniform over the grid) takes Zt = Z1 and pt = p without the second expf.
// The write pass recomputes the exponentials from the kept differences:
//   dlogits_v = gscale ((1 - a) m_y (p_v - [v == y]) + a t (pt_v - qt_v)),   p_v = exp(dx_v) / Z1.
// Six exponentials per class (four at t == 1) make the launch instruction-bound with expf (16 instructions each: 22 us
// at 960 x 5001 against 9 us for the plain head), so every one of them is v_exp_f32 of a product, exp(d s) =
// exp2(fl(d c)) with c = fl(s log2 e) formed once per thread: one multiply and one transcendental.  All arguments are
// <= 0.  What that costs in accuracy is a relative |d s| u more per exponential than expf (the rounding of c and of the
// product sit in the exponent); tests/test_gpu_distill.py's error model carries it.
// Barriers: max x (the first-maximum index is posted behind it), max u, and the four sums (the index rides on it); the
// register row issues the teacher's loads in front of the student's walk, so that both rows are in flight together, and
// the re-reading row posts the teacher's maximum on the barrier of the student's.
//
// The register row (NV4 >= 1) keeps dx and du of the row in VGPRs (2 x 4 NV4 values per thread; NV4 = 8 holds 64 and does
// not spill: profiles/distill_resource_usage.txt), so either row is read once and the gradient written once; it needs BOTH
// rows float4-addressable.  The re-reading row (NV4 == 0) reads them (from the L2) in each pass.
// Pad columns [V, ld) of the student: as in seqops.hip (masked to -inf as they are read; written as zero inside the
// register window, neither read nor written otherwise).  Pad columns [V, ld_teacher) of the teacher are never read: the
// quad that straddles V is fetched by scalar loads of its valid columns.
#include "tnt_rowhead.h"

namespace {

constexpr float DS_LO = 1e-7f;
constexpr float DS_HI = 1.f - 1e-7f;

constexpr float DS_LOG2E = 1.44269504088896340736f;

// exp(d s) for d <= 0 with c = fl(s log2 e): one multiply, one v_exp_f32 (-inf gives 0; a result below FLT_MIN may be
// flushed to 0).  Not expf: p_y here agrees with tnt_softmax_cce_f32's up to |d| u relative, not bit for bit, so this must
// not be reused where the decision of ce's clip has to be the plain head's own.
__device__ __forceinline__ float ds_exp(float d, float c) { return __builtin_amdgcn_exp2f(d * c); }

// the teacher row's load on the register row: TntRow<NV4>::max()'s, without ever touching a pad column and without
// waiting for the data
template <int NV4>
__device__ __forceinline__ void distill_teacher_load(TntRow<NV4>& w) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int j = 4 * (tid + 256 * i);
    w.d[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (j + 3 < w.V) {
      w.d[i] = *reinterpret_cast<const float4*>(w.x + j);
    } else if (j < w.V) {
      w.d[i].x = w.x[j];
      if (j + 1 < w.V) w.d[i].y = w.x[j + 1];
      if (j + 2 < w.V) w.d[i].z = w.x[j + 2];
    }
  }
}

template <int NV4>
__device__ __forceinline__ float distill_teacher_max(const TntRow<NV4>& w, float* shm) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV4; ++i) m = fmaxf(m, fmaxf(fmaxf(w.d[i].x, w.d[i].y), fmaxf(w.d[i].z, w.d[i].w)));
  return tnt_block_max4(m, shm);
}

struct DsSums {
  float z1, zt, zu, d;
};

// one class's part of the four sums from its kept differences; T1: t == 1; ct = fl(log2 e / t)
template <bool T1>
__device__ __forceinline__ void distill_acc(float dx, float du, float ct, DsSums& s) {
  const float e1 = ds_exp(dx, DS_LOG2E);
  s.z1 += e1;
  if (!T1) s.zt += ds_exp(dx, ct);
  const float eu = ds_exp(du, ct);
  s.zu += eu;
  s.d += eu > 0.f ? eu * (du - dx) : 0.f;
}

struct DsRow {
  float c1;     // gscale (1 - a) m_y / Z1: what multiplies exp(dx_v)
  float ct;     // gscale a t / Zt
  float cu;     // gscale a t / Zu
  float gy;     // gscale (1 - a) m_y: what the target's own class subtracts
};

template <bool T1>
__device__ __forceinline__ float distill_grad(float dx, float du, float ct, const DsRow& r) {
  const float e1 = ds_exp(dx, DS_LOG2E);
  const float et = T1 ? e1 : ds_exp(dx, ct);
  return (r.c1 * e1 + r.ct * et) - r.cu * ds_exp(du, ct);
}

// NV4 >= 1: register-resident rows (V <= 1024 * NV4, both lds % 4 == 0, 16-byte aligned rows), which also zeroes the
// student-side pad columns of dlogits inside its window; NV4 == 0: re-reading rows (any V, lds, alignment), which neither
// reads nor writes a pad column.  Column c belongs to the thread that stores it: (c >> 2) & 255 resp. c & 255.
template <int NV4>
__global__ __launch_bounds__(256) void softmax_cce_distill_kernel(const float* logits, const float* teacher,
                                                                  const int* target, float* loss_row, float* kl_row,
                                                                  float* correct_row, float* dlogits, int V, int ld,
                                                                  int ldt, float gscale, float alpha, float temp) {
  __shared__ float shm[4], shu[4], sh1[4], sht[4], shz[4], shd[4];
  __shared__ int shi[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  const float* u = teacher + (long)row * ldt;
  TntRow<NV4> wx{x, V}, wu{u, V};
  int am;
  float m, mu;
  if constexpr (NV4 > 0) {
    distill_teacher_load(wu);                                 // in flight while the student's row is walked
    m = wx.max_first(shm, shi, am);                           // the first barrier
    mu = distill_teacher_max(wu, shu);                        // the second barrier
  } else {
    float v = -INFINITY;
    for (int j = tid; j < V; j += 256) v = fmaxf(v, u[j]);
    tnt_wave_post(tnt_wave_max(v), shu);                      // rides on the barrier of the student's maximum
    m = wx.max_first(shm, shi, am);
    mu = fmaxf(fmaxf(shu[0], shu[1]), fmaxf(shu[2], shu[3]));
  }
  const int y = target[row];
  const bool has_y = y >= 0 && y < V;
  const float xy = has_y ? x[y] : -INFINITY;                  // before any thread overwrites the row (aliasing)
  const float it = 1.f / temp;
  const bool t1 = temp == 1.f;                                // uniform over the grid
  const float ct = t1 ? DS_LOG2E : it * DS_LOG2E;
  DsSums s{0.f, 0.f, 0.f, 0.f};
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      float4& a = wx.d[i];
      float4& b = wu.d[i];
      a.x -= m; a.y -= m; a.z -= m; a.w -= m;
      b.x -= mu; b.y -= mu; b.z -= mu; b.w -= mu;
    }
    if (t1) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        distill_acc<true>(wx.d[i].x, wu.d[i].x, ct, s); distill_acc<true>(wx.d[i].y, wu.d[i].y, ct, s);
        distill_acc<true>(wx.d[i].z, wu.d[i].z, ct, s); distill_acc<true>(wx.d[i].w, wu.d[i].w, ct, s);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        distill_acc<false>(wx.d[i].x, wu.d[i].x, ct, s); distill_acc<false>(wx.d[i].y, wu.d[i].y, ct, s);
        distill_acc<false>(wx.d[i].z, wu.d[i].z, ct, s); distill_acc<false>(wx.d[i].w, wu.d[i].w, ct, s);
      }
    }
  } else {
    if (t1) for (int j = tid; j < V; j += 256) distill_acc<true>(x[j] - m, u[j] - mu, ct, s);
    else for (int j = tid; j < V; j += 256) distill_acc<false>(x[j] - m, u[j] - mu, ct, s);
  }
  // the four sums on one barrier; also: every read of the student row above precedes every write below
  tnt_wave_post(tnt_wave_sum(s.z1), sh1);
  if (!t1) tnt_wave_post(tnt_wave_sum(s.zt), sht);
  tnt_wave_post(tnt_wave_sum(s.d), shd);
  const float Zu = tnt_block_sum4(s.zu, shz);
  const float Z1 = (sh1[0] + sh1[1]) + (sh1[2] + sh1[3]);
  const float Zt = t1 ? Z1 : (sht[0] + sht[1]) + (sht[2] + sht[3]);
  const float D = (shd[0] + shd[1]) + (shd[2] + shd[3]);
  am = wx.first(shi, am);
  const float invZ = 1.f / Z1;
  const float py = has_y ? ds_exp(xy - m, DS_LOG2E) * invZ : 0.f;
  const float my = (py >= DS_LO && py <= DS_HI) ? 1.f : 0.f;  // keras: zero gradient where the clip of ce is active
  if (tid == 0) {
    if (loss_row || kl_row) {
      const float kl = (D * it) / Zu - logf(Zu) + logf(Zt);
      if (kl_row) kl_row[row] = kl;
      if (loss_row) {
        const float ce = -logf(fminf(fmaxf(py, DS_LO), DS_HI));
        loss_row[row] = (1.f - alpha) * ce + (alpha * temp * temp) * kl;
      }
    }
    if (correct_row) correct_row[row] = (am == y) ? 1.f : 0.f;
  }
  if (!dlogits) return;
  float* drow = dlogits + (long)row * ld;
  DsRow r;
  r.gy = gscale * ((1.f - alpha) * my);
  r.c1 = r.gy * invZ;
  r.ct = (gscale * (alpha * temp)) / Zt;
  r.cu = (gscale * (alpha * temp)) / Zu;
  if constexpr (NV4 > 0) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      const int j = 4 * (tid + 256 * i);
      if (j >= ld) continue;
      const float4 a = wx.d[i], b = wu.d[i];
      float4 g;
      if (t1) {
        g = make_float4(distill_grad<true>(a.x, b.x, ct, r), distill_grad<true>(a.y, b.y, ct, r),
                        distill_grad<true>(a.z, b.z, ct, r), distill_grad<true>(a.w, b.w, ct, r));
      } else {
        g = make_float4(distill_grad<false>(a.x, b.x, ct, r), distill_grad<false>(a.y, b.y, ct, r),
                        distill_grad<false>(a.z, b.z, ct, r), distill_grad<false>(a.w, b.w, ct, r));
      }
      *reinterpret_cast<float4*>(drow + j) = g;
    }
  } else {
    // logits may alias dlogits: every thread reads its own elements before overwriting them
    if (t1) for (int j = tid; j < V; j += 256) drow[j] = distill_grad<true>(x[j] - m, u[j] - mu, ct, r);
    else for (int j = tid; j < V; j += 256) drow[j] = distill_grad<false>(x[j] - m, u[j] - mu, ct, r);
  }
  // the thread that owns column y patches it after its own store (same thread, same address: program order)
  const auto owner = [](int c) { return NV4 > 0 ? (c >> 2) & 255 : c & 255; };
  if (has_y && owner(y) == tid) drow[y] -= r.gy;
}

}  // namespace

extern "C" int32_t tnt_softmax_cce_distill_f32(const float* logits, const float* teacher, const int32_t* target,
                                               float* loss_row, float* kl_row, float* correct_row, float* dlogits,
                                               int32_t rows, int32_t V, int32_t ld, int32_t ld_teacher, float gscale,
                                               float alpha, float temperature, void* stream) {
  if (rows == 0) return 0;
  if (rows < 0) return TNT_BADARG(7);
  if (V <= 0) return TNT_BADARG(8);
  if (ld < V) return TNT_BADARG(9);
  if (ld_teacher < V) return TNT_BADARG(10);
  if (!logits) return TNT_BADARG(0);
  if (!teacher) return TNT_BADARG(1);
  if (!target) return TNT_BADARG(2);
  if (!(alpha >= 0.f && alpha <= 1.f)) return TNT_BADARG(12);                               // NaN fails both compares
  if (!(temperature > 0.f && temperature <= 3.402823466e38f)) return TNT_BADARG(13);
  const void* t = teacher;
  if (t == loss_row || t == kl_row || t == correct_row || t == dlogits) return TNT_BADARG(1);
  hipStream_t s = tnt_stream(stream);
  const bool al = (ld % 4 == 0) && (ld_teacher % 4 == 0) && tnt_aligned16(logits) && tnt_aligned16(teacher) &&
                  (!dlogits || tnt_aligned16(dlogits));
  tnt_row_ladder(al, V, [&](auto n) {
    hipLaunchKernelGGL((softmax_cce_distill_kernel<decltype(n)::value>), dim3(rows), dim3(256), 0, s, logits, teacher,
                       target, loss_row, kl_row, correct_row, dlogits, V, ld, ld_teacher, gscale, alpha, temperature);
  });
  TNT_LAUNCH_CHECK();
  return 0;
}
