// Learning-rate schedules evaluated on the device (tnt_lr_schedule_f32; the definition and the parameter layout are in
// include/tnt_hip.h, restated by tests/lr_schedule_oracle.py): lr = schedule(*step), the Keras rule with step = the
// model's adam_t, the updates applied so far.
//
// One thread.  The step counter and the 16 float64 parameters are read when the launch runs, so a recorded launch plan
// or a hipGraph replays it with the live counter: the launch sits in front of the first launch of the training step
// that reads lr (ModelBase._lr_schedule_launch).  Everything is float64 and the result is rounded once to float32.
//
// The float64 expressions are written out operation by operation and must stay that way on the device: contraction is
// off for the whole file, so 1 + rate * p is a product and a sum (two roundings, as the host oracle computes it) and
// not one fma.  The kinds that use only + - * / and comparisons then give the oracle's bits; pow and cos are the
// device library's, a few float64 ulps from the host's.
#include "tnt_common.h"

#pragma clang fp contract(off)

namespace {

enum { LS_CONSTANT = 0, LS_EXPONENTIAL = 1, LS_INVERSE_TIME = 2, LS_COSINE = 3, LS_COSINE_RESTARTS = 4, LS_POLYNOMIAL = 5,
       LS_PIECEWISE = 6, LS_PIECEWISE_WARM = 7 };

constexpr int LS_RESTART_TRIPS = 4096;      // bound of the restart loop: the descriptor admits t_mul = 1 or >= 1.05 (< 900 trips)
constexpr double LS_PI = 3.14159265358979323846;

__device__ __forceinline__ double ls_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// values[i] of the first i with s <= bounds[i], else values[nb]; unused bounds hold +inf and unused values the last one
__device__ __forceinline__ double ls_piecewise(const double* bounds, const double* values, int nb, int64_t s) {
  const double sd = (double)s;
  for (int i = 0; i < nb; ++i)
    if (sd <= bounds[i]) return values[i];
  return values[nb];
}

// the schedule of kind k at s >= 0 updates, f = the kind's fields
__device__ double ls_eval(int k, const double* f, int64_t s) {
  switch (k) {
    case LS_CONSTANT:
      return f[0];
    case LS_EXPONENTIAL:
    case LS_INVERSE_TIME: {
      const double lr0 = f[0], rate = f[2];
      const int64_t D = (int64_t)f[1];
      if (D < 1) return ls_nan();
      const double p = f[3] != 0.0 ? (double)(s / D) : (double)s / (double)D;
      return k == LS_EXPONENTIAL ? lr0 * pow(rate, p) : lr0 / (1.0 + rate * p);
    }
    case LS_COSINE: {
      const double lr0 = f[0], alpha = f[2];
      const int64_t D = (int64_t)f[1];
      if (D < 1) return ls_nan();
      const double c = (double)(s < D ? s : D) / (double)D;
      return lr0 * ((1.0 - alpha) * 0.5 * (1.0 + cos(LS_PI * c)) + alpha);
    }
    case LS_COSINE_RESTARTS: {
      const double lr0 = f[0], t_mul = f[2], m_mul = f[3], alpha = f[4];
      const int64_t first = (int64_t)f[1];
      if (first < 1) return ls_nan();
      double P = (double)first, r, m;
      if (t_mul == 1.0) {
        r = (double)(s % first);
        m = pow(m_mul, (double)(s / first));
      } else {
        r = (double)s;
        m = 1.0;
        for (int trip = 0; r >= P; ++trip) {
          if (trip == LS_RESTART_TRIPS) return ls_nan();
          r -= P;
          P *= t_mul;
          m *= m_mul;
        }
      }
      return lr0 * ((1.0 - alpha) * m * 0.5 * (1.0 + cos(LS_PI * r / P)) + alpha);
    }
    case LS_POLYNOMIAL: {
      const double lr0 = f[0], end = f[2], power = f[3];
      int64_t D = (int64_t)f[1];
      if (D < 1) return ls_nan();
      if (f[4] != 0.0) {
        const int64_t mult = s / D + (s % D != 0 ? 1 : 0);      // ceil(s / D) in integers
        D *= mult > 1 ? mult : 1;
      } else if (s > D) {
        s = D;
      }
      const double p = (double)s / (double)D;
      return (lr0 - end) * pow(1.0 - p, power) + end;
    }
    default:
      return ls_nan();
  }
}

__global__ __launch_bounds__(64) void lr_schedule_kernel(const int64_t* __restrict__ step, const double* __restrict__ params,
                                                         float* __restrict__ lr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double* p = params;               // uniform reads of read-only memory: no private copy, no scratch
  int64_t s = step[0];
  if (s < 0) s = 0;
  const double kd = p[0];
  const int k = kd >= 0.0 && kd <= 7.0 && kd == (double)(int)kd ? (int)kd : -1;        // NaN and fractions: unknown
  double out;
  if (k == LS_PIECEWISE) {                   // no warm-up fields: 7 bounds, 8 values
    out = ls_piecewise(p + 1, p + 8, 7, s);
  } else {
    const int64_t w = (int64_t)p[1];
    const double start = p[2];
    const double* f = p + 3;
    if (k < 0 || !(p[1] >= 0.0) || (double)w != p[1]) {
      out = ls_nan();
    } else if (s < w) {                      // the ramp from start to the schedule's first value
      const double a0 = k == LS_PIECEWISE_WARM ? ls_piecewise(f, f + 6, 6, 0) : ls_eval(k, f, 0);
      out = start + (a0 - start) * (double)s / (double)w;
    } else {
      out = k == LS_PIECEWISE_WARM ? ls_piecewise(f, f + 6, 6, s - w) : ls_eval(k, f, s - w);
    }
  }
  lr[0] = (float)out;
}

}  // namespace

extern "C" int32_t tnt_lr_schedule_f32(const int64_t* step, const double* params, float* lr, void* stream) {
  if (step == nullptr) return TNT_BADARG(1);
  if (params == nullptr) return TNT_BADARG(2);
  if (lr == nullptr) return TNT_BADARG(3);
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, tnt_stream(stream), step, params, lr);
  TNT_LAUNCH_CHECK();
  return 0;
}
