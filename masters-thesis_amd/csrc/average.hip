// Weight averaging over the flat parameter arena (tnt_weight_average_f32, tnt_swap_f32; the definitions are in
// include/tnt_hip.h, restated by tests/average_oracle.py): an exponential moving average (tfa.optimizers.MovingAverage)
// or an equal-weight running mean (tfa.optimizers.SWA) of the parameters, one launch behind the optimizer update.
//
// Every decision is taken on the device from the live step counter (the model's adam_t) and the guard word, so a recorded
// launch plan or a hipGraph replays the launch unchanged: whether to seed (copy), to skip this step, or to blend, and the
// blend's decay.  The scalars are uniform over the launch: every thread derives them from the same two words.
//
// A pure stream, 12 bytes per parameter (theta read, avg read + written).  As adam_fin_kernel (optim.hip) found, such a
// stream is bound by latency x bytes in flight, not by HBM, with one 16-byte load per lane and trip: every lane keeps AV_U
// rounds of float4 loads of both operands in flight.  avg is touched by nothing else in the step: it moves with
// non-temporal loads and stores (tnt_stream_policy_nt) so that it does not push theta, which the next forward reads
// again, out of the Infinity Cache; theta is read with plain loads.  No atomics, no LDS, no scratch; every address is
// written by one thread.
#include "tnt_common.h"

namespace {

constexpr int AV_THREADS = 256;
constexpr int AV_U = 4;                        // rounds of 16-byte loads in flight per lane
constexpr int AV_CHUNK = AV_THREADS * AV_U;    // float4s per workgroup and trip
constexpr int AV_MAX_GRID = 2048;              // 8 workgroups per CU; the rest of the range is grid-strided

enum { AV_SKIP = 0, AV_COPY = 1, AV_BLEND = 2 };

struct AvgArgs {
  const int64_t* step; const uint32_t* guard;
  double momentum; int64_t start_step; int32_t kind, dynamic, every;
};

// what this launch does, and the blend's float32 constant c = 1 - decay (decay in float64)
__device__ __forceinline__ int avg_plan(const AvgArgs& a, float& c) {
  c = 0.f;
  if (a.guard && a.guard[0] != 0u) return AV_SKIP;      // the step's forward pass was invalid: nothing is read or written
  const int64_t t = a.step[0];
  const int64_t s = a.start_step > 1 ? a.start_step : 1;
  if (t <= s) return AV_COPY;
  const int64_t r = t - s;
  if (r % a.every != 0) return AV_SKIP;
  const double k = (double)(r / a.every);               // samples behind the seed, >= 1
  double d;
  if (a.kind == 1) d = k / (k + 1.0);
  else { d = a.momentum; if (a.dynamic) d = fmin(d, (1.0 + k) / (10.0 + k)); }
  c = (float)(1.0 - d);
  return AV_BLEND;
}

template <bool NT>
__global__ __launch_bounds__(AV_THREADS) void weight_average_kernel(const float* __restrict__ theta, float* __restrict__ avg,
                                                                    int64_t n, AvgArgs a) {
  float c;
  const int mode = avg_plan(a, c);
  if (mode == AV_SKIP) return;
  const int tid = threadIdx.x;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * AV_CHUNK;
  for (int64_t base = (int64_t)blockIdx.x * AV_CHUNK + tid; base < n4; base += stride) {
    float4 w[AV_U], e[AV_U];
#pragma unroll
    for (int u = 0; u < AV_U; ++u) {
      const int64_t i = base + u * AV_THREADS;
      if (i < n4) {
        w[u] = *reinterpret_cast<const float4*>(theta + 4 * i);
        if (mode == AV_BLEND) e[u] = tnt_ld4<NT>(avg + 4 * i);
      }
    }
#pragma unroll
    for (int u = 0; u < AV_U; ++u) {
      const int64_t i = base + u * AV_THREADS;
      if (i < n4) {
        if (mode == AV_BLEND) {
          e[u].x = fmaf(c, w[u].x - e[u].x, e[u].x);
          e[u].y = fmaf(c, w[u].y - e[u].y, e[u].y);
          e[u].z = fmaf(c, w[u].z - e[u].z, e[u].z);
          e[u].w = fmaf(c, w[u].w - e[u].w, e[u].w);
          tnt_st4<NT>(avg + 4 * i, e[u]);
        } else {
          tnt_st4<NT>(avg + 4 * i, w[u]);
        }
      }
    }
  }
  const int64_t i = 4 * n4 + tid;                          // the n % 4 tail: workgroup 0, one element per thread
  if (blockIdx.x == 0 && i < n) {
    const float w = theta[i];
    avg[i] = mode == AV_BLEND ? fmaf(c, w - avg[i], avg[i]) : w;
  }
}

__global__ __launch_bounds__(AV_THREADS) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  const int tid = threadIdx.x;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * AV_CHUNK;
  for (int64_t base = (int64_t)blockIdx.x * AV_CHUNK + tid; base < n4; base += stride) {
    if (base + (AV_U - 1) * AV_THREADS < n4) {             // a whole trip: AV_U rounds of both operands in flight
      static_assert(AV_U == 4, "the trip below is written out for four rounds");
      float* const a0 = a + 4 * base; float* const b0 = b + 4 * base;
      constexpr int R = 4 * AV_THREADS;                    // floats between two rounds
      const float4 x0 = *reinterpret_cast<const float4*>(a0), x1 = *reinterpret_cast<const float4*>(a0 + R);
      const float4 x2 = *reinterpret_cast<const float4*>(a0 + 2 * R), x3 = *reinterpret_cast<const float4*>(a0 + 3 * R);
      const float4 y0 = *reinterpret_cast<const float4*>(b0), y1 = *reinterpret_cast<const float4*>(b0 + R);
      const float4 y2 = *reinterpret_cast<const float4*>(b0 + 2 * R), y3 = *reinterpret_cast<const float4*>(b0 + 3 * R);
      *reinterpret_cast<float4*>(a0) = y0; *reinterpret_cast<float4*>(a0 + R) = y1;
      *reinterpret_cast<float4*>(a0 + 2 * R) = y2; *reinterpret_cast<float4*>(a0 + 3 * R) = y3;
      *reinterpret_cast<float4*>(b0) = x0; *reinterpret_cast<float4*>(b0 + R) = x1;
      *reinterpret_cast<float4*>(b0 + 2 * R) = x2; *reinterpret_cast<float4*>(b0 + 3 * R) = x3;
    } else {
      for (int64_t i = base; i < n4; i += AV_THREADS) {
        const float4 x = *reinterpret_cast<const float4*>(a + 4 * i);
        const float4 y = *reinterpret_cast<const float4*>(b + 4 * i);
        *reinterpret_cast<float4*>(a + 4 * i) = y;
        *reinterpret_cast<float4*>(b + 4 * i) = x;
      }
    }
  }
  const int64_t i = 4 * n4 + tid;
  if (blockIdx.x == 0 && i < n) {
    const float x = a[i];
    a[i] = b[i];
    b[i] = x;
  }
}

int av_grid(int64_t n) {
  const int64_t chunks = ((n >> 2) + AV_CHUNK - 1) / AV_CHUNK;
  return (int)(chunks < 1 ? 1 : (chunks > AV_MAX_GRID ? AV_MAX_GRID : chunks));
}

}  // namespace

extern "C" int32_t tnt_weight_average_f32(const float* theta, float* avg, int64_t n, const int64_t* step, int32_t kind,
                                          const double* momentum, int32_t dynamic, int64_t start_step, int32_t every,
                                          const uint32_t* guard, void* stream) {
  if (int32_t rc = tnt_check_stream_pair(theta, avg, n)) return rc;
  if (step == nullptr || momentum == nullptr) return TNT_BADARG(5);
  if (kind != 0 && kind != 1) return TNT_BADARG(6);
  const double mom = *momentum;
  if (!(mom >= 0.0 && mom < 1.0)) return TNT_BADARG(7);          // NaN included
  if (start_step < 0) return TNT_BADARG(8);
  if (every < 1) return TNT_BADARG(9);
  if (n == 0) return 0;
  const AvgArgs a{step, guard, mom, start_step, kind, dynamic != 0, every};
  if (tnt_stream_policy_nt())
    hipLaunchKernelGGL(weight_average_kernel<true>, dim3(av_grid(n)), dim3(AV_THREADS), 0, tnt_stream(stream), theta, avg, n, a);
  else
    hipLaunchKernelGGL(weight_average_kernel<false>, dim3(av_grid(n)), dim3(AV_THREADS), 0, tnt_stream(stream), theta, avg, n, a);
  TNT_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t tnt_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (int32_t rc = tnt_check_stream_pair(a, b, n)) return rc;
  if (n == 0) return 0;
  hipLaunchKernelGGL(swap_kernel, dim3(av_grid(n)), dim3(AV_THREADS), 0, tnt_stream(stream), a, b, n);
  TNT_LAUNCH_CHECK();
  return 0;
}
