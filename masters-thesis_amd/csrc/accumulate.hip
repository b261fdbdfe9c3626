// Gradient accumulation over the flat gradient arena (tnt_grad_accumulate_f32; the definition is in include/tnt_hip.h,
// restated by tests/accum_oracle.py): the sum over the k micro-steps of a window that takes the place of data parallel's
// all-reduce over ranks.  OPEN copies the micro-step's gradient into the accumulator, ADD adds it, CLOSE adds the
// accumulator into the gradient arena, where the update launches behind it find the window's sum.  The Embedding's
// IndexedSlices squared norm (one float) travels the same way, and OPEN / ADD advance the dropout stream's step counter in
// the place of the update's tick that a non-updating micro-step does not run.
//
// Plain float32 adds, acc + grad in that order, one thread per address: no atomic and no cross-thread reduction, so the
// result equals numpy float32 doing the same adds and a replay is bit-reproducible.  The guard word is read by every
// thread; with it set the launch reads, writes and advances nothing.
//
// The stream is average.hip's: one float4 per lane and round, AC_U rounds of both operands in flight, a capped grid with a
// grid stride, the n % 4 tail in workgroup 0.  8 bytes per element in OPEN, 12 in ADD and CLOSE.
//   acc   is touched by nothing else in the step: non-temporal loads and stores under the TNT_STREAM_NT policy, so that
//         an arena-sized buffer does not push the weights and activations of the next forward out of the Infinity Cache.
//   grad  plain loads and stores in every phase.  In CLOSE the norm launch reads the sums straight afterwards and the
//         update launches once more, so they should stay in the L2s / the Infinity Cache.  In OPEN / ADD nothing reads
//         grad again before the next backward overwrites it, which argued for non-temporal loads; measured
//         (profiles/grad_accum_grad_policy_ab.txt), the micro-step takes the same time either way (the arms differ by
//         less than two runs of one arm do), and the launch alone, repeated over the same buffers, is 7 to 12 % slower
//         non-temporal over config 2's arena and 20 to 65 % over config 3's.  Plain is the simpler kernel, so plain.
// No LDS, no scratch (profiles/grad_accum_resource_usage.txt).
#include "tnt_common.h"

namespace {

constexpr int AC_THREADS = 256;
constexpr int AC_U = 4;                        // rounds of 16-byte loads in flight per lane
constexpr int AC_CHUNK = AC_THREADS * AC_U;    // float4s per workgroup and trip
constexpr int AC_MAX_GRID = 2048;              // 8 workgroups per CU; the rest of the range is grid-strided

enum { AC_OPEN = 0, AC_ADD = 1, AC_CLOSE = 2 };

struct AccScalars {
  float* sq_acc; float* sq_slot; uint32_t* drop_step; const uint32_t* guard;
};

__device__ __forceinline__ float4 ac_add4(const float4& a, const float4& g) {
  return make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
}

template <int PHASE, bool NT>
__global__ __launch_bounds__(AC_THREADS) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ grad,
                                                                     int64_t n, AccScalars s) {
  if (s.guard && s.guard[0] != 0u) return;                 // the micro-step's forward was invalid: the window stays as it was
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) {                       // the scalars: one thread
    if (s.sq_acc) {
      if (PHASE == AC_OPEN) s.sq_acc[0] = s.sq_slot[0];
      else if (PHASE == AC_ADD) s.sq_acc[0] = s.sq_acc[0] + s.sq_slot[0];
      else s.sq_slot[0] = s.sq_acc[0] + s.sq_slot[0];
    }
    if (PHASE != AC_CLOSE && s.drop_step) s.drop_step[0] += 1u;
  }
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * AC_CHUNK;
  for (int64_t base = (int64_t)blockIdx.x * AC_CHUNK + tid; base < n4; base += stride) {
    float4 a[AC_U], g[AC_U];
#pragma unroll
    for (int u = 0; u < AC_U; ++u) {
      const int64_t i = base + u * AC_THREADS;
      if (i < n4) {
        g[u] = tnt_ld4<false>(grad + 4 * i);
        if (PHASE != AC_OPEN) a[u] = tnt_ld4<NT>(acc + 4 * i);
      }
    }
#pragma unroll
    for (int u = 0; u < AC_U; ++u) {
      const int64_t i = base + u * AC_THREADS;
      if (i < n4) {
        if (PHASE == AC_OPEN) tnt_st4<NT>(acc + 4 * i, g[u]);
        else if (PHASE == AC_ADD) tnt_st4<NT>(acc + 4 * i, ac_add4(a[u], g[u]));
        else tnt_st4<false>(grad + 4 * i, ac_add4(a[u], g[u]));
      }
    }
  }
  const int64_t i = 4 * n4 + tid;                          // the n % 4 tail: workgroup 0, one element per thread
  if (blockIdx.x == 0 && i < n) {
    if (PHASE == AC_OPEN) acc[i] = grad[i];
    else if (PHASE == AC_ADD) acc[i] = acc[i] + grad[i];
    else grad[i] = acc[i] + grad[i];
  }
}

int ac_grid(int64_t n) {
  const int64_t chunks = ((n >> 2) + AC_CHUNK - 1) / AC_CHUNK;
  return (int)(chunks < 1 ? 1 : (chunks > AC_MAX_GRID ? AC_MAX_GRID : chunks));
}

template <int PHASE>
void ac_launch(float* acc, float* grad, int64_t n, const AccScalars& s, hipStream_t stream) {
  if (tnt_stream_policy_nt())
    hipLaunchKernelGGL((grad_accumulate_kernel<PHASE, true>), dim3(ac_grid(n)), dim3(AC_THREADS), 0, stream, acc, grad, n, s);
  else
    hipLaunchKernelGGL((grad_accumulate_kernel<PHASE, false>), dim3(ac_grid(n)), dim3(AC_THREADS), 0, stream, acc, grad, n, s);
}

}  // namespace

extern "C" int32_t tnt_grad_accumulate_f32(float* acc, float* grad, int64_t n, int32_t phase, float* sq_acc, float* sq_slot,
                                           uint32_t* drop_step, const uint32_t* guard, void* stream) {
  if (int32_t rc = tnt_check_stream_pair(acc, grad, n)) return rc;
  if (phase < AC_OPEN || phase > AC_CLOSE) return TNT_BADARG(5);
  if ((sq_acc == nullptr) != (sq_slot == nullptr)) return TNT_BADARG(6);
  if (sq_acc != nullptr && sq_acc == sq_slot) return TNT_BADARG(7);
  // an empty arena still does the scalar work; with neither there is nothing to launch
  if (n == 0 && sq_acc == nullptr && (drop_step == nullptr || phase == AC_CLOSE)) return 0;
  const AccScalars s{sq_acc, sq_slot, drop_step, guard};
  if (phase == AC_OPEN) ac_launch<AC_OPEN>(acc, grad, n, s, tnt_stream(stream));
  else if (phase == AC_ADD) ac_launch<AC_ADD>(acc, grad, n, s, tnt_stream(stream));
  else ac_launch<AC_CLOSE>(acc, grad, n, s, tnt_stream(stream));
  TNT_LAUNCH_CHECK();
  return 0;
}
