// Constrained caption decoding (tnt_decode_constrain_f32; the definition is in include/tnt_hip.h): the repetition penalty
// and the bans (bad ids, minimum length, no-repeat n-gram) of one decode step, applied to the step's logits in place from
// a token history that lives on the device, in front of the softmax launch.
//
// One wave per row, lane j holds h_j (i <= 64 history tokens):
//   1. history: lane j < i-1 loads hist_in[parent[r]][j], lane i-1 loads last_token[r]; every lane j < i stores its token
//      to hist_out[r][j].  Two dependent loads per row; the beam reorder of the history is this gather.
//   2. n-gram: lane j decides whether the n-gram that ENDS at position j starts with the last n-1 tokens (n-1 pairs of wave
//      shuffles); if so its own token h_j is banned.
//   3. one pass of i shuffles gives every lane (a) whether an earlier lane holds the same token (then it is not the first
//      occurrence and stores nothing) and (b) whether ANY lane holding the same token is banned by 2.
//   4. the first occurrence of an in-range token v decides v's final value -- -inf when banned by 2, by the bad-id list or
//      by the minimum length, else the logit penalised once -- and stores it.  Lane l < n_bad stores -inf at bad_ids[l], lane
//      0 stores -inf at end_id while i < m.  Every store to one address carries the same value (a banned history token is
//      -inf from whichever lane writes it), so no order between lanes matters; no atomics, no LDS, no scratch memory.
#include "tnt_common.h"

namespace {

constexpr int DC_WAVES = 4;       // rows per workgroup

__global__ __launch_bounds__(DC_WAVES * 64) void decode_constrain_kernel(
    float* __restrict__ logits, int ld, int V, int rows, int i, const int* __restrict__ hist_in,
    int* __restrict__ hist_out, int ldh, const int* __restrict__ last_token, const int* __restrict__ parent,
    const int* __restrict__ fin, float theta, int n, int m, int end_id, const int* __restrict__ bad_ids, int n_bad) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * DC_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;                               // whole waves leave: the shuffles below see full waves

  // ---- 1. the row's history
  int h = -1;
  if (lane < i - 1) {
    int p = parent ? parent[r] : r;
    if (p < 0 || p >= rows) p = r;                     // device data: never read outside the buffer
    h = hist_in[(long)p * ldh + lane];
  } else if (lane == i - 1) {
    h = last_token[r];
  }
  if (lane < i) hist_out[(long)r * ldh + lane] = h;
  if (fin && fin[r] != 0) return;                      // wave-uniform

  // ---- 2. does the n-gram ending at this lane's position repeat the current context?
  bool hit = false;
  if (n >= 1 && i >= n) {
    hit = lane >= n - 1 && lane < i;
    for (int t = 0; t < n - 1; ++t) {                  // h_{lane-n+1+t} against h_{i-n+1+t}
      const int a = __shfl(h, (lane - n + 1 + t) & 63, 64);
      const int b = __shfl(h, i - n + 1 + t, 64);
      hit = hit && a == b;
    }
  }

  // ---- 3. first occurrence, and the ban of the token over all of its occurrences
  bool dup = false, banned = false;
  for (int s = 0; s < i; ++s) {
    const int hs = __shfl(h, s, 64);
    const int bs = __shfl((int)hit, s, 64);
    if (hs == h) {
      dup = dup || s < lane;
      banned = banned || bs != 0;
    }
  }
  const int bad = lane < n_bad ? bad_ids[lane] : -1;
  for (int s = 0; s < n_bad; ++s) {
    const int b = __shfl(bad, s, 64);                  // every lane takes part in every shuffle: no short circuit around it
    banned = banned || b == h;
  }
  const bool end_ban = i < m && end_id >= 0 && end_id < V;
  banned = banned || (end_ban && h == end_id);

  // ---- 4. the stores
  float* x = logits + (long)r * ld;
  if (lane < i && !dup && h >= 0 && h < V) {
    if (banned) {
      x[h] = -INFINITY;
    } else if (theta != 1.f) {
      const float v = x[h];
      x[h] = v > 0.f ? v / theta : v * theta;
    }
  }
  if (bad >= 0 && bad < V) x[bad] = -INFINITY;
  if (lane == 0 && end_ban) x[end_id] = -INFINITY;
}

}  // namespace

extern "C" int32_t tnt_decode_constrain_f32(float* logits, int32_t ld, int32_t V, int32_t rows, int32_t i,
                                            const int32_t* hist_in, int32_t* hist_out, int32_t ldh,
                                            const int32_t* last_token, const int32_t* parent, const int32_t* fin,
                                            float theta, int32_t n, int32_t m, int32_t end_id, const int32_t* bad_ids,
                                            int32_t n_bad, void* stream) {
  if (!logits) return TNT_BADARG(0);
  if (V <= 0) return TNT_BADARG(2);
  if (ld < V) return TNT_BADARG(1);
  if (rows <= 0) return TNT_BADARG(3);
  if (i < 0 || i > 64) return TNT_BADARG(4);
  if (i > 0 && !hist_in) return TNT_BADARG(5);
  if (!hist_out) return TNT_BADARG(6);
  if (ldh < (i > 1 ? i : 1)) return TNT_BADARG(7);
  if (hist_in) {                                       // the [rows][ldh] extents must not overlap (equal pointers included)
    const uintptr_t a = (uintptr_t)hist_in, b = (uintptr_t)hist_out, bytes = (uintptr_t)rows * (uintptr_t)ldh * sizeof(int32_t);
    if (a < b + bytes && b < a + bytes) return TNT_BADARG(6);
  }
  if (i > 0 && !last_token) return TNT_BADARG(8);
  if (!(theta >= 1.f) || theta > 3.402823466e38f) return TNT_BADARG(11);
  if (n < 0) return TNT_BADARG(12);
  if (m < 0) return TNT_BADARG(13);
  if (m > 0 && end_id < 0) return TNT_BADARG(14);
  if (n_bad < 0 || n_bad > 64) return TNT_BADARG(16);
  if (n_bad > 0 && !bad_ids) return TNT_BADARG(15);
  hipLaunchKernelGGL(decode_constrain_kernel, dim3((rows + DC_WAVES - 1) / DC_WAVES), dim3(DC_WAVES * 64), 0,
                     tnt_stream(stream), logits, ld, V, rows, i, hist_in, hist_out, ldh, last_token, parent, fin, theta, n,
                     m, end_id, bad_ids, n_bad);
  TNT_LAUNCH_CHECK();
  return 0;
}
