// Greedy feedback step of the free-running decoder (lc_NIC.call_naive_attention, lc_NIC.py:175-221): the argmax of
// step i's output row becomes step i+1's token, its Embedding row (through the LSTM layer's per-call input dropout)
// becomes step i+1's text input, and the text half of step i+1's LSTM input projection is formed -- one launch per step,
// no host round trip.
//
// Argmax is taken over the logits, not over the softmax probabilities the reference takes it over (lc_NIC.py:219): the
// two differ only where two distinct logits round to the same float32 probability (the softmax is monotone), in which
// case the reference's tf.argmax picks the lower index of the tied probabilities and this kernel the larger logit.
//
// Workgroup (bx, by): batch rows 16 bx .. 16 bx + 15 (one MFMA row tile) x projection columns 64 by .. 64 by + 63.
//   1. every workgroup takes the argmax of its own 16 rows (the logits are read from L2; B * V * 4 bytes per step),
//      4 rows per wave, float4 loads, 16 of them in flight per lane;
//   2. the 16 gathered Embedding rows, masked, go to LDS (workgroups with by == 0 also store them and the ids);
//   3. each wave forms a 16 x 16 tile of text . Wt on v_mfma_f32_16x16x4_f32 (two accumulators over alternating k steps),
//      the w column streamed through registers 128 rows ahead.
// No workgroup waits for another one.
#include "tnt_common.h"
#include "tnt_rng.h"

namespace {

constexpr int GF_ROWS = 16;          // batch rows per workgroup
constexpr int GF_COLS = 64;          // projection columns per workgroup: 4 waves x 16
constexpr int GF_MAX_E = 1016;       // LDS image 16 x (E + 4) floats <= 64 KiB

struct GfArgs {
  const float* logits; int ld, V;
  const float* table; int E;
  const float* w; int ldw, N;
  int* fed; int T, col;
  float* text; int ldt;
  float* xz; int ldz;
  int B;
  float rate, scale; uint64_t seed; uint32_t site, step; const uint32_t* step_dev;
  int lwidth, lcol0;
  int vec;                           // logits rows 16-byte aligned (ld % 4 == 0, aligned base)
};

// (value, index) ordering of the argmax: larger value first, on equal values the lower index; NaN never wins (every
// comparison with it is false), so a row of NaNs keeps the sentinel index
__device__ __forceinline__ void gf_take(float v, int j, float& best, int& bi) {
  if (v > best || (v == best && j < bi)) { best = v; bi = j; }
}

__global__ __launch_bounds__(256) void greedy_feedback_kernel(GfArgs a) {
  extern __shared__ float4 gf_lds4[];
  float* s_text = reinterpret_cast<float*>(gf_lds4);
  __shared__ int s_id[GF_ROWS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GF_ROWS;
  const int lds = a.E + 4;

  // ---- 1. argmax of rows row0 + 4 wave + q: the wave's 4 rows together, 4 float4 loads per row in flight per lane (16
  // independent loads before the first compare: a loop of one load per iteration waits out an L2 round trip per load)
  {
    float best[4];
    int bi[4];
    const float* x[4];
    bool live[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = row0 + wave * 4 + q;
      live[q] = r < a.B;                                         // wave-uniform
      x[q] = a.logits + (long)(live[q] ? r : 0) * a.ld;
      best[q] = -INFINITY;
      bi[q] = 0x7fffffff;
    }
    int j0 = 0;
    if (a.vec) {
      const int v4 = a.V >> 2;
      const float qnan = __builtin_nanf("");
      for (int k = lane; k < v4; k += 256) {
        float4 v[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int kk = k + 64 * u;
            // (outside the row: NaN, which never wins -- -inf would, with an index past the row, on a row of NaNs)
            v[q][u] = (live[q] && kk < v4) ? reinterpret_cast<const float4*>(x[q])[kk] : make_float4(qnan, qnan, qnan, qnan);
          }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = 4 * (k + 64 * u);
            gf_take(v[q][u].x, j, best[q], bi[q]); gf_take(v[q][u].y, j + 1, best[q], bi[q]);
            gf_take(v[q][u].z, j + 2, best[q], bi[q]); gf_take(v[q][u].w, j + 3, best[q], bi[q]);
          }
      }
      j0 = v4 << 2;
    }
    for (int j = j0 + lane; j < a.V; j += 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (live[q]) gf_take(x[q][j], j, best[q], bi[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(best[q], m);
        const int oi = __shfl_xor(bi[q], m);
        if (ov > best[q] || (ov == best[q] && oi < bi[q])) { best[q] = ov; bi[q] = oi; }
      }
      // always a valid row of the table (a padding row of the tile, or a row without a winner: 0)
      if (lane == 0) s_id[wave * 4 + q] = (live[q] && bi[q] >= 0 && bi[q] < a.V) ? bi[q] : 0;
    }
  }
  __syncthreads();
  const bool lead = blockIdx.y == 0;
  if (lead && threadIdx.x < GF_ROWS && row0 + (int)threadIdx.x < a.B)
    a.fed[(long)(row0 + threadIdx.x) * a.T + a.col] = s_id[threadIdx.x];

  // ---- 2. gather + the LSTM input mask of step col (rows_per_site = B: local row b, element b lwidth + lcol0 + j)
  const uint32_t step = a.step + (a.step_dev ? a.step_dev[0] : 0u);
  const int e4 = a.E >> 2;
  for (int c = threadIdx.x; c < GF_ROWS * e4; c += 256) {
    const int rr = c / e4, j = (c - rr * e4) * 4, r = row0 + rr;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < a.B) {
      v = *reinterpret_cast<const float4*>(a.table + (long)s_id[rr] * a.E + j);
      if (a.rate > 0.f) {
        bool k[4];
        tnt_keep4((uint64_t)r * (uint64_t)a.lwidth + (uint64_t)(a.lcol0 + j), a.rate, a.seed, a.site, step, k);
        v = make_float4(k[0] ? v.x * a.scale : 0.f, k[1] ? v.y * a.scale : 0.f, k[2] ? v.z * a.scale : 0.f,
                        k[3] ? v.w * a.scale : 0.f);
      }
      if (lead) *reinterpret_cast<float4*>(a.text + (long)r * a.ldt + j) = v;
    }
    *reinterpret_cast<float4*>(s_text + rr * lds + j) = v;
  }
  __syncthreads();

  // ---- 3. xz[16 x 16 of this wave] = text . w   (A[l&15][k = l>>4], B[k = l>>4][l&15]; C col = l&15, row = 4(l>>4) + reg)
  const int n = blockIdx.y * GF_COLS + wave * 16 + (lane & 15);
  const bool nok = n < a.N;
  const int kq = lane >> 4;
  const float* arow = s_text + (lane & 15) * lds + kq;
  const float* wcol = a.w + (long)kq * a.ldw + (nok ? n : 0);
  floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  // the w column is streamed 32 k steps (128 rows) at a time, the next block's 32 loads issued before this block's MFMAs
  constexpr int KB = 32;
  const int nblk = a.E / (4 * KB);
  int k0 = 0;
  if (nblk > 0) {
    float bc[KB], bn[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) bc[s] = nok ? wcol[(long)(4 * s) * a.ldw] : 0.f;
    for (int blk = 0; blk < nblk; ++blk, k0 += 4 * KB) {
      const bool more = blk + 1 < nblk;
#pragma unroll
      for (int s = 0; s < KB; ++s) bn[s] = (nok && more) ? wcol[(long)(k0 + 4 * KB + 4 * s) * a.ldw] : 0.f;
#pragma unroll
      for (int s = 0; s < KB; s += 2) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * s], bc[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * s + 4], bc[s + 1], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < KB; ++s) bc[s] = bn[s];
    }
  }
  for (; k0 < a.E; k0 += 4) {                                    // E % 128 != 0: the remaining k steps
    const float b0 = nok ? wcol[(long)k0 * a.ldw] : 0.f;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0], b0, acc0, 0, 0, 0);
  }
  if (nok) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = row0 + kq * 4 + g;
      if (r < a.B) a.xz[(long)r * a.ldz + n] = acc0[g] + acc1[g];
    }
  }
}

}  // namespace

extern "C" int32_t tnt_greedy_feedback_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                           const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T, int32_t col,
                                           float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B, float rate,
                                           uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                           int32_t lwidth, int32_t lcol0, void* stream) {
  if (B <= 0) return 0;
  if (V <= 0 || ld < V) return TNT_BADARG(2);
  if (E <= 0 || (E & 3) || E > GF_MAX_E || !tnt_aligned16(table)) return TNT_BADARG(5);
  if (N <= 0 || ldw < N) return TNT_BADARG(7);
  if (col < 0 || col >= T) return TNT_BADARG(11);
  if ((ldt & 3) || ldt < E || !tnt_aligned16(text)) return TNT_BADARG(13);
  if (ldz < N) return TNT_BADARG(15);
  if (!(rate >= 0.f && rate < 1.f)) return TNT_BADARG(17);
  if (rate > 0.f && ((lwidth & 3) || (lcol0 & 3) || lcol0 + E > lwidth)) return TNT_BADARG(22);
  GfArgs a;
  a.logits = logits; a.ld = ld; a.V = V; a.table = table; a.E = E; a.w = w; a.ldw = ldw; a.N = N;
  a.fed = fed; a.T = T; a.col = col; a.text = text; a.ldt = ldt; a.xz = xz; a.ldz = ldz; a.B = B;
  a.rate = rate; a.scale = 1.0f / (1.0f - rate); a.seed = seed; a.site = site; a.step = step; a.step_dev = step_dev;
  a.lwidth = lwidth; a.lcol0 = lcol0;
  a.vec = ((ld & 3) == 0 && tnt_aligned16(logits)) ? 1 : 0;
  const dim3 grid((B + GF_ROWS - 1) / GF_ROWS, (N + GF_COLS - 1) / GF_COLS);
  const size_t lds_bytes = (size_t)GF_ROWS * (E + 4) * sizeof(float);
  hipLaunchKernelGGL(greedy_feedback_kernel, grid, dim3(256), lds_bytes, tnt_stream(stream), a);
  TNT_LAUNCH_CHECK();
  return 0;
}
