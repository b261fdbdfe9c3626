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

// The mask in front of the LSTM input mask (tnt_scheduled_feedback2_f32: the Embedding Dropout): row b, element
// b lwidth + lcol0 + j of the stream (seed, site, step + *step_dev); rate 0: none.
struct GfMask {
  float rate, scale; uint32_t site; int lwidth, lcol0;
};

// 2. the 16 rows' Embedding rows (id s_id[rr]) through [kText: the mask tm, then] the LSTM input mask of step col
// (rows_per_site = B: local row b, element b lwidth + lcol0 + j) -> LDS image s_text [16][E + 4]; the lead workgroup of a
// row tile also stores them to text.  nthr threads, this one tid.  Elementwise: the values do not depend on nthr.  The
// two masks are applied in the order and with the arithmetic of tnt_embedding_fwd_drop2_f32 (emb_fwd_drop_kernel).
template <bool kText>
__device__ __forceinline__ void gf_gather(const GfArgs& a, const GfMask& tm, const int* s_id, float* s_text, int row0,
                                          bool lead, int tid, int nthr) {
  const uint32_t step = a.step + (a.step_dev ? a.step_dev[0] : 0u);
  const int e4 = a.E >> 2, lds = a.E + 4;
  for (int c = tid; c < GF_ROWS * e4; c += nthr) {
    const int rr = c / e4, j = (c - rr * e4) * 4, r = row0 + rr;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < a.B) {
      v = *reinterpret_cast<const float4*>(a.table + (long)s_id[rr] * a.E + j);
      if (kText && tm.rate > 0.f) {
        bool k[4];
        tnt_keep4((uint64_t)r * (uint64_t)tm.lwidth + (uint64_t)(tm.lcol0 + j), tm.rate, a.seed, tm.site, step, k);
        v = make_float4(k[0] ? v.x * tm.scale : 0.f, k[1] ? v.y * tm.scale : 0.f, k[2] ? v.z * tm.scale : 0.f,
                        k[3] ? v.w * tm.scale : 0.f);
      }
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
}

// 3. one wave: xz[16 rows of the tile x column n = this lane's (lane & 15)] = text . w on v_mfma_f32_16x16x4_f32
// (A[l&15][k = l>>4], B[k = l>>4][l&15]; C col = l&15, row = 4(l>>4) + reg).  Both feedback kernels call this, so their
// projections are the same bits.
__device__ __forceinline__ void gf_project(const GfArgs& a, const float* s_text, int row0, int n, int lane) {
  const int lds = a.E + 4;
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

__global__ __launch_bounds__(256) void greedy_feedback_kernel(GfArgs a) {
  extern __shared__ float4 gf_lds4[];
  float* s_text = reinterpret_cast<float*>(gf_lds4);
  __shared__ int s_id[GF_ROWS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GF_ROWS;

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
  if (blockIdx.y == 0 && threadIdx.x < GF_ROWS && row0 + (int)threadIdx.x < a.B)
    a.fed[(long)(row0 + threadIdx.x) * a.T + a.col] = s_id[threadIdx.x];

  // ---- 2. gather + the LSTM input mask; 3. text . w
  gf_gather<false>(a, GfMask{}, s_id, s_text, row0, blockIdx.y == 0, threadIdx.x, 256);
  __syncthreads();
  gf_project(a, s_text, row0, blockIdx.y * GF_COLS + wave * 16 + (lane & 15), lane);
}


// ============================================================================================ scheduled sampling
// tnt_scheduled_feedback_f32 (definition in include/tnt_hip.h): the same gather and projection, but each row's token is a
// coin between the ground truth and the model's own token, and the row's decision is made once per workgroup by one wave.
// Workgroup (bx, by): rows 16 bx .. 16 bx + 15 x projection columns 128 by .. 128 by + 127 (8 waves x 16): twice the
// columns of greedy_feedback_kernel per decision, so the logits are read by N / 128 workgroups instead of N / 64, and a row
// whose coin picks the ground truth is not read at all.
//   1. wave w decides rows 2w, 2w + 1: the coin; then (model rows only) the argmax (greedy) or the categorical draw of
//      tnt_sample_rows_f32 at temperature 1 (sample): its 256 contiguous chunks, 4 per lane, the chunk sums in the same
//      serial order, the serial prefix over them, the same target search -- the same id as that kernel;
//   2., 3. gf_gather, gf_project.
// tnt_scheduled_feedback2_f32 is the same kernel with the Embedding Dropout in front of the LSTM input mask (kText: the
// attention model, whose teacher-forced text rows carry both masks); with its rate 0 it computes the bits of the first.
constexpr int SF_WAVES = 8;
constexpr int SF_COLS = SF_WAVES * 16;

struct SfArgs {
  GfArgs g;
  int kind, mode;                    // kind 0 linear, 1 inverse sigmoid; mode 0 greedy, 1 sample
  const double* sched;               // device [3]: linear p0, slope, p_max; inverse sigmoid k, -, p_max
  const int64_t* counter;            // updates applied so far (the model's adam_t)
  uint32_t coin_site, draw_site;
  GfMask text;                       // kText only: the mask in front of the LSTM input mask
};

// p of the schedule at the live counter: float64, rounded once to float32 (model_base.scheduled_p restates it)
__device__ __forceinline__ float sf_prob(const SfArgs& sa) {
  const double i = (double)sa.counter[0];
  const double s0 = sa.sched[0], s1 = sa.sched[1], s2 = sa.sched[2];
  double p;
  if (sa.kind == 0) {
    p = __dadd_rn(s0, __dmul_rn(s1, i));                        // no contraction to an fma: the host rounds twice
    p = fmin(fmax(p, 0.0), s2);
  } else {
    p = s2 * (1.0 - s0 / (s0 + exp(i / s0)));
  }
  return (float)p;
}

// Philox word of element e (tnt_rng.h's stream), select chain (a runtime index would send the 4 words to scratch memory)
__device__ __forceinline__ uint32_t sf_word(uint64_t e, uint64_t seed, uint32_t site, uint32_t step) {
  const uint64_t g = e >> 2;
  const TntPhilox4 r = tnt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t sel = (uint32_t)e & 3u;
  return sel == 0u ? r.v[0] : (sel == 1u ? r.v[1] : (sel == 2u ? r.v[2] : r.v[3]));
}

// argmax of one row by one wave (gf_take's order): the id, always in [0, V)
__device__ __forceinline__ int sf_argmax_row(const float* x, int V, int vec, int lane) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  int j0 = 0;
  if (vec) {
    const int v4 = V >> 2;
    const float qnan = __builtin_nanf("");
    for (int k = lane; k < v4; k += 256) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = k + 64 * u;
        v[u] = kk < v4 ? reinterpret_cast<const float4*>(x)[kk] : make_float4(qnan, qnan, qnan, qnan);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = 4 * (k + 64 * u);
        gf_take(v[u].x, j, best, bi); gf_take(v[u].y, j + 1, best, bi);
        gf_take(v[u].z, j + 2, best, bi); gf_take(v[u].w, j + 3, best, bi);
      }
    }
    j0 = v4 << 2;
  }
  for (int j = j0 + lane; j < V; j += 64) gf_take(x[j], j, best, bi);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(best, m);
    const int oi = __shfl_xor(bi, m);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  return (bi >= 0 && bi < V) ? bi : 0;
}

// tnt_sample_rows_f32's draw (from_logits, temperature 1) of one row by one wave: lane l owns chunks l, l + 64, l + 128,
// l + 192 of that kernel's 256 chunks of C = ceil(V / 256) contiguous columns.  part: 257 floats of LDS for this wave.
// Returns the id (0 where no chunk takes the target: a row of NaNs or -infs).
__device__ __forceinline__ int sf_sample_row(const float* x, int V, float u, float* part, int lane) {
  const int C = (V + 255) / 256;
  float mx = -INFINITY;
  for (int q = 0; q < 4; ++q) {
    const int t = lane + 64 * q, j0 = t * C, j1 = min(V, j0 + C);
    for (int j = j0; j < j1; ++j) mx = fmaxf(mx, x[j]);
  }
  mx = tnt_wave_max(mx);
  for (int q = 0; q < 4; ++q) {
    const int t = lane + 64 * q, j0 = t * C, j1 = min(V, j0 + C);
    float loc = 0.f;
    for (int j = j0; j < j1; ++j) loc += expf((x[j] - mx) * 1.0f);
    part[t + 1] = loc;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if (lane == 0) {                      // fixed-order prefix over the 256 chunk sums
    part[0] = 0.f;
    float run = 0.f;
    for (int t = 1; t <= 256; ++t) { run += part[t]; part[t] = run; }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float target = u * part[256];
  const int tlast = (V - 1) / C;
  int pick = -1;
  for (int q = 0; q < 4; ++q) {
    const int t = lane + 64 * q, j0 = t * C, j1 = min(V, j0 + C);
    if (part[t] <= target && (target < part[t + 1] || t == tlast)) {
      float run = part[t];
      int pk = j1 - 1;
      for (int j = j0; j < j1; ++j) {
        run += expf((x[j] - mx) * 1.0f);
        if (run > target) { pk = j; break; }
      }
      pick = pk;
    }
  }
  // at most one chunk takes the target; the wave agrees on it
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) pick = max(pick, __shfl_xor(pick, m));
  return (pick >= 0 && pick < V) ? pick : 0;
}

template <bool kText>
__global__ __launch_bounds__(SF_WAVES * 64) void scheduled_feedback_kernel(SfArgs sa) {
  const GfArgs& a = sa.g;
  extern __shared__ float4 gf_lds4[];
  float* s_text = reinterpret_cast<float*>(gf_lds4);
  __shared__ int s_id[GF_ROWS];
  __shared__ float s_part[SF_WAVES][257];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GF_ROWS;
  const bool lead = blockIdx.y == 0;
  const uint32_t step = a.step + (a.step_dev ? a.step_dev[0] : 0u);
  const float p = sf_prob(sa);
  const uint32_t thr = tnt_keep_threshold(p);

  // ---- 1. the decisions of rows 2 wave, 2 wave + 1 (wave-uniform branches)
#pragma unroll
  for (int q = 0; q < GF_ROWS / SF_WAVES; ++q) {
    const int rr = wave * (GF_ROWS / SF_WAVES) + q, r = row0 + rr;
    int id = 0;
    if (r < a.B) {
      long at = (long)r * a.T + a.col;
      // the coin: element r of the coin site dropped at rate p (tnt_keep's rule) feeds the model's token
      const bool model = (sf_word((uint64_t)r, a.seed, sa.coin_site, step) >> 8) < thr;
      if (!model) {
        id = min(max(a.fed[at], 0), a.V - 1);                   // the ground truth, not written back
      } else {
        const float* x = a.logits + (long)r * a.ld;
        if (sa.mode == 0) {
          id = sf_argmax_row(x, a.V, a.vec, lane);
        } else {
          const float u = (float)(sf_word((uint64_t)r, a.seed, sa.draw_site, step) >> 8) * 5.9604644775390625e-08f;
          id = sf_sample_row(x, a.V, u, s_part[wave], lane);
        }
        if (lead && lane == 0) a.fed[at] = id;
      }
    }
    if (lane == 0) s_id[rr] = id;
  }
  __syncthreads();

  // ---- 2. gather + the LSTM input mask; 3. text . w
  gf_gather<kText>(a, sa.text, s_id, s_text, row0, lead, threadIdx.x, SF_WAVES * 64);
  __syncthreads();
  gf_project(a, s_text, row0, blockIdx.y * SF_COLS + wave * 16 + (lane & 15), lane);
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

namespace {

// argument checks and launch of both scheduled-sampling entry points (text_mask == nullptr: tnt_scheduled_feedback_f32)
int32_t sf_launch(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E, const float* w, int32_t ldw,
                  int32_t N, int32_t* fed, int32_t T, int32_t col, float* text, int32_t ldt, float* xz, int32_t ldz,
                  int32_t B, float rate, uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                  int32_t lwidth, int32_t lcol0, int32_t kind, int32_t mode, const double* sched, const int64_t* counter,
                  uint32_t coin_site, uint32_t draw_site, const GfMask* text_mask, void* stream) {
  if (B <= 0) return 0;
  if (V <= 0 || ld < V || !logits) return TNT_BADARG(2);
  if (E <= 0 || (E & 3) || E > GF_MAX_E || !tnt_aligned16(table)) return TNT_BADARG(5);
  if (N <= 0 || ldw < N || !w) return TNT_BADARG(7);
  if (!fed) return TNT_BADARG(9);
  if (col < 1 || col >= T) return TNT_BADARG(11);
  if ((ldt & 3) || ldt < E || !text || !tnt_aligned16(text)) return TNT_BADARG(13);
  if (ldz < N || !xz) return TNT_BADARG(15);
  if (!(rate >= 0.f && rate < 1.f)) return TNT_BADARG(17);
  if (rate > 0.f && ((lwidth & 3) || (lcol0 & 3) || lcol0 + E > lwidth)) return TNT_BADARG(22);
  if (kind != 0 && kind != 1) return TNT_BADARG(24);
  if (mode != 0 && mode != 1) return TNT_BADARG(25);
  if (!sched) return TNT_BADARG(26);
  if (!counter) return TNT_BADARG(27);
  if (text_mask) {
    const GfMask& m = *text_mask;
    if (!(m.rate >= 0.f && m.rate < 1.f)) return TNT_BADARG(30);
    if (m.rate > 0.f && ((m.lwidth & 3) || (m.lcol0 & 3) || m.lcol0 < 0 || m.lcol0 + E > m.lwidth)) return TNT_BADARG(32);
  }
  SfArgs sa;
  GfArgs& a = sa.g;
  a.logits = logits; a.ld = ld; a.V = V; a.table = table; a.E = E; a.w = w; a.ldw = ldw; a.N = N;
  a.fed = fed; a.T = T; a.col = col; a.text = text; a.ldt = ldt; a.xz = xz; a.ldz = ldz; a.B = B;
  a.rate = rate; a.scale = 1.0f / (1.0f - rate); a.seed = seed; a.site = site; a.step = step; a.step_dev = step_dev;
  a.lwidth = lwidth; a.lcol0 = lcol0;
  a.vec = ((ld & 3) == 0 && tnt_aligned16(logits)) ? 1 : 0;
  sa.kind = kind; sa.mode = mode; sa.sched = sched; sa.counter = counter;
  sa.coin_site = coin_site; sa.draw_site = draw_site;
  sa.text = text_mask ? *text_mask : GfMask{0.f, 1.f, 0u, 0, 0};
  const dim3 grid((B + GF_ROWS - 1) / GF_ROWS, (N + SF_COLS - 1) / SF_COLS);
  const size_t lds_bytes = (size_t)GF_ROWS * (E + 4) * sizeof(float);
  if (text_mask)
    hipLaunchKernelGGL(scheduled_feedback_kernel<true>, grid, dim3(SF_WAVES * 64), lds_bytes, tnt_stream(stream), sa);
  else
    hipLaunchKernelGGL(scheduled_feedback_kernel<false>, grid, dim3(SF_WAVES * 64), lds_bytes, tnt_stream(stream), sa);
  TNT_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int32_t tnt_scheduled_feedback_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                              const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T,
                                              int32_t col, float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B,
                                              float rate, uint64_t seed, uint32_t site, uint32_t step,
                                              const uint32_t* step_dev, int32_t lwidth, int32_t lcol0, int32_t kind,
                                              int32_t mode, const double* sched, const int64_t* counter,
                                              uint32_t coin_site, uint32_t draw_site, void* stream) {
  return sf_launch(logits, ld, V, table, E, w, ldw, N, fed, T, col, text, ldt, xz, ldz, B, rate, seed, site, step, step_dev,
                   lwidth, lcol0, kind, mode, sched, counter, coin_site, draw_site, nullptr, stream);
}

extern "C" int32_t tnt_scheduled_feedback2_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                               const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T,
                                               int32_t col, float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B,
                                               float rate, uint64_t seed, uint32_t site, uint32_t step,
                                               const uint32_t* step_dev, int32_t lwidth, int32_t lcol0, int32_t kind,
                                               int32_t mode, const double* sched, const int64_t* counter,
                                               uint32_t coin_site, uint32_t draw_site, float rate_t, uint32_t site_t,
                                               int32_t lwidth_t, int32_t lcol0_t, void* stream) {
  const GfMask tm{rate_t, 1.0f / (1.0f - rate_t), site_t, lwidth_t, lcol0_t};
  return sf_launch(logits, ld, V, table, E, w, ldw, N, fed, T, col, text, ldt, xz, ldz, B, rate, seed, site, step, step_dev,
                   lwidth, lcol0, kind, mode, sched, counter, coin_site, draw_site, &tm, stream);
}
