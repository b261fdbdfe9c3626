// The learned initial LSTM state of the attention model (Xu et al. 2015, section 3.1.2; the reference names it
// learn_init_state, lc_NIC.py:169-173, and never builds its layers).  Definition: include/tnt_hip.h.
//   m[b][d] = (1/R) sum_r F[b][r][d],   h0 = tanh(m Wh + bh),   c0 = tanh(m Wc + bc)
// The tensors are small (F is B R D floats, D <= 64; the weights 2 D U): every kernel here is one pass with a fixed
// summation order, no atomics and no scratch, so two runs give the same bits.
#include "tnt_common.h"

namespace {
constexpr int IS_T = 256;            // threads of the forward and the input-gradient workgroups
constexpr int IS_DMAX = 64;          // widest region feature

// ---------------------------------------------------------------------------------------------------
// Forward: workgroup b owns scan b, so its bits depend on F[b] and the weights alone (not on B, not on the row's place).
//   phase 1: thread (g, d) = (t / D, t % D), t < G D with G = 256 / D region groups, adds F[b][r][d] for r = g, g + G, ... in
//            ascending order (consecutive threads read consecutive floats); thread d then adds the G partials in group order
//            and divides by R.
//   phase 2: thread t owns the units u = t, t + 256, ...: acc = b[u], then fma(m[d], W[d][u], acc) for d ascending (W rows
//            coalesced over u), tanhf (ocml: relative accuracy, also for small arguments).
__global__ __launch_bounds__(IS_T) void init_state_fwd_kernel(const float* __restrict__ F, const float* __restrict__ Wh,
                                                               const float* __restrict__ bh, const float* __restrict__ Wc,
                                                               const float* __restrict__ bc, float* __restrict__ fmean,
                                                               float* __restrict__ h0, float* __restrict__ c0, int R, int D,
                                                               int U) {
  __shared__ float red[IS_T];
  __shared__ float ms[IS_DMAX];
  const int b = blockIdx.x, t = threadIdx.x;
  const int G = IS_T / D;
  const float* Fb = F + (long)b * R * D;
  if (t < G * D) {
    const int g = t / D;
    const long step = (long)G * D;
    const float* p = Fb + t;                       // element (r = g, d = t % D)
    float s = 0.f;
    int r = g;
    for (; r + 3 * G < R; r += 4 * G) {            // four loads in flight, added in order
      const float x0 = p[0], x1 = p[step], x2 = p[2 * step], x3 = p[3 * step];
      s += x0; s += x1; s += x2; s += x3;
      p += 4 * step;
    }
    for (; r < R; r += G) { s += p[0]; p += step; }
    red[t] = s;
  }
  __syncthreads();
  if (t < D) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += red[g * D + t];
    const float m = s / (float)R;
    ms[t] = m;
    if (fmean != nullptr) fmean[(long)b * D + t] = m;
  }
  __syncthreads();
  for (int u = t; u < U; u += IS_T) {
    float ah = bh[u], ac = bc[u];
    for (int d = 0; d < D; ++d) {
      const float m = ms[d];
      ah = fmaf(m, Wh[(long)d * U + u], ah);
      ac = fmaf(m, Wc[(long)d * U + u], ac);
    }
    h0[(long)b * U + u] = tanhf(ah);
    c0[(long)b * U + u] = tanhf(ac);
  }
}

// ---------------------------------------------------------------------------------------------------
// Backward, launch 1: the parameter gradients.  Workgroup (x, y) of 64 threads: y = 0 the hidden layer, 1 the carry layer;
// thread t owns the unit u = 64 x + t and keeps its column of dW (DP >= D accumulators) and its db in registers.  It walks
// the samples in ascending order: g = ds[b][u] (1 - s[b][u]^2), db += g, dW[d] = fma(fmean[b][d], g, dW[d]); the means of
// 16 samples at a time sit in LDS (zero past D, so the unrolled column needs no bound test).  Written, not accumulated.
template <int DP>
__global__ __launch_bounds__(64) void init_state_bwd_w_kernel(const float* __restrict__ dh0, const float* __restrict__ dc0,
                                                              const float* __restrict__ h0, const float* __restrict__ c0,
                                                              const float* __restrict__ fmean, float* __restrict__ dWh,
                                                              float* __restrict__ dbh, float* __restrict__ dWc,
                                                              float* __restrict__ dbc, int B, int D, int U) {
  constexpr int TB = 16;
  __shared__ float ms[TB][DP];
  const int t = threadIdx.x, u = blockIdx.x * 64 + t;
  const bool carry = blockIdx.y != 0;
  const float* ds = carry ? dc0 : dh0;
  const float* st = carry ? c0 : h0;
  float* dW = carry ? dWc : dWh;
  float* db = carry ? dbc : dbh;
  const bool mine = u < U;
  float acc[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) acc[d] = 0.f;
  float accb = 0.f;
  for (int b0 = 0; b0 < B; b0 += TB) {
    const int nb = min(TB, B - b0);
    __syncthreads();                               // the tile before has been read
    for (int e = t; e < TB * DP; e += 64) {
      const int bb = e / DP, d = e - bb * DP;
      ms[bb][d] = (bb < nb && d < D) ? fmean[(long)(b0 + bb) * D + d] : 0.f;
    }
    __syncthreads();
    if (mine) {
      for (int bb = 0; bb < nb; ++bb) {
        const long e = (long)(b0 + bb) * U + u;
        const float s = st[e];
        const float g = ds[e] * (1.f - s * s);
        accb += g;
#pragma unroll
        for (int d = 0; d < DP; ++d) acc[d] = fmaf(ms[bb][d], g, acc[d]);
      }
    }
  }
  if (mine) {
    db[u] = accb;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) dW[(long)d * U + u] = acc[d];
  }
}

// Backward, launch 2: the gradient of the region features.  Workgroup (b, y): dm[d] = sum_u gh[u] Wh[d][u] + gc[u] Wc[d][u]
// (2 U terms), then dF[b][r][d] += dm[d] / R over slice y of the sample's R D floats.  Every workgroup of a sample forms the
// same dm: wave w owns d = w, w + 4, ...; lane l adds its u = l, l + 64, ... in ascending order (gh, gc of 1024 units at a
// time in LDS, the W rows coalesced over u), then the wave butterfly (tnt_wave_sum: fixed partners, fixed order).
__global__ __launch_bounds__(IS_T) void init_state_bwd_f_kernel(const float* __restrict__ dh0, const float* __restrict__ dc0,
                                                                const float* __restrict__ h0, const float* __restrict__ c0,
                                                                const float* __restrict__ Wh, const float* __restrict__ Wc,
                                                                float* __restrict__ dF, int R, int D, int U) {
  constexpr int UT = 1024, ND = IS_DMAX / 4;
  __shared__ float gh[UT], gc[UT];
  __shared__ float dms[IS_DMAX];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  float acc[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) acc[k] = 0.f;
  for (int u0 = 0; u0 < U; u0 += UT) {
    const int nu = min(UT, U - u0);
    __syncthreads();
    for (int e = t; e < nu; e += IS_T) {
      const long i = (long)b * U + u0 + e;
      const float sh = h0[i], sc = c0[i];
      gh[e] = dh0[i] * (1.f - sh * sh);
      gc[e] = dc0[i] * (1.f - sc * sc);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const int d = w + 4 * k;
      if (d < D) {
        const float* wh = Wh + (long)d * U + u0;
        const float* wc = Wc + (long)d * U + u0;
        float a = acc[k];
        for (int e = lane; e < nu; e += 64) {
          a = fmaf(gh[e], wh[e], a);
          a = fmaf(gc[e], wc[e], a);
        }
        acc[k] = a;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    const int d = w + 4 * k;
    if (d < D) {                                   // (wave-uniform: every lane of the wave takes part in the butterfly)
      const float s = tnt_wave_sum(acc[k]);
      if (lane == 0) dms[d] = s / (float)R;
    }
  }
  __syncthreads();
  const long n = (long)R * D;
  const long per = (n + gridDim.y - 1) / gridDim.y;
  const long e0 = (long)blockIdx.y * per, e1 = min(n, e0 + per);
  float* dFb = dF + (long)b * n;
  for (long e = e0 + t; e < e1; e += IS_T) dFb[e] += dms[(int)(e % D)];
}
}  // namespace

extern "C" int32_t tnt_init_state_fwd_f32(const float* F, const float* Wh, const float* bh, const float* Wc, const float* bc,
                                          float* fmean, float* h0, float* c0, int32_t B, int32_t R, int32_t D, int32_t U,
                                          void* stream) {
  if (F == nullptr || Wh == nullptr || bh == nullptr || Wc == nullptr || bc == nullptr || h0 == nullptr || c0 == nullptr)
    return TNT_BADARG(1);
  if (B <= 0 || R <= 0 || U <= 0) return TNT_BADARG(9);
  if (D <= 0 || D > IS_DMAX) return TNT_BADARG(11);
  hipLaunchKernelGGL(init_state_fwd_kernel, dim3(B), dim3(IS_T), 0, tnt_stream(stream), F, Wh, bh, Wc, bc, fmean, h0, c0, R, D,
                     U);
  TNT_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t tnt_init_state_bwd_f32(const float* dh0, const float* dc0, const float* h0, const float* c0,
                                          const float* fmean, const float* Wh, const float* Wc, float* dWh, float* dbh,
                                          float* dWc, float* dbc, float* dF, int32_t B, int32_t R, int32_t D, int32_t U,
                                          void* stream) {
  if (dh0 == nullptr || dc0 == nullptr || h0 == nullptr || c0 == nullptr || fmean == nullptr || Wh == nullptr ||
      Wc == nullptr)
    return TNT_BADARG(1);
  const int nw = (dWh != nullptr) + (dbh != nullptr) + (dWc != nullptr) + (dbc != nullptr);
  if (nw != 0 && nw != 4) return TNT_BADARG(8);            // the four parameter gradients: all of them or none
  if (B <= 0 || R <= 0 || U <= 0) return TNT_BADARG(13);
  if (D <= 0 || D > IS_DMAX) return TNT_BADARG(15);
  if (nw == 4) {
    const dim3 gw((U + 63) / 64, 2);
    void (*kw)(const float*, const float*, const float*, const float*, const float*, float*, float*, float*, float*, int, int,
               int) = D <= 16 ? init_state_bwd_w_kernel<16> : D <= 32 ? init_state_bwd_w_kernel<32> : init_state_bwd_w_kernel<64>;
    hipLaunchKernelGGL(kw, gw, dim3(64), 0, tnt_stream(stream), dh0, dc0, h0, c0, fmean, dWh, dbh, dWc, dbc, B, D, U);
    TNT_LAUNCH_CHECK();
  }
  if (dF == nullptr) return 0;
  // slices of a sample's R D floats: enough workgroups to cover the chip at small B, each with at least one pass of work
  const long n = (long)R * D;
  int ny = B >= 256 ? 1 : 256 / B;
  if (ny > 8) ny = 8;
  if ((long)ny > (n + IS_T - 1) / IS_T) ny = (int)((n + IS_T - 1) / IS_T);
  hipLaunchKernelGGL(init_state_bwd_f_kernel, dim3(B, ny), dim3(IS_T), 0, tnt_stream(stream), dh0, dc0, h0, c0, Wh, Wc, dF, R,
                     D, U);
  TNT_LAUNCH_CHECK();
  return 0;
}
