// ROUGE-L of captions on the device (tnt_caption_rouge_f32; the definition is in include/tnt_hip.h): the longest common
// subsequence of each of the K sampled captions of a scan (and of its greedy caption) with each of the scan's references,
// pycocoevalcap's F-score of the two separately maximised ratios, and the advantages tnt_scst_cce_f32 reads.  The
// candidate, reference and output layout is tnt_caption_reward_f32's (reward.hip), so that the self-critical step puts
// either launch in the same place.
//
// A caption holds at most 64 tokens and a wave has 64 lanes, so a caption is one token per lane and a set of its
// positions is one 64-bit word.  One workgroup of 1024 threads (16 waves) per scan b; its rows are the C = K (+ 1: the
// greedy caption) candidates and then the M references, S = C + M <= 25:
//   0. stage: wave w takes the rows w, w + 16: lane t loads token t, the row goes to LDS (row stride 65 words), and
//      the row's length is the position of the first set bit of __ballot(terminator or t >= L).
//   1. wave w takes the (candidate c, reference j) pairs w, w + 16, ... of the (K+1) x M grid.  Lane i holds token i of
//      the candidate and token i of the reference.  For each word of the reference (a wave-uniform loop; word q is a
//      lane read of lane q's register, no memory access sits in the dependent chain) the match vector is
//      Mv = __ballot(i < len_c && tok_i == word), and the bit-vector recurrence of the LCS (Allison & Dix 1986 in
//      Hyyro's 2004 form) advances: u = V & Mv; V = (V + u) | (V - u), from V = all ones.  Bit i of V is 0 where the
//      DP row increases at column i, so lcs = popcount(~V & __ballot(i < len_c)).  The vectors are wave-uniform: they
//      live in scalar registers, and there is no DP table.  The length mask is a ballot, never a shift by the length:
//      a length of 64 is legal.
//   2. thread c turns its row of lcs values into the score (float64, each operation rounded on its own), thread k < K
//      into the advantage (one float32 rounding).
// Tokens are only compared.  No atomics, no scratch memory, fixed order: deterministic.
#include "tnt_common.h"

namespace {

constexpr int RG_THREADS = 1024;               // 16 waves: the 25 rows in two rounds, the 136 pairs in nine
constexpr int RG_WAVES = RG_THREADS / 64;
constexpr int RG_MAXK = 16;                 // samples per scan
constexpr int RG_MAXC = RG_MAXK + 1;        // candidates: the samples and the greedy caption
constexpr int RG_MAXM = 8;                  // references per scan
constexpr int RG_MAXS = RG_MAXC + RG_MAXM;  // rows staged
constexpr int RG_MAXL = 64;                 // tokens per row: one per lane
constexpr int RG_LDT = RG_MAXL + 1;         // LDS row stride of the tokens

struct RougeArgs {
  const int* fed; const int* last; const int* greedy; const int* refs; const int* n_refs;
  int T, ldg, M, Lr, B, K, end_id, baseline;
  double beta;
  float* adv; double* score; int* counted; int* lcs;
};

__global__ __launch_bounds__(RG_THREADS) void caption_rouge_kernel(RougeArgs a) {
  __shared__ int tok[RG_MAXS * RG_LDT];
  __shared__ int len[RG_MAXS];
  __shared__ int lc[RG_MAXC * RG_MAXM];
  __shared__ double sc[RG_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, K = a.K, M = a.M, Lr = a.Lr;
  const int C = K + (a.baseline == 0 ? 1 : 0), S = C + M;
  const int nref = __builtin_amdgcn_readfirstlane(min(max(a.n_refs[b], 0), M));   // uniform: kept in a scalar register

  // ---- 0. stage: a row per wave and round, its length from one ballot
  for (int s = wave; s < S; s += RG_WAVES) {
    const int L = s < C ? T : Lr;
    int v = 0;
    if (s < K) {
      const long r = (long)b * K + s;
      if (lane < T - 1) v = a.fed[r * T + 1 + lane];
      else if (lane == T - 1) v = a.last[r];
    } else if (s < C) {
      if (lane < T) v = a.greedy[(long)lane * a.ldg + b];
    } else if (s - C < nref && lane < Lr) {
      v = a.refs[((long)b * M + (s - C)) * Lr + lane];
    }
    tok[s * RG_LDT + lane] = v;
    const unsigned long long stop = __ballot(lane >= L || v == 0 || (a.end_id >= 0 && v == a.end_id));
    const int n = stop != 0ull ? __ffsll((long long)stop) - 1 : RG_MAXL;
    if (lane == 0) {
      len[s] = n;
      if (s < K) a.counted[(long)b * K + s] = min(n + 1, T);
    }
  }
  __syncthreads();

  // ---- 1. the (candidate, reference) pairs: a pair per wave and round
  for (int x = wave; x < (K + 1) * M; x += RG_WAVES) {
    const int c = x / M, j = x - c * M;
    int l = 0;
    if (c < C && j < nref) {
      const int nc = __builtin_amdgcn_readfirstlane(len[c]), nr = __builtin_amdgcn_readfirstlane(len[C + j]);
      const int mine = tok[c * RG_LDT + lane];           // lane i: token i of the candidate ...
      const int theirs = tok[(C + j) * RG_LDT + lane];   // ... and of the reference: word q is a lane read, not a memory read
      const unsigned long long in = __ballot(lane < nc);  // the length mask: a ballot, never 1 << len (len = 64 is legal)
      unsigned long long V = ~0ull;
      for (int q = 0; q < nr; ++q) {                      // __ballot(lane < nc && mine == word), without a branch per word
        const unsigned long long u = V & in & __ballot(mine == __builtin_amdgcn_readlane(theirs, q));
        V = (V + u) | (V - u);
      }
      l = __popcll(~V & in);
    }
    if (lane == 0) {
      lc[c * RG_MAXM + j] = l;
      if (a.lcs) a.lcs[((long)b * (K + 1) + c) * M + j] = l;
    }
  }
  __syncthreads();

  // ---- 2. the score: the two ratios are maximised separately over the references that hold a word
  if (tid < C) {
    const int nc = len[tid];
    double P = 0.0, R = 0.0;
    if (nc > 0) {
      for (int j = 0; j < nref; ++j) {
        const int nr = len[C + j];
        if (nr == 0) continue;
        const double l = (double)lc[tid * RG_MAXM + j];
        P = fmax(P, l / (double)nc);
        R = fmax(R, l / (double)nr);
      }
    }
    double u = 0.0;
    if (P != 0.0) {
#pragma clang fp contract(off)                          // the header's order: every product and sum rounded on its own, no fma
      const double b2 = a.beta * a.beta;
      const double num = ((1.0 + b2) * P) * R;
      const double den = R + b2 * P;
      u = num / den;
    }
    sc[tid] = u;
  }
  __syncthreads();

  // ---- the advantages
  if (tid < K) {
    const double own = sc[tid];
    double base;
    if (a.baseline == 0) {
      base = sc[K];
    } else {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += sc[k];
      base = (s - own) / (double)(K - 1);
    }
    a.adv[(long)b * K + tid] = (float)(own - base);
    if (a.score) a.score[(long)b * (K + 1) + tid] = own;
  }
  if (tid == K && a.score) a.score[(long)b * (K + 1) + K] = a.baseline == 0 ? sc[K] : 0.0;
}

bool rg_overlap(const void* p, uintptr_t np, const void* q, uintptr_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p != nullptr && q != nullptr && a < b + nq && b < a + np;
}

}  // namespace

extern "C" int32_t tnt_caption_rouge_f32(const int32_t* fed, int32_t T, const int32_t* last, const int32_t* greedy,
                                         int32_t ldg, const int32_t* refs, const int32_t* n_refs, int32_t M, int32_t Lr,
                                         int32_t B, int32_t K, int32_t end_id, const double* beta_host, int32_t baseline, float* adv,
                                         double* score, int32_t* counted, int32_t* lcs, void* stream) {
  if (!fed) return TNT_BADARG(0);
  if (T < 1 || T > RG_MAXL) return TNT_BADARG(1);
  if (!last) return TNT_BADARG(2);
  if (B <= 0) return TNT_BADARG(9);
  if (K < 1 || K > RG_MAXK) return TNT_BADARG(10);
  if (!beta_host) return TNT_BADARG(12);
  const double beta = *beta_host;                      // a host pointer, read now: this ABI passes a float64 by address
  if (!(beta > 0.0) || !(beta * beta <= 1.7976931348623157e308)) return TNT_BADARG(12);        // NaN fails both
  if (baseline != 0 && baseline != 1) return TNT_BADARG(13);
  if (baseline == 0 && !greedy) return TNT_BADARG(3);
  if (baseline == 0 && ldg < B) return TNT_BADARG(4);
  if (baseline == 1 && K < 2) return TNT_BADARG(10);
  if (!refs) return TNT_BADARG(5);
  if (!n_refs) return TNT_BADARG(6);
  if (M < 1 || M > RG_MAXM) return TNT_BADARG(7);
  if (Lr < 1 || Lr > RG_MAXL) return TNT_BADARG(8);
  if (!adv) return TNT_BADARG(14);
  if (!counted) return TNT_BADARG(16);
  {                                                    // the inputs are read while the outputs are written
    const uintptr_t uB = (uintptr_t)B, R = uB * (uintptr_t)K, i4 = sizeof(int32_t);
    const void* in[5] = {fed, last, baseline == 0 ? greedy : nullptr, refs, n_refs};
    const uintptr_t nin[5] = {R * (uintptr_t)T * i4, R * i4, (((uintptr_t)T - 1) * (uintptr_t)(ldg > 0 ? ldg : 0) + uB) * i4,
                              uB * (uintptr_t)M * (uintptr_t)Lr * i4, uB * i4};
    const void* out[4] = {adv, score, counted, lcs};
    const uintptr_t nout[4] = {R * sizeof(float), uB * (uintptr_t)(K + 1) * sizeof(double), R * i4,
                               uB * (uintptr_t)(K + 1) * (uintptr_t)M * i4};
    const int code[4] = {14, 15, 16, 17};
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 5; ++i)
        if (rg_overlap(in[i], nin[i], out[o], nout[o])) return TNT_BADARG(code[o]);
      for (int p = 0; p < o; ++p)
        if (rg_overlap(out[p], nout[p], out[o], nout[o])) return TNT_BADARG(code[o]);
    }
  }
  RougeArgs a;
  a.fed = fed; a.last = last; a.greedy = baseline == 0 ? greedy : nullptr; a.refs = refs; a.n_refs = n_refs;
  a.T = T; a.ldg = ldg; a.M = M; a.Lr = Lr; a.B = B; a.K = K; a.end_id = end_id; a.baseline = baseline; a.beta = beta;
  a.adv = adv; a.score = score; a.counted = counted; a.lcs = lcs;
  hipLaunchKernelGGL(caption_rouge_kernel, dim3(B), dim3(RG_THREADS), 0, tnt_stream(stream), a);
  TNT_LAUNCH_CHECK();
  return 0;
}
