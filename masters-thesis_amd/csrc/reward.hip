// Caption rewards of the self-critical step, scored on the device (tnt_caption_reward_f32; the definition is in
// include/tnt_hip.h): CIDEr-D against a corpus table of document frequencies, or BLEU-4 against several references, of
// the K sampled captions of a scan (and its greedy caption), and from them the advantages tnt_scst_cce_f32 reads.
//
// One workgroup of 256 threads per scan b.  Its sequences are the C = K (+ 1: the greedy caption) candidates and then
// the M references, S = C + M <= 25 rows of at most 64 tokens:
//   0. stage: the rows go to LDS once (row stride 65 words: the rows start in different banks), thread s finds the
//      length of row s (the tokens before the first end_id or 0).
//   1. dealt over the (row s, position p) pairs: per order k the number of times the k-gram at p occurs in s, or 0 when
//      it occurred before p (a gram is counted at its first position) or runs past the end; four counts <= 64 packed
//      into one word hc[s][p], as in mbr.hip.  kind 0: the gram's 64-bit key is searched in the table (binary search,
//      integer) and the entry's idf, or log(ndoc), goes to idv[s][p][k]: each gram is looked up once.
//   2. kind 0: thread (s, k) sums the row's squared tf-idf norm in ascending p; then thread (c, j) walks the first
//      positions of candidate c, counts each gram in reference j (integer compares on a sliding window), and sums the
//      clipped tf-idf products per order in ascending p: evaluate.CiderD._sim's terms in its order.
//      kind 1: the (c, p < T, j < n_refs) triples are dealt over the threads, each leaves the packed counts of the grams
//      at (c, p) in reference j; thread c then clips by the maximum over j and sums: evaluate.sentence_bleu's p_k.
//   3. thread c turns its sums into the score (float64), thread k < K into the advantage (one float32 rounding).
// Tokens are compared, or packed into a key; they never index anything.  No atomics, no scratch memory, fixed summation
// orders: deterministic.
#include "tnt_common.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr int RW_MAXK = 16;                 // samples per scan
constexpr int RW_MAXC = RW_MAXK + 1;        // candidates: the samples and the greedy caption
constexpr int RW_MAXM = 8;                  // references per scan
constexpr int RW_MAXS = RW_MAXC + RW_MAXM;  // rows staged
constexpr int RW_MAXL = 64;                 // tokens per row
constexpr int RW_MAXO = 4;                  // n-gram order (CIDEr-D's n, BLEU-4)
constexpr int RW_LDT = RW_MAXL + 1;         // LDS row stride of the tokens and the counts
constexpr double RW_EPS = 0.1;              // evaluate.sentence_bleu's method-1 epsilon

struct RewardArgs {
  const int* fed; const int* last; const int* greedy; const int* refs; const int* n_refs;
  const unsigned long long* keys; const double* idf; const double* params;
  int T, ldg, M, Lr, n_keys, B, K, end_id, kind, baseline;
  float* adv; double* score; int* counted;
};

// the length m <= lim of the common prefix of the window x0..x3 and the gram g0..g3: branch-free, on registers
__device__ __forceinline__ int rw_prefix(int x0, int x1, int x2, int x3, int g0, int g1, int g2, int g3, int lim) {
  int m = x0 == g0;
  m += (m == 1) & (x1 == g1);
  m += (m == 2) & (x2 == g2);
  m += (m == 3) & (x3 == g3);
  return min(m, lim);
}

// one in the bytes [0, m) of a word, 0 <= m <= 4: an occurrence of the k-gram for every k <= m
__device__ __forceinline__ unsigned rw_ones(int m) { return m == 0 ? 0u : (0x01010101u >> (8 * (RW_MAXO - m))); }

__device__ __forceinline__ int rw_byte(unsigned w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

// the packed counts, per order, of the gram g0..g3 (kmax orders) in the row r of n tokens
__device__ __forceinline__ unsigned rw_count(const int* r, int n, int g0, int g1, int g2, int g3, int kmax) {
  unsigned cnt = 0;
  int x0 = r[0], x1 = r[1], x2 = r[2], x3 = r[3];
  for (int q = 0; q < n; ++q) {
    cnt += rw_ones(rw_prefix(x0, x1, x2, x3, g0, g1, g2, g3, min(kmax, n - q)));
    x0 = x1; x1 = x2; x2 = x3; x3 = r[q + 4];
  }
  return cnt;
}

// the indices of four keys in the ascending table of n entries, or -1 (also where want[k] is false): the four lower
// bounds walk the table side by side, so that a level costs one memory latency, not four.  Branch-free halving
// (Khuong & Morin 2017): the answer stays inside [base, base + m]; every index read is below n.
__device__ __forceinline__ void rw_find4(const unsigned long long* keys, int n, const unsigned long long (&key)[RW_MAXO],
                                         const bool (&want)[RW_MAXO], int (&f)[RW_MAXO]) {
  int base[RW_MAXO] = {0, 0, 0, 0};
  for (int m = n; m > 1;) {
    const int half = m >> 1;
#pragma unroll
    for (int k = 0; k < RW_MAXO; ++k)
      if (want[k] && keys[base[k] + half - 1] < key[k]) base[k] += half;
    m -= half;
  }
#pragma unroll
  for (int k = 0; k < RW_MAXO; ++k) {
    f[k] = -1;
    if (want[k] && n > 0) {
      unsigned long long v = keys[base[k]];
      int i = base[k];
      if (v < key[k]) { ++i; v = i < n ? keys[i] : 0ull; }          // a key is never 0: its first word is >= 1
      if (v == key[k]) f[k] = i;
    }
  }
}

__global__ __launch_bounds__(RW_THREADS) void caption_reward_kernel(RewardArgs a) {
  __shared__ int tok[RW_MAXS * RW_LDT + RW_MAXO];       // the tail words: grams and windows are loaded unguarded, up to
                                                        // word len + 3 of a row (compared under lim only)
  __shared__ unsigned hc[RW_MAXS * RW_LDT];
  // kind 0: idv[s][p][k], the idf of the k-gram at (s, p) (RW_MAXS * 64 * 4 doubles);
  // kind 1: wk[c][p][j], the packed counts of the grams at (c, p) in reference j (RW_MAXC * 64 * 8 words)
  __shared__ double idv[RW_MAXS * RW_MAXL * RW_MAXO];
  int* const wk = reinterpret_cast<int*>(idv);
  __shared__ double norm[RW_MAXS * RW_MAXO];
  __shared__ double sim[RW_MAXC * RW_MAXM];
  __shared__ double sc[RW_MAXC];
  __shared__ int len[RW_MAXS];
  static_assert(RW_MAXC * RW_MAXL * RW_MAXM * sizeof(int) <= sizeof(idv), "idv holds either use");
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.T, K = a.K, M = a.M, Lr = a.Lr;
  const int C = K + (a.baseline == 0 ? 1 : 0), S = C + M;
  const int nref = min(max(a.n_refs[b], 0), M);
  const int Lm = max(T, Lr);                            // the positions a row can hold: what is dealt over the threads
  const double logn = a.kind == 0 ? a.params[0] : 0.0;  // the idf of a gram that is in no table entry

  // ---- 0. stage
  for (int x = tid; x < S * Lm; x += RW_THREADS) {
    const int s = x / Lm, t = x - s * Lm;
    int v = 0;
    if (s < K) {
      const long r = (long)b * K + s;
      if (t < T - 1) v = a.fed[r * T + 1 + t];
      else if (t == T - 1) v = a.last[r];
    } else if (s < C) {
      if (t < T) v = a.greedy[(long)t * a.ldg + b];
    } else if (s - C < nref && t < Lr) {
      v = a.refs[((long)b * M + (s - C)) * Lr + t];
    }
    tok[s * RW_LDT + t] = v;
  }
  if (tid < S) tok[tid * RW_LDT + RW_MAXL] = 0;
  if (tid < RW_MAXO) tok[S * RW_LDT + tid] = 0;
  __syncthreads();
  if (tid < S) {
    const int* h = tok + tid * RW_LDT;
    const int L = tid < C ? T : Lr;
    int n = 0;
    while (n < L && h[n] != 0 && !(a.end_id >= 0 && h[n] == a.end_id)) ++n;
    len[tid] = n;
    if (tid < K) a.counted[(long)b * K + tid] = min(n + 1, T);
  }
  __syncthreads();

  // ---- 1. per (row, position): the gram's count in the row at its first position, per order; kind 0: its table index
  for (int x = tid; x < S * Lm; x += RW_THREADS) {
    const int s = x / Lm, p = x - s * Lm;
    const int n = len[s];
    if (p >= n) continue;
    const int* h = tok + s * RW_LDT;
    const int kmax = min(RW_MAXO, n - p);
    const int g0 = h[p], g1 = h[p + 1], g2 = h[p + 2], g3 = h[p + 3];
    unsigned cnt = 0, seen = 0;                         // cnt: a byte per order; seen: bit k-1, the k-gram occurs before p
    int x0 = h[0], x1 = h[1], x2 = h[2], x3 = h[3];     // the window slides: one LDS read per position
    for (int q = 0; q < n; ++q) {
      const int m = rw_prefix(x0, x1, x2, x3, g0, g1, g2, g3, min(kmax, n - q));        // q == p: kmax
      if (q < p) seen |= (1u << m) - 1u;
      else cnt += rw_ones(m);
      x0 = x1; x1 = x2; x2 = x3; x3 = h[q + 4];
    }
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < RW_MAXO; ++k)
      if (!((seen >> k) & 1u)) w |= cnt & (0xffu << (8 * k));
    hc[s * RW_LDT + p] = w;
    if (a.kind == 0) {
      const int g[RW_MAXO] = {g0, g1, g2, g3};
      unsigned long long key[RW_MAXO], acc = 0;
      bool want[RW_MAXO], ok = true;                    // ok: every word of the gram so far is a table word, 1 .. 65535
#pragma unroll
      for (int k = 0; k < RW_MAXO; ++k) {
        ok = ok && k < kmax && g[k] >= 1 && g[k] <= 65535;
        acc |= (unsigned long long)(unsigned)(g[k] & 0xffff) << (16 * k);
        key[k] = acc;
        want[k] = ok && rw_byte(w, k) != 0;             // looked up once, at the gram's first position
      }
      int f[RW_MAXO];
      rw_find4(a.keys, a.n_keys, key, want, f);
#pragma unroll
      for (int k = 0; k < RW_MAXO; ++k) idv[(s * RW_MAXL + p) * RW_MAXO + k] = f[k] < 0 ? logn : a.idf[f[k]];
    }
  }
  __syncthreads();

  if (a.kind == 0) {
    const double sigma = a.params[1];
    // ---- 2a. the squared norm of every row's tf-idf vector, per order
    if (tid < S * RW_MAXO) {
      const int s = tid >> 2, k = tid & 3;
      const int n = len[s];
      double sq = 0.0;
      for (int p = 0; p < n; ++p) {
        const int tf = rw_byte(hc[s * RW_LDT + p], k);
        if (tf == 0) continue;
        const double v = (double)tf * idv[(s * RW_MAXL + p) * RW_MAXO + k];
        sq += v * v;
      }
      norm[tid] = sq;
    }
    __syncthreads();
    // ---- 2b. the pairs (candidate, reference)
    for (int x = tid; x < C * nref; x += RW_THREADS) {
      const int c = x / nref, j = x - c * nref;
      const int nh = len[c], nr = len[C + j];
      const int* h = tok + c * RW_LDT;
      const int* r = tok + (C + j) * RW_LDT;
      double num[RW_MAXO] = {0.0, 0.0, 0.0, 0.0};
      for (int p = 0; p < nh; ++p) {
        const unsigned w = hc[c * RW_LDT + p];
        if (w == 0) continue;                           // every gram at p occurred before
        const unsigned cnt = rw_count(r, nr, h[p], h[p + 1], h[p + 2], h[p + 3], min(RW_MAXO, nh - p));
#pragma unroll
        for (int k = 0; k < RW_MAXO; ++k) {
          const int tfc = rw_byte(w, k), tfj = rw_byte(cnt, k);
          if (tfc == 0 || tfj == 0) continue;
          const double i = idv[(c * RW_MAXL + p) * RW_MAXO + k];
          const double vc = (double)tfc * i, vr = (double)tfj * i;
          num[k] += fmin(vc, vr) * vr;
        }
      }
      const double d = (double)(nh - nr);
      const double pen = exp(-(d * d) / (2.0 * sigma * sigma));
      double total = 0.0;
#pragma unroll
      for (int k = 0; k < RW_MAXO; ++k) {
        const double den = norm[c * RW_MAXO + k] * norm[(C + j) * RW_MAXO + k];
        total += (den != 0.0 ? num[k] / sqrt(den) : 0.0) * pen;
      }
      sim[c * RW_MAXM + j] = total / (double)RW_MAXO;
    }
    __syncthreads();
    // ---- 3. the mean over the references, times 10
    if (tid < C) {
      double s = 0.0;
      for (int j = 0; j < nref; ++j) s += sim[tid * RW_MAXM + j];
      sc[tid] = nref > 0 ? 10.0 * s / (double)nref : 0.0;
    }
  } else {
    // ---- 2. the triples (candidate, position, reference): the grams' counts in the reference
    for (int x = tid; x < C * T * nref; x += RW_THREADS) {
      const int c = x / (T * nref), y = x - c * (T * nref), p = y / nref, j = y - p * nref;
      const int nh = len[c];
      unsigned cnt = 0;
      if (p < nh) {
        const unsigned w = hc[c * RW_LDT + p];
        if (w != 0) {
          const int* h = tok + c * RW_LDT;
          cnt = rw_count(tok + (C + j) * RW_LDT, len[C + j], h[p], h[p + 1], h[p + 2], h[p + 3], min(RW_MAXO, nh - p));
        }
      }
      wk[(c * RW_MAXL + p) * RW_MAXM + j] = (int)cnt;
    }
    __syncthreads();
    // ---- 3. clipped precisions, brevity penalty, the score
    if (tid < C) {
      const int nh = len[tid];
      int clip[RW_MAXO] = {0, 0, 0, 0};
      for (int p = 0; p < nh; ++p) {
        const unsigned w = hc[tid * RW_LDT + p];
        if (w == 0) continue;
        int mx[RW_MAXO] = {0, 0, 0, 0};
        for (int j = 0; j < nref; ++j) {
          const unsigned cnt = (unsigned)wk[(tid * RW_MAXL + p) * RW_MAXM + j];
#pragma unroll
          for (int k = 0; k < RW_MAXO; ++k) mx[k] = max(mx[k], rw_byte(cnt, k));
        }
#pragma unroll
        for (int k = 0; k < RW_MAXO; ++k) clip[k] += min(rw_byte(w, k), mx[k]);
      }
      double u = 0.0;
      if (nref > 0 && nh > 0 && clip[0] > 0) {
        int rl = 0, best = 0x7fffffff;                  // the closest reference length, the shorter on a tie
        for (int j = 0; j < nref; ++j) {
          const int l = len[C + j], d = abs(l - nh);
          if (d < best || (d == best && l < rl)) { best = d; rl = l; }
        }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < RW_MAXO; ++k) {
          const double nk = clip[k] > 0 ? (double)clip[k] : RW_EPS;
          s += 0.25 * log(nk / (double)max(1, nh - k));
        }
        const double bp = nh > rl ? 1.0 : exp(1.0 - (double)rl / (double)nh);
        u = bp * exp(s);
      }
      sc[tid] = u;
    }
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

bool rw_overlap(const void* p, uintptr_t np, const void* q, uintptr_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p != nullptr && q != nullptr && a < b + nq && b < a + np;
}

}  // namespace

extern "C" int32_t tnt_caption_reward_f32(const int32_t* fed, int32_t T, const int32_t* last, const int32_t* greedy,
                                          int32_t ldg, const int32_t* refs, const int32_t* n_refs, int32_t M, int32_t Lr,
                                          const uint64_t* keys, const double* idf, int32_t n_keys, const double* params,
                                          int32_t B, int32_t K, int32_t end_id, int32_t kind, int32_t baseline,
                                          float* adv, double* score, int32_t* counted, void* stream) {
  if (!fed) return TNT_BADARG(0);
  if (T < 1 || T > RW_MAXL) return TNT_BADARG(1);
  if (!last) return TNT_BADARG(2);
  if (B <= 0) return TNT_BADARG(13);
  if (K < 1 || K > RW_MAXK) return TNT_BADARG(14);
  if (kind != 0 && kind != 1) return TNT_BADARG(16);
  if (baseline != 0 && baseline != 1) return TNT_BADARG(17);
  if (baseline == 0 && !greedy) return TNT_BADARG(3);
  if (baseline == 0 && ldg < B) return TNT_BADARG(4);
  if (baseline == 1 && K < 2) return TNT_BADARG(14);
  if (!refs) return TNT_BADARG(5);
  if (!n_refs) return TNT_BADARG(6);
  if (M < 1 || M > RW_MAXM) return TNT_BADARG(7);
  if (Lr < 1 || Lr > RW_MAXL) return TNT_BADARG(8);
  if (n_keys < 0) return TNT_BADARG(11);
  if (kind == 0 && n_keys > 0 && !keys) return TNT_BADARG(9);
  if (kind == 0 && n_keys > 0 && !idf) return TNT_BADARG(10);
  if (kind == 0 && !params) return TNT_BADARG(12);
  if (!adv) return TNT_BADARG(18);
  if (!counted) return TNT_BADARG(20);
  {                                                    // the inputs are read while the outputs are written
    const uintptr_t uB = (uintptr_t)B, R = uB * (uintptr_t)K, i4 = sizeof(int32_t);
    const bool tab = kind == 0 && n_keys > 0;
    const void* in[8] = {fed, last, baseline == 0 ? greedy : nullptr, refs, n_refs, tab ? keys : nullptr,
                         tab ? idf : nullptr, kind == 0 ? params : nullptr};
    const uintptr_t nin[8] = {R * (uintptr_t)T * i4, R * i4, (((uintptr_t)T - 1) * (uintptr_t)(ldg > 0 ? ldg : 0) + uB) * i4,
                              uB * (uintptr_t)M * (uintptr_t)Lr * i4, uB * i4, (uintptr_t)n_keys * sizeof(uint64_t),
                              (uintptr_t)n_keys * sizeof(double), 2 * sizeof(double)};
    const void* out[3] = {adv, score, counted};
    const uintptr_t nout[3] = {R * sizeof(float), uB * (uintptr_t)(K + 1) * sizeof(double), R * i4};
    const int code[3] = {18, 19, 20};
    for (int o = 0; o < 3; ++o) {
      for (int i = 0; i < 8; ++i)
        if (rw_overlap(in[i], nin[i], out[o], nout[o])) return TNT_BADARG(code[o]);
      for (int p = 0; p < o; ++p)
        if (rw_overlap(out[p], nout[p], out[o], nout[o])) return TNT_BADARG(code[o]);
    }
  }
  RewardArgs a;
  a.fed = fed; a.last = last; a.greedy = baseline == 0 ? greedy : nullptr; a.refs = refs; a.n_refs = n_refs;
  a.keys = reinterpret_cast<const unsigned long long*>(keys); a.idf = idf; a.params = params;
  a.T = T; a.ldg = ldg; a.M = M; a.Lr = Lr; a.n_keys = kind == 0 ? n_keys : 0; a.B = B; a.K = K; a.end_id = end_id;
  a.kind = kind; a.baseline = baseline;
  a.adv = adv; a.score = score; a.counted = counted;
  hipLaunchKernelGGL(caption_reward_kernel, dim3(B), dim3(RW_THREADS), 0, tnt_stream(stream), a);
  TNT_LAUNCH_CHECK();
  return 0;
}
