// Scoring of generated token sequences: the two integer kernels behind fairseq-generate's closing
// line (fairseq scoring/bleu.py over libbleu's bleu_add, scoring/wer.py) and behind the reference's
// scripts/wer.py.  A batch is n_pairs right-padded int32 rows ref [n_pairs][ld_ref], pred [n_pairs][ld_pred]
// with int32 lengths per row; every pair is independent: one block per pair, everything in LDS.
//
//   ngram_stats    libbleu's bleu_add.  The reference's unk becomes -999, both sequences are trimmed
//                  (right: eos / pad down to one token; then left: pad).  n-grams are compared by exact
//                  token equality, without libbleu's FNV hash: the ref_len + pred_len tokens are sorted
//                  once (64-bit keys: token above position) and a token's rank is the sorted index of its
//                  value's first occurrence, < 8192, 13 bits.  An n-gram (n <= 4) is then the 52-bit
//                  concatenation of its tokens' ranks, equal exactly when the tokens are.  Per n one
//                  bitonic sort of (code << 1 | side) over both sequences' n-grams puts every distinct
//                  n-gram in one run, the reference's occurrences first; the thread at the head of a run
//                  finds both counts by two binary searches and adds min(c_ref, c_pred).  The cost per
//                  pair is O(L log^2 L), not O(L^2).
//   edit_distance  unit-cost Levenshtein over exactly the given lengths, by anti-diagonals: cell (i, j)
//                  of diagonal k = i + j reads diagonals k - 1 and k - 2, kept in three rotating LDS
//                  rows indexed by i; one barrier per diagonal.
//
// Integers only; the only atomics are integer adds (LDS, and one per pair and counter into the
// persistent int64 device totals), so every run gives the same bits.
#include "common.h"
#include "../../include/mms2ut.h"

namespace {

constexpr int SC_MAX_LEN = MMS_SCORE_MAX_LEN;
constexpr int SC_MAX_KEYS = 2 * SC_MAX_LEN;               // both sequences' tokens / n-grams in one sort
constexpr int SC_RANK_BITS = 13;
constexpr int SC_HDR = 16;                                // ints of per-block scalars in front of the arrays
constexpr int SC_UNK_REPLACED = -999;                     // fairseq scoring/bleu.py Scorer.add
static_assert((1 << SC_RANK_BITS) == SC_MAX_KEYS && 4 * SC_RANK_BITS + 1 <= 64, "rank width");
typedef unsigned long long u64k;

inline int pow2_at_least(int n, int lo) {
  int p = lo;
  while (p < n) p <<= 1;
  return p;
}

// ascending bitonic sort of keys[0 .. N), N a power of two >= 2; block-uniform call
template <int THREADS>
MMS_DEV void sc_sort(u64k* keys, int N, int tid) {
  for (int size = 2; size <= N; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = tid; p < (N >> 1); p += THREADS) {
        const int i = 2 * p - (p & (stride - 1)), j = i + stride;
        const u64k a = keys[i], c = keys[j];
        if ((a > c) == ((i & size) == 0)) {
          keys[i] = c;
          keys[j] = a;
        }
      }
      __syncthreads();
    }
}

// first index in sorted keys[0 .. n) whose key is >= target (n where none is)
MMS_DEV int sc_lower_bound(const u64k* keys, int n, u64k target) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

MMS_DEV int sc_clamp_len(const int* lens, int b, int ld) { return min(max(lens[b], 0), ld); }

// LDS: keys [cap] u64 | hdr [SC_HDR] int | rk [cap] u16.  cap = a power of two >= ld_ref + ld_pred.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) ngram_stats_kernel(
    const int* __restrict__ ref, long ld_ref, const int* __restrict__ ref_len, const int* __restrict__ pred,
    long ld_pred, const int* __restrict__ pred_len, int pad, int eos, int unk, int cap, u64k* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
  u64k* keys = reinterpret_cast<u64k*>(sc_smem);
  int* hdr = reinterpret_cast<int*>(sc_smem + (size_t)cap * sizeof(u64k));
  unsigned short* rk = reinterpret_cast<unsigned short*>(hdr + SC_HDR);
  const int tid = threadIdx.x, b = blockIdx.x;
  const int* r = ref + (long)b * ld_ref;
  const int* p = pred + (long)b * ld_pred;
  const int rl0 = sc_clamp_len(ref_len, b, (int)ld_ref), pl0 = sc_clamp_len(pred_len, b, (int)ld_pred);
  const bool has_unk = unk >= 0;
  auto rtok = [&](int i) {
    const int t = r[i];
    return (has_unk && t == unk) ? SC_UNK_REPLACED : t;
  };
  // hdr: 0 / 2 last kept index of the right trim (ref / pred), 1 / 3 first non-pad index, 4 .. 7 match_n
  if (tid < SC_HDR) hdr[tid] = (tid == 1 || tid == 3) ? 0x7fffffff : 0;
  __syncthreads();
  {
    int mr = 0, mp = 0;
    for (int i = 1 + tid; i < rl0; i += THREADS) {
      const int t = rtok(i);
      if (t != eos && t != pad) mr = i;
    }
    for (int i = 1 + tid; i < pl0; i += THREADS) {
      const int t = p[i];
      if (t != eos && t != pad) mp = i;
    }
    if (mr > 0) atomicMax(&hdr[0], mr);
    if (mp > 0) atomicMax(&hdr[2], mp);
  }
  __syncthreads();
  const int rl1 = rl0 > 0 ? hdr[0] + 1 : 0, pl1 = pl0 > 0 ? hdr[2] + 1 : 0;
  {
    int fr = 0x7fffffff, fp = 0x7fffffff;
    for (int i = tid; i < rl1; i += THREADS)
      if (rtok(i) != pad) {
        fr = i;
        break;
      }
    for (int i = tid; i < pl1; i += THREADS)
      if (p[i] != pad) {
        fp = i;
        break;
      }
    if (fr < rl1) atomicMin(&hdr[1], fr);
    if (fp < pl1) atomicMin(&hdr[3], fp);
  }
  __syncthreads();
  const int r0 = min(hdr[1], rl1), p0 = min(hdr[3], pl1);
  const int rlen = rl1 - r0, plen = pl1 - p0;             // the trimmed sequences: r[r0 ..], p[p0 ..]
  const int M = rlen + plen;                              // <= cap

  if (rlen > 0 && plen > 0) {
    // token ranks: sort (token, position), rank = the sorted index of the value's first occurrence
    const int N = max(2, 1 << (32 - __clz(max(M - 1, 1))));
    for (int c = tid; c < N; c += THREADS) {
      u64k key = ~0ull;                                   // padding sorts last (a position is never 2^32 - 1)
      if (c < M) {
        const int t = c < rlen ? rtok(r0 + c) : p[p0 + c - rlen];
        key = ((u64k)((unsigned)t ^ 0x80000000u) << 32) | (unsigned)c;
      }
      keys[c] = key;
    }
    __syncthreads();
    sc_sort<THREADS>(keys, N, tid);
    for (int i = tid; i < M; i += THREADS) {
      const u64k key = keys[i];
      rk[(unsigned)key] = (unsigned short)sc_lower_bound(keys, i + 1, key & 0xffffffff00000000ull);
    }
    __syncthreads();
    for (int n = 1; n <= 4; ++n) {
      const int cr = rlen - n + 1, cp = plen - n + 1;
      if (cr <= 0 || cp <= 0) break;                      // block-uniform
      const int M2 = cr + cp;
      const int N2 = max(2, 1 << (32 - __clz(max(M2 - 1, 1))));
      for (int c = tid; c < N2; c += THREADS) {
        u64k key = ~0ull;
        if (c < M2) {
          const int side = c < cr ? 0 : 1;
          const int at = side ? rlen + (c - cr) : c;      // the n-gram's first token in rk
          u64k code = 0;
          for (int k = 0; k < n; ++k) code = (code << SC_RANK_BITS) | rk[at + k];
          key = (code << 1) | (u64k)side;
        }
        keys[c] = key;
      }
      __syncthreads();
      sc_sort<THREADS>(keys, N2, tid);
      int m = 0;
      for (int i = tid; i < M2; i += THREADS) {
        const u64k key = keys[i];
        if ((key & 1) || (i > 0 && (keys[i - 1] >> 1) == (key >> 1))) continue;   // not the head of a run with a ref
        const u64k code = key >> 1;
        const int a = sc_lower_bound(keys, M2, (code << 1) | 1), e = sc_lower_bound(keys, M2, (code + 1) << 1);
        m += min(a - i, e - a);
      }
      if (m > 0) atomicAdd(&hdr[3 + n], m);
      __syncthreads();                                    // the searches are done before the next fill
    }
  }
  if (tid == 0) {
    if (rlen > 0) atomicAdd(&stats[0], (u64k)rlen);
    if (plen > 0) atomicAdd(&stats[1], (u64k)plen);
    for (int n = 1; n <= 4; ++n) {
      if (hdr[3 + n] > 0) atomicAdd(&stats[2 * n], (u64k)hdr[3 + n]);
      if (plen >= n) atomicAdd(&stats[2 * n + 1], (u64k)(plen - n + 1));
    }
  }
}

// LDS: a [cap_r] ref tokens | bt [cap_p] pred tokens | 3 x d [cap_r + 4] diagonals (cap_*: multiples of 4)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) edit_distance_kernel(
    const int* __restrict__ ref, long ld_ref, const int* __restrict__ ref_len, const int* __restrict__ pred,
    long ld_pred, const int* __restrict__ pred_len, int unk, int cap_r, int cap_p, int* __restrict__ dist,
    u64k* __restrict__ totals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
  int* a = reinterpret_cast<int*>(sc_smem);
  int* bt = a + cap_r;
  int* d = bt + cap_p;
  const int dstride = cap_r + 4;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int m = sc_clamp_len(ref_len, b, (int)ld_ref), n = sc_clamp_len(pred_len, b, (int)ld_pred);
  int res = m + n;                                        // one side empty: all insertions or deletions
  if (m > 0 && n > 0) {                                   // block-uniform
    const int* r = ref + (long)b * ld_ref;
    const int* p = pred + (long)b * ld_pred;
    for (int i = tid; i < m; i += THREADS) {
      const int t = r[i];
      a[i] = (unk >= 0 && t == unk) ? SC_UNK_REPLACED : t;
    }
    for (int j = tid; j < n; j += THREADS) bt[j] = p[j];
    __syncthreads();
    int *p2 = d, *p1 = d + dstride, *cur = d + 2 * dstride;
    for (int k = 0; k <= m + n; ++k) {
      const int ilo = max(0, k - n), ihi = min(m, k);
      for (int i = ilo + tid; i <= ihi; i += THREADS) {
        const int j = k - i;
        int v;
        if (i == 0) v = j;
        else if (j == 0) v = i;
        else v = min(min(p1[i - 1], p1[i]) + 1, p2[i - 1] + (a[i - 1] != bt[j - 1] ? 1 : 0));
        cur[i] = v;
      }
      __syncthreads();
      int* t = p2;
      p2 = p1;
      p1 = cur;
      cur = t;
    }
    res = p1[m];                                          // diagonal m + n holds the one cell (m, n)
  }
  if (tid == 0) {
    if (dist) dist[b] = res;
    if (res > 0) atomicAdd(&totals[0], (u64k)res);
    if (m > 0) atomicAdd(&totals[1], (u64k)m);
  }
}

// more than 64 KiB of dynamic LDS needs the attribute (a property of the current device's copy of the kernel)
constexpr int SC_MAX_LDS = 96 * 1024;                     // both kernels need 82 KiB at the length limit
template <typename K>
int sc_allow_lds(K kernel, size_t bytes, const char* what) {
  MMS_REQUIRE(bytes <= (size_t)SC_MAX_LDS, "%s: %zu bytes of LDS", what, bytes);
  if (bytes <= 64 * 1024) return 0;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, SC_MAX_LDS);
  MMS_REQUIRE(e == hipSuccess, "%s: cannot raise the dynamic LDS limit: %s", what, hipGetErrorString(e));
  return 0;
}

int sc_check(const char* what, const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, const int32_t* pred,
             int64_t ld_pred, const int32_t* pred_len, int n_pairs, const void* out) {
  MMS_REQUIRE(n_pairs >= 0, "%s: n_pairs %d", what, n_pairs);
  MMS_REQUIRE(ld_ref >= 0 && ld_pred >= 0, "%s: row strides %lld, %lld", what, (long long)ld_ref, (long long)ld_pred);
  MMS_REQUIRE(ld_ref <= SC_MAX_LEN && ld_pred <= SC_MAX_LEN,
              "%s: sequences of up to %lld (ref) and %lld (pred) tokens exceed the limit of %d tokens per sequence",
              what, (long long)ld_ref, (long long)ld_pred, SC_MAX_LEN);
  if (n_pairs == 0) return 0;
  MMS_REQUIRE(ref_len && pred_len && out, "%s: null buffer", what);
  MMS_REQUIRE((ref || ld_ref == 0) && (pred || ld_pred == 0), "%s: null sequences", what);
  MMS_REQUIRE(((uintptr_t)out & 7) == 0, "%s: misaligned int64 totals", what);
  return 0;
}

}  // namespace

extern "C" int mms2ut_ngram_stats(const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, const int32_t* pred,
                                  int64_t ld_pred, const int32_t* pred_len, int n_pairs, int pad, int eos, int unk,
                                  int64_t* stats, hipStream_t s) {
  if (sc_check("ngram_stats", ref, ld_ref, ref_len, pred, ld_pred, pred_len, n_pairs, stats)) return 1;
  if (n_pairs == 0) return 0;
  const int cap = pow2_at_least((int)(ld_ref + ld_pred), 64);
  const size_t lds = (size_t)cap * sizeof(u64k) + SC_HDR * sizeof(int) + (size_t)cap * sizeof(unsigned short);
  u64k* st = reinterpret_cast<u64k*>(stats);
  if (cap <= 1024) {                                      // short pairs: small blocks, many per CU
    hipLaunchKernelGGL(ngram_stats_kernel<256>, dim3(n_pairs), dim3(256), lds, s, ref, (long)ld_ref, ref_len, pred,
                       (long)ld_pred, pred_len, pad, eos, unk, cap, st);
  } else {
    if (sc_allow_lds(ngram_stats_kernel<1024>, lds, "ngram_stats")) return 1;
    hipLaunchKernelGGL(ngram_stats_kernel<1024>, dim3(n_pairs), dim3(1024), lds, s, ref, (long)ld_ref, ref_len, pred,
                       (long)ld_pred, pred_len, pad, eos, unk, cap, st);
  }
  return mms::check_launch("ngram_stats");
}

extern "C" int mms2ut_edit_distance(const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, const int32_t* pred,
                                    int64_t ld_pred, const int32_t* pred_len, int n_pairs, int unk, int32_t* dist,
                                    int64_t* totals, hipStream_t s) {
  if (sc_check("edit_distance", ref, ld_ref, ref_len, pred, ld_pred, pred_len, n_pairs, totals)) return 1;
  if (n_pairs == 0) return 0;
  const int cap_r = ((int)ld_ref + 3) & ~3, cap_p = ((int)ld_pred + 3) & ~3;
  const size_t lds = ((size_t)cap_r + cap_p + 3 * (size_t)(cap_r + 4)) * sizeof(int);
  u64k* tot = reinterpret_cast<u64k*>(totals);
  if (ld_ref <= 512) {                                    // a diagonal has at most ld_ref + 1 cells
    hipLaunchKernelGGL(edit_distance_kernel<256>, dim3(n_pairs), dim3(256), lds, s, ref, (long)ld_ref, ref_len, pred,
                       (long)ld_pred, pred_len, unk, cap_r, cap_p, dist, tot);
  } else {
    if (sc_allow_lds(edit_distance_kernel<1024>, lds, "edit_distance")) return 1;
    hipLaunchKernelGGL(edit_distance_kernel<1024>, dim3(n_pairs), dim3(1024), lds, s, ref, (long)ld_ref, ref_len, pred,
                       (long)ld_pred, pred_len, unk, cap_r, cap_p, dist, tot);
  }
  return mms::check_launch("edit_distance");
}
