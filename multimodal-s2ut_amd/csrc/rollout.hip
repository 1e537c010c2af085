// Attention rollout of a ViT (Abnar & Zuidema 2020, as the reference's vit_rollout.py computes it): the
// map of the image regions the class token draws on.  Three kernels, every stored value fp32 past the scores:
//
//   rollout_probs    head-fused attention probabilities of one layer from the packed fp16 q|k|v that
//                    mha_fwd reads.  A block of 4 waves owns 16 query rows and all T key columns: wave w
//                    holds the 16-column tiles w, w + 4, ... as MFMA accumulators (v_mfma_f32_16x16x32_f16,
//                    D[row][col], lane l owning column l & 15 and rows 4 (l >> 4) + r), so a row's
//                    softmax statistics are a 16-lane DPP reduction plus four values through LDS, summed in
//                    wave order.  Per head: S = Q K^T * scale, a full-row softmax, and the fold into the
//                    running mean / max / min in registers; heads run 0 .. H - 1, the mean multiplies by
//                    1 / H at the end.  No [H, T, T] tensor, no atomics: every run gives the same bits.
//   rollout_discard  zeroes the k smallest entries of each [T, T] matrix, never flat index 0.  The inputs
//                    are non-negative, so the bit pattern orders them: a 4-pass, 8-bit radix select on
//                    32-bit LDS counters finds the k-th smallest pattern and how many of its equals to
//                    take; those are taken in flat-index order (an ordered block scan, run only when not
//                    all equals go).  Integer work only; a NaN or a negative pattern is just a large key.
//   rollout_chain    per image, fp32 in and out, the sums in between carried in double: a_l = (F_l + I) / 2,
//                    its row sums s (fixed order; one launch over every row of every matrix), a_l[i][j] /=
//                    s[j] (the reference's a / a.sum(-1), which divides column j by row j's sum) or /= s[i]
//                    (normalization = row), then row 0 of a_L ... a_1 as a row vector times a matrix, from
//                    a_L down, one block per image, and mask = R[0, 1:] / max.  An empty or non-finite
//                    result sets the image's flag and writes zeros.
#include <math.h>

#include "common.h"
#include "../../include/mms2ut.h"

namespace {

constexpr int RP_WAVES = 4;
constexpr int RP_TILES = (MMS_ROLLOUT_MAX_T + 16 * RP_WAVES - 1) / (16 * RP_WAVES);   // column tiles per wave
constexpr int RD_THREADS = 1024, RC_THREADS = 1024, RC_WAVES = RC_THREADS / 64, RS_WAVES = 4;

template <int MODE>
MMS_DEV float fold(float f, float p, bool first) {
  if (MODE == MMS_ROLLOUT_MEAN) return f + p;          // f starts at 0
  if (first) return p;
  return MODE == MMS_ROLLOUT_MAX ? fmaxf(f, p) : fminf(f, p);
}

template <int HD, int MODE>
__global__ void __launch_bounds__(RP_WAVES * 64)
rollout_probs_kernel(const h16* __restrict__ q, const h16* __restrict__ k, long ldq, long ldk, int H, int T, float scale,
                     float* __restrict__ out, long out_batch) {
  __shared__ float red_max[RP_WAVES][16], red_sum[RP_WAVES][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, r0 = blockIdx.x * 16;
  const int ntile = (T + 15) / 16;
  // rows past T read row T - 1 (in bounds) and are not stored; key columns past T are masked below
  const h16* qrow = q + ((long)b * T + min(r0 + l15, T - 1)) * ldq + 8 * g;
  const h16* kbase = k + (long)b * T * ldk + 8 * g;
  float f[RP_TILES][4];
#pragma unroll
  for (int t = 0; t < RP_TILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) f[t][r] = 0.f;

  for (int h = 0; h < H; ++h) {
    h16x8 qf[HD / 32];
#pragma unroll
    for (int s = 0; s < HD / 32; ++s) qf[s] = *reinterpret_cast<const h16x8*>(qrow + h * HD + 32 * s);
    float sc[RP_TILES][4];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < RP_TILES; ++t) {
      const int ct = w + RP_WAVES * t;
      if (ct < ntile) {                                  // wave-uniform
        const int col = ct * 16 + l15;
        const h16* krow = kbase + (long)min(col, T - 1) * ldk + h * HD;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < HD / 32; ++s)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[s], *reinterpret_cast<const h16x8*>(krow + 32 * s), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc[t][r] = col < T ? acc[r] * scale : -INFINITY;
          mx[r] = fmaxf(mx[r], sc[t][r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] = -INFINITY;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = row16_max(mx[r]);
    if (l15 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red_max[w][4 * g + r] = mx[r];
    }
    __syncthreads();
    float sm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = red_max[0][4 * g + r];
#pragma unroll
      for (int u = 1; u < RP_WAVES; ++u) m = fmaxf(m, red_max[u][4 * g + r]);
      mx[r] = m;                                         // finite: column 0 is a key of every row
      sm[r] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < RP_TILES; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[t][r] = __expf(sc[t][r] - mx[r]);             // exp(-inf) = 0 in the masked columns
        sm[r] += sc[t][r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) sm[r] = row16_sum(sm[r]);
    if (l15 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red_sum[w][4 * g + r] = sm[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = red_sum[0][4 * g + r];
#pragma unroll
      for (int u = 1; u < RP_WAVES; ++u) s += red_sum[u][4 * g + r];
      sm[r] = s;
    }
#pragma unroll
    for (int t = 0; t < RP_TILES; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) f[t][r] = fold<MODE>(f[t][r], sc[t][r] / sm[r], h == 0);
  }

  const float inv = 1.f / (float)H;
  float* o = out + (long)b * out_batch;
#pragma unroll
  for (int t = 0; t < RP_TILES; ++t) {
    const int col = (w + RP_WAVES * t) * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * g + r;
      if (row < T && col < T) o[(long)row * T + col] = MODE == MMS_ROLLOUT_MEAN ? f[t][r] * inv : f[t][r];
    }
  }
}

template <int HD>
void launch_probs(int mode, dim3 grid, hipStream_t s, const h16* q, const h16* k, long ldq, long ldk, int H, int T,
                  float scale, float* out, long out_batch) {
  const dim3 blk(RP_WAVES * 64);
  if (mode == MMS_ROLLOUT_MEAN)
    hipLaunchKernelGGL((rollout_probs_kernel<HD, MMS_ROLLOUT_MEAN>), grid, blk, 0, s, q, k, ldq, ldk, H, T, scale, out, out_batch);
  else if (mode == MMS_ROLLOUT_MAX)
    hipLaunchKernelGGL((rollout_probs_kernel<HD, MMS_ROLLOUT_MAX>), grid, blk, 0, s, q, k, ldq, ldk, H, T, scale, out, out_batch);
  else
    hipLaunchKernelGGL((rollout_probs_kernel<HD, MMS_ROLLOUT_MIN>), grid, blk, 0, s, q, k, ldq, ldk, H, T, scale, out, out_batch);
}

// ------------------------------------------------------------------------------------------ discard

__global__ void __launch_bounds__(RD_THREADS) rollout_discard_kernel(float* __restrict__ x, int n, int k) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_rem, s_cnt;
  __shared__ unsigned wtot[RD_THREADS / 64];
  unsigned* p = reinterpret_cast<unsigned*>(x) + (long)blockIdx.x * n;
  const int tid = threadIdx.x;
  if (k >= n) {                                          // everything goes, but flat index 0
    for (int i = 1 + tid; i < n; i += RD_THREADS) p[i] = 0u;
    return;
  }
  // the k-th smallest pattern, a digit of 8 bits per pass from the top: prefix = the digits found so far,
  // rem = its rank (1-based) among the entries that share them
  unsigned prefix = 0u, rem = (unsigned)k, cnt = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += RD_THREADS) {
      const unsigned key = p[i];
      if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0u, bin = 255u, c = hist[255];
      for (unsigned d = 0; d < 256u; ++d) {
        const unsigned hd = hist[d];
        if (cum + hd >= rem) { bin = d; c = hd; break; }
        cum += hd;
      }
      s_prefix = prefix | (bin << shift);
      s_rem = rem - cum;
      s_cnt = c;
    }
    __syncthreads();
    prefix = s_prefix, rem = s_rem, cnt = s_cnt;
  }
  // entries below the pattern go; of its cnt equals, the first rem in flat-index order
  if (rem >= cnt) {
    for (int i = tid; i < n; i += RD_THREADS)
      if (i != 0 && p[i] <= prefix) p[i] = 0u;
    return;
  }
  const int lane = tid & 63, w = tid >> 6;
  unsigned base = 0u;
  for (int c0 = 0; c0 < n; c0 += RD_THREADS) {           // block-uniform trip count
    const int i = c0 + tid;
    const unsigned key = i < n ? p[i] : 0xffffffffu;
    const bool eq = i < n && key == prefix;
    const unsigned long long bal = __ballot(eq);
    const unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned woff = 0u, total = 0u;
    for (int u = 0; u < RD_THREADS / 64; ++u) {
      const unsigned c = wtot[u];
      if (u < w) woff += c;
      total += c;
    }
    if (i < n && i != 0 && (key < prefix || (eq && base + woff + before < rem))) p[i] = 0u;
    base += total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ chain

// The matrices and the mask are fp32; the sums in between are carried in double.  An fp32 chain sat 3.1 x as
// far from float64 as torch's fp32 evaluation at T = 577 (2.0e-7 against 6.4e-8, both about an ulp of 1.0),
// past the tests' allowance of 3 x; in double only the final rounding is left, and the division by s moves
// out of the sum at no cost in accuracy.

// sums[row] = sum_j (a[row][j] + [i == j]) / 2 for every row of every matrix (row = (matrix, i)): one wave per
// row, a lane's columns in order, then the wave's fixed tree
__global__ void __launch_bounds__(RS_WAVES * 64)
rollout_rowsum_kernel(const float* __restrict__ a, long rows, int T, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                               // the whole wave leaves
  const int i = (int)(row % T);
  const float* r = a + row * T;
  double acc = 0.0;
  for (int j = lane; j < T; j += 64) acc += ((double)r[j] + (i == j ? 1.0 : 0.0)) * 0.5;
  acc = wave_sum_d(acc);
  if (lane == 0) sums[row] = acc;
}

__global__ void __launch_bounds__(RC_THREADS)
rollout_chain_kernel(const float* __restrict__ a, const double* __restrict__ sums, int L, int T, int row_norm,
                     float* __restrict__ mask, int* __restrict__ bad) {
  __shared__ double vbuf[2][MMS_ROLLOUT_MAX_T], u[MMS_ROLLOUT_MAX_T], part[RC_WAVES][64];
  __shared__ double s_max;
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* A = a + (long)blockIdx.x * L * T * T;
  const double* S = sums + (long)blockIdx.x * L * T;
  for (int j = tid; j < T; j += RC_THREADS) vbuf[0][j] = j == 0 ? 1.0 : 0.0;
  __syncthreads();
  int cur = 0;
  const int per = (T + RC_WAVES - 1) / RC_WAVES;         // rows of a wave's share of a product
  for (int l = L - 1; l >= 0; --l) {
    const float* M = A + (long)l * T * T;
    const double* s = S + (long)l * T;
    double* vn = vbuf[cur ^ 1];
    // v a_l [j] = (sum_i v_i e_ij) / s_j (reference) or sum_i (v_i / s_i) e_ij (row), e = (M + I) / 2
    for (int i = tid; i < T; i += RC_THREADS) u[i] = row_norm ? vbuf[cur][i] / s[i] : vbuf[cur][i];
    __syncthreads();
    const int i0 = w * per, i1 = min(i0 + per, T);
    for (int j0 = 0; j0 < T; j0 += 64) {
      const int j = j0 + lane;
      double acc = 0.0;
      if (j < T)
        for (int i = i0; i < i1; ++i) acc += u[i] * (((double)M[(long)i * T + j] + (i == j ? 1.0 : 0.0)) * 0.5);
      part[w][lane] = acc;
      __syncthreads();
      if (w == 0 && j < T) {
        double r = part[0][lane];
        for (int x = 1; x < RC_WAVES; ++x) r += part[x][lane];
        vn[j] = row_norm ? r : r / s[j];
      }
      __syncthreads();
    }
    cur ^= 1;
  }
  // mask = v[1:] / max(v[1:]); max <= 0 (nothing reaches a patch) or a non-finite entry: flag, zeros
  if (tid == 0) {
    double m = -INFINITY;
    int nf = 0;
    for (int j = 1; j < T; ++j) {
      const double x = vbuf[cur][j];
      nf |= !(fabs(x) <= 3.402823466e38);
      m = fmax(m, x);
    }
    s_max = m;
    s_bad = nf || !(m > 0.0);
    bad[blockIdx.x] = s_bad;
  }
  __syncthreads();
  const bool ok = !s_bad;
  const double m = s_max;
  for (int j = 1 + tid; j < T; j += RC_THREADS) mask[(long)blockIdx.x * (T - 1) + j - 1] = ok ? (float)(vbuf[cur][j] / m) : 0.f;
}

}  // namespace

extern "C" int mms2ut_rollout_probs_f16(const mms2ut_half* q, const mms2ut_half* k, int64_t ldq, int64_t ldk, int B, int H,
                                        int T, int hd, float scale, int fusion, float* out, int64_t out_batch,
                                        hipStream_t s) {
  MMS_REQUIRE(hd == 64 || hd == 96 || hd == 128, "rollout_probs: head dim %d is not supported (64, 96, 128)", hd);
  MMS_REQUIRE(T >= 1 && T <= MMS_ROLLOUT_MAX_T, "rollout_probs: T must be in [1, %d] (got %d)", MMS_ROLLOUT_MAX_T, T);
  MMS_REQUIRE(B >= 0 && B <= 65535 && H >= 1, "rollout_probs: B in [0, 65535] and H >= 1 required");
  MMS_REQUIRE(fusion == MMS_ROLLOUT_MEAN || fusion == MMS_ROLLOUT_MAX || fusion == MMS_ROLLOUT_MIN,
              "rollout_probs: fusion %d (0 mean, 1 max, 2 min)", fusion);
  MMS_REQUIRE(q && k && out, "rollout_probs: null buffer");
  MMS_REQUIRE(ldq >= (int64_t)H * hd && ldk >= (int64_t)H * hd && ldq % 8 == 0 && ldk % 8 == 0 &&
              ((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)out & 3) == 0,
              "rollout_probs: rows must be 16-byte aligned and hold H * hd columns");
  MMS_REQUIRE(out_batch >= (int64_t)T * T, "rollout_probs: out_batch %lld is below T * T", (long long)out_batch);
  if (B == 0) return 0;
  const dim3 grid((T + 15) / 16, B);
  const h16* qq = reinterpret_cast<const h16*>(q);
  const h16* kk = reinterpret_cast<const h16*>(k);
  if (hd == 64) launch_probs<64>(fusion, grid, s, qq, kk, ldq, ldk, H, T, scale, out, out_batch);
  else if (hd == 96) launch_probs<96>(fusion, grid, s, qq, kk, ldq, ldk, H, T, scale, out, out_batch);
  else launch_probs<128>(fusion, grid, s, qq, kk, ldq, ldk, H, T, scale, out, out_batch);
  return mms::check_launch("rollout_probs");
}

extern "C" int mms2ut_rollout_discard_f32(float* x, int nmat, int64_t n, int64_t k, hipStream_t s) {
  MMS_REQUIRE(nmat >= 0 && n >= 1 && n <= (int64_t)MMS_ROLLOUT_MAX_T * MMS_ROLLOUT_MAX_T,
              "rollout_discard: nmat >= 0 and n in [1, %d] required", MMS_ROLLOUT_MAX_T * MMS_ROLLOUT_MAX_T);
  MMS_REQUIRE(k >= 0 && k <= n, "rollout_discard: k must be in [0, n] (got %lld of %lld)", (long long)k, (long long)n);
  MMS_REQUIRE(x && ((uintptr_t)x & 3) == 0, "rollout_discard: null or misaligned buffer");
  if (nmat == 0 || k == 0) return 0;
  hipLaunchKernelGGL(rollout_discard_kernel, dim3(nmat), dim3(RD_THREADS), 0, s, x, (int)n, (int)k);
  return mms::check_launch("rollout_discard");
}

extern "C" int mms2ut_rollout_chain_f32(const float* a, int B, int L, int T, int normalization, double* sums, float* mask,
                                        int32_t* bad, hipStream_t s) {
  MMS_REQUIRE(T >= 2 && T <= MMS_ROLLOUT_MAX_T, "rollout_chain: T must be in [2, %d] (got %d)", MMS_ROLLOUT_MAX_T, T);
  MMS_REQUIRE(B >= 0 && L >= 1, "rollout_chain: B >= 0 and L >= 1 required");
  MMS_REQUIRE(normalization == MMS_ROLLOUT_NORM_REFERENCE || normalization == MMS_ROLLOUT_NORM_ROW,
              "rollout_chain: normalization %d (0 reference, 1 row)", normalization);
  MMS_REQUIRE(a && sums && mask && bad && ((uintptr_t)sums & 7) == 0, "rollout_chain: null or misaligned buffer");
  if (B == 0) return 0;
  const long rows = (long)B * L * T;
  MMS_REQUIRE((rows + RS_WAVES - 1) / RS_WAVES <= 0x7fffffffL, "rollout_chain: B * L * T = %ld rows are too many", rows);
  hipLaunchKernelGGL(rollout_rowsum_kernel, dim3((unsigned)((rows + RS_WAVES - 1) / RS_WAVES)), dim3(RS_WAVES * 64), 0, s, a,
                     rows, T, sums);
  hipLaunchKernelGGL(rollout_chain_kernel, dim3(B), dim3(RC_THREADS), 0, s, a, (const double*)sums, L, T,
                     normalization == MMS_ROLLOUT_NORM_ROW ? 1 : 0, mask, bad);
  return mms::check_launch("rollout_chain");
}
