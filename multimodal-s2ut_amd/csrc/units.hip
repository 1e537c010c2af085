// Speech-to-unit quantisation (forward only): the kernels of multimodal-s2ut_amd/units.py that the
// wav2vec2 path (asr.hip) does not have.  HuBERT's extractor layers 1.. and its positional
// convolution run on asr.hip's asr_conv, the post-LN layers on the GEMM / LayerNorm / attention
// kernels of the training path.
//
//   hubert_conv0       feature-extractor layer 0 of the group-norm family: Conv1d(1 -> C, k taps,
//                      stride s), GroupNorm with one group per channel (each channel's mean and biased
//                      variance over all T0 frames of the utterance), affine, GELU, fp16 [T0, C] out.
//                      The convolution is cheap (Cin = 1), so no fp32 [T0, C] image is kept: a
//                      statistics pass computes it and sums v and v^2 per channel in double
//                      over GN_PARTS slices of the frames, a fold adds the slices in slice order (no
//                      atomics: bitwise reproducible) and a second pass recomputes the convolution,
//                      normalises and stores.  The only rounding to fp16 is that store.
//   kmeans_assign      nearest centroid of fp16 rows X [R, d]: argmin_c |C_c|^2 - 2 x.C_c on
//                      v_mfma_f32_16x16x32_f16.  Each fp32 centroid enters as two fp16 images, hi =
//                      fp16(C) and lo = fp16((C - hi) * 2^11): x.hi and x.lo accumulate apart in fp32
//                      (fp16 products are exact there) and join as hi + lo * 2^-11, so the centroids
//                      carry 22 bits.  A block owns 64 rows (16 per wave) and one chunk of the
//                      centroid axis and keeps a running (min score, index) per row; the scores never
//                      reach memory.  Per chunk a (score, index) pair per row goes to a workspace.
//   kmeans_fold        one block per utterance: folds the chunk partials in chunk order (the lowest
//                      index wins a tie), writes the per-frame codes, compacts the run starts
//                      (ctc_greedy's scan without a blank) and flags a non-finite best score.
//   kmeans_topk        kmeans_assign's GEMM and score with the top_k <= 32 smallest (score, index) pairs per
//                      row kept in LDS, ordered by (score, index): the first pair is kmeans_assign's choice
//                      bit for bit.  Per chunk a list of top_k pairs per row goes to a workspace.
//   kmeans_topk_fold   one thread per frame: merges the chunks' lists and writes the indices and the
//                      Euclidean distances sqrt(max(|x|^2 + score, 0)), the input of units_beam.hip.
#include "common.h"
#include "../../include/mms2ut.h"

#include <limits.h>

namespace {

// ---------------------------------------------------------------------------------------------
// layer 0 with GroupNorm over time
// ---------------------------------------------------------------------------------------------
constexpr int GN_PARTS = MMS_HUBERT_GN_PARTS;
constexpr int GN_THREADS = 256;
constexpr int GN_CPT = MMS_ASR_CONV0_MAX_C / GN_THREADS;      // channels per thread
constexpr int GN_MAX_K = MMS_ASR_CONV0_MAX_K, GN_MAX_S = MMS_ASR_CONV0_MAX_S;
constexpr int GN_FR_STAT = 64;    // frames staged at a time by the statistics pass
constexpr int GN_FR = 16;         // frames per block of the second pass

// the taps of this thread's channels, and the bias (0 without one)
struct GnTaps {
  float w[GN_CPT][GN_MAX_K];
  float b[GN_CPT];
};

MMS_DEV void gn_load_taps(GnTaps& tp, const float* __restrict__ w, const float* __restrict__ bias, int k, int C) {
#pragma unroll
  for (int u = 0; u < GN_CPT; ++u) {
    const int c = threadIdx.x + u * GN_THREADS;
    tp.b[u] = (bias && c < C) ? bias[c] : 0.f;
#pragma unroll
    for (int j = 0; j < GN_MAX_K; ++j) tp.w[u][j] = (j < k && c < C) ? w[j * C + c] : 0.f;
  }
}

// xs[0, nfr * s - s + k) = the samples of frames [t0, t0 + nfr), normalised when stats is given
MMS_DEV void gn_stage(float* xs, const float* __restrict__ x, long n, const float* __restrict__ stats, long t0, int nfr,
                      int k, int s) {
  const int nx = (nfr - 1) * s + k;
  const float mean = stats ? stats[0] : 0.f, rstd = stats ? stats[1] : 1.f;
  for (int i = threadIdx.x; i < nx; i += GN_THREADS) {
    const long src = t0 * s + i;
    float v = 0.f;                                        // past the end: frames >= T0 only
    if (src < n) v = stats ? (x[src] - mean) * rstd : x[src];
    xs[i] = v;
  }
}

// one output of the convolution: an fp32 fma chain (the second pass), or the same chain in double (the
// statistics: with few frames nothing averages the fp32 chain's rounding out of a channel's variance)
template <typename T>
MMS_DEV T gn_point(const float* xs, int f, int s, int k, const GnTaps& tp, int u) {
  T v = (T)tp.b[u];
#pragma unroll
  for (int j = 0; j < GN_MAX_K; ++j)
    if (j < k) v = fma((T)xs[f * s + j], (T)tp.w[u][j], v);
  return v;
}

// ws[part][c][0 / 1] = the sum of v / of v^2 over the part's slice of the frames (0 for an empty slice)
__global__ void __launch_bounds__(GN_THREADS) hubert_conv0_stats_kernel(
    const float* __restrict__ x, long n, const float* __restrict__ stats, const float* __restrict__ w,
    const float* __restrict__ bias, int k, int s, long T0, int C, double* __restrict__ ws) {
  __shared__ float xs[(GN_FR_STAT - 1) * GN_MAX_S + GN_MAX_K];
  GnTaps tp;
  gn_load_taps(tp, w, bias, k, C);
  const long per = (T0 + GN_PARTS - 1) / GN_PARTS;
  const long f0 = min(T0, (long)blockIdx.x * per), f1 = min(T0, f0 + per);
  double sum[GN_CPT], sq[GN_CPT];
#pragma unroll
  for (int u = 0; u < GN_CPT; ++u) sum[u] = sq[u] = 0.0;
  for (long t0 = f0; t0 < f1; t0 += GN_FR_STAT) {
    const int nfr = (int)min((long)GN_FR_STAT, f1 - t0);
    __syncthreads();                                      // the previous chunk's reads are done
    gn_stage(xs, x, n, stats, t0, nfr, k, s);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < GN_CPT; ++u) {
      if (threadIdx.x + u * GN_THREADS >= C) continue;
      for (int f = 0; f < nfr; ++f) {
        const double v = gn_point<double>(xs, f, s, k, tp, u);
        sum[u] += v;
        sq[u] += v * v;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < GN_CPT; ++u) {
    const int c = threadIdx.x + u * GN_THREADS;
    if (c >= C) continue;
    double* o = ws + ((long)blockIdx.x * C + c) * 2;
    o[0] = sum[u];
    o[1] = sq[u];
  }
}

// mr[c] = (mean, 1 / sqrt(var + eps)): the parts added in part order, the variance E[v^2] - mean^2 in double
__global__ void __launch_bounds__(GN_THREADS) hubert_conv0_fold_kernel(const double* __restrict__ ws, long T0, int C,
                                                                       float eps, float* __restrict__ mr) {
  const int c = blockIdx.x * GN_THREADS + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int p = 0; p < GN_PARTS; ++p) {
    s += ws[((long)p * C + c) * 2];
    q += ws[((long)p * C + c) * 2 + 1];
  }
  const double mean = s / (double)T0;
  const double var = fmax(q / (double)T0 - mean * mean, 0.0);
  mr[2 * c] = (float)mean;
  mr[2 * c + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

__global__ void __launch_bounds__(GN_THREADS) hubert_conv0_apply_kernel(
    const float* __restrict__ x, long n, const float* __restrict__ stats, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ mr, const float* __restrict__ gn_g,
    const float* __restrict__ gn_b, int k, int s, long T0, int C, h16* __restrict__ y, long ldy) {
  __shared__ float xs[(GN_FR - 1) * GN_MAX_S + GN_MAX_K];
  GnTaps tp;
  gn_load_taps(tp, w, bias, k, C);
  const long t0 = (long)blockIdx.x * GN_FR;
  const int nfr = (int)min((long)GN_FR, T0 - t0);
  gn_stage(xs, x, n, stats, t0, nfr, k, s);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < GN_CPT; ++u) {
    const int c = threadIdx.x + u * GN_THREADS;
    if (c >= C) continue;
    const float mean = mr[2 * c], rstd = mr[2 * c + 1], g = gn_g[c], be = gn_b[c];
    for (int f = 0; f < nfr; ++f)
      y[(t0 + f) * ldy + c] = (h16)gelu_erf((gn_point<float>(xs, f, s, k, tp, u) - mean) * rstd * g + be);
  }
}

// ---------------------------------------------------------------------------------------------
// nearest centroid
// ---------------------------------------------------------------------------------------------
constexpr int KM_THREADS = 256;
constexpr int KM_ROWS = 64;       // rows per block: 16 per wave
constexpr int KM_NT = 4;          // centroid tiles of 16 whose accumulators a wave holds at once
constexpr int KM_PASS = KM_NT * 16;
constexpr float KM_LO_SCALE = 1.f / (float)MMS_KMEANS_LO_SCALE;

MMS_DEV bool km_better(float s, int i, float bs, int bi) { return s < bs || (s == bs && i < bi); }

// one pass of a wave: the hi and lo products of its 16 rows of X with the nt tiles of 16 centroids from c0
MMS_DEV void km_pass(const h16* __restrict__ xr, bool rv, int d, const h16* __restrict__ Chi, const h16* __restrict__ Clo,
                     int c0, int nt, int l15, int lk, f32x4 (&ah)[KM_NT], f32x4 (&al)[KM_NT]) {
  const int nsteps = (d + 31) >> 5;
#pragma unroll
  for (int t = 0; t < KM_NT; ++t) ah[t] = al[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsteps; ++s) {
    const int kk = s * 32 + lk;
    const bool kv = kk < d;                               // d is a multiple of 8: whole pieces
    h16x8 xf = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rv && kv) xf = *reinterpret_cast<const h16x8*>(xr + kk);
    h16x8 hf[KM_NT], lf[KM_NT];
#pragma unroll
    for (int t = 0; t < KM_NT; ++t) {
      hf[t] = lf[t] = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (t < nt && kv) {                                 // rows < round_up(Kc, 16): inside the images
        const long off = (long)(c0 + t * 16 + l15) * d + kk;
        hf[t] = *reinterpret_cast<const h16x8*>(Chi + off);
        lf[t] = *reinterpret_cast<const h16x8*>(Clo + off);
      }
    }
#pragma unroll
    for (int t = 0; t < KM_NT; ++t)
      if (t < nt) {
        ah[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(hf[t], xf, ah[t], 0, 0, 0);
        al[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lf[t], xf, al[t], 0, 0, 0);
      }
  }
}

// centroid c's score from its accumulators: |C_c|^2 - 2 (x.hi + x.lo / 2^11)
MMS_DEV float km_score(float hi, float lo, float cn) { return fmaf(-2.f, fmaf(lo, KM_LO_SCALE, hi), cn); }

__global__ void __launch_bounds__(KM_THREADS) kmeans_assign_kernel(
    const h16* __restrict__ X, long ldx, int R, int d, const h16* __restrict__ Chi, const h16* __restrict__ Clo,
    const float* __restrict__ cn, int Kc, int chunk, float* __restrict__ pscore, int* __restrict__ pidx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lk = (lane >> 4) * 8;
  const int r0 = blockIdx.x * KM_ROWS + wave * 16;
  if (r0 >= R) return;                                    // wave-uniform; the kernel has no block barrier
  const int r = r0 + l15;
  const bool rv = r < R;
  const h16* __restrict__ xr = X + (long)(rv ? r : 0) * ldx;
  const int cbeg = blockIdx.y * chunk, cend = min(Kc, cbeg + chunk);
  float best = INFINITY;
  int bi = INT_MAX;
  for (int c0 = cbeg; c0 < cend; c0 += KM_PASS) {
    const int nt = min(KM_NT, (cend - c0 + 15) >> 4);     // tiles that hold a real centroid
    f32x4 ah[KM_NT], al[KM_NT];
    km_pass(xr, rv, d, Chi, Clo, c0, nt, l15, lk, ah, al);
    // D[row = centroid (lane>>4)*4 + e][col = row of X lane&15]: ascending centroids within a lane
#pragma unroll
    for (int t = 0; t < KM_NT; ++t) {
      if (t >= nt) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + t * 16 + (lane >> 4) * 4 + e;
        if (c >= cend) continue;                          // the padded centroids take no part
        const float sc = km_score(ah[t][e], al[t][e], cn[c]);
        if (sc < best) {                                  // strict: the lowest index wins a tie
          best = sc;
          bi = c;
        }
      }
    }
  }
  // the four lanes that share a row of X
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    const float os = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (km_better(os, oi, best, bi)) {
      best = os;
      bi = oi;
    }
  }
  if (lane < 16 && rv) {
    pscore[(long)blockIdx.y * R + r] = best;
    pidx[(long)blockIdx.y * R + r] = bi;
  }
}

constexpr int KF_THREADS = 256;

__global__ void __launch_bounds__(KF_THREADS) kmeans_fold_kernel(
    const float* __restrict__ pscore, const int* __restrict__ pidx, int nchunks, long R, int Tmax,
    const int* __restrict__ lens, int* code, int* __restrict__ merged, int* __restrict__ count, int* __restrict__ bad) {
  __shared__ int wtot[KF_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int T = lens ? min(max(lens[b], 0), Tmax) : Tmax;
  int* cb = code + (long)b * Tmax;
  int* mb = merged + (long)b * Tmax;
  int notfin = 0;
  for (int t = tid; t < T; t += KF_THREADS) {
    const long row = (long)b * Tmax + t;
    float best = INFINITY;
    int bi = INT_MAX;
    for (int ch = 0; ch < nchunks; ++ch) {                // chunks ascend in centroid index
      const float s = pscore[ch * R + row];
      if (s < best) {
        best = s;
        bi = pidx[ch * R + row];
      }
    }
    if (!isfinite(best)) notfin = 1;                      // -inf, or no score that compares (NaN everywhere)
    cb[t] = bi == INT_MAX ? 0 : bi;
  }
  notfin = __syncthreads_or(notfin);                      // also orders the codes written above for the block
  if (tid == 0) bad[b] = notfin;
  int base = 0;
  for (int c0 = 0; c0 < T; c0 += KF_THREADS) {
    const int t = c0 + tid;
    int id = 0;
    bool keep = false;
    if (t < T) {
      id = cb[t];
      keep = t == 0 || id != cb[t - 1];
    }
    int inc = keep ? 1 : 0;                               // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int i = 0; i < KF_THREADS / 64; ++i) {
      if (i < wave) woff += wtot[i];
      total += wtot[i];
    }
    if (keep) mb[base + woff + inc - 1] = id;
    base += total;
    __syncthreads();                                      // wtot is rewritten by the next chunk
  }
  if (tid == 0) count[b] = base;
}

// ---------------------------------------------------------------------------------------------
// the top_k nearest centroids
// ---------------------------------------------------------------------------------------------
constexpr int KT_MAX = MMS_KMEANS_TOPK_MAX;
constexpr int KT_LD = KT_MAX + 1;                         // a row's list in LDS: odd stride, rows on distinct banks
constexpr int KTF_THREADS = 64;

// A row's list: k (score, index) pairs ascending by (score, index), (inf, INT_MAX) where empty.  (s, i)
// enters if it is better than the last pair; a NaN never does.  One lane per list at a time.
MMS_DEV void kt_insert(volatile float* ls, volatile int* li, int k, float s, int i) {
  if (!km_better(s, i, ls[k - 1], li[k - 1])) return;
  int j = k - 1;
  while (j > 0 && km_better(s, i, ls[j - 1], li[j - 1])) {
    ls[j] = ls[j - 1];
    li[j] = li[j - 1];
    --j;
  }
  ls[j] = s;
  li[j] = i;
}

// kmeans_assign_kernel with a list of k per row in place of the one best.  A wave touches only the lists
// of its own 16 rows, so the kernel has no block barrier; the four lanes that share a row take turns.
__global__ void __launch_bounds__(KM_THREADS) kmeans_topk_kernel(
    const h16* __restrict__ X, long ldx, int R, int d, const h16* __restrict__ Chi, const h16* __restrict__ Clo,
    const float* __restrict__ cn, int Kc, int chunk, int k, float* __restrict__ pscore, int* __restrict__ pidx) {
  __shared__ float ls[KM_ROWS * KT_LD];
  __shared__ int li[KM_ROWS * KT_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lk = (lane >> 4) * 8, grp = lane >> 4;
  const int r0 = blockIdx.x * KM_ROWS + wave * 16;
  if (r0 >= R) return;                                    // wave-uniform
  const int r = r0 + l15;
  const bool rv = r < R;
  const h16* __restrict__ xr = X + (long)(rv ? r : 0) * ldx;
  const int cbeg = blockIdx.y * chunk, cend = min(Kc, cbeg + chunk);
  volatile float* ms = ls + (wave * 16 + l15) * KT_LD;
  volatile int* mi = li + (wave * 16 + l15) * KT_LD;
  for (int j = grp; j < k; j += 4) {
    ms[j] = INFINITY;
    mi[j] = INT_MAX;
  }
  for (int c0 = cbeg; c0 < cend; c0 += KM_PASS) {
    const int nt = min(KM_NT, (cend - c0 + 15) >> 4);
    f32x4 ah[KM_NT], al[KM_NT];
    km_pass(xr, rv, d, Chi, Clo, c0, nt, l15, lk, ah, al);
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_wave_barrier();                    // LDS operations of a wave complete in order
      if (grp != g) continue;
#pragma unroll
      for (int t = 0; t < KM_NT; ++t) {
        if (t >= nt) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c0 + t * 16 + grp * 4 + e;
          if (c < cend) kt_insert(ms, mi, k, km_score(ah[t][e], al[t][e], cn[c]), c);
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (rv)
    for (int j = grp; j < k; j += 4) {
      const long o = ((long)blockIdx.y * R + r) * k + j;
      pscore[o] = ms[j];
      pidx[o] = mi[j];
    }
}

// One thread per frame of utterance blockIdx.y: merges the chunks' lists (each ascending, so a chunk is
// left at its first pair that does not enter), then dist = sqrt(max(|x|^2 + score, 0)).  bad[b] (zeroed by
// the caller) is set where a kept score, a norm or a distance is not finite, a list is short of k
// comparable scores, or the k distances are all 0 (their sum is the beam's divisor).
__global__ void __launch_bounds__(KTF_THREADS) kmeans_topk_fold_kernel(
    const float* __restrict__ pscore, const int* __restrict__ pidx, int nchunks, long R, int Tmax,
    const int* __restrict__ lens, const float* __restrict__ xnorm, int k, int* __restrict__ idx,
    float* __restrict__ dist, int* __restrict__ bad) {
  __shared__ float ls[KTF_THREADS * KT_LD];
  __shared__ int li[KTF_THREADS * KT_LD];
  const int b = blockIdx.y, t = blockIdx.x * KTF_THREADS + threadIdx.x;
  const int T = lens ? min(max(lens[b], 0), Tmax) : Tmax;
  if (t >= T) return;                                     // no barrier in this kernel
  const long row = (long)b * Tmax + t;
  volatile float* ms = ls + threadIdx.x * KT_LD;
  volatile int* mi = li + threadIdx.x * KT_LD;
  for (int j = 0; j < k; ++j) {
    ms[j] = INFINITY;
    mi[j] = INT_MAX;
  }
  for (int ch = 0; ch < nchunks; ++ch) {
    const long o = ((long)ch * R + row) * k;
    for (int j = 0; j < k; ++j) {
      const float s = pscore[o + j];
      const int i = pidx[o + j];
      if (!km_better(s, i, ms[k - 1], mi[k - 1])) break;
      kt_insert(ms, mi, k, s, i);
    }
  }
  const float xn = xnorm[row];
  int notfin = isfinite(xn) ? 0 : 1;
  float last = 0.f;
  for (int j = 0; j < k; ++j) {
    const float s = ms[j];
    const int i = mi[j];
    const float v = xn + s;
    if (!isfinite(s) || !isfinite(v)) notfin = 1;
    last = v > 0.f ? (float)sqrt((double)v) : 0.f;        // correctly rounded: the double root carries 53 bits
    idx[row * k + j] = i == INT_MAX ? 0 : i;
    dist[row * k + j] = last;
  }
  if (notfin || last == 0.f) bad[b] = 1;                  // every writer stores the same value
}

}  // namespace

extern "C" int mms2ut_hubert_conv0(const float* x, int64_t n, const float* stats, const float* w, const float* bias,
                                   const float* gn_g, const float* gn_b, float eps, int k, int stride, int C,
                                   double* ws, float* mr, void* y, int64_t ldy, hipStream_t s) {
  MMS_REQUIRE(x && w && gn_g && gn_b && ws && mr && y, "hubert_conv0: null buffer");
  MMS_REQUIRE(k >= 1 && k <= GN_MAX_K && stride >= 1 && stride <= GN_MAX_S,
              "hubert_conv0: kernel size must be in [1, %d] and stride in [1, %d] (got %d, %d)", GN_MAX_K, GN_MAX_S, k,
              stride);
  MMS_REQUIRE(C >= 1 && C <= MMS_ASR_CONV0_MAX_C && ldy >= C, "hubert_conv0: channels must be in [1, %d] (got %d)",
              MMS_ASR_CONV0_MAX_C, C);
  MMS_REQUIRE(eps >= 0.f, "hubert_conv0: eps must be >= 0");
  MMS_REQUIRE(n >= k && (n - k) / stride + 1 < (1L << 31), "hubert_conv0: %ld samples for a kernel of %d", (long)n, k);
  const long T0 = (long)((n - k) / stride + 1);
  hipLaunchKernelGGL(hubert_conv0_stats_kernel, dim3(GN_PARTS), dim3(GN_THREADS), 0, s, x, (long)n, stats, w, bias, k,
                     stride, T0, C, ws);
  hipLaunchKernelGGL(hubert_conv0_fold_kernel, dim3((C + GN_THREADS - 1) / GN_THREADS), dim3(GN_THREADS), 0, s, ws, T0, C,
                     eps, mr);
  hipLaunchKernelGGL(hubert_conv0_apply_kernel, dim3((unsigned)((T0 + GN_FR - 1) / GN_FR)), dim3(GN_THREADS), 0, s, x,
                     (long)n, stats, w, bias, mr, gn_g, gn_b, k, stride, T0, C, reinterpret_cast<h16*>(y), (long)ldy);
  return mms::check_launch("hubert_conv0");
}

extern "C" int mms2ut_kmeans_chunks(int R, int Kc, int chunk, int* chunk_out, int* nchunks) {
  MMS_REQUIRE(R >= 1 && Kc >= 1 && chunk >= 0 && chunk % KM_PASS == 0 && chunk_out && nchunks,
              "kmeans_chunks: R, Kc >= 1 and a chunk that is 0 or a multiple of %d (got %d, %d, %d)", KM_PASS, R, Kc, chunk);
  if (chunk == 0) {
    // few rows: one pass of 64 centroids per block, so that a single utterance still spreads over the chip
    // (249 rows: 64 blocks instead of 16); from about two blocks per CU on, four passes per block are faster
    const long blocks = (long)((R + KM_ROWS - 1) / KM_ROWS) * ((Kc + KM_PASS - 1) / KM_PASS);
    chunk = blocks <= MMS_KMEANS_SMALL_BLOCKS ? KM_PASS : 4 * KM_PASS;
  }
  *chunk_out = chunk;
  *nchunks = (int)(((long)Kc + chunk - 1) / chunk);
  return 0;
}

extern "C" int mms2ut_kmeans_assign(const void* X, int64_t ldx, int R, int d, const void* c_hi, const void* c_lo,
                                    const float* cnorm, int Kc, int chunk, float* pscore, int32_t* pidx, hipStream_t s) {
  MMS_REQUIRE(X && c_hi && c_lo && cnorm && pscore && pidx, "kmeans_assign: null buffer");
  MMS_REQUIRE(R >= 1 && Kc >= 1, "kmeans_assign: R %d, Kc %d", R, Kc);
  MMS_REQUIRE(d >= 8 && d % 8 == 0 && ldx >= d && ldx % 8 == 0, "kmeans_assign: d must be a multiple of 8 with 16-byte "
              "aligned rows (d %d, ldx %ld)", d, (long)ldx);
  MMS_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)c_hi & 15) == 0 && ((uintptr_t)c_lo & 15) == 0,
              "kmeans_assign: misaligned buffer");
  MMS_REQUIRE(chunk >= KM_PASS && chunk % KM_PASS == 0, "kmeans_assign: chunk must be a positive multiple of %d (got %d)",
              KM_PASS, chunk);
  const long nchunks = ((long)Kc + chunk - 1) / chunk;
  MMS_REQUIRE(nchunks <= 65535, "kmeans_assign: %ld chunks", nchunks);
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((R + KM_ROWS - 1) / KM_ROWS, (unsigned)nchunks), dim3(KM_THREADS), 0, s,
                     reinterpret_cast<const h16*>(X), (long)ldx, R, d, reinterpret_cast<const h16*>(c_hi),
                     reinterpret_cast<const h16*>(c_lo), cnorm, Kc, chunk, pscore, pidx);
  return mms::check_launch("kmeans_assign");
}

extern "C" int mms2ut_kmeans_topk(const void* X, int64_t ldx, int R, int d, const void* c_hi, const void* c_lo,
                                  const float* cnorm, int Kc, int chunk, int top_k, float* pscore, int32_t* pidx,
                                  hipStream_t s) {
  MMS_REQUIRE(X && c_hi && c_lo && cnorm && pscore && pidx, "kmeans_topk: null buffer");
  MMS_REQUIRE(R >= 1 && Kc >= 1, "kmeans_topk: R %d, Kc %d", R, Kc);
  MMS_REQUIRE(top_k >= 1 && top_k <= KT_MAX && top_k <= Kc, "kmeans_topk: top_k must be in [1, min(%d, Kc = %d)] (got %d)",
              KT_MAX, Kc, top_k);
  MMS_REQUIRE(d >= 8 && d % 8 == 0 && ldx >= d && ldx % 8 == 0, "kmeans_topk: d must be a multiple of 8 with 16-byte "
              "aligned rows (d %d, ldx %ld)", d, (long)ldx);
  MMS_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)c_hi & 15) == 0 && ((uintptr_t)c_lo & 15) == 0,
              "kmeans_topk: misaligned buffer");
  MMS_REQUIRE(chunk >= KM_PASS && chunk % KM_PASS == 0, "kmeans_topk: chunk must be a positive multiple of %d (got %d)",
              KM_PASS, chunk);
  const long nchunks = ((long)Kc + chunk - 1) / chunk;
  MMS_REQUIRE(nchunks <= 65535, "kmeans_topk: %ld chunks", nchunks);
  hipLaunchKernelGGL(kmeans_topk_kernel, dim3((R + KM_ROWS - 1) / KM_ROWS, (unsigned)nchunks), dim3(KM_THREADS), 0, s,
                     reinterpret_cast<const h16*>(X), (long)ldx, R, d, reinterpret_cast<const h16*>(c_hi),
                     reinterpret_cast<const h16*>(c_lo), cnorm, Kc, chunk, top_k, pscore, pidx);
  return mms::check_launch("kmeans_topk");
}

extern "C" int mms2ut_kmeans_topk_fold(const float* pscore, const int32_t* pidx, int nchunks, int B, int Tmax,
                                       const int32_t* lens, const float* xnorm, int top_k, int32_t* idx, float* dist,
                                       int32_t* bad, hipStream_t s) {
  MMS_REQUIRE(pscore && pidx && xnorm && idx && dist && bad, "kmeans_topk_fold: null buffer");
  MMS_REQUIRE(nchunks >= 1 && B >= 1 && B <= 65535 && Tmax >= 1 && (long)B * Tmax < (1L << 31),
              "kmeans_topk_fold: nchunks %d, B %d, Tmax %d", nchunks, B, Tmax);
  MMS_REQUIRE(top_k >= 1 && top_k <= KT_MAX, "kmeans_topk_fold: top_k must be in [1, %d] (got %d)", KT_MAX, top_k);
  hipLaunchKernelGGL(kmeans_topk_fold_kernel, dim3((Tmax + KTF_THREADS - 1) / KTF_THREADS, B), dim3(KTF_THREADS), 0, s,
                     pscore, pidx, nchunks, (long)B * Tmax, Tmax, lens, xnorm, top_k, idx, dist, bad);
  return mms::check_launch("kmeans_topk_fold");
}

extern "C" int mms2ut_kmeans_fold(const float* pscore, const int32_t* pidx, int nchunks, int B, int Tmax,
                                  const int32_t* lens, int32_t* code, int32_t* merged, int32_t* count, int32_t* bad,
                                  hipStream_t s) {
  MMS_REQUIRE(pscore && pidx && code && merged && count && bad, "kmeans_fold: null buffer");
  MMS_REQUIRE(nchunks >= 1 && B >= 1 && B <= 65535 && Tmax >= 1 && (long)B * Tmax < (1L << 31),
              "kmeans_fold: nchunks %d, B %d, Tmax %d", nchunks, B, Tmax);
  hipLaunchKernelGGL(kmeans_fold_kernel, dim3(B), dim3(KF_THREADS), 0, s, pscore, pidx, nchunks, (long)B * Tmax, Tmax, lens,
                     code, merged, count, bad);
  return mms::check_launch("kmeans_fold");
}
