// Unit codebook training (multimodal-s2ut_amd/kmeans.py): scikit-learn's MiniBatchKMeans.fit on fp16 feature
// rows, on the device.  The assignment itself is units.hip's kmeans_assign; what is here is the learning
// loop around it.  No float atomics anywhere: every sum has a fixed order, every run gives the same bits.
//
//   kmeans_row_norms   |x|^2 of fp16 rows (fp16 products are exact in fp32; lanes add in fp32, the wave in
//                      double), one wave per row.
//   kmeans_gather      rows (fp16, or widened to fp32: the initial centres) and their norms gathered by an
//                      index vector into a contiguous batch; indices may repeat.
//   kmeans_train_fold  kmeans_assign's chunk partials -> per row its code and best score (chunk order: the
//                      lowest index wins a tie), and max(|x|^2 + best, 0) summed in double per block of 256
//                      rows; kmeans_finish adds the blocks in block order and, inside a fit, runs
//                      scikit-learn's EWA-inertia stopping rule on the device (state below).
//   kmeans_accumulate  per-centroid fp32 sum of the batch's rows and their count.  One block per centroid;
//                      each wave owns 256 columns and scans the codes 64 at a time: the ballot of
//                      "code == mine" is that centroid's list of rows in index order, walked bit by bit.
//                      Nothing of size [rows, K] is formed, and a centroid that owns every row or none is
//                      the same loop.
//   kmeans_update      one launch: centre = (centre * count + sum) / (count + m) in double where m > 0,
//                      the running counts (int64), and the c_hi / c_lo / cnorm images kmeans_assign reads;
//                      a centre that is not finite or outside fp16's range raises a device flag.
//   kmeans_pp          k-means++ over the seeding subset, K - 1 rounds of two launches and no host read:
//                      squared distances (sum (x - c)^2 in fp32, clamped at 0) of the round's candidates to
//                      every row, min'd with the running closest distance, potentials in double per block;
//                      then one block adds the potentials in a fixed order, takes the lowest (the lowest
//                      trial index on a tie), and finds the next round's candidates as the searchsorted of
//                      uniform * potential in the double inclusive cumulative sum of the closest distances.
//
// state (doubles, MMS_KMEANS_STATE of them): [0] steps run, [1] EWA inertia, [2] its minimum, [3] steps
// without improvement, [4] done.  Once done is set every kernel of a step returns at once, so the host may
// queue steps ahead and read the state only now and then: the result does not depend on how often.
#include "common.h"
#include "../../include/mms2ut.h"

#include <limits.h>

namespace {

constexpr int KT_THREADS = 256;
constexpr int KT_WAVES = KT_THREADS / 64;
constexpr int KPP_MAX_T = MMS_KMEANS_PP_MAX_TRIALS;
constexpr int KPP_ROWS = MMS_KMEANS_PP_ROWS;   // rows per block of the distance kernel: 4 per wave, many blocks
constexpr int KPP_PICK_THREADS = 1024;
constexpr float KM_LO = (float)MMS_KMEANS_LO_SCALE;
enum { ST_STEPS = 0, ST_EWA, ST_EWA_MIN, ST_NO_IMPROVEMENT, ST_DONE };

MMS_DEV bool km_done(const double* st) { return st && st[ST_DONE] != 0.0; }

// the waves' values in wave order (call from every thread of the block; ws: KT_WAVES doubles of LDS)
MMS_DEV double block_sum_d(double v, double* ws) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = ws[0];
#pragma unroll
  for (int i = 1; i < KT_WAVES; ++i) s += ws[i];
  return s;
}

__global__ void __launch_bounds__(KT_THREADS) km_row_norms_kernel(const h16* __restrict__ X, long ldx, long R, int d,
                                                                  float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
  if (r >= R) return;                                     // wave-uniform
  const h16* __restrict__ xr = X + r * ldx;
  float acc = 0.f;
  for (int k = lane * 8; k < d; k += 512) {
    const h16x8 v = *reinterpret_cast<const h16x8*>(xr + k);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf((float)v[e], (float)v[e], acc);
  }
  const double s = wave_sum_d((double)acc);
  if (lane == 0) norms[r] = (float)s;
}

template <bool WIDE>
__global__ void __launch_bounds__(KT_THREADS) km_gather_kernel(const h16* __restrict__ X, long ldx, long N,
                                                               const float* __restrict__ norms,
                                                               const int* __restrict__ idx, int R, int d,
                                                               void* __restrict__ out, float* __restrict__ nout,
                                                               const double* __restrict__ st) {
  if (km_done(st)) return;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
  if (r >= R) return;
  const long src = min(max((long)idx[r], 0L), N - 1);     // the host checks the indices; never read outside X
  const h16* __restrict__ xr = X + src * ldx;
  for (int k = lane * 8; k < d; k += 512) {
    const h16x8 v = *reinterpret_cast<const h16x8*>(xr + k);
    if (WIDE) {
      float* o = reinterpret_cast<float*>(out) + (long)r * d + k;
      *reinterpret_cast<f32x4*>(o) = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
    } else {
      *reinterpret_cast<h16x8*>(reinterpret_cast<h16*>(out) + (long)r * d + k) = v;
    }
  }
  if (lane == 0 && nout) nout[r] = norms[src];
}

__global__ void __launch_bounds__(KT_THREADS) km_train_fold_kernel(const float* __restrict__ pscore,
                                                                   const int* __restrict__ pidx, int nchunks, int R,
                                                                   const float* __restrict__ xnorm,
                                                                   int* __restrict__ code, float* __restrict__ best_out,
                                                                   double* __restrict__ partials, int* __restrict__ bad,
                                                                   const double* __restrict__ st) {
  __shared__ double ws[KT_WAVES];
  if (km_done(st)) return;                                // block-uniform
  const int r = blockIdx.x * KT_THREADS + threadIdx.x;
  double v = 0.0;
  if (r < R) {
    float best = INFINITY;
    int bi = INT_MAX;
    for (int ch = 0; ch < nchunks; ++ch) {                // chunks ascend in centroid index
      const float s = pscore[(long)ch * R + r];
      if (s < best) {
        best = s;
        bi = pidx[(long)ch * R + r];
      }
    }
    if (!isfinite(best)) *bad = 1;                        // every writer stores the same value
    code[r] = bi == INT_MAX ? 0 : bi;
    best_out[r] = best;
    v = fmax((double)xnorm[r] + (double)best, 0.0);
  }
  const double s = block_sum_d(v, ws);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one thread: the batch inertia, and inside a fit MiniBatchKMeans._mini_batch_convergence with tol = 0
__global__ void km_finish_kernel(const double* __restrict__ partials, int nparts, int R, double* __restrict__ inertia,
                                 double* __restrict__ st, double alpha, int max_no_improvement) {
  if (threadIdx.x || km_done(st)) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += partials[p];
  if (inertia) *inertia = s;
  if (!st) return;
  const double step = st[ST_STEPS];
  st[ST_STEPS] = step + 1.0;
  if (step == 0.0) return;                                // the first step's inertia is the initialisation's
  const double b = s / (double)R;
  // no contraction: the same roundings as the host arithmetic this restates
  const double ewa = step == 1.0 ? b : __dadd_rn(__dmul_rn(st[ST_EWA], 1.0 - alpha), __dmul_rn(b, alpha));
  st[ST_EWA] = ewa;
  if (step == 1.0 || ewa < st[ST_EWA_MIN]) {
    st[ST_NO_IMPROVEMENT] = 0.0;
    st[ST_EWA_MIN] = ewa;
  } else {
    st[ST_NO_IMPROVEMENT] += 1.0;
  }
  if (max_no_improvement >= 0 && st[ST_NO_IMPROVEMENT] >= (double)max_no_improvement) st[ST_DONE] = 1.0;
}

__global__ void __launch_bounds__(KT_THREADS) km_accumulate_kernel(const h16* __restrict__ Xb, long ldx,
                                                                   const int* __restrict__ code, int R, int d,
                                                                   float* __restrict__ sums, int* __restrict__ cnt,
                                                                   const double* __restrict__ st) {
  if (km_done(st)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x;
  for (int base = 0; base < d; base += KT_THREADS * 4) {
    const int wcol = base + wave * 256;                   // this wave's first column
    const bool counts = base == 0 && wave == 0;
    if (wcol >= d && !counts) continue;                   // wave-uniform; the kernel has no block barrier
    const int col = wcol + lane * 4;
    const bool cv = col < d;                              // d is a multiple of 8: whole pieces
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int n = 0;
    for (int r0 = 0; r0 < R; r0 += 64) {
      const int r = r0 + lane;
      unsigned long long m = __ballot(r < R && code[r] == c);   // this centroid's rows, ascending from bit 0
      n += __popcll(m);
      while (m) {                                         // wave-uniform
        const int rr = r0 + __ffsll((long long)m) - 1;
        m &= m - 1;
        if (cv) {
          const h16x4 v = *reinterpret_cast<const h16x4*>(Xb + (long)rr * ldx + col);
          a0 += (float)v[0];
          a1 += (float)v[1];
          a2 += (float)v[2];
          a3 += (float)v[3];
        }
      }
    }
    if (cv) *reinterpret_cast<f32x4*>(sums + (long)c * d + col) = f32x4{a0, a1, a2, a3};
    if (counts && lane == 0) cnt[c] = n;
  }
}

__global__ void __launch_bounds__(KT_THREADS) km_update_kernel(float* __restrict__ C, long long* __restrict__ counts,
                                                               const float* __restrict__ sums,
                                                               const int* __restrict__ cnt, int d, h16* __restrict__ hi,
                                                               h16* __restrict__ lo, float* __restrict__ cn,
                                                               int* __restrict__ bad, const double* __restrict__ st) {
  __shared__ double ws[KT_WAVES];
  if (km_done(st)) return;
  const int c = blockIdx.x;
  const int m = cnt ? cnt[c] : 0;
  const long long n0 = m > 0 ? counts[c] : 0;
  float* __restrict__ cr = C + (long)c * d;
  double q = 0.0;
  bool wild = false;
  for (int k = threadIdx.x; k < d; k += KT_THREADS) {
    float v = cr[k];
    if (m > 0) {                                          // a centroid without rows keeps its value
      // no contraction: the roundings of the plain double expression
      v = (float)(__dadd_rn(__dmul_rn((double)v, (double)n0), (double)sums[(long)c * d + k]) / (double)(n0 + m));
      cr[k] = v;
    }
    const h16 h = (h16)v;
    hi[(long)c * d + k] = h;
    lo[(long)c * d + k] = (h16)((v - (float)h) * KM_LO);
    q += (double)v * (double)v;
    if (!(fabsf(v) <= 65504.f)) wild = true;              // also NaN
  }
  if (wild) *bad = 1;
  const double s = block_sum_d(q, ws);                    // its barrier: every thread has read counts[c]
  if (threadIdx.x == 0) {
    cn[c] = (float)s;
    if (m > 0) counts[c] = n0 + m;
  }
}

// ---------------------------------------------------------------------------------------------
// k-means++
// ---------------------------------------------------------------------------------------------
__global__ void kpp_first_kernel(int* cand, int first) {
  if (threadIdx.x == 0) cand[0] = first;
}

// dist[t][r] = min(closest[r], |x_r - x_cand[t]|^2); partials[block][t] = its sum over the block's rows
__global__ void __launch_bounds__(KT_THREADS) kpp_dist_kernel(const h16* __restrict__ Xs, int n, int d,
                                                              const int* __restrict__ cand, int T,
                                                              const float* __restrict__ closest,
                                                              float* __restrict__ dist, double* __restrict__ partials) {
  __shared__ double ps[KT_WAVES][KPP_MAX_T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const h16* cr[KPP_MAX_T];
  double pot[KPP_MAX_T];
#pragma unroll
  for (int t = 0; t < KPP_MAX_T; ++t) {
    cr[t] = Xs + (long)min(max(t < T ? cand[t] : 0, 0), n - 1) * d;
    pot[t] = 0.0;
  }
  for (int i = 0; i < KPP_ROWS / KT_WAVES; ++i) {
    const int r = blockIdx.x * KPP_ROWS + wave * (KPP_ROWS / KT_WAVES) + i;
    if (r >= n) break;                                    // wave-uniform
    float acc[KPP_MAX_T];
#pragma unroll
    for (int t = 0; t < KPP_MAX_T; ++t) acc[t] = 0.f;
    for (int k = lane * 8; k < d; k += 512) {
      const h16x8 x = *reinterpret_cast<const h16x8*>(Xs + (long)r * d + k);
#pragma unroll
      for (int t = 0; t < KPP_MAX_T; ++t) {
        if (t >= T) continue;
        const h16x8 y = *reinterpret_cast<const h16x8*>(cr[t] + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float df = (float)x[e] - (float)y[e];
          acc[t] = fmaf(df, df, acc[t]);
        }
      }
    }
    const float cl = closest ? closest[r] : INFINITY;
#pragma unroll
    for (int t = 0; t < KPP_MAX_T; ++t) {
      if (t >= T) continue;                               // wave-uniform
      const float s = fminf(fmaxf(wave_sum(acc[t]), 0.f), cl);
      if (lane == 0) dist[(long)t * n + r] = s;
      pot[t] += (double)s;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < KPP_MAX_T; ++t) ps[wave][t] = pot[t];
  }
  __syncthreads();
  if (threadIdx.x < T) {
    double s = ps[0][threadIdx.x];
    for (int w = 1; w < KT_WAVES; ++w) s += ps[w][threadIdx.x];
    partials[(long)blockIdx.x * T + threadIdx.x] = s;
  }
}

// One block of 16 waves.  Fixes centre c: the candidate of the lowest potential (the lowest trial on a tie; wave t
// adds candidate t's block partials lane-strided, then across the lanes: a fixed order); closest = its distances;
// and, given the next round's uniforms u[0, Tn), that round's candidates: the first row whose inclusive cumulative
// closest distance (double: each wave scans its share of the rows 64 at a time on top of the earlier waves' totals)
// reaches u * potential, the last row if none does.  Every wave that reaches a value bids its first such row with an
// integer minimum, so the first row wins whatever the rounding of the scan.
__global__ void __launch_bounds__(KPP_PICK_THREADS) kpp_pick_kernel(const double* __restrict__ partials, int nblk, int T,
                                                                    int* __restrict__ cand, const float* __restrict__ dist,
                                                                    int n, float* __restrict__ closest,
                                                                    int* __restrict__ chosen, int c,
                                                                    const double* __restrict__ u, int Tn) {
  __shared__ double pots[KPP_MAX_T];
  __shared__ double wtot[KPP_PICK_THREADS / 64];
  __shared__ int best_s;
  __shared__ int next[KPP_MAX_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave < T) {                                         // wave-uniform; T <= 16 waves
    double s = 0.0;
    for (int b = lane; b < nblk; b += 64) s += partials[(long)b * T + wave];
    s = wave_sum_d(s);
    if (lane == 0) pots[wave] = s;
  }
  if (tid < KPP_MAX_T) next[tid] = n - 1;
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int t = 1; t < T; ++t)
      if (pots[t] < pots[best]) best = t;
    best_s = best;
    chosen[c] = min(max(cand[best], 0), n - 1);
  }
  __syncthreads();
  const int best = best_s;
  const double pot = pots[best];
  const float* __restrict__ db = dist + (long)best * n;
  const int per = (((n + KPP_PICK_THREADS / 64 - 1) / (KPP_PICK_THREADS / 64)) + 63) & ~63;   // rows per wave: whole 64s
  const int w0 = min(n, wave * per), w1 = min(n, w0 + per);
  double loc = 0.0;
  for (int i = w0 + lane; i < w1; i += 64) {
    const float v = db[i];
    closest[i] = v;
    loc += (double)v;
  }
  if (!u) return;                                         // block-uniform: the last centre has no next round
  loc = wave_sum_d(loc);
  if (lane == 0) wtot[wave] = loc;
  __syncthreads();
  double pre = 0.0;                                       // the rows before this wave's
  for (int w = 0; w < wave; ++w) pre += wtot[w];
  double vals[KPP_MAX_T];
#pragma unroll
  for (int t = 0; t < KPP_MAX_T; ++t) vals[t] = t < Tn ? __dmul_rn(u[t], pot) : 0.0;
  unsigned open = Tn >= 32 ? 0xffffffffu : (1u << Tn) - 1u;   // the values this wave has not reached yet (wave-uniform)
  for (int b = w0; b < w1 && open; b += 64) {
    const int i = b + lane;
    double inc = i < w1 ? (double)db[i] : 0.0;            // inclusive scan of the 64 rows, in row order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    const double cum = pre + inc;
#pragma unroll
    for (int t = 0; t < KPP_MAX_T; ++t) {
      if (!(open >> t & 1u)) continue;
      const unsigned long long m = __ballot(i < w1 && cum >= vals[t]);
      if (m) {
        open &= ~(1u << t);
        if (lane == 0) atomicMin(&next[t], b + __ffsll((long long)m) - 1);
      }
    }
    pre += __shfl(inc, 63, 64);
  }
  __syncthreads();
  if (tid < Tn) cand[tid] = next[tid];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mms2ut_kmeans_row_norms(const void* X, int64_t ldx, int64_t R, int d, float* norms, hipStream_t s) {
  MMS_REQUIRE(X && norms && aligned16(X), "kmeans_row_norms: null or misaligned buffer");
  MMS_REQUIRE(R >= 1 && (R + KT_WAVES - 1) / KT_WAVES < (1L << 31) && d >= 8 && d % 8 == 0 && ldx >= d && ldx % 8 == 0,
              "kmeans_row_norms: R %ld, d %d, ldx %ld (d and ldx multiples of 8)", (long)R, d, (long)ldx);
  hipLaunchKernelGGL(km_row_norms_kernel, dim3((unsigned)((R + KT_WAVES - 1) / KT_WAVES)), dim3(KT_THREADS), 0, s,
                     reinterpret_cast<const h16*>(X), (long)ldx, (long)R, d, norms);
  return mms::check_launch("kmeans_row_norms");
}

extern "C" int mms2ut_kmeans_gather(const void* X, int64_t ldx, int64_t N, const float* norms, const int32_t* idx, int R,
                                    int d, void* out, int wide, float* norms_out, const double* state, hipStream_t s) {
  MMS_REQUIRE(X && idx && out && aligned16(X) && aligned16(out), "kmeans_gather: null or misaligned buffer");
  MMS_REQUIRE((norms != nullptr) == (norms_out != nullptr), "kmeans_gather: norms and norms_out go together");
  MMS_REQUIRE(N >= 1 && R >= 1 && d >= 8 && d % 8 == 0 && ldx >= d && ldx % 8 == 0,
              "kmeans_gather: N %ld, R %d, d %d, ldx %ld (d and ldx multiples of 8)", (long)N, R, d, (long)ldx);
  const dim3 grid((R + KT_WAVES - 1) / KT_WAVES), block(KT_THREADS);
  const h16* Xh = reinterpret_cast<const h16*>(X);
  if (wide)
    hipLaunchKernelGGL(km_gather_kernel<true>, grid, block, 0, s, Xh, (long)ldx, (long)N, norms, idx, R, d, out, norms_out,
                       state);
  else
    hipLaunchKernelGGL(km_gather_kernel<false>, grid, block, 0, s, Xh, (long)ldx, (long)N, norms, idx, R, d, out,
                       norms_out, state);
  return mms::check_launch("kmeans_gather");
}

extern "C" int mms2ut_kmeans_train_fold(const float* pscore, const int32_t* pidx, int nchunks, int R, const float* xnorm,
                                        int32_t* code, float* best, double* partials, double* inertia, int32_t* bad,
                                        double* state, double alpha, int max_no_improvement, hipStream_t s) {
  MMS_REQUIRE(pscore && pidx && xnorm && code && best && partials && bad, "kmeans_train_fold: null buffer");
  MMS_REQUIRE(inertia || state, "kmeans_train_fold: neither an inertia nor a state to write");
  MMS_REQUIRE(nchunks >= 1 && R >= 1, "kmeans_train_fold: nchunks %d, R %d", nchunks, R);
  MMS_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "kmeans_train_fold: alpha %g outside [0, 1]", alpha);
  const int nparts = (R + KT_THREADS - 1) / KT_THREADS;
  hipLaunchKernelGGL(km_train_fold_kernel, dim3(nparts), dim3(KT_THREADS), 0, s, pscore, pidx, nchunks, R, xnorm, code, best,
                     partials, bad, state);
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(64), 0, s, partials, nparts, R, inertia, state, alpha,
                     max_no_improvement);
  return mms::check_launch("kmeans_train_fold");
}

extern "C" int mms2ut_kmeans_accumulate(const void* Xb, int64_t ldx, const int32_t* code, int R, int d, int K, float* sums,
                                        int32_t* cnt, const double* state, hipStream_t s) {
  MMS_REQUIRE(Xb && code && sums && cnt && aligned16(Xb) && aligned16(sums), "kmeans_accumulate: null or misaligned buffer");
  MMS_REQUIRE(R >= 1 && K >= 1 && d >= 8 && d % 8 == 0 && ldx >= d && ldx % 8 == 0,
              "kmeans_accumulate: R %d, K %d, d %d, ldx %ld (d and ldx multiples of 8)", R, K, d, (long)ldx);
  hipLaunchKernelGGL(km_accumulate_kernel, dim3(K), dim3(KT_THREADS), 0, s, reinterpret_cast<const h16*>(Xb), (long)ldx, code,
                     R, d, sums, cnt, state);
  return mms::check_launch("kmeans_accumulate");
}

extern "C" int mms2ut_kmeans_update(float* C, int64_t* counts, const float* sums, const int32_t* cnt, int K, int d, void* c_hi,
                                    void* c_lo, float* cnorm, int32_t* bad, const double* state, hipStream_t s) {
  MMS_REQUIRE(C && c_hi && c_lo && cnorm && bad, "kmeans_update: null buffer");
  MMS_REQUIRE((sums != nullptr) == (cnt != nullptr) && (cnt == nullptr || counts != nullptr),
              "kmeans_update: sums, cnt and counts go together");
  MMS_REQUIRE(K >= 1 && d >= 8 && d % 8 == 0, "kmeans_update: K %d, d %d (a multiple of 8)", K, d);
  hipLaunchKernelGGL(km_update_kernel, dim3(K), dim3(KT_THREADS), 0, s, C, reinterpret_cast<long long*>(counts), sums, cnt, d,
                     reinterpret_cast<h16*>(c_hi), reinterpret_cast<h16*>(c_lo), cnorm, bad, state);
  return mms::check_launch("kmeans_update");
}

extern "C" int mms2ut_kmeans_pp(const void* Xs, int n, int d, int K, int T, int first, const double* u, float* closest,
                                float* dist, double* partials, int32_t* cand, int32_t* chosen, hipStream_t s) {
  MMS_REQUIRE(Xs && closest && dist && partials && cand && chosen && aligned16(Xs), "kmeans_pp: null or misaligned buffer");
  MMS_REQUIRE(n >= 1 && K >= 1 && d >= 8 && d % 8 == 0, "kmeans_pp: n %d, K %d, d %d (a multiple of 8)", n, K, d);
  MMS_REQUIRE(T >= 1 && T <= KPP_MAX_T, "kmeans_pp: %d trials per centre (1 .. %d)", T, KPP_MAX_T);
  MMS_REQUIRE(first >= 0 && first < n && (K == 1 || u), "kmeans_pp: first row %d of %d, or no uniforms", first, n);
  const h16* X = reinterpret_cast<const h16*>(Xs);
  const int nblk = (n + KPP_ROWS - 1) / KPP_ROWS;
  hipLaunchKernelGGL(kpp_first_kernel, dim3(1), dim3(64), 0, s, cand, first);
  for (int c = 0; c < K; ++c) {
    const int Tc = c == 0 ? 1 : T;                        // centre 0 is given; the others have T candidates
    hipLaunchKernelGGL(kpp_dist_kernel, dim3(nblk), dim3(KT_THREADS), 0, s, X, n, d, cand, Tc,
                       c == 0 ? (const float*)nullptr : closest, dist, partials);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(KPP_PICK_THREADS), 0, s, partials, nblk, Tc, cand, dist, n, closest,
                       chosen, c, c + 1 < K ? u + (long)c * T : (const double*)nullptr, T);
  }
  return mms::check_launch("kmeans_pp");
}

extern "C" int mms2ut_kmeans_step(const mms2ut_kmeans_step_args* a, const int32_t* idx, hipStream_t s) {
  MMS_REQUIRE(a && idx, "kmeans_step: null arguments");
  MMS_REQUIRE(a->state && a->code && a->best && a->partials && a->bad && a->xnorm_b && a->pscore && a->pidx && a->chunk >= 1,
              "kmeans_step: null buffer");
  MMS_REQUIRE(a->alpha >= 0.0 && a->alpha <= 1.0, "kmeans_step: alpha %g outside [0, 1]", a->alpha);
  int rc = mms2ut_kmeans_gather(a->X, a->ldx, a->N, a->norms, idx, a->R, a->d, a->Xb, 0, a->xnorm_b, a->state, s);
  if (rc) return rc;
  rc = mms2ut_kmeans_assign(a->Xb, a->d, a->R, a->d, a->c_hi, a->c_lo, a->cnorm, a->K, a->chunk, a->pscore, a->pidx, s);
  if (rc) return rc;
  const int nchunks = (int)(((long)a->K + a->chunk - 1) / a->chunk);
  const int nparts = (a->R + KT_THREADS - 1) / KT_THREADS;
  hipLaunchKernelGGL(km_train_fold_kernel, dim3(nparts), dim3(KT_THREADS), 0, s, a->pscore, a->pidx, nchunks, a->R, a->xnorm_b,
                     a->code, a->best, a->partials, a->bad, a->state);
  rc = mms2ut_kmeans_accumulate(a->Xb, a->d, a->code, a->R, a->d, a->K, a->sums, a->cnt, a->state, s);
  if (rc) return rc;
  rc = mms2ut_kmeans_update(a->C, a->counts, a->sums, a->cnt, a->K, a->d, a->c_hi, a->c_lo, a->cnorm, a->bad, a->state, s);
  if (rc) return rc;
  // last: the step that meets the stopping rule still keeps its update, as in scikit-learn's loop
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(64), 0, s, a->partials, nparts, a->R, (double*)nullptr, a->state, a->alpha,
                     a->max_no_improvement);
  return mms::check_launch("kmeans_step");
}
