// wav2vec2 CTC transcription (forward only): the kernels in front of and behind the transformer body
// of multimodal-s2ut_amd/asr.py.  The body itself runs on the GEMM, LayerNorm and flash-attention
// kernels the training path already has.
//
// Activations are time-major fp16 rows [T, C], as in the vocoder (vocoder.hip).
//
//   wave_stats         mean and 1 / sqrt(var + eps) of one utterance: per-block partial sums in double,
//                      folded in block order by every reader (no atomics), two passes (the variance
//                      is the mean squared deviation, so a DC offset costs no precision).
//   asr_conv0          feature-extractor layer 0 in one launch: fp32 waveform in, normalised as it is
//                      read, Conv1d(1 -> C, k taps, stride s) + bias, LayerNorm over the C channels of
//                      each frame, GELU, fp16 [T0, C] out.  16 frames per block, one thread per channel
//                      pair; memory bound.
//   asr_conv           implicit-GEMM Conv1d with a stride and groups: the tile of conv1d_tm.h, which
//                      vocoder.hip's conv1d_tm_kernel runs too (one weight image, one tiling, one
//                      split of K over the waves when the grid is small).  The operand row of output q,
//                      tap j is input row stride * q + j - pad, read from the block's staged rows in
//                      LDS; the reduction runs over (tap, cin).  blockIdx.z is the group.  Epilogue:
//                      y = acc + bias (the extractor's layers 1..), y = GELU(acc + bias) (HuBERT's, which
//                      have no norm) or y = res + GELU(acc + bias) (the positional convolution: 128
//                      taps, 16 groups, K = 8192 per group).
//   asr_ln_gelu        in place over fp16 rows: GELU(LayerNorm(x)); one wave per row.  The extractor's
//                      LayerNorm spans all C output channels of a frame and a conv block owns 64 of
//                      them, so it runs as this row kernel behind the convolution.
//   ctc_greedy         one block per utterance: bias + per-frame argmax over the fp32 logits (lowest
//                      index on ties), then a block prefix sum compacts the ids that start a run and
//                      are not the blank.  Only ids, a count and a non-finite flag leave the device.
#include "conv1d_tm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// utterance statistics
// ---------------------------------------------------------------------------------------------
constexpr int AS_PARTS = MMS_ASR_STAT_PARTS;
constexpr int AS_THREADS = 256;

MMS_DEV double as_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

MMS_DEV double as_fold(const double* part) {
  double s = 0.0;
  for (int i = 0; i < AS_PARTS; ++i) s += part[i];
  return s;
}

// pass 0: ws[b] = sum of the block's slice.  pass 1: ws[AS_PARTS + b] = its sum of (x - mean)^2, the
// mean folded from pass 0's partials.
__global__ void __launch_bounds__(AS_THREADS) wave_stats_part_kernel(const float* __restrict__ x, long n, double* ws,
                                                                     int pass) {
  __shared__ double red[AS_THREADS / 64];
  const double mean = pass ? as_fold(ws) / (double)n : 0.0;
  const long per = (n + AS_PARTS - 1) / AS_PARTS;
  const long i0 = (long)blockIdx.x * per, i1 = min(n, i0 + per);
  double acc = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += AS_THREADS) {
    const double d = (double)x[i] - mean;
    acc += pass ? d * d : d;
  }
  acc = as_block_sum(acc, red);
  if (threadIdx.x == 0) ws[pass * AS_PARTS + blockIdx.x] = acc;
}

__global__ void wave_stats_fold_kernel(const double* __restrict__ ws, long n, float eps, float* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  const double mean = as_fold(ws) / (double)n, var = as_fold(ws + AS_PARTS) / (double)n;
  stats[0] = (float)mean;
  stats[1] = (float)(1.0 / sqrt(var + (double)eps));
}

// ---------------------------------------------------------------------------------------------
// layer 0: normalise, Conv1d(1 -> C), LayerNorm over C, GELU
// ---------------------------------------------------------------------------------------------
constexpr int A0_FR = 16;         // frames per block
constexpr int A0_THREADS = 256;
constexpr int A0_CPT = MMS_ASR_CONV0_MAX_C / A0_THREADS;      // channels per thread
constexpr int A0_MAX_K = MMS_ASR_CONV0_MAX_K, A0_MAX_S = MMS_ASR_CONV0_MAX_S;

__global__ void __launch_bounds__(A0_THREADS) asr_conv0_kernel(
    const float* __restrict__ x, long n, const float* __restrict__ stats, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps, int k,
    int s, int T0, int C, h16* __restrict__ y, long ldy) {
  __shared__ float xs[(A0_FR - 1) * A0_MAX_S + A0_MAX_K];
  __shared__ float red[A0_FR][A0_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int t0 = blockIdx.x * A0_FR;
  const int nx = (A0_FR - 1) * s + k;
  const float mean = stats[0], rstd = stats[1];
  for (int i = tid; i < nx; i += A0_THREADS) {
    const long src = (long)t0 * s + i;
    xs[i] = src < n ? (x[src] - mean) * rstd : 0.f;        // past the end: frames >= T0 only
  }
  __syncthreads();
  float v[A0_CPT][A0_FR];
#pragma unroll
  for (int u = 0; u < A0_CPT; ++u) {
    const int c = tid + u * A0_THREADS;
    const float b = c < C ? bias[c] : 0.f;
#pragma unroll
    for (int f = 0; f < A0_FR; ++f) v[u][f] = b;
    if (c < C) {
      for (int j = 0; j < k; ++j) {
        const float wv = w[j * C + c];
#pragma unroll
        for (int f = 0; f < A0_FR; ++f) v[u][f] += xs[f * s + j] * wv;
      }
    }
  }
  // LayerNorm over the channels of each frame: the mean, then the mean squared deviation
  float mu[A0_FR], rs[A0_FR];
#pragma unroll
  for (int f = 0; f < A0_FR; ++f) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < A0_CPT; ++u) t += v[u][f];          // channels >= C hold 0
    t = wave_sum(t);
    if ((tid & 63) == 0) red[f][wave] = t;
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < A0_FR; ++f) mu[f] = ((red[f][0] + red[f][1]) + (red[f][2] + red[f][3])) / (float)C;
  __syncthreads();
#pragma unroll
  for (int f = 0; f < A0_FR; ++f) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < A0_CPT; ++u) {
      const float d = tid + u * A0_THREADS < C ? v[u][f] - mu[f] : 0.f;
      t += d * d;
    }
    t = wave_sum(t);
    if ((tid & 63) == 0) red[f][wave] = t;
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < A0_FR; ++f)
    rs[f] = 1.f / sqrtf(((red[f][0] + red[f][1]) + (red[f][2] + red[f][3])) / (float)C + eps);
#pragma unroll
  for (int u = 0; u < A0_CPT; ++u) {
    const int c = tid + u * A0_THREADS;
    if (c >= C) continue;
    const float g = ln_g[c], be = ln_b[c];
#pragma unroll
    for (int f = 0; f < A0_FR; ++f) {
      const int t = t0 + f;
      if (t < T0) y[(long)t * ldy + c] = (h16)gelu_erf((v[u][f] - mu[f]) * rs[f] * g + be);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// strided / grouped implicit-GEMM Conv1d
// ---------------------------------------------------------------------------------------------
constexpr int AC_ROWS = MMS_ASR_CONV_MAX_ROWS;        // staged rows of a 128-position block
constexpr int AC_ROWS_SPLIT = AC_ROWS - 96;           // of a 32-position block: (32 - 128) * stride fewer, stride >= 1

// what conv1d_tm_tile needs of one group (blockIdx.z)
struct AsrConvView {
  const mms2ut_asr_conv_args& a;
  const h16* x;
  const h16* w;
  const float* bias;
  const h16* res;
  h16* y;
  const int T_in, nq;
  const long ldx;
  MMS_DEV AsrConvView(const mms2ut_asr_conv_args& a_, int grp)
      : a(a_), x(reinterpret_cast<const h16*>(a_.x) + (long)grp * a_.Cin),
        w(reinterpret_cast<const h16*>(a_.w) + (long)grp * a_.w_group),
        bias(a_.bias ? a_.bias + (long)grp * a_.Cout : nullptr),
        res(a_.res ? reinterpret_cast<const h16*>(a_.res) + (long)grp * a_.Cout : nullptr),
        y(reinterpret_cast<h16*>(a_.y) + (long)grp * a_.Cout), T_in(a_.T_in), nq(a_.T_out), ldx(a_.ldx) {}
  MMS_DEV int rows(int TM) const { return (TM - 1) * a.stride + a.taps; }  // <= the LDS rows (host check)
  MMS_DEV long row0(int q0) const { return (long)q0 * a.stride - a.pad; }
  MMS_DEV int lds_row(int p, int j) const { return p * a.stride + j; }
  MMS_DEV h16x8 stage(h16x8 v) const { return v; }
  MMS_DEV void emit(int q, int co, f32x4 v) const {
    if (res) {
      const h16x4 rv = *reinterpret_cast<const h16x4*>(res + (long)q * a.ldres + co);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)rv[e] + gelu_erf(v[e]);
    } else if (a.gelu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
    }
    conv_store4(y + (long)q * a.ldy + co, v);
  }
};

template <bool SPLITK>
__global__ void __launch_bounds__(CT_THREADS) asr_conv_kernel(const mms2ut_asr_conv_args a) {
  __shared__ __attribute__((aligned(16))) h16 xs[(SPLITK ? AC_ROWS_SPLIT : AC_ROWS) * CT_LD];
  __shared__ f32x4 red[conv_red_elems(SPLITK)];
  conv1d_tm_tile<SPLITK>(AsrConvView(a, blockIdx.z), a.Cin, a.Cout, a.taps, xs, red);
}

// ---------------------------------------------------------------------------------------------
// GELU(LayerNorm(row)) in place: one wave per row, a lane holds up to two 16-byte pieces
// ---------------------------------------------------------------------------------------------
constexpr int AL_MAX_C = MMS_ASR_LN_MAX_C;
constexpr int AL_PIECES = AL_MAX_C / 8 / 64;

__global__ void __launch_bounds__(256) asr_ln_gelu_kernel(h16* __restrict__ x, long ld, int T, int C,
                                                          const float* __restrict__ g, const float* __restrict__ b,
                                                          float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= T) return;                                   // wave-uniform
  const int nv = C >> 3;
  h16* xr = x + (long)row * ld;
  float v[AL_PIECES][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < AL_PIECES; ++u) {
    const int i = lane + u * 64;
    h16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nv) h = *reinterpret_cast<const h16x8*>(xr + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[u][e] = (float)h[e];
      s += v[u][e];
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int u = 0; u < AL_PIECES; ++u)
    if (lane + u * 64 < nv) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[u][e] - mean;
        sq += d * d;
      }
    }
  const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
  for (int u = 0; u < AL_PIECES; ++u) {
    const int i = lane + u * 64;
    if (i >= nv) continue;
    h16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (h16)gelu_erf((v[u][e] - mean) * rstd * g[i * 8 + e] + b[i * 8 + e]);
    *reinterpret_cast<h16x8*>(xr + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// CTC greedy: argmax per frame, then compaction of the run starts that are not the blank
// ---------------------------------------------------------------------------------------------
constexpr int CG_THREADS = 256;

__global__ void __launch_bounds__(CG_THREADS) ctc_greedy_kernel(
    float* __restrict__ logits, long ld, int V, int Tmax, const int* __restrict__ lens, const float* __restrict__ bias,
    int blank, int* ids, int* __restrict__ out, int* __restrict__ count, int* __restrict__ bad) {
  __shared__ int wtot[CG_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int T = lens ? min(max(lens[b], 0), Tmax) : Tmax;
  float* L = logits + (long)b * Tmax * ld;
  int* idb = ids + (long)b * Tmax;
  int* ob = out + (long)b * Tmax;
  int notfin = 0;
  for (int t = tid; t < T; t += CG_THREADS) {
    float* r = L + (long)t * ld;
    float best = -INFINITY;
    int bi = 0;
    for (int v = 0; v < V; ++v) {
      float z = r[v];
      if (bias) {
        z += bias[v];
        r[v] = z;
      }
      if (!isfinite(z)) notfin = 1;
      if (z > best) {                                     // strict: the lowest index wins a tie
        best = z;
        bi = v;
      }
    }
    idb[t] = bi;
  }
  notfin = __syncthreads_or(notfin);                      // also orders the ids written above for the block
  if (tid == 0) bad[b] = notfin;
  int base = 0;
  for (int c0 = 0; c0 < T; c0 += CG_THREADS) {
    const int t = c0 + tid;
    int id = blank;
    bool keep = false;
    if (t < T) {
      id = idb[t];
      keep = id != blank && (t == 0 || id != idb[t - 1]);
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
    for (int i = 0; i < CG_THREADS / 64; ++i) {
      if (i < wave) woff += wtot[i];
      total += wtot[i];
    }
    if (keep) ob[base + woff + inc - 1] = id;
    base += total;
    __syncthreads();                                      // wtot is rewritten by the next chunk
  }
  if (tid == 0) count[b] = base;
}

}  // namespace

extern "C" int mms2ut_wave_stats(const float* x, int64_t n, float eps, double* ws, float* stats, hipStream_t s) {
  MMS_REQUIRE(x && ws && stats && n >= 1, "wave_stats: null buffer or empty waveform");
  MMS_REQUIRE(eps >= 0.f, "wave_stats: eps must be >= 0");
  for (int pass = 0; pass < 2; ++pass)
    hipLaunchKernelGGL(wave_stats_part_kernel, dim3(AS_PARTS), dim3(AS_THREADS), 0, s, x, (long)n, ws, pass);
  hipLaunchKernelGGL(wave_stats_fold_kernel, dim3(1), dim3(64), 0, s, ws, (long)n, eps, stats);
  return mms::check_launch("wave_stats");
}

extern "C" int mms2ut_asr_conv0(const float* x, int64_t n, const float* stats, const float* w, const float* bias,
                                const float* ln_g, const float* ln_b, float eps, int k, int stride, int C, void* y,
                                int64_t ldy, hipStream_t s) {
  MMS_REQUIRE(x && stats && w && bias && ln_g && ln_b && y, "asr_conv0: null buffer");
  MMS_REQUIRE(k >= 1 && k <= A0_MAX_K && stride >= 1 && stride <= A0_MAX_S,
              "asr_conv0: kernel size must be in [1, %d] and stride in [1, %d] (got %d, %d)", A0_MAX_K, A0_MAX_S, k, stride);
  MMS_REQUIRE(C >= 1 && C <= MMS_ASR_CONV0_MAX_C && ldy >= C, "asr_conv0: channels must be in [1, %d] (got %d)",
              MMS_ASR_CONV0_MAX_C, C);
  MMS_REQUIRE(n >= k && (n - k) / stride + 1 < (1L << 31), "asr_conv0: %ld samples for a kernel of %d", (long)n, k);
  const int T0 = (int)((n - k) / stride + 1);
  hipLaunchKernelGGL(asr_conv0_kernel, dim3((T0 + A0_FR - 1) / A0_FR), dim3(A0_THREADS), 0, s, x, (long)n, stats, w, bias,
                     ln_g, ln_b, eps, k, stride, T0, C, reinterpret_cast<h16*>(y), (long)ldy);
  return mms::check_launch("asr_conv0");
}

extern "C" int mms2ut_asr_conv(const mms2ut_asr_conv_args* a, hipStream_t s) {
  MMS_REQUIRE(a, "asr_conv: null args");
  const long wx = (long)a->groups * a->Cin, wy = (long)a->groups * a->Cout;
  if (int rc = conv_check("asr_conv", " per group", a->Cin, a->Cout, a->x, a->ldx, wx, a->w, a->bias, a->y, a->ldy,
                          a->res, a->ldres, wy))
    return rc;
  MMS_REQUIRE(a->taps >= 1 && a->stride >= 1 && a->pad >= 0 && a->groups >= 1 && a->groups <= 65535,
              "asr_conv: taps, stride, groups >= 1 and pad >= 0");
  MMS_REQUIRE(127L * a->stride + a->taps <= AC_ROWS, "asr_conv: 127 * stride + taps must be at most %d (stride %d, taps %d)",
              AC_ROWS, a->stride, a->taps);
  MMS_REQUIRE(a->T_in >= 1 && a->T_out >= 1, "asr_conv: empty problem");
  // every output reads rows inside [-pad, T_in + pad): nothing but the padding is made up
  MMS_REQUIRE((long)(a->T_out - 1) * a->stride + a->taps <= (long)a->T_in + 2L * a->pad,
              "asr_conv: %d outputs need more than the %d input rows and padding %d", a->T_out, a->T_in, a->pad);
  MMS_REQUIRE(a->w_group % 8 == 0, "asr_conv: misaligned buffer");
  conv_tm_launch(asr_conv_kernel<true>, asr_conv_kernel<false>, *a, a->Cin, a->Cout, a->taps, a->T_out, a->groups, s);
  return mms::check_launch("asr_conv");
}

extern "C" int mms2ut_asr_ln_gelu(void* x, int64_t ld, int T, int C, const float* g, const float* b, float eps,
                                  hipStream_t s) {
  MMS_REQUIRE(x && g && b && T >= 1, "asr_ln_gelu: null buffer or no rows");
  MMS_REQUIRE(C >= 8 && C % 8 == 0 && C <= AL_MAX_C && ld >= C && ld % 8 == 0 && ((uintptr_t)x & 15) == 0,
              "asr_ln_gelu: C must be a multiple of 8 in [8, %d] with 16-byte aligned rows (C %d)", AL_MAX_C, C);
  hipLaunchKernelGGL(asr_ln_gelu_kernel, dim3((T + 3) / 4), dim3(256), 0, s, reinterpret_cast<h16*>(x), (long)ld, T, C, g,
                     b, eps);
  return mms::check_launch("asr_ln_gelu");
}

extern "C" int mms2ut_ctc_greedy(float* logits, int64_t ld, int V, int B, int Tmax, const int32_t* lens,
                                 const float* bias, int blank, int32_t* ids, int32_t* out, int32_t* count,
                                 int32_t* bad, hipStream_t s) {
  MMS_REQUIRE(logits && ids && out && count && bad, "ctc_greedy: null buffer");
  MMS_REQUIRE(V >= 1 && ld >= V && B >= 1 && B <= 65535 && Tmax >= 1, "ctc_greedy: V %d, ld %ld, B %d, Tmax %d", V,
              (long)ld, B, Tmax);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(CG_THREADS), 0, s, logits, (long)ld, V, Tmax, lens, bias, blank, ids,
                     out, count, bad);
  return mms::check_launch("ctc_greedy");
}
