// Unit vocoder (CodeHiFiGAN, forward only): the kernels behind multimodal-s2ut_amd/vocoder.py.
//
// Activations are time-major fp16 rows [T, C].  A convolution tap is then a row-shifted read and the
// GEMM reduction runs over (tap, cin); there is no im2col image anywhere.
//
//   conv1d_tm_kernel   implicit-GEMM Conv1d with a dilation: the tile of conv1d_tm.h (128 output
//                      positions, or 32 where the waves split K, x up to 64 output channels) over the
//                      staged rows [q0 - pad, q0 - pad + positions + (taps-1)*dil), input leaky-ReLU
//                      applied on the way into LDS; output q reads tap j at row q + j*dil.  Epilogue
//                      in the same launch: + bias, + residual row, leaky-ReLU, y = scale * v or
//                      y += scale * v.
//   the same kernel    runs ConvTranspose1d as a polyphase convolution: output phase r = (t' + p)
//                      mod u is an ordinary convolution over ceil(k/u) taps with its own weight
//                      image (blockIdx.z = r) whose output rows are q*u + r - p.
//   conv_post_tanh     Cout = 1: one thread per sample, fp32 weights in LDS, tanh, fp32 output.
//   embed_repeat       out[t'] = dict[codes[src(t')]], src from the inclusive prefix sum of the
//                      durations (binary search), or src = t' without durations.
//   var_pred_layer     one layer of the duration predictor, all fp32: Conv1d + ReLU + LayerNorm,
//                      and on the last layer the projection, exp, round-half-even and clamp.
#include "conv1d_tm.h"

namespace {

constexpr int VC_HALO = MMS_VOC_MAX_SPAN;

MMS_DEV h16x8 lrelu8(h16x8 v, float slope) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = (float)v[e];
    v[e] = (h16)(f > 0.f ? f : f * slope);
  }
  return v;
}

// what conv1d_tm_tile needs of one output phase (blockIdx.z)
struct VocConvView {
  const mms2ut_conv1d_tm_args& a;
  const int phase;
  const h16* x;
  const h16* w;
  const float* bias;
  const int T_in, nq;
  const long ldx;
  MMS_DEV VocConvView(const mms2ut_conv1d_tm_args& a_, int z)
      : a(a_), phase(z), x(reinterpret_cast<const h16*>(a_.x)),
        w(reinterpret_cast<const h16*>(a_.w) + (long)z * a_.w_phase), bias(a_.bias), T_in(a_.T_in), nq(a_.nq),
        ldx(a_.ldx) {}
  MMS_DEV int rows(int TM) const { return TM + (a.taps - 1) * a.dil; }     // <= TM + VC_HALO (host check)
  MMS_DEV int row0(int q0) const { return q0 - a.pad; }
  MMS_DEV int lds_row(int p, int j) const { return p + j * a.dil; }
  MMS_DEV h16x8 stage(h16x8 v) const { return a.in_act ? lrelu8(v, a.in_slope) : v; }
  MMS_DEV void emit(int q, int co, f32x4 v) const {
    const long orow = (long)q * a.ostride + phase + a.ooff;
    if (orow < 0 || orow >= a.T_out) return;
    const h16* __restrict__ res = reinterpret_cast<const h16*>(a.res);
    if (res) {
      const h16x4 rv = *reinterpret_cast<const h16x4*>(res + orow * a.ldres + co);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
    }
    if (a.out_act) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.out_slope;
    }
    h16* yp = reinterpret_cast<h16*>(a.y) + orow * a.ldy + co;
    if (a.acc != MMS_VOC_ACC_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= a.scale;
      if (a.acc == MMS_VOC_ACC_ADD) {
        const h16x4 pv = *reinterpret_cast<const h16x4*>(yp);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)pv[e];
      }
    }
    conv_store4(yp, v);
  }
};

template <bool SPLITK>
__global__ void __launch_bounds__(CT_THREADS) conv1d_tm_kernel(const mms2ut_conv1d_tm_args a) {
  __shared__ __attribute__((aligned(16))) h16 xs[(conv_tile_positions(SPLITK) + VC_HALO) * CT_LD];
  __shared__ f32x4 red[conv_red_elems(SPLITK)];
  conv1d_tm_tile<SPLITK>(VocConvView(a, blockIdx.z), a.Cin, a.Cout, a.taps, xs, red);
}

int conv_launch(const mms2ut_conv1d_tm_args& a, const char* what, hipStream_t s) {
  if (int rc = conv_check(what, "", a.Cin, a.Cout, a.x, a.ldx, a.Cin, a.w, a.bias, a.y, a.ldy, a.res, a.ldres, a.Cout))
    return rc;
  MMS_REQUIRE(a.taps >= 1 && a.dil >= 1 && (long)(a.taps - 1) * a.dil <= VC_HALO,
              "%s: (taps - 1) * dilation must be in [0, %d] (taps %d, dilation %d)", what, VC_HALO, a.taps, a.dil);
  MMS_REQUIRE(a.T_in >= 1 && a.T_out >= 1 && a.nq >= 1 && a.phases >= 1 && a.ostride >= 1, "%s: empty problem", what);
  MMS_REQUIRE(a.acc >= MMS_VOC_ACC_NONE && a.acc <= MMS_VOC_ACC_ADD, "%s: acc mode %d", what, a.acc);
  MMS_REQUIRE(a.phases <= 65535, "%s: grid too large", what);
  conv_tm_launch(conv1d_tm_kernel<true>, conv1d_tm_kernel<false>, a, a.Cin, a.Cout, a.taps, a.nq, a.phases, s);
  return mms::check_launch(what);
}

// ---------------------------------------------------------------------------------------------
// conv_post + tanh: y[t] = tanh(b + sum_{j, ci} lrelu(x[t + j - pad, ci]) w[j, ci])
// ---------------------------------------------------------------------------------------------
constexpr int VP_THREADS = 256;
constexpr int VP_MAX_W = 2048;    // taps * Cin fp32 weights in LDS

__global__ void __launch_bounds__(VP_THREADS) conv_post_tanh_kernel(
    const h16* __restrict__ x, long ldx, int T, int Cin, const float* __restrict__ w, float bias, int taps, int pad,
    float slope, float* __restrict__ y) {
  __shared__ float ws[VP_MAX_W];
  for (int i = threadIdx.x; i < taps * Cin; i += VP_THREADS) ws[i] = w[i];
  __syncthreads();
  const int t = blockIdx.x * VP_THREADS + threadIdx.x;
  if (t >= T) return;
  float s = bias;
  for (int j = 0; j < taps; ++j) {
    const int row = t + j - pad;
    if (row < 0 || row >= T) continue;
    const h16* xr = x + (long)row * ldx;
    const float* wr = ws + j * Cin;
    for (int c = 0; c < Cin; c += 8) {
      const h16x8 v = *reinterpret_cast<const h16x8*>(xr + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        s += (f > 0.f ? f : f * slope) * wr[c + e];
      }
    }
  }
  y[t] = tanhf(s);
}

// ---------------------------------------------------------------------------------------------
// embedding gather + duration repeat: 16-byte units, one per thread
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) embed_repeat_kernel(
    const h16* __restrict__ dict, int n_embed, int D, const int64_t* __restrict__ codes, int T,
    const int64_t* __restrict__ cum, long T_out, h16* __restrict__ out) {
  const int dv = D >> 3;
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= T_out * dv) return;
  const long t = u / dv;
  const int c = (int)(u - t * dv) * 8;
  long src = t;
  if (cum) {                                              // first i with cum[i] > t
    int lo = 0, hi = T - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    src = lo;
  }
  h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (src < T) {
    const int64_t code = codes[src];
    if (code >= 0 && code < n_embed) v = *reinterpret_cast<const h16x8*>(dict + code * D + c);
  }
  *reinterpret_cast<h16x8*>(out + t * D + c) = v;
}

// ---------------------------------------------------------------------------------------------
// duration predictor layer, fp32 throughout: VR_FR frames per block, one thread per channel
// ---------------------------------------------------------------------------------------------
constexpr int VR_FR = 4;
constexpr int VR_THREADS = 256;
constexpr int VR_MAX_IN = 4096;   // (VR_FR + taps - 1) * Cin floats of input rows in LDS

MMS_DEV float vr_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VR_THREADS / 64; ++i) s += red[i];
  return s;
}

__global__ void __launch_bounds__(VR_THREADS) var_pred_layer_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ idx, int n_rows, int T, int Cin,
    const float* __restrict__ w, const float* __restrict__ b, int taps, int pad, int Cout,
    const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps, float* __restrict__ out,
    const float* __restrict__ proj_w, float proj_b, float* __restrict__ logd, int32_t* __restrict__ dur) {
  __shared__ float xin[VR_MAX_IN];
  __shared__ float red[VR_THREADS / 64];
  const int t0 = blockIdx.x * VR_FR, co = threadIdx.x;
  const int nrow = VR_FR + taps - 1;
  for (int i = threadIdx.x; i < nrow * Cin; i += VR_THREADS) {
    const int rr = i / Cin, c = i - rr * Cin;
    const int row = t0 + rr - pad;
    float v = 0.f;
    if (row >= 0 && row < T) {
      long src = row;
      if (idx) { src = idx[row]; if (src < 0 || src >= n_rows) src = -1; }
      if (src >= 0) v = x[src * Cin + c];
    }
    xin[i] = v;
  }
  __syncthreads();
  float acc[VR_FR];
#pragma unroll
  for (int f = 0; f < VR_FR; ++f) acc[f] = 0.f;
  if (co < Cout) {
    const float bb = b[co];
#pragma unroll
    for (int f = 0; f < VR_FR; ++f) acc[f] = bb;
    for (int j = 0; j < taps; ++j)
      for (int c = 0; c < Cin; ++c) {
        const float wv = w[((long)j * Cin + c) * Cout + co];
#pragma unroll
        for (int f = 0; f < VR_FR; ++f) acc[f] += xin[(f + j) * Cin + c] * wv;
      }
#pragma unroll
    for (int f = 0; f < VR_FR; ++f) acc[f] = fmaxf(acc[f], 0.f);
  }
#pragma unroll
  for (int f = 0; f < VR_FR; ++f) {                       // uniform trip count: block reductions inside
    const float mean = vr_block_sum(co < Cout ? acc[f] : 0.f, red) / (float)Cout;
    const float d = co < Cout ? acc[f] - mean : 0.f;
    const float var = vr_block_sum(d * d, red) / (float)Cout;
    const float h = co < Cout ? d * rsqrtf(var + eps) * ln_g[co] + ln_b[co] : 0.f;
    const int t = t0 + f;
    if (proj_w) {
      const float p = vr_block_sum(co < Cout ? h * proj_w[co] : 0.f, red) + proj_b;
      if (threadIdx.x == 0 && t < T) {
        logd[t] = p;
        dur[t] = (int32_t)fmaxf(rintf(expf(p) - 1.f), 1.f);
      }
    } else if (co < Cout && t < T) {
      out[(long)t * Cout + co] = h;
    }
  }
}

}  // namespace

extern "C" int mms2ut_conv1d_tm_packed_halves(int Cin, int Cout, int taps, int64_t* out) {
  MMS_REQUIRE(out && Cin >= 8 && Cin % 8 == 0 && Cout >= 8 && Cout % 8 == 0 && taps >= 1,
              "conv1d_tm_packed_halves: channel widths must be multiples of 8 and >= 8 (Cin %d, Cout %d), taps >= 1",
              Cin, Cout);
  *out = conv_ksteps(Cin, taps) * ((Cout + 15) & ~15) * 32;
  return 0;
}

extern "C" int mms2ut_conv1d_tm(const mms2ut_conv1d_tm_args* a, hipStream_t s) {
  MMS_REQUIRE(a, "conv1d_tm: null args");
  MMS_REQUIRE(a->phases == 1 && a->ostride == 1 && a->ooff == 0 && a->nq == a->T_out,
              "conv1d_tm: a plain convolution has one phase and nq == T_out");
  return conv_launch(*a, "conv1d_tm", s);
}

extern "C" int mms2ut_conv_transpose1d_tm(const void* x, int64_t ldx, int T, int Cin, const void* w_packed,
                                          const float* bias, void* y, int64_t ldy, int Cout, int k, int stride,
                                          int padding, int in_act, float in_slope, hipStream_t s) {
  MMS_REQUIRE(T >= 1 && k >= 1 && stride >= 1 && padding >= 0, "conv_transpose1d_tm: T, k, stride >= 1 and padding >= 0");
  const long T_out = (long)(T - 1) * stride - 2L * padding + k;
  MMS_REQUIRE(T_out >= 1 && T_out < (1L << 31), "conv_transpose1d_tm: output length %ld", T_out);
  mms2ut_conv1d_tm_args a = {};
  a.x = x; a.ldx = ldx; a.T_in = T; a.Cin = Cin;
  a.w = w_packed; a.bias = bias;
  a.y = y; a.ldy = ldy; a.T_out = (int)T_out; a.Cout = Cout;
  a.taps = (k + stride - 1) / stride;                     // taps of one output phase, stored reversed
  a.dil = 1;
  a.pad = a.taps - 1;
  a.nq = T + a.taps - 1;
  a.phases = stride; a.ostride = stride; a.ooff = -padding;
  a.in_act = in_act; a.in_slope = in_slope;
  a.acc = MMS_VOC_ACC_NONE; a.scale = 1.f;
  int64_t per_phase = 0;
  if (int rc = mms2ut_conv1d_tm_packed_halves(Cin, Cout, a.taps, &per_phase)) return rc;
  a.w_phase = per_phase;
  return conv_launch(a, "conv_transpose1d_tm", s);
}

extern "C" int mms2ut_conv_post_tanh(const void* x, int64_t ldx, int T, int Cin, const float* w, float bias,
                                     int taps, int pad, float in_slope, float* y, hipStream_t s) {
  MMS_REQUIRE(x && w && y && T >= 1, "conv_post_tanh: null buffer or empty input");
  MMS_REQUIRE(Cin >= 8 && Cin % 8 == 0 && ldx >= Cin && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0,
              "conv_post_tanh: Cin must be a multiple of 8 and >= 8 with 16-byte aligned rows (Cin %d)", Cin);
  MMS_REQUIRE(taps >= 1 && pad >= 0 && (long)taps * Cin <= VP_MAX_W, "conv_post_tanh: taps * Cin must be in [1, %d]", VP_MAX_W);
  hipLaunchKernelGGL(conv_post_tanh_kernel, dim3((T + VP_THREADS - 1) / VP_THREADS), dim3(VP_THREADS), 0, s,
                     reinterpret_cast<const h16*>(x), (long)ldx, T, Cin, w, bias, taps, pad, in_slope, y);
  return mms::check_launch("conv_post_tanh");
}

extern "C" int mms2ut_embed_repeat(const void* dict, int n_embed, int D, const int64_t* codes, int T,
                                   const int64_t* cum, int64_t T_out, void* out, hipStream_t s) {
  MMS_REQUIRE(dict && codes && out && T >= 1 && T_out >= 1 && n_embed >= 1, "embed_repeat: null buffer or empty input");
  MMS_REQUIRE(D >= 8 && D % 8 == 0 && ((uintptr_t)dict & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "embed_repeat: D must be a multiple of 8 and >= 8 with 16-byte aligned rows (D %d)", D);
  MMS_REQUIRE(cum || T_out == T, "embed_repeat: without durations T_out must equal T");
  const int64_t units = T_out * (D >> 3);
  MMS_REQUIRE((units + 255) / 256 < (1L << 31), "embed_repeat: output too large");
  hipLaunchKernelGGL(embed_repeat_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const h16*>(dict), n_embed, D, codes, T, cum, (long)T_out,
                     reinterpret_cast<h16*>(out));
  return mms::check_launch("embed_repeat");
}

extern "C" int mms2ut_var_pred_layer_f32(const float* x, const int64_t* idx, int n_rows, int T, int Cin,
                                         const float* w, const float* b, int taps, int pad, int Cout,
                                         const float* ln_g, const float* ln_b, float eps, float* out,
                                         const float* proj_w, float proj_b, float* logd, int32_t* dur,
                                         hipStream_t s) {
  MMS_REQUIRE(x && w && b && ln_g && ln_b && T >= 1 && n_rows >= 1, "var_pred_layer: null buffer or empty input");
  MMS_REQUIRE(Cout >= 1 && Cout <= VR_THREADS, "var_pred_layer: hidden width must be in [1, %d] (got %d)", VR_THREADS, Cout);
  MMS_REQUIRE(taps >= 1 && pad >= 0 && Cin >= 1 && (long)(VR_FR + taps - 1) * Cin <= VR_MAX_IN,
              "var_pred_layer: (%d + taps - 1) * Cin must be at most %d (taps %d, Cin %d)", VR_FR, VR_MAX_IN, taps, Cin);
  MMS_REQUIRE(proj_w ? (logd && dur) : (out != nullptr), "var_pred_layer: output buffer missing");
  hipLaunchKernelGGL(var_pred_layer_kernel, dim3((T + VR_FR - 1) / VR_FR), dim3(VR_THREADS), 0, s, x, idx, n_rows, T,
                     Cin, w, b, taps, pad, Cout, ln_g, ln_b, eps, out, proj_w, proj_b, logd, dur);
  return mms::check_launch("var_pred_layer");
}

// ---------------------------------------------------------------------------------------------
// the whole generator: the same launches through the same launchers, issued from here
// ---------------------------------------------------------------------------------------------
namespace {

struct VocPlan {
  int64_t T[MMS_VOC_MAX_STAGES + 1];      // rows entering stage i; T[n_stages] = samples
  int ch[MMS_VOC_MAX_STAGES + 1];         // channels entering stage i
  int64_t slot;                           // halves per workspace slot (a multiple of 8)
};
constexpr int VOC_SLOTS = 5;              // X (upsampled), XS (stage sum), TT (conv1 out), H0, H1

int voc_plan(const mms2ut_hifigan* m, int64_t T_frames, VocPlan& p) {
  MMS_REQUIRE(m, "hifigan: null model");
  MMS_REQUIRE(m->n_stages >= 1 && m->n_stages <= MMS_VOC_MAX_STAGES && m->nk >= 1 && m->nk <= MMS_VOC_MAX_RESBLOCKS,
              "hifigan: %d stages / %d ResBlocks per stage (at most %d / %d)", m->n_stages, m->nk, MMS_VOC_MAX_STAGES,
              MMS_VOC_MAX_RESBLOCKS);
  MMS_REQUIRE(T_frames >= 1 && T_frames < (1L << 31), "hifigan: %ld frames", (long)T_frames);
  MMS_REQUIRE(m->pre.k % 2 == 1 && m->post_k % 2 == 1, "hifigan: conv_pre / conv_post kernel sizes must be odd");
  p.T[0] = T_frames;
  p.ch[0] = m->C0;
  int64_t slot = T_frames * (m->C0 > m->D ? m->C0 : m->D);
  for (int i = 0; i < m->n_stages; ++i) {
    const mms2ut_voc_up& u = m->ups[i];
    MMS_REQUIRE(u.k >= u.u && u.u >= 1, "hifigan: ups[%d] kernel %d / stride %d", i, u.k, u.u);
    p.T[i + 1] = (p.T[i] - 1) * u.u - 2 * ((u.k - u.u) / 2) + u.k;
    p.ch[i + 1] = u.cout;
    MMS_REQUIRE(p.T[i + 1] >= 1 && p.T[i + 1] < (1L << 31), "hifigan: stage %d length %ld", i, (long)p.T[i + 1]);
    slot = slot > p.T[i + 1] * u.cout ? slot : p.T[i + 1] * u.cout;
    for (int j = 0; j < m->nk; ++j) {
      MMS_REQUIRE(m->nd[j] >= 1 && m->nd[j] <= MMS_VOC_MAX_DILS, "hifigan: ResBlock %d has %d dilations (1 .. %d)", j,
                  m->nd[j], MMS_VOC_MAX_DILS);
      for (int d = 0; d < m->nd[j]; ++d)
        MMS_REQUIRE(m->c1[i][j][d].k % 2 == 1 && m->c2[i][j][d].k % 2 == 1, "hifigan: ResBlock kernel sizes must be odd");
    }
  }
  p.slot = (slot + 7) & ~(int64_t)7;
  return 0;
}

int voc_conv(const mms2ut_voc_conv& c, const h16* x, int64_t T, int Cin, int Cout, h16* y, int in_act, float in_slope,
             const h16* res, int acc, float scale, int out_act, float out_slope, hipStream_t s) {
  mms2ut_conv1d_tm_args a = {};
  a.x = x; a.ldx = Cin; a.T_in = (int)T; a.Cin = Cin;
  a.w = c.w; a.bias = c.b;
  a.y = y; a.ldy = Cout; a.T_out = (int)T; a.Cout = Cout;
  a.taps = c.k; a.dil = c.dil; a.pad = c.dil * (c.k - 1) / 2;
  a.nq = (int)T; a.phases = 1; a.ostride = 1; a.ooff = 0;
  a.in_act = in_act; a.in_slope = in_slope;
  a.res = res; a.ldres = Cout;
  a.acc = acc; a.scale = scale;
  a.out_act = out_act; a.out_slope = out_slope;
  return mms2ut_conv1d_tm(&a, s);
}

}  // namespace

extern "C" int mms2ut_hifigan_sizes(const mms2ut_hifigan* m, int64_t T_frames, int64_t* ws_halves, int64_t* T_wave) {
  VocPlan p;
  if (int rc = voc_plan(m, T_frames, p)) return rc;
  if (ws_halves) *ws_halves = VOC_SLOTS * p.slot;
  if (T_wave) *T_wave = p.T[m->n_stages];
  return 0;
}

extern "C" int mms2ut_hifigan_fwd(const mms2ut_hifigan* m, const int64_t* codes, int T, const int64_t* cum,
                                  int64_t T_frames, void* ws, float* wave, int* launches, hipStream_t s) {
  VocPlan p;
  if (int rc = voc_plan(m, T_frames, p)) return rc;
  MMS_REQUIRE(ws && wave && codes && ((uintptr_t)ws & 15) == 0, "hifigan_fwd: null or misaligned buffer");
  h16* X = reinterpret_cast<h16*>(ws);
  h16 *XS = X + p.slot, *TT = X + 2 * p.slot, *H[2] = {X + 3 * p.slot, X + 4 * p.slot};
  int n = 0;
  if (int rc = mms2ut_embed_repeat(m->dict, m->n_embed, m->D, codes, T, cum, T_frames, X, s)) return rc;
  if (int rc = voc_conv(m->pre, X, T_frames, m->D, m->C0, XS, 0, 0.f, nullptr, MMS_VOC_ACC_NONE, 1.f, 0, 0.f, s)) return rc;
  n += 2;
  const float inv_nk = 1.0f / (float)m->nk;
  for (int i = 0; i < m->n_stages; ++i) {
    const mms2ut_voc_up& u = m->ups[i];
    const int ch = u.cout;
    const int64_t Ti = p.T[i + 1];
    if (int rc = mms2ut_conv_transpose1d_tm(XS, p.ch[i], (int)p.T[i], p.ch[i], u.w, u.b, X, ch, ch, u.k, u.u,
                                            (u.k - u.u) / 2, 1, m->slope, s))
      return rc;
    ++n;
    for (int j = 0; j < m->nk; ++j) {
      const h16* h = X;
      for (int d = 0; d < m->nd[j]; ++d) {
        if (int rc = voc_conv(m->c1[i][j][d], h, Ti, ch, ch, TT, 1, m->slope, nullptr, MMS_VOC_ACC_NONE, 1.f, 1, m->slope, s))
          return rc;
        const bool last = d + 1 == m->nd[j];
        h16* out = last ? XS : H[d & 1];
        const int acc = last ? (j == 0 ? MMS_VOC_ACC_SET : MMS_VOC_ACC_ADD) : MMS_VOC_ACC_NONE;
        if (int rc = voc_conv(m->c2[i][j][d], TT, Ti, ch, ch, out, 0, 0.f, h, acc, last ? inv_nk : 1.f, 0, 0.f, s)) return rc;
        h = out;
        n += 2;
      }
    }
  }
  const int L = m->n_stages;
  if (int rc = mms2ut_conv_post_tanh(XS, p.ch[L], (int)p.T[L], p.ch[L], m->post_w, m->post_b, m->post_k,
                                     (m->post_k - 1) / 2, m->post_slope, wave, s))
    return rc;
  if (launches) *launches = n + 1;
  return 0;
}
