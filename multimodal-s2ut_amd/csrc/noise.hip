// Noise augmentation (--noise-config-yaml) on the waveform batch in HBM, in front of the fbank kernel:
// the reference's per-utterance CPU mix (mm_s2ut/data/audio_utils.py:27-42 select_noise, :161-233
// add_noise_v2 with normalize=True, called from speech_to_speech_dataset.py:217-240) as three short
// memory-bound launches over grid (B, MMS_NOISE_SPLIT): block (b, s) owns the s-th slice of
// utterance b, the pattern of the CMVN kernels in fbank.hip.
//
//   1. noise_partial_kernel: fp64 slice partials of sum|x| and sum|seg|.  The addends are multiples
//      of 2^-15 below 1 and an utterance has far fewer than 2^20 samples, so the fp64 sums are exact
//      and do not depend on order, slice count or alignment.
//   2. noise_mix_kernel: every block folds its utterance's partials in slice order, forms the two
//      amplitudes and the noise gain in fp32 exactly as torch does (one rounding per operation, see
//      the contraction pragma below), writes y = x (1 - f) + seg g in place and keeps the slice's
//      max|y|.
//   3. noise_norm_kernel: folds the maxima, writes y / max(max|y|, 1) x 2^15 (a true division).
//
// The wave batch is stored x 2^15 (manifest.read_wav) and the reference mixes samples in [-1, 1):
// both scalings are exact in fp32.  The noise bank is int16 in HBM, converted on load.  With
// n_mix > 1 the noise sample is floor(mean of the clips' samples): -1 where the integer sum of the
// samples is negative, else 0.  Utterances with apply == 0 are never touched.  No float
// atomics anywhere: results are bitwise reproducible and independent of an utterance's placement.
#include "common.h"
#include "../../include/mms2ut.h"

// The reference multiplies and adds in separate in-place steps, so every operation is rounded on
// its own.  hipcc's default (-ffp-contract=fast-honor-pragmas) fuses a*b + c into an FMA, and the
// HIP headers define __fmul_rn / __fadd_rn as plain * and + compiled under that default, so they are
// fused all the same once inlined (seen in the ISA).  Contraction is switched off for this whole
// file and the arithmetic is written with its own one-operation helpers; a / b is IEEE-rounded
// (hipcc's default, no fast-math in this build).
#pragma clang fp contract(off)

namespace {

MMS_DEV float nz_mul(float a, float b) { return a * b; }
MMS_DEV float nz_add(float a, float b) { return a + b; }
MMS_DEV float nz_sub(float a, float b) { return a - b; }
MMS_DEV float nz_div(float a, float b) { return a / b; }

constexpr int NZ_THREADS = 256;
constexpr float NZ_DOWN = 1.f / 32768.f, NZ_UP = 32768.f;

// One block's view of its utterance slice and the noise behind it.
struct NoiseSlice {
  float* x;                                      // first sample of the slice
  long n;                                        // samples in the slice
  long t0;                                       // the slice's first sample within the utterance
  long T;                                        // utterance length
  long L;                                        // noise length (the shortest chosen clip)
  long s0;                                       // crop start, reduced mod L
  float f;                                       // noise amplitude factor 1 / (10^(SNR/20) + 1)
  int K;
  const int16_t* clip[MMS_NOISE_MAX_MIX];
};

// false: nothing to do for this block (apply == 0, an empty slice, or a params row that the host
// validation should have refused: a clip id out of range or an empty clip)
MMS_DEV bool noise_slice(NoiseSlice& S, float* wave, const int64_t* wave_off, const int16_t* bank,
                         const int64_t* bank_off, int n_clips, const int32_t* params, int n_mix) {
  const int b = blockIdx.x, sl = blockIdx.y, ns = gridDim.y;
  const int32_t* p = params + (long)b * (3 + n_mix);
  if (p[0] == 0) return false;
  const long w0 = wave_off[b];
  S.T = wave_off[b + 1] - w0;
  if (S.T <= 0) return false;
  S.t0 = S.T * sl / ns;
  S.n = S.T * (sl + 1) / ns - S.t0;
  S.x = wave + w0 + S.t0;
  S.f = __builtin_bit_cast(float, p[2]);
  S.K = n_mix;
  long L = -1;
#pragma unroll                                   // constant indices: clip[] stays in registers
  for (int k = 0; k < MMS_NOISE_MAX_MIX; ++k) {
    S.clip[k] = bank;
    if (k < n_mix) {
      const int c = p[3 + k];
      if (c < 0 || c >= n_clips) return false;
      const long c0 = bank_off[c], len = bank_off[c + 1] - c0;
      S.clip[k] = bank + c0;
      L = (L < 0 || len < L) ? len : L;
    }
  }
  if (L <= 0) return false;
  S.L = L;
  const long s = (long)p[1] % L;
  S.s0 = s < 0 ? s + L : s;
  return true;
}

// the noise sample at index j of the (cut) noise signal, 0 <= j < L, in [-1, 1)
MMS_DEV float noise_at(const NoiseSlice& S, long j) {
  if (S.K == 1) return (float)S.clip[0][j] * NZ_DOWN;
  int sum = 0;
#pragma unroll
  for (int k = 0; k < MMS_NOISE_MAX_MIX; ++k)
    if (k < S.K) sum += S.clip[k][j];
  return sum < 0 ? -1.f : 0.f;
}

// One pass over the slice: utterances lie back to back at arbitrary sample offsets, so up to three
// head samples come before the first 16-byte boundary and up to three tail samples after the last
// whole vector.  one(i, j): sample i of the slice with noise index j; four(i, j): samples i .. i+3,
// 16-byte aligned, noise indices j, j+1, ... each wrapped at L (noise_next).
MMS_DEV long noise_next(const NoiseSlice& S, long j) { return j + 1 == S.L ? 0 : j + 1; }

template <typename One, typename Four>
MMS_DEV void noise_sweep(const NoiseSlice& S, One one, Four four) {
  long head = (long)(((16 - ((uintptr_t)S.x & 15)) & 15) >> 2);
  head = head < S.n ? head : S.n;
  const long nv = (S.n - head) >> 2, tail0 = head + 4 * nv;
  const long base = S.s0 + S.t0;                 // noise index of slice sample 0, before the wrap
  const long tid = threadIdx.x;
  if (tid < head) one(tid, (base + tid) % S.L);
  if (tid < S.n - tail0) one(tail0 + tid, (base + tail0 + tid) % S.L);
  if (tid < nv) {
    // the index advances by 4 * NZ_THREADS samples per trip: one 64-bit remainder up front, then
    // an add and a conditional subtract
    const long step = (4L * NZ_THREADS) % S.L;
    long j = (base + head + 4 * tid) % S.L;
    for (long v = tid; v < nv; v += NZ_THREADS) {
      four(head + 4 * v, j);
      j += step;
      j = j >= S.L ? j - S.L : j;
    }
  }
}

MMS_DEV float noise_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ws: [B][MMS_NOISE_SPLIT][3] fp64 = {sum|x|, sum|seg|, max|y|} per slice
__global__ void __launch_bounds__(NZ_THREADS) noise_partial_kernel(
    float* __restrict__ wave, const int64_t* __restrict__ wave_off, const int16_t* __restrict__ bank,
    const int64_t* __restrict__ bank_off, int n_clips, const int32_t* __restrict__ params, int n_mix,
    double* __restrict__ ws) {
  NoiseSlice S;
  if (!noise_slice(S, wave, wave_off, bank, bank_off, n_clips, params, n_mix)) return;
  double sx = 0.0, sn = 0.0;
  noise_sweep(
      S,
      [&](long i, long j) {
        sx += (double)fabsf(S.x[i] * NZ_DOWN);
        sn += (double)fabsf(noise_at(S, j));
      },
      [&](long i, long j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(S.x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sx += (double)fabsf(v[e] * NZ_DOWN);
          sn += (double)fabsf(noise_at(S, j));
          j = noise_next(S, j);
        }
      });
  __shared__ double s_x[NZ_THREADS / 64], s_n[NZ_THREADS / 64];
  sx = wave_sum_d(sx);
  sn = wave_sum_d(sn);
  if ((threadIdx.x & 63) == 0) {
    s_x[threadIdx.x >> 6] = sx;
    s_n[threadIdx.x >> 6] = sn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, q = 0.0;
    for (int w = 0; w < NZ_THREADS / 64; ++w) { a += s_x[w]; q += s_n[w]; }
    double* out = ws + ((long)blockIdx.x * gridDim.y + blockIdx.y) * 3;
    out[0] = a;
    out[1] = q;
  }
}

__global__ void __launch_bounds__(NZ_THREADS) noise_mix_kernel(
    float* __restrict__ wave, const int64_t* __restrict__ wave_off, const int16_t* __restrict__ bank,
    const int64_t* __restrict__ bank_off, int n_clips, const int32_t* __restrict__ params, int n_mix,
    double* __restrict__ ws) {
  NoiseSlice S;
  if (!noise_slice(S, wave, wave_off, bank, bank_off, n_clips, params, n_mix)) return;
  double* part = ws + (long)blockIdx.x * gridDim.y * 3;
  double a = 0.0, q = 0.0;
  for (int sl = 0; sl < (int)gridDim.y; ++sl) { a += part[3 * sl]; q += part[3 * sl + 1]; }
  // torch: sum|.| (fp32) / length; f * clean_amp; new_amp / (noise_amp + 1e-14); 1 - f
  const float len = (float)S.T;
  const float clean_amp = nz_div((float)a, len);
  const float noise_amp = nz_div((float)q, len);
  const float new_amp = nz_mul(S.f, clean_amp);
  const float g = nz_div(new_amp, nz_add(noise_amp, 1e-14f));
  const float keep = nz_sub(1.f, S.f);
  float mx = 0.f;
  noise_sweep(
      S,
      [&](long i, long j) {
        const float y = nz_add(nz_mul(S.x[i] * NZ_DOWN, keep), nz_mul(noise_at(S, j), g));
        mx = fmaxf(mx, fabsf(y));
        S.x[i] = y;
      },
      [&](long i, long j) {
        f32x4 v = *reinterpret_cast<const f32x4*>(S.x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = nz_add(nz_mul(v[e] * NZ_DOWN, keep), nz_mul(noise_at(S, j), g));
          mx = fmaxf(mx, fabsf(v[e]));
          j = noise_next(S, j);
        }
        *reinterpret_cast<f32x4*>(S.x + i) = v;
      });
  __shared__ float s_m[NZ_THREADS / 64];
  mx = noise_wave_max(mx);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.f;
    for (int w = 0; w < NZ_THREADS / 64; ++w) m = fmaxf(m, s_m[w]);
    part[3 * blockIdx.y + 2] = (double)m;
  }
}

__global__ void __launch_bounds__(NZ_THREADS) noise_norm_kernel(
    float* __restrict__ wave, const int64_t* __restrict__ wave_off, const int16_t* __restrict__ bank,
    const int64_t* __restrict__ bank_off, int n_clips, const int32_t* __restrict__ params, int n_mix,
    const double* __restrict__ ws) {
  NoiseSlice S;
  if (!noise_slice(S, wave, wave_off, bank, bank_off, n_clips, params, n_mix)) return;
  const double* part = ws + (long)blockIdx.x * gridDim.y * 3;
  float m = 1.f;                                 // abs_max.clamp(min=1.0)
  for (int sl = 0; sl < (int)gridDim.y; ++sl) m = fmaxf(m, (float)part[3 * sl + 2]);
  noise_sweep(
      S, [&](long i, long) { S.x[i] = nz_div(S.x[i], m) * NZ_UP; },
      [&](long i, long) {
        f32x4 v = *reinterpret_cast<const f32x4*>(S.x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = nz_div(v[e], m) * NZ_UP;
        *reinterpret_cast<f32x4*>(S.x + i) = v;
      });
}

}  // namespace

extern "C" int mms2ut_noise_mix_f32(float* wave, const int64_t* wave_off, int B, const int16_t* bank,
                                    const int64_t* bank_off, int n_clips, const int32_t* params, int n_mix,
                                    double* ws, hipStream_t s) {
  MMS_REQUIRE(B >= 0 && n_clips >= 1, "noise_mix: B >= 0 and at least one clip required");
  MMS_REQUIRE(n_mix >= 1 && n_mix <= MMS_NOISE_MAX_MIX, "noise_mix: n_mix must be in [1, %d]", MMS_NOISE_MAX_MIX);
  if (B == 0) return 0;
  MMS_REQUIRE(wave && wave_off && bank && bank_off && params && ws, "noise_mix: null buffer");
  MMS_REQUIRE(((uintptr_t)wave & 3) == 0 && ((uintptr_t)ws & 7) == 0, "noise_mix: wave / ws misaligned");
  const dim3 grid(B, MMS_NOISE_SPLIT), block(NZ_THREADS);
  hipLaunchKernelGGL(noise_partial_kernel, grid, block, 0, s, wave, wave_off, bank, bank_off, n_clips, params, n_mix, ws);
  if (int rc = mms::check_launch("noise_partial")) return rc;
  hipLaunchKernelGGL(noise_mix_kernel, grid, block, 0, s, wave, wave_off, bank, bank_off, n_clips, params, n_mix, ws);
  if (int rc = mms::check_launch("noise_mix")) return rc;
  hipLaunchKernelGGL(noise_norm_kernel, grid, block, 0, s, wave, wave_off, bank, bank_off, n_clips, params, n_mix, ws);
  return mms::check_launch("noise_norm");
}
