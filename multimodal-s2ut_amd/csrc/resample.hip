// Sample-rate conversion of a batch of mono fp32 clips laid back to back in HBM: bandlimited sinc
// interpolation in the polyphase form of torchaudio.functional.resample (restated from its published
// source; prepare.resample_taps builds the table in fp64).  With o = orig / gcd, n = new / gcd,
//   y[j n + i] = sum_{c < K} h[i][c] xp[j o + c],   xp[t] = x[t - width] inside the clip, 0 outside,
// and a clip of L samples gives ceil(n L / o) outputs.
//
// One launch, grid (B, tiles of the longest clip).  A block owns JT = G x MMS_RESAMPLE_R consecutive
// output frames of one clip (a frame = the n outputs that share an input position j o):
//   1. the (JT - 1) o + K input samples the tile touches are staged in LDS, zero where the index falls
//      outside the clip.  This is the only place the input is read, and the guard is on the clip's own
//      length, so a neighbour's samples are never seen however the clips are packed.
//   2. thread item q = (g, i), g < G, i < H = ceil(n / 2), owns the phases i and i + H of the frames
//      j0 + g + r G, r < MMS_RESAMPLE_R: 2 R accumulators.  Per tap it loads h[i][c] and h[i + H][c]
//      from the tap-major table ([K][n]: consecutive lanes, consecutive phases, coalesced lines that
//      stay in L2; the next RS_U taps are in flight while the current ones are used) and R input
//      samples from LDS, for 2 R FMAs.  Lanes of one frame read one LDS word (broadcast); neighbouring
//      frames lie o words apart, so for odd o the n == 1 case is conflict-free too.  An item whose
//      second phase does not exist (n == 1, i.e. every integer decimation such as 48000 -> 16000, and
//      the last item of a group for odd n) still runs the second chain on a copy of its first phase
//      and drops it at the store: no divergent branch in the tap loop, at the price of half the FMAs
//      and tap loads of the one-phase case (the LDS reads, the binding port, are not doubled).
// Each output is one chain of K FMAs in tap order: the rounding of an output depends on its phase and
// its inputs alone, so a clip's result has the same bits alone, anywhere in a batch and on every run.
// The multi-phase tables (22050 -> 16000: 786 KB) do not fit in LDS.  HBM traffic is small next to the
// arithmetic (K FMAs per output sample): what bounds the kernel is the LDS read port and the FMA
// issue, one ds_read_b32 per two FMAs.  No atomics, plain vector stores.
#include "common.h"
#include "../../include/mms2ut.h"

namespace {

constexpr int RS_THREADS = MMS_RESAMPLE_THREADS, RS_R = MMS_RESAMPLE_R;
constexpr int RS_U = 8;                          // taps per trip of the inner loop

// manifest.write_wav's rounding: rint (half to even), then clip
MMS_DEV int16_t rs_int16(float v) { return (int16_t)(int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }

// frame groups per tile: MMS_RESAMPLE_TILE outputs or up to twice that, so that the block's threads
// are busy in the last pass over the items too, then cut to the LDS window.  0: no tile fits.  The
// window sets the blocks per CU: with MMS_RESAMPLE_TILE 4096 the corpus rates ran 14-25 % longer
// (profiles/resample_tile_ab.txt).
int resample_groups(int o, int n, int K) {
  const long H = (n + 1) / 2;                      // items per frame group: a thread owns two phases
  const long G0 = (MMS_RESAMPLE_TILE / (2 * RS_R) + H - 1) / H;
  long G = G0;
  double best = 0.0;
  for (long g = G0; g <= 2 * G0; ++g) {            // the first G whose items fill >= 90 % of the passes
    const long slots = (H * g + RS_THREADS - 1) / RS_THREADS * RS_THREADS;
    const double eff = (double)(H * g) / (double)slots;
    if (eff > best) { best = eff; G = g; }
    if (eff >= 0.9) break;
  }
  if (K > MMS_RESAMPLE_LDS_FLOATS) return 0;       // refused by name in mms2ut_resample_plan
  const long fit = ((MMS_RESAMPLE_LDS_FLOATS - K) / o + 1) / RS_R;   // (G R - 1) o + K <= LDS floats
  G = G < fit ? G : fit;
  return (int)G;
}

__global__ void __launch_bounds__(RS_THREADS) resample_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ in_off, const int64_t* __restrict__ out_off,
    const float* __restrict__ taps, int o, int n, int width, int K, int G, float* __restrict__ y,
    int16_t* __restrict__ y16) {
  extern __shared__ __align__(16) float xs[];
  const int b = blockIdx.x;
  const long x0 = in_off[b], L = in_off[b + 1] - x0;
  const long y0 = out_off[b], room = out_off[b + 1] - y0;
  long Lout = (L * n + o - 1) / o;
  Lout = Lout < room ? Lout : room;              // never past the clip's own output slot
  const long JT = (long)G * RS_R, j0 = (long)blockIdx.y * JT;
  if (L <= 0 || j0 * n >= Lout) return;          // block-uniform: before the barrier
  const int W = (int)(JT - 1) * o + K;
  const long src0 = j0 * o - width;
  for (int t = threadIdx.x; t < W; t += RS_THREADS) {
    const long s = src0 + t;
    xs[t] = (s >= 0 && s < L) ? x[x0 + s] : 0.f;
  }
  __syncthreads();
  const int H = (n + 1) >> 1, items = H * G, stride = G * o;
  const int Kmain = K / RS_U * RS_U;
  for (int q = threadIdx.x; q < items; q += RS_THREADS) {
    const int g = q / H, i = q - g * H;
    const long m0 = (j0 + g) * n + i;            // the item's outputs: m0 + r G n, and H further on
    if (m0 >= Lout) continue;
    const bool two = i + H < n;                  // odd n: the last item of a group has one phase
    const float* hp0 = taps + i;
    const float* hp1 = taps + (two ? i + H : i);
    const float* xp = xs + g * o;
    float acc0[RS_R], acc1[RS_R], n0[RS_U], n1[RS_U];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {             // index clamped: never past the table
      const long cc = u < K ? u : K - 1;
      n0[u] = hp0[cc * n];
      n1[u] = hp1[cc * n];
    }
    for (int c0 = 0; c0 < Kmain; c0 += RS_U) {
      float h0[RS_U], h1[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        h0[u] = n0[u];
        h1[u] = n1[u];
        const int c = c0 + RS_U + u;             // the next trip's taps (clamped in the last one)
        const long cc = c < K ? c : K - 1;
        n0[u] = hp0[cc * n];
        n1[u] = hp1[cc * n];
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
          const float xv = xp[r * stride + c0 + u];
          acc0[r] = fmaf(h0[u], xv, acc0[r]);
          acc1[r] = fmaf(h1[u], xv, acc1[r]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {             // the K % RS_U taps left: already loaded
      if (Kmain + u < K) {
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
          const float xv = xp[r * stride + Kmain + u];
          acc0[r] = fmaf(n0[u], xv, acc0[r]);
          acc1[r] = fmaf(n1[u], xv, acc1[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const long m = m0 + (long)r * G * n;
      if (m < Lout) {
        y[y0 + m] = acc0[r];
        if (y16) y16[y0 + m] = rs_int16(acc0[r]);
      }
      if (two && m + H < Lout) {
        y[y0 + m + H] = acc1[r];
        if (y16) y16[y0 + m + H] = rs_int16(acc1[r]);
      }
    }
  }
}

}  // namespace

extern "C" int mms2ut_resample_plan(int o, int n, int K, int* tile_frames) {
  MMS_REQUIRE(o >= 1 && n >= 1 && K >= 1 && tile_frames, "resample_plan: o, n, K >= 1 required");
  MMS_REQUIRE((long)K * n <= MMS_RESAMPLE_MAX_TAPS, "resample: a table of %ld taps (K %d x %d phases) exceeds the cap of %d",
              (long)K * n, K, n, MMS_RESAMPLE_MAX_TAPS);
  MMS_REQUIRE(K <= MMS_RESAMPLE_LDS_FLOATS, "resample: K %d taps per phase exceed the LDS window of %d floats", K,
              MMS_RESAMPLE_LDS_FLOATS);
  const int G = resample_groups(o, n, K);
  MMS_REQUIRE(G >= 1, "resample: no tile fits in LDS (o %d, K %d: the %d frames a thread owns need more than %d floats)", o, K,
              RS_R, MMS_RESAMPLE_LDS_FLOATS);
  *tile_frames = G * RS_R;
  return 0;
}

extern "C" int mms2ut_resample_f32(const float* x, const int64_t* in_off, const int64_t* out_off, int B,
                                   int64_t max_out, const float* taps, int o, int n, int width, int K, float* y,
                                   int16_t* y16, hipStream_t s) {
  MMS_REQUIRE(B >= 0 && max_out >= 0, "resample: B >= 0 and max_out >= 0 required");
  MMS_REQUIRE(width >= 0 && K == 2 * width + o, "resample: K must be 2 width + o (K %d, width %d, o %d)", K, width, o);
  int JT = 0;
  if (int rc = mms2ut_resample_plan(o, n, K, &JT)) return rc;
  if (B == 0 || max_out == 0) return 0;
  MMS_REQUIRE(x && in_off && out_off && taps && y, "resample: null buffer");
  const int64_t per_tile = (int64_t)JT * n, tiles = (max_out + per_tile - 1) / per_tile;
  MMS_REQUIRE(tiles <= 65535, "resample: a clip of %ld outputs needs %ld tiles (at most 65535)", (long)max_out, (long)tiles);
  const size_t lds = sizeof(float) * ((size_t)(JT - 1) * o + K);
  hipLaunchKernelGGL(resample_kernel, dim3(B, (unsigned)tiles), dim3(RS_THREADS), lds, s, x, in_off, out_off, taps, o,
                     n, width, K, JT / RS_R, y, y16);
  return mms::check_launch("resample");
}
