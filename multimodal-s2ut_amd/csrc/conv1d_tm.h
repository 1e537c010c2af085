// The implicit-GEMM Conv1d tile over time-major fp16 rows [T, C], on v_mfma_f32_16x16x32_f16: the one
// definition behind vocoder.hip's conv1d_tm_kernel (dilation, polyphase ConvTranspose1d) and asr.hip's
// asr_conv_kernel (stride, groups), and the host-side rules both launchers follow.
//
// One block owns 128 output positions (32 where the waves split K, see conv_splits) x up to 64 output
// channels.  Per 64-wide slice of Cin it stages the input rows its outputs read once into LDS (rows
// outside [0, T_in) as zeros: the padding at both sequence ends), then every K-step of 32 reads its
// operand as one 16-byte LDS read per lane.  The reduction runs over (tap, cin); there is no im2col
// image anywhere.  The weights were repacked at load into the MFMA A-operand image
// ([K-step][cout][32], vocoder.pack_conv_weight), so a lane's fragment is one 16-byte global read,
// shared through L1/L2 by all blocks.  The product is computed transposed (A = weights, B =
// activations): a lane then holds four consecutive output channels of one position and writes them
// with one 8-byte store.
//
// What differs between the two kernels comes in through a view struct (see conv1d_tm_tile).
#pragma once
#include "common.h"
#include "../../include/mms2ut.h"

namespace {

constexpr int CT_TN = 64;         // output channels per block (up to 4 MFMA row tiles)
constexpr int CT_CHUNK = MMS_VOC_CIN_CHUNK;
constexpr int CT_LD = CT_CHUNK + 8;   // LDS row stride in halves: 144 B, rows 16-byte aligned
constexpr int CT_THREADS = 256;
constexpr int CT_GROUP = 4;       // K-steps whose weight fragments are loaded together
constexpr int CT_SPLIT_MIN_STEPS = 4, CT_SPLIT_MAX_BLOCKS = 256;    // when the waves split K (conv_splits)

constexpr int conv_tile_positions(bool splitk) { return splitk ? 32 : 128; }
constexpr int conv_red_elems(bool splitk) { return splitk ? 3 * 8 * 64 : 1; }   // f32x4 each

// SPLITK false: the block owns 128 positions, wave w rows [32 w, 32 w + 32), every wave walks all
// K-steps.  SPLITK true: the block owns 32 positions, wave w takes K-steps w, w + 4, ... and wave 0
// adds the four partial tiles (in wave order) before the epilogue.
//
// xs: (at least v.rows(TM)) * CT_LD halves of LDS, 16-byte aligned; red: conv_red_elems(SPLITK).
// A View is built for one blockIdx.z and supplies
//   x, w, bias        base pointers of this z (bias may be null); T_in, ldx of x; nq output positions
//   rows(TM)          staged rows of a block of TM positions
//   row0(q0)          the global input row staged as LDS row 0 of the block that starts at position q0
//   lds_row(p, j)     the staged row that position p of the block reads at tap j
//   stage(v)          the input activation, applied to 8 halves on their way into LDS
//   emit(q, co, v)    the epilogue: v = acc + bias of position q, channels [co, co + 4)
template <bool SPLITK, class View>
MMS_DEV void conv1d_tm_tile(const View& v, int Cin, int Cout, int taps, h16* xs, f32x4* red) {
  constexpr int TM = conv_tile_positions(SPLITK);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lk = (lane >> 4) * 8;
  const int q0 = blockIdx.x * TM, co0 = blockIdx.y * CT_TN;
  const int CoutP = (Cout + 15) & ~15;
  const int nb = min(CT_TN / 16, (CoutP - co0) / 16);
  const h16* __restrict__ x = v.x;
  const h16* __restrict__ w = v.w;
  const int rows = v.rows(TM);                            // <= the LDS rows (host check)
  const auto row0 = v.row0(q0);
  const int wrow = SPLITK ? 0 : wave * 32;
  const int s_first = SPLITK ? wave : 0, s_stride = SPLITK ? 4 : 1;

  f32x4 acc[CT_TN / 16][2];
#pragma unroll
  for (int g = 0; g < CT_TN / 16; ++g)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[g][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  int sbase = 0;
  for (int c0 = 0; c0 < Cin; c0 += CT_CHUNK) {
    const int cw = min(CT_CHUNK, Cin - c0), cv = cw >> 3;
    __syncthreads();                                      // the previous slice's reads are done
    for (int u = tid; u < rows * cv; u += CT_THREADS) {
      const int rr = u / cv, cc = (u - rr * cv) * 8;
      const auto row = row0 + rr;
      h16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
      if (row >= 0 && row < v.T_in) h = v.stage(*reinterpret_cast<const h16x8*>(x + (long)row * v.ldx + c0 + cc));
      *reinterpret_cast<h16x8*>(xs + rr * CT_LD + cc) = h;
    }
    __syncthreads();
    const int nsteps = (taps * cw + 31) >> 5;
    // The weights of a launch are cold and every block walks them in step, so a K-step's fragment
    // load costs a full memory latency: CT_GROUP steps' loads are issued before their MFMAs.
    for (int s0 = s_first; s0 < nsteps; s0 += CT_GROUP * s_stride) {
      h16x8 wf[CT_GROUP][CT_TN / 16];
#pragma unroll
      for (int u = 0; u < CT_GROUP; ++u) {
        const int s = s0 + u * s_stride;
        const h16* wp = w + ((long)(sbase + s) * CoutP + co0 + l15) * 32 + lk;
#pragma unroll
        for (int g = 0; g < CT_TN / 16; ++g)
          if (s < nsteps && g < nb) wf[u][g] = *reinterpret_cast<const h16x8*>(wp + g * 16 * 32);
      }
#pragma unroll
      for (int u = 0; u < CT_GROUP; ++u) {
        const int s = s0 + u * s_stride;
        if (s < nsteps) {
          const int kk = s * 32 + lk;
          const int j = kk / cw, c = kk - j * cw;
          const bool valid = j < taps;                    // the K tail of the last step: zero weights too
          h16x8 xf[2];
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            xf[f] = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (valid) xf[f] = *reinterpret_cast<const h16x8*>(xs + v.lds_row(wrow + f * 16 + l15, j) * CT_LD + c);
          }
#pragma unroll
          for (int g = 0; g < CT_TN / 16; ++g)
            if (g < nb) {
#pragma unroll
              for (int f = 0; f < 2; ++f)
                acc[g][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][g], xf[f], acc[g][f], 0, 0, 0);
            }
        }
      }
    }
    sbase += nsteps;
  }

  if (SPLITK) {
    if (wave > 0) {
#pragma unroll
      for (int g = 0; g < CT_TN / 16; ++g)
#pragma unroll
        for (int f = 0; f < 2; ++f) red[((wave - 1) * 8 + g * 2 + f) * 64 + lane] = acc[g][f];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int wv = 0; wv < 3; ++wv)
#pragma unroll
      for (int g = 0; g < CT_TN / 16; ++g)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[g][f] += red[(wv * 8 + g * 2 + f) * 64 + lane];
  }

  // D[row = cout (lane>>4)*4 + e][col = position lane&15]
#pragma unroll
  for (int g = 0; g < CT_TN / 16; ++g) {
    if (g >= nb) continue;
    const int co = co0 + g * 16 + (lane >> 4) * 4;
    if (co >= Cout) continue;                             // Cout is a multiple of 8: whole groups of 4
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (v.bias) b = *reinterpret_cast<const f32x4*>(v.bias + co);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int q = q0 + wrow + f * 16 + l15;
      if (q < v.nq) v.emit(q, co, acc[g][f] + b);
    }
  }
}

// rounds one epilogue result to fp16 and stores it: the only rounding of a convolution
MMS_DEV void conv_store4(h16* yp, f32x4 v) {
  h16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (h16)v[e];
  *reinterpret_cast<h16x4*>(yp) = o;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// K-steps of 32 of one weight image: every Cin slice rounds its taps * width up on its own
inline long conv_ksteps(int Cin, int taps) {
  long steps = 0;
  for (int c0 = 0; c0 < Cin; c0 += CT_CHUNK) steps += ((long)taps * min(CT_CHUNK, Cin - c0) + 31) / 32;
  return steps;
}

// Fewer blocks than CUs and a long reduction: the K-steps' weight loads are a serial latency chain
// per wave, so the waves of a block share it out (and the blocks shrink to 32 positions, four times
// as many).  With more blocks the short tile loses: it stages up to 96 rows for 32 outputs.
// The choice depends on the problem's shape alone, so a shape always takes the same path.
inline bool conv_splits(long steps, long blocks128) {
  return steps >= CT_SPLIT_MIN_STEPS && blocks128 < CT_SPLIT_MAX_BLOCKS;
}

// launches the SPLITK or the plain instantiation over nq positions x Cout x nz (phases / groups)
template <class Args>
inline void conv_tm_launch(void (*split)(Args), void (*plain)(Args), const Args& a, int Cin, int Cout, int taps, int nq,
                           int nz, hipStream_t s) {
  const int cy = (Cout + CT_TN - 1) / CT_TN;
  if (conv_splits(conv_ksteps(Cin, taps), (long)((nq + 127) / 128) * cy * nz)) {
    hipLaunchKernelGGL(split, dim3((nq + 31) / 32, cy, nz), dim3(CT_THREADS), 0, s, a);
  } else {
    hipLaunchKernelGGL(plain, dim3((nq + 127) / 128, cy, nz), dim3(CT_THREADS), 0, s, a);
  }
}

// The preconditions of the tile that do not depend on the entry point.  Cin, Cout: of one weight image;
// wx, wy: the widths the rows of x and of y / res must cover (all groups); per: " per group" or "".
inline int conv_check(const char* what, const char* per, int Cin, int Cout, const void* x, long ldx, long wx,
                      const void* w, const float* bias, const void* y, long ldy, const void* res, long ldres, long wy) {
  MMS_REQUIRE(Cin >= 8 && Cin % 8 == 0 && Cout >= 8 && Cout % 8 == 0,
              "%s: channel widths%s must be multiples of 8 and >= 8 (Cin %d, Cout %d)", what, per, Cin, Cout);
  MMS_REQUIRE(x && w && y, "%s: null buffer", what);
  MMS_REQUIRE(ldx >= wx && ldx % 8 == 0 && ldy >= wy && ldy % 4 == 0 && (!res || (ldres >= wy && ldres % 4 == 0)),
              "%s: row strides must cover the width and keep rows 16-byte (x) / 8-byte (y, res) aligned", what);
  MMS_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)y & 7) == 0 &&
                  ((uintptr_t)res & 7) == 0 && ((uintptr_t)bias & 15) == 0, "%s: misaligned buffer", what);
  MMS_REQUIRE((Cout + CT_TN - 1) / CT_TN <= 65535, "%s: grid too large", what);
  return 0;
}

}  // namespace
