// Shared pieces of the MFMA GEMM kernels (gemm.hip: 128x128 / tall / 256x256 tiles; the GEMM lab,
// scripts/micro): launch parameters, tile order, LDS fragment reads, fused epilogues.  Everything
// but GemmP has internal linkage.
#pragma once
#include "common.h"
#include "../../include/mms2ut.h"

// Launch parameters of every GEMM kernel
namespace mmsg {
struct GemmP {
  const h16* A; const h16* B; void* C;
  int M, N, K;
  long lda, ldb, ldc;
  int bdiv;  // batch index z -> (z / bdiv, z % bdiv)
  long sA1, sA2, sB1, sB2, sC1, sC2;
  int splitk; int kchunk; long sCsplit;
  // epilogue
  float alpha;
  const h16* bias;
  const h16* aux; long ldaux; long sX1, sX2;
  h16* out2; long ldo2;
  float p; uint32_t thresh; uint64_t seed, offset; long ld_rng;
  int vec16;  // every fp16 row operand of the epilogue is 16-B aligned at 8-column granularity (3: and
              // the fp32-staged epilogue forced, mms2ut_gemm_set_epilogue)
  float* rowsum; long ld_rowsum;  // RS kernels: split-K partial A-row sums (bias gradient)
  h16* rowsum16;                  // RS kernels, unsplit: the fp16 A-row sums (grouped wgrad)
  int group_m;  // tile-rows per L2 group (tile_coords)
  unsigned long long* stamps;  // profiling: per block {first, last} s_memrealtime tick, or null
};

}  // namespace mmsg

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
#ifndef MMS_GEMM_PRIO
#define MMS_GEMM_PRIO 1
#endif
// raise wave priority around the MFMA block of a k-step — for the fp16-output (forward / dgrad,
// critical-path) GEMMs only, so that their waves win issue slots over the side stream's
// weight-gradient (fp32 slab) GEMM waves sharing a CU
constexpr bool PRIO = MMS_GEMM_PRIO;
constexpr int TILE_BYTES = 128 * 64 * 2;  // 16 KiB per operand per stage

using mmsg::GemmP;

// Live kernel timing (bench roofline): with P.stamps set, thread 0 of every block stores the
// block's start tick and its end tick (after the block's last global store has completed) at
// stamps[2 * blockIdx.x].  A launch's duration is max(end) - min(start) over its blocks — the
// dispatch span rocprofv3's kernel trace reports, measured inside the real (overlapped) step.
// One 16-B store per block; nothing is recorded when stamps is null.
MMS_DEV unsigned long long stamp_now() { return __builtin_amdgcn_s_memrealtime(); }
MMS_DEV void stamp_end(unsigned long long* stamps, unsigned long long t0) {
  if (!stamps) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t1 = stamp_now();
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u64x2*>(stamps + 2 * (long)blockIdx.x) = u64x2{t0, t1};
  }
}

MMS_DEV int swz_mn(int k) { return ((k & 3) | ((k >> 1) & 4)) << 1; }

// fragment for rows [sub, sub+16) and k in [kk*32, kk*32+32): lane l holds X(sub + (l&15), kk*32 + 8(l>>4) + j)
template <bool KC>
MMS_DEV h16x8 read_frag(const char* lds, int sub, int kk, int lane) {
  if (KC) {
    const int r = sub + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    s16x8 v = *reinterpret_cast<const s16x8*>(lds + r * 128 + ((c ^ (r & 7)) << 4));
    return __builtin_bit_cast(h16x8, v);
  } else {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int col = sub + 4 * p;                // element column (row of the logical operand)
    const int chunk = col >> 3, inb = (col & 7) * 2;
    const int k1 = kk * 32 + 8 * g + q, k2 = k1 + 4;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const char* a1 = lds + k1 * 256 + ((chunk ^ swz_mn(k1)) << 4) + inb;
    const char* a2 = lds + k2 * 256 + ((chunk ^ swz_mn(k2)) << 4) + inb;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a1));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a2));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(h16x8, v);
  }
}

MMS_DEV float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
// the derivative of common.h's gelu_erf
MMS_DEV float gelu_grad_(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * __expf(-0.5f * z * z);
}

// ------------------------------------------------------------------------------------------
// What each epilogue form needs.  MMS_EPI_F32 (the split-K / weight-gradient slab) is alpha * acc
// and nothing else.
// ------------------------------------------------------------------------------------------
template <int EPI>
constexpr bool epi_drops() {
  return EPI == MMS_EPI_RELU_DROP || EPI == MMS_EPI_DROP_RESID || EPI == MMS_EPI_GELU_DROP ||
         EPI == MMS_EPI_GELU_DROP_BWD;
}
// adds P.bias (when set): every fp16 form but the two that scale an incoming gradient
template <int EPI>
constexpr bool epi_adds_bias() {
  return EPI != MMS_EPI_F32 && EPI != MMS_EPI_RELU_DROP_BWD && EPI != MMS_EPI_GELU_DROP_BWD;
}
// reads a row operand at the element's (m, n): aux (residual: DROP_RESID; o: GATE; fc1 output:
// RELU_DROP_BWD; pre-activation z: GELU_DROP_BWD) or the old C (F16_ACC).  GATE reads a second
// operand, t, at aux + N of the same row.
template <int EPI>
constexpr bool epi_reads_row() {
  return EPI == MMS_EPI_DROP_RESID || EPI == MMS_EPI_GATE || EPI == MMS_EPI_RELU_DROP_BWD ||
         EPI == MMS_EPI_F16_ACC || EPI == MMS_EPI_GELU_DROP_BWD;
}
// writes P.out2: the gate (GATE), the fp16 pre-activation z (GELU_DROP)
template <int EPI>
constexpr bool epi_writes_out2() { return EPI == MMS_EPI_GATE || EPI == MMS_EPI_GELU_DROP; }

// One element of an fp16 form: x = acc * alpha + bias, a the row operand (aux / old C), a2 GATE's
// second operand (aux + N), keep the element's dropout bit, dscale = 1 / (1 - p) (1 without dropout).
// Returns the fp32 value that the caller rounds to fp16 and sets o2 to the out2 value of the forms
// that write one.  reg_epilogue, perm_epilogue and the staged fast path call this, so the fp32 ->
// fp16 rounding points (GELU_DROP applies gelu to the ROUNDED z) are the same on all of them.
// epilogue_store / epilogue_store8 below still spell the same expressions out form by form: hipcc
// fuses a form's last multiply with the fp16 rounding (v_fma_mixlo_f16: one rounding instead of two)
// or not depending on how those loops vectorise, and written through this function they fused
// where the former code did not (ReLU-dropout and gate outputs differed in rare last bits).
template <int EPI>
MMS_DEV float epi_element(float x, float a, float a2, bool keep, float dscale, h16& o2) {
  if (EPI == MMS_EPI_RELU_DROP) return keep ? fmaxf(x, 0.f) * dscale : 0.f;
  if (EPI == MMS_EPI_DROP_RESID) return a + (keep ? x * dscale : 0.f);
  if (EPI == MMS_EPI_GATE) {   // a = o, a2 = t
    const float g = sigmoidf_(x);
    o2 = (h16)g;
    return a2 + g * (a - a2);
  }
  if (EPI == MMS_EPI_RELU_DROP_BWD) return a > 0.f ? x * dscale : 0.f;   // (the mask is folded into a)
  if (EPI == MMS_EPI_F16_ACC) return a + x;
  if (EPI == MMS_EPI_GELU_DROP) {
    o2 = (h16)x;
    return keep ? gelu_erf((float)o2) * dscale : 0.f;
  }
  if (EPI == MMS_EPI_GELU_DROP_BWD) return keep ? x * dscale * gelu_grad_(a) : 0.f;
  return x;
}

// Keep bits of a lane's runs of W (4 / 8) consecutive dropout counters.  init() takes the first and
// the last counter the lane will ask for: while they share the counter's high word (always, unless
// the lane's elements straddle a 2^33 boundary) the seed / high-word half of the hash is one
// constant, one mixer per pair of elements instead of two; when that holds for the whole wave
// (the compiler versions the caller's loop on it) a run's pair index is pbase + dpair in 32-bit
// arithmetic, no 64-bit counter per run.  A run starts on a multiple of 4 columns, so an even
// offset and ld_rng keep its first counter even.  Bit-identical to mms_keep4 on every tier
// (tests/test_rng_ref.py).
template <int W>
struct KeepRuns {
  uint32_t hmix = 0, pbase = 0;
  bool same_hi = false, fast = false;
  MMS_DEV void init(const GemmP& P, uint64_t cf, uint64_t cl) {
    same_hi = mms_same_hi(cf, cl) && ((cf & 1) == 0) && ((P.ld_rng & 1) == 0);
    hmix = mms_hi_mix(P.seed, cf);
    pbase = (uint32_t)(cf >> 1);
    fast = __all(same_hi);
  }
  // the run at (m, n): counters offset + m ld_rng + n .. + W - 1; dpair = its pair index less cf's
  MMS_DEV void run(const GemmP& P, uint32_t dpair, int m, int n, bool (&keep)[W]) const {
    if (fast) {
      const uint32_t p0 = pbase + dpair;
#pragma unroll
      for (int t = 0; t < W / 2; ++t) {
        const uint32_t hv = mms_mix32((p0 + t) ^ hmix);
        keep[2 * t] = (hv & 0xffffU) >= P.thresh;
        keep[2 * t + 1] = (hv >> 16) >= P.thresh;
      }
    } else {
      const uint64_t c0 = P.offset + (uint64_t)m * P.ld_rng + n;
#pragma unroll
      for (int t = 0; t < W / 4; ++t) {
        bool k[4];
        if (same_hi) mms_keep4_hi(hmix, c0 + 4 * t, P.thresh, k);
        else mms_keep4(P.seed, c0 + 4 * t, P.thresh, k);
#pragma unroll
        for (int e = 0; e < 4; ++e) keep[4 * t + e] = k[e];
      }
    }
  }
};

template <int EPI>
MMS_DEV void epilogue_store(const GemmP& P, void* Cz, const h16* auxz, int m, int n, f32x4 v) {
  if (m >= P.M) return;
  const int N = P.N;
  float x[4] = {v[0] * P.alpha, v[1] * P.alpha, v[2] * P.alpha, v[3] * P.alpha};
  if (EPI == MMS_EPI_F32) {
    float* C = reinterpret_cast<float*>(Cz) + (long)m * P.ldc;
    if (n + 3 < N) {
      *reinterpret_cast<f32x4*>(C + n) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
      for (int r = 0; r < 4; ++r) if (n + r < N) C[n + r] = x[r];
    }
    return;
  }
  const bool full = n + 3 < N;
  if (epi_adds_bias<EPI>() && P.bias) {
    if (full) {
      const h16x4 bv = *reinterpret_cast<const h16x4*>(P.bias + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] += (float)bv[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (n + r < N) x[r] += (float)P.bias[n + r];
    }
  }
  h16* C = reinterpret_cast<h16*>(Cz) + (long)m * P.ldc;
  // 4-wide operand fetches (aux row / existing C), zero beyond N
  auto ld4 = [&](const h16* row, int col, float (&v)[4]) {
    if (full) {
      const h16x4 t = *reinterpret_cast<const h16x4*>(row + col);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (float)t[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (n + r < N) ? (float)row[col + r] : 0.f;
    }
  };
  bool keep[4] = {true, true, true, true};
  if (epi_drops<EPI>() && P.thresh)
    mms_keep4(P.seed, P.offset + (uint64_t)m * P.ld_rng + n, P.thresh, keep);
  const float dscale = P.thresh ? 1.f / (1.f - P.p) : 1.f;
  float o[4];
  if (EPI == MMS_EPI_RELU_DROP) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = keep[r] ? fmaxf(x[r], 0.f) * dscale : 0.f;
  } else if (EPI == MMS_EPI_DROP_RESID) {
    float a[4];
    ld4(auxz + (long)m * P.ldaux, n, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = a[r] + (keep[r] ? x[r] * dscale : 0.f);
  } else if (EPI == MMS_EPI_GATE) {
    float ov[4], tv[4];
    ld4(auxz + (long)m * P.ldaux, n, ov);
    ld4(auxz + (long)m * P.ldaux + N, n, tv);
    float g[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      g[r] = sigmoidf_(x[r]);
      o[r] = tv[r] + g[r] * (ov[r] - tv[r]);
    }
    h16* g_row = P.out2 + (long)m * P.ldo2;
    if (full) {
      *reinterpret_cast<h16x4*>(g_row + n) = h16x4{(h16)g[0], (h16)g[1], (h16)g[2], (h16)g[3]};
    } else {
      for (int r = 0; r < 4; ++r) if (n + r < N) g_row[n + r] = (h16)g[r];
    }
  } else if (EPI == MMS_EPI_RELU_DROP_BWD) {
    float h[4];
    ld4(auxz + (long)m * P.ldaux, n, h);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = h[r] > 0.f ? x[r] * dscale : 0.f;
  } else if (EPI == MMS_EPI_F16_ACC) {
    float c[4];
    ld4(C, n, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = c[r] + x[r];
  } else if (EPI == MMS_EPI_GELU_DROP) {
    h16 zh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      zh[r] = (h16)x[r];
      o[r] = keep[r] ? gelu_erf((float)zh[r]) * dscale : 0.f;
    }
    h16* z_row = P.out2 + (long)m * P.ldo2;
    if (full) {
      *reinterpret_cast<h16x4*>(z_row + n) = h16x4{zh[0], zh[1], zh[2], zh[3]};
    } else {
      for (int r = 0; r < 4; ++r) if (n + r < N) z_row[n + r] = zh[r];
    }
  } else if (EPI == MMS_EPI_GELU_DROP_BWD) {
    float z[4];
    ld4(auxz + (long)m * P.ldaux, n, z);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = keep[r] ? x[r] * dscale * gelu_grad_(z[r]) : 0.f;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = x[r];
  }
  if (full) {
    *reinterpret_cast<h16x4*>(C + n) = h16x4{(h16)o[0], (h16)o[1], (h16)o[2], (h16)o[3]};
  } else {
    for (int r = 0; r < 4; ++r) if (n + r < N) C[n + r] = (h16)o[r];
  }
}

// 8 consecutive columns n..n+7 (n % 8 == 0) of row m: 16-B operand loads / stores when aligned,
// otherwise two 4-wide calls of epilogue_store (which also handles the N tail)
template <int EPI>
MMS_DEV void epilogue_store8(const GemmP& P, void* Cz, const h16* auxz, int m, int n, const float (&v)[8]) {
  if (m >= P.M || n >= P.N) return;
  const int N = P.N;
  if (EPI == MMS_EPI_F32) {
    float* C = reinterpret_cast<float*>(Cz) + (long)m * P.ldc;
    if (n + 7 < N) {
      *reinterpret_cast<f32x4*>(C + n) = f32x4{v[0] * P.alpha, v[1] * P.alpha, v[2] * P.alpha, v[3] * P.alpha};
      *reinterpret_cast<f32x4*>(C + n + 4) = f32x4{v[4] * P.alpha, v[5] * P.alpha, v[6] * P.alpha, v[7] * P.alpha};
    } else {
      for (int r = 0; r < 8; ++r) if (n + r < N) C[n + r] = v[r] * P.alpha;
    }
    return;
  }
  if (!(P.vec16 && n + 7 < N)) {
    epilogue_store<EPI>(P, Cz, auxz, m, n, f32x4{v[0], v[1], v[2], v[3]});
    epilogue_store<EPI>(P, Cz, auxz, m, n + 4, f32x4{v[4], v[5], v[6], v[7]});
    return;
  }
  float x[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) x[r] = v[r] * P.alpha;
  if (epi_adds_bias<EPI>() && P.bias) {
    const h16x8 bv = *reinterpret_cast<const h16x8*>(P.bias + n);
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] += (float)bv[r];
  }
  h16* C = reinterpret_cast<h16*>(Cz) + (long)m * P.ldc;
  auto ld8 = [&](const h16* src, float (&o)[8]) {
    const h16x8 t = *reinterpret_cast<const h16x8*>(src);
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = (float)t[r];
  };
  bool keep[8] = {true, true, true, true, true, true, true, true};
  if (epi_drops<EPI>() && P.thresh) {
    const uint64_t c0 = P.offset + (uint64_t)m * P.ld_rng + n;
    bool k0[4], k1[4];
    mms_keep4(P.seed, c0, P.thresh, k0);
    mms_keep4(P.seed, c0 + 4, P.thresh, k1);
#pragma unroll
    for (int r = 0; r < 4; ++r) { keep[r] = k0[r]; keep[r + 4] = k1[r]; }
  }
  const float dscale = P.thresh ? 1.f / (1.f - P.p) : 1.f;
  float o[8];
  if (EPI == MMS_EPI_RELU_DROP) {
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = keep[r] ? fmaxf(x[r], 0.f) * dscale : 0.f;
  } else if (EPI == MMS_EPI_DROP_RESID) {
    float a[8];
    ld8(auxz + (long)m * P.ldaux + n, a);
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = a[r] + (keep[r] ? x[r] * dscale : 0.f);
  } else if (EPI == MMS_EPI_GATE) {
    float ov[8], tv[8], g[8];
    ld8(auxz + (long)m * P.ldaux + n, ov);
    ld8(auxz + (long)m * P.ldaux + N + n, tv);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      g[r] = sigmoidf_(x[r]);
      o[r] = tv[r] + g[r] * (ov[r] - tv[r]);
    }
    h16x8 gv;
#pragma unroll
    for (int r = 0; r < 8; ++r) gv[r] = (h16)g[r];
    *reinterpret_cast<h16x8*>(P.out2 + (long)m * P.ldo2 + n) = gv;
  } else if (EPI == MMS_EPI_RELU_DROP_BWD) {
    float h[8];
    ld8(auxz + (long)m * P.ldaux + n, h);
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = h[r] > 0.f ? x[r] * dscale : 0.f;
  } else if (EPI == MMS_EPI_F16_ACC) {
    float c[8];
    ld8(C + n, c);
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = c[r] + x[r];
  } else if (EPI == MMS_EPI_GELU_DROP) {
    h16x8 zv;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      zv[r] = (h16)x[r];
      o[r] = keep[r] ? gelu_erf((float)zv[r]) * dscale : 0.f;
    }
    *reinterpret_cast<h16x8*>(P.out2 + (long)m * P.ldo2 + n) = zv;
  } else if (EPI == MMS_EPI_GELU_DROP_BWD) {
    float z[8];
    ld8(auxz + (long)m * P.ldaux + n, z);
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = keep[r] ? x[r] * dscale * gelu_grad_(z[r]) : 0.f;
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = x[r];
  }
  h16x8 ov8;
#pragma unroll
  for (int r = 0; r < 8; ++r) ov8[r] = (h16)o[r];
  *reinterpret_cast<h16x8*>(C + n) = ov8;
}

// Block -> (z, tm, tn).  The grid is 1-D over tiles_m * tiles_n * nz.  Workgroups are dispatched
// round-robin over the 8 XCDs, each with a private 4 MiB L2, so the linear id is first remapped
// (bijectively) to give every XCD one contiguous range of the z-major tile space: a split-K
// slice, or a batch entry, stays on one XCD.  Inside a z slice tiles go in groups of GROUP_M
// tile-rows, column by column, so the ~64 blocks an XCD runs at once share 8 A row-panels and 8
// B column-panels (~3 MiB at K = 768) instead of streaming the whole B operand per row.
MMS_DEV void tile_coords(int bid, int tiles_m, int tiles_n, int total, int& z, int& tm, int& tn, int GROUP_M) {
  const int q = total / 8, r = total % 8, x = bid % 8;
  const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
  const int ntiles = tiles_m * tiles_n;
  z = id / ntiles;
  const int t = id % ntiles;
  const int per_group = GROUP_M * tiles_n;
  const int g = t / per_group, first_m = g * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int w = t % per_group;
  tm = first_m + w % gsize;
  tn = w / gsize;
}

// Register epilogue (round 6): for the epilogues whose element math needs no operand in row-major
// order (plain / bias, ReLU-dropout) the math runs on the accumulators in the MFMA layout (lane l:
// row 16 i + (l & 15), columns 16 j + 4 (l >> 4) .. + 3), the fp16 results go through the wave's own
// LDS slot (FR x 16 rows x 128 B, half the bytes of the fp32 staging, one pass for up to 8 fragments)
// and come back row-major for 16-B stores of whole 128-B row segments.  Same per-element arithmetic
// and the same dropout counters as the staged path: bit-identical.  The slot is written and read by
// one wave only, so no workgroup barrier sits between the two.  The NT LDS-DMA kernels use the
// permuted form below (perm_epilogue), which also carries the operand-reading epilogues; this one
// serves the kernels whose weight rows are not permuted (register-staged, 256x256, TN / NN, grouped).
template <int EPI>
constexpr bool epi_regs() { return EPI == MMS_EPI_F16 || EPI == MMS_EPI_RELU_DROP; }

// The choice between this and the staged path must be the same for every wave of a block: the two
// lay their LDS slots out differently (the tall kernel packs the fp16 slots) and the staged path
// holds workgroup barriers.  N % 64 == 0 makes every wave's 64 columns lie wholly inside N or wholly
// outside it (such a wave has nothing to do).
MMS_DEV bool reg_epilogue_ok(const GemmP& P) { return P.vec16 == 1 && P.N % 64 == 0; }   // 3: staged (test hook)

// rows bm + 64 wm + 16 i + (l & 15), columns bn + 64 wn ..+ 64 (caller: reg_epilogue_ok(P));
// SLOTB: bytes between consecutive waves' slots (>= FR * 2048)
template <int EPI, int FR, int SLOTB>
MMS_DEV void reg_epilogue(const GemmP& P, char* smem, const f32x4 (&acc)[FR][4], int bm, int bn, int wm, int wn,
                          int wid, int lane, void* Cz) {
  static_assert(SLOTB >= FR * 2048, "staging slot too small");
  if (bn + wn * 64 >= P.N) return;   // wave-uniform: all 64 columns past N
  char* stage = smem + wid * SLOTB;
  const int rl = lane & 15, g = lane >> 4;
  const int m0 = bm + wm * 64 + rl, nw = bn + wn * 64 + 4 * g;
  float bv[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[j][e] = 0.f;
  if (epi_adds_bias<EPI>() && P.bias) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const h16x4 b4 = *reinterpret_cast<const h16x4*>(P.bias + nw + 16 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[j][e] = (float)b4[e];
    }
  }
  constexpr bool DROPS = epi_drops<EPI>();
  const float dscale = P.thresh ? 1.f / (1.f - P.p) : 1.f;
  // the lane's 4 FR runs: rows m0 + 16 i, columns nw + 16 j .. + 3
  KeepRuns<4> kr;
  if (DROPS && P.thresh)
    kr.init(P, P.offset + (uint64_t)m0 * P.ld_rng + nw,
            P.offset + (uint64_t)(m0 + 16 * (FR - 1)) * P.ld_rng + nw + 51);
#pragma unroll
  for (int i = 0; i < FR; ++i) {
    const int rr = i * 16 + rl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bool keep[4] = {true, true, true, true};
      if (DROPS && P.thresh)   // (dpair: 16 i rows and 16 j columns on, in pairs; ld_rng even on that path)
        kr.run(P, (uint32_t)(8 * i) * (uint32_t)P.ld_rng + 8 * j, m0 + 16 * i, nw + 16 * j, keep);
      h16x4 o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h16 o2 = (h16)0.f;   // (no form served here writes out2)
        o4[e] = (h16)epi_element<EPI>(acc[i][j][e] * P.alpha + bv[j][e], 0.f, 0.f, keep[e], dscale, o2);
      }
      // 16-B chunk 2 j + (g >> 1) of row rr, 8-B half g & 1; chunks XOR-swizzled by (rr >> 1) & 7 and
      // halves by rr & 1: a ds_write_b64 16-lane group (16 rows, one (j, g)) covers the 32 write banks
      // once, ds_read_b128's lane groups read distinct chunks (PMC: SQ_LDS_BANK_CONFLICT 0)
      const int ch = (2 * j + (g >> 1)) ^ ((rr >> 1) & 7);
      *reinterpret_cast<h16x4*>(stage + rr * 128 + (ch << 4) + (((g ^ rr) & 1) << 3)) = o4;
    }
  }
  // the slot is re-read by other lanes of this wave: drain its LDS writes first (DS operations of a
  // wave complete in order, the wait makes that explicit at the cost of one short stall)
  // (same-box A/B with / without the wait: step 15.58-15.60 vs 15.57-15.66 ms, profiles/round6_reg_epilogue_drain_ab.txt)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  const int q = lane & 7;
  h16* C = reinterpret_cast<h16*>(Cz);
  const int n = bn + wn * 64 + 8 * q;
#pragma unroll
  for (int pass = 0; pass < 2 * FR; ++pass) {
    const int rr = pass * 8 + (lane >> 3);
    typedef unsigned int u32x4_ __attribute__((ext_vector_type(4)));
    u32x4_ v = *reinterpret_cast<const u32x4_*>(stage + rr * 128 + ((q ^ ((rr >> 1) & 7)) << 4));
    if (rr & 1) v = u32x4_{v[2], v[3], v[0], v[1]};   // odd rows store their two halves swapped
    const int m = bm + wm * 64 + rr;
    if (m < P.M) *reinterpret_cast<u32x4_*>(C + (long)m * P.ldc + n) = v;
  }
}

// Permuted register epilogue: the NT LDS-DMA kernels (gemm_dma_kernel<true, true>, gemm_tall_kernel)
// fill LDS row 16 j + 4 g + e of a wave's 64-row strip of the weight from weight row
//   c(j, g, e) = 32 (j >> 1) + 8 g + 4 (j & 1) + e        (perm_row: a rotation of bits 2-4)
// of that strip (the source address of the DMA is per lane, the LDS image and the fragment reads do
// not change).  Accumulator (j, g, e) is then output column c(j, g, e): per row a lane owns columns
// 32 h + 8 g .. + 7 (h = 0, 1: accumulators 2 h and 2 h + 1), two whole 16-B runs, so the epilogues
// that read a row operand (residual, pre-activation, gate, accumulated C) load it straight into the
// MFMA layout with 16-B loads — issued under the last k-step (perm_prefetch), not behind the k-loop
// and a barrier — and the element math runs on the accumulators.  Same expressions, fp32 -> fp16
// rounding points and dropout counters (offset + m ld_rng + n of the element's true (m, n)) as the
// staged path: bit-identical.  Launch-uniform choice (reg_epilogue_ok), as for reg_epilogue.
// The results go out through the wave's fp16 slot (whole 128-B row segments); storing a lane's two
// 16-B runs straight from the MFMA layout (16 rows x 64 B per instruction, no LDS) measured level
// and is not in the tree.
template <int EPI>
constexpr bool epi_perm() {
  return EPI == MMS_EPI_F16 || EPI == MMS_EPI_RELU_DROP || EPI == MMS_EPI_DROP_RESID || EPI == MMS_EPI_GATE ||
         EPI == MMS_EPI_RELU_DROP_BWD || EPI == MMS_EPI_F16_ACC;
}
MMS_DEV int perm_row(int r) { return (r & ~0x1c) | ((r & 0x0c) << 1) | ((r & 0x10) >> 2); }

// a wave's row operands in the MFMA layout: [i][h] = row 16 i + (l & 15), columns 32 h + 8 (l >> 4) .. + 7
template <int EPI, int FR>
struct PermOperands {
  h16x8 ax[FR][2];                              // aux row / existing C
  h16x8 ax2[EPI == MMS_EPI_GATE ? FR : 1][2];   // GATE: aux + N
  h16x8 bias[2];
};

// GATE on a tall tile (FR > 4) loads its two operands in the epilogue instead, one fragment ahead of
// the math: 2 x 2 FR operand vectors beside the k-step's fragments, or beside the epilogue's
// temporaries, spill (192-row tiles)
template <int EPI, int FR>
constexpr bool perm_gate_late() { return EPI == MMS_EPI_GATE && FR > 4; }

// rows bm + 64 wm + 16 i + (l & 15), columns bn + 64 wn ..+ 64 (as reg_epilogue); zero where there is
// nothing to read (rows past M, no bias, a wave whose columns lie past N)
template <int EPI, int FR>
MMS_DEV void perm_prefetch(const GemmP& P, PermOperands<EPI, FR>& op, int bm, int bn, int wm, int wn, int lane,
                           const void* Cz, const h16* auxz) {
  h16x8 z8;
#pragma unroll
  for (int e = 0; e < 8; ++e) z8[e] = (h16)0.f;
  constexpr bool LOADS = epi_reads_row<EPI>() && !perm_gate_late<EPI, FR>();
  op.bias[0] = op.bias[1] = z8;
#pragma unroll
  for (int i = 0; i < FR; ++i) op.ax[i][0] = op.ax[i][1] = z8;
#pragma unroll
  for (int i = 0; i < (EPI == MMS_EPI_GATE ? FR : 1); ++i) op.ax2[i][0] = op.ax2[i][1] = z8;
  if (bn + wn * 64 >= P.N) return;   // wave-uniform
  const int m0 = bm + wm * 64 + (lane & 15), nw = bn + wn * 64 + 8 * (lane >> 4);
  if (epi_adds_bias<EPI>() && P.bias) {
#pragma unroll
    for (int h = 0; h < 2; ++h) op.bias[h] = *reinterpret_cast<const h16x8*>(P.bias + nw + 32 * h);
  }
  if (LOADS) {
    const h16* src = EPI == MMS_EPI_F16_ACC ? reinterpret_cast<const h16*>(Cz) : auxz;
    const long ld = EPI == MMS_EPI_F16_ACC ? P.ldc : P.ldaux;
#pragma unroll
    for (int i = 0; i < FR; ++i) {
      const int m = m0 + 16 * i;
      if (m < P.M) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          op.ax[i][h] = *reinterpret_cast<const h16x8*>(src + (long)m * ld + nw + 32 * h);
          if (EPI == MMS_EPI_GATE)
            op.ax2[EPI == MMS_EPI_GATE ? i : 0][h] = *reinterpret_cast<const h16x8*>(src + (long)m * ld + P.N + nw + 32 * h);
        }
      }
    }
  }
}

// caller: reg_epilogue_ok(P), the weight rows permuted, op from perm_prefetch with the same arguments
template <int EPI, int FR, int SLOTB>
MMS_DEV void perm_epilogue(const GemmP& P, char* smem, const f32x4 (&acc)[FR][4], PermOperands<EPI, FR>& op,
                           int bm, int bn, int wm, int wn, int wid, int lane, void* Cz, const h16* auxz) {
  static_assert(SLOTB >= FR * 2048, "staging slot too small");
  if (bn + wn * 64 >= P.N) return;   // wave-uniform: all 64 columns past N
  // GATE on a tall tile: fragment i + 1's operands are loaded ahead of fragment i's math (by themselves
  // the loads cannot move up past the previous fragment's out2 stores)
  constexpr bool GATE_LATE = perm_gate_late<EPI, FR>();
  h16x8 nx[2], nx2[2];
  auto load_gate = [&](int i) {
    const int m = bm + wm * 64 + (lane & 15) + 16 * i;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      nx[h] = nx2[h] = op.bias[h];   // (any defined value: rows past M are not stored)
      if (m < P.M) {
        const h16* src = auxz + (long)m * P.ldaux + bn + wn * 64 + 8 * (lane >> 4) + 32 * h;
        nx[h] = *reinterpret_cast<const h16x8*>(src);
        nx2[h] = *reinterpret_cast<const h16x8*>(src + P.N);
      }
    }
  };
  if (GATE_LATE) load_gate(0);
  char* stage = smem + wid * SLOTB;
  const int rl = lane & 15, g = lane >> 4;
  const int m0 = bm + wm * 64 + rl, nw = bn + wn * 64 + 8 * g;
  h16* C = reinterpret_cast<h16*>(Cz);
  float bv[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[h][e] = (float)op.bias[h][e];   // zero without a bias
  constexpr bool DROPS = epi_drops<EPI>();
  const float dscale = P.thresh ? 1.f / (1.f - P.p) : 1.f;
  // the lane's 2 FR runs: rows m0 + 16 i, columns nw + 32 h .. + 7
  KeepRuns<8> kr;
  if (DROPS && P.thresh)
    kr.init(P, P.offset + (uint64_t)m0 * P.ld_rng + nw,
            P.offset + (uint64_t)(m0 + 16 * (FR - 1)) * P.ld_rng + nw + 39);
#pragma unroll
  for (int i = 0; i < FR; ++i) {
    const int rr = i * 16 + rl, m = m0 + 16 * i;
    if (GATE_LATE) {
#pragma unroll
      for (int h = 0; h < 2; ++h) { op.ax[0][h] = nx[h]; op.ax2[0][h] = nx2[h]; }
      if (i + 1 < FR) load_gate(i + 1);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = acc[i][2 * h + (e >> 2)][e & 3] * P.alpha + bv[h][e];
      bool keep[8] = {true, true, true, true, true, true, true, true};
      if (DROPS && P.thresh)   // (dpair: 16 i rows and 32 h columns on, in pairs; ld_rng even on that path)
        kr.run(P, (uint32_t)(8 * i) * (uint32_t)P.ld_rng + 16 * h, m, nw + 32 * h, keep);
      const h16x8& a8 = op.ax[GATE_LATE ? 0 : i][h];
      const h16x8& t8 = op.ax2[(EPI == MMS_EPI_GATE && !GATE_LATE) ? i : 0][h];   // GATE only
      h16x8 o8, p8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        h16 o2 = (h16)0.f;
        o8[e] = (h16)epi_element<EPI>(x[e], (float)a8[e], (float)t8[e], keep[e], dscale, o2);
        p8[e] = o2;
      }
      if (epi_writes_out2<EPI>() && m < P.M) *reinterpret_cast<h16x8*>(P.out2 + (long)m * P.ldo2 + nw + 32 * h) = p8;
      // 16-B chunk 4 h + g of row rr, XOR-swizzled by rr & 7: a ds_write_b128 group (8 lanes: 8 rows,
      // one chunk) covers the 32 write banks once; the read-back's lane groups read distinct chunks
      *reinterpret_cast<h16x8*>(stage + rr * 128 + (((4 * h + g) ^ (rr & 7)) << 4)) = o8;
    }
  }
  // the slot is re-read by other lanes of this wave: drain its LDS writes first (as reg_epilogue)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  const int q = lane & 7;
  const int n = bn + wn * 64 + 8 * q;
#pragma unroll
  for (int pass = 0; pass < 2 * FR; ++pass) {
    const int rr = pass * 8 + (lane >> 3);
    typedef unsigned int u32x4_ __attribute__((ext_vector_type(4)));
    const u32x4_ v = *reinterpret_cast<const u32x4_*>(stage + rr * 128 + ((q ^ (rr & 7)) << 4));
    const int mr = bm + wm * 64 + rr;
    if (mr < P.M) *reinterpret_cast<u32x4_*>(C + (long)mr * P.ldc + n) = v;
  }
}

// Epilogue through LDS: each wave parks its 64x64 fp32 accumulator tile in 16 KiB of the (now idle)
// operand ring, XOR-swizzled by row, then re-reads it row-major so a lane owns 8 consecutive
// columns: every global load/store of the epilogue covers whole 128-B row segments instead of
// 16 rows x 32 B.  Caller guarantees all waves are past their last operand read.
// FR: 16-row fragments of the wave's tile in this pass (4 = 64 rows; 2 = 32 rows); SLOT: floats of
// LDS between consecutive waves' staging areas (>= FR * 16 * 64)
template <int EPI, int FR = 4, int SLOT = 64 * 64>
MMS_DEV void staged_epilogue(const GemmP& P, char* smem, const f32x4 (&acc)[FR][4], int bm, int bn,
                             int wm, int wn, int wid, int lane, void* Cz, const h16* auxz) {
  static_assert(SLOT >= FR * 16 * 64, "staging slot too small");
  if constexpr (epi_regs<EPI>()) {
    if (reg_epilogue_ok(P)) {   // launch-uniform: every wave of the block takes the same path
      reg_epilogue<EPI, FR, SLOT * 4>(P, smem, acc, bm, bn, wm, wn, wid, lane, Cz);
      return;
    }
  }
  constexpr int PASSES = FR * 2;   // 8 rows per pass
  float* stage = reinterpret_cast<float*>(smem) + wid * SLOT;
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = i * 16 + (lane & 15);
      const int c = j * 4 + (lane >> 4);
      *reinterpret_cast<f32x4*>(stage + r * 64 + ((c ^ (r & 15)) << 2)) = acc[i][j];
    }
  __syncthreads();
  const int q = lane & 7;
  const int n = bn + wn * 64 + 8 * q;
  auto stage8 = [&](int r, float (&v)[8]) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(stage + r * 64 + (((2 * q) ^ (r & 15)) << 2));
    const f32x4 hi = *reinterpret_cast<const f32x4*>(stage + r * 64 + (((2 * q + 1) ^ (r & 15)) << 2));
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  };
  if (EPI == MMS_EPI_F32 || !(P.vec16 && n + 7 < P.N)) {
#pragma unroll 2
    for (int pass = 0; pass < PASSES; ++pass) {
      const int r = pass * 8 + (lane >> 3);
      float v[8];
      stage8(r, v);
      epilogue_store8<EPI>(P, Cz, auxz, bm + wm * 64 + r, n, v);
    }
    return;
  }
  // Fast path (every fp16 row operand 16-B aligned, 8 whole columns): the global operand loads of
  // all 8 rows (aux / existing C, bias) are issued before the first store.  Interleaved per row,
  // hipcc must keep each row's loads behind the previous row's stores (they may alias), which
  // serialised the epilogue into 8 dependent global round trips.
  const int m0 = bm + wm * 64 + (lane >> 3);
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (epi_adds_bias<EPI>() && P.bias) {
    const h16x8 b8 = *reinterpret_cast<const h16x8*>(P.bias + n);
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = (float)b8[e];
  }
  h16* C = reinterpret_cast<h16*>(Cz);
  h16x8 ax[8], ax2[8];
  const h16x8 z8 = {(h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f};
#pragma unroll
  for (int pass = 0; pass < PASSES; ++pass) {
    const int m = m0 + 8 * pass;
    ax[pass] = z8;
    ax2[pass] = z8;
    if (epi_reads_row<EPI>() && m < P.M) {
      if (EPI == MMS_EPI_F16_ACC) {
        ax[pass] = *reinterpret_cast<const h16x8*>(C + (long)m * P.ldc + n);
      } else {
        ax[pass] = *reinterpret_cast<const h16x8*>(auxz + (long)m * P.ldaux + n);
        if (EPI == MMS_EPI_GATE) ax2[pass] = *reinterpret_cast<const h16x8*>(auxz + (long)m * P.ldaux + P.N + n);
      }
    }
  }
  const float dscale = P.thresh ? 1.f / (1.f - P.p) : 1.f;
  constexpr bool DROPS = epi_drops<EPI>();
  // the lane's PASSES runs: rows m0 + 8 pass, columns n .. n + 7
  KeepRuns<8> kr;
  if (DROPS && P.thresh)
    kr.init(P, P.offset + (uint64_t)m0 * P.ld_rng + n,
            P.offset + (uint64_t)(m0 + 8 * (PASSES - 1)) * P.ld_rng + n + 7);
#pragma unroll
  for (int pass = 0; pass < PASSES; ++pass) {
    const int m = m0 + 8 * pass;
    if (m >= P.M) continue;
    float x[8];
    stage8(pass * 8 + (lane >> 3), x);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = x[e] * P.alpha + bv[e];
    bool keep[8] = {true, true, true, true, true, true, true, true};
    if (DROPS && P.thresh)   // (dpair: 8 pass rows on, in pairs; ld_rng even on that path)
      kr.run(P, (uint32_t)(4 * pass) * (uint32_t)P.ld_rng, m, n, keep);
    h16x8 o8, p8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      h16 o2 = (h16)0.f;
      o8[e] = (h16)epi_element<EPI>(x[e], (float)ax[pass][e], (float)ax2[pass][e], keep[e], dscale, o2);
      p8[e] = o2;
    }
    if (epi_writes_out2<EPI>()) *reinterpret_cast<h16x8*>(P.out2 + (long)m * P.ldo2 + n) = p8;
#if defined(MMS_LAB_NOSTORE)   // lab ablation build (scripts/micro): the epilogue without its C stores
    asm volatile("" ::"v"(o8));
#else
    *reinterpret_cast<h16x8*>(C + (long)m * P.ldc + n) = o8;
#endif
  }
}

// ------------------------------------------------------------------------------------------
// BK = 32 variant: 16 KiB stages, a 4-deep ring in the same 64 KiB (2 blocks per CU), so two
// k-tiles stay in flight across every barrier (counted vmcnt, raw s_barrier) instead of one.
// K-contiguous images are [128 rows][32 k] (64-B rows, chunk ^ f(row), f = bits 1,2 of the
// row: conflict-free for ds_read_b128's lane groups); MN-contiguous images are the BK = 64
// layout's first 32 k-rows.
// ------------------------------------------------------------------------------------------
constexpr int BK32 = 32, T32_BYTES = 128 * 32 * 2, ST32 = 4;
MMS_DEV int swz32(int r) { return ((r >> 1) & 1) | (((r >> 2) & 1) << 1); }

template <bool KC>
MMS_DEV h16x8 read_frag32(const char* lds, int sub, int lane) {
  if (KC) {
    const int r = sub + (lane & 15);
    const int c = lane >> 4;
    s16x8 v = *reinterpret_cast<const s16x8*>(lds + r * 64 + ((c ^ swz32(r)) << 4));
    return __builtin_bit_cast(h16x8, v);
  }
  return read_frag<false>(lds, sub, 0, lane);
}

typedef __attribute__((address_space(3))) void lds_void;

// one 128-row x 64-k operand stage by LDS-DMA: 16 wave-instructions, wave `wid` issues 4.
// perm (K-contiguous weight of a permuted-epilogue launch): LDS row r comes from operand row
// perm_row(r); the chunk swizzle stays that of the LDS row, which is what the fragment reads undo
template <bool KC>
MMS_DEV void dma_tile(__amdgpu_buffer_rsrc_t rs, char* lds, long ld, int row0, int k0rel, int wid, int lane,
                      bool perm = false) {
#ifdef MMS_GEMM_NODMA   // ablation build: no operand traffic (garbage output)
  return;
#endif
  // 16 wave-instructions per 16 KiB tile: wave `wid` issues 4 of them
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ins = wid * 4 + i;
    int voff;
    if (KC) {
      const int row = ins * 8 + (lane >> 3), slot = lane & 7;
      const int c = slot ^ (row & 7);
      voff = (int)(((long)(row0 + (perm ? perm_row(row) : row)) * ld + k0rel + c * 8) * 2);
    } else {
      const int kr = ins * 4 + (lane >> 4), slot = lane & 15;
      const int c = slot ^ swz_mn(kr);
      voff = (int)(((long)(k0rel + kr) * ld + row0 + c * 8) * 2);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(lds + ins * 1024), 16, voff, 0, 0, 0);
  }
}

template <int N>
MMS_DEV void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

#define MMS_EPI_CASES CASE(MMS_EPI_F16) CASE(MMS_EPI_RELU_DROP) CASE(MMS_EPI_DROP_RESID) CASE(MMS_EPI_F32) \
    CASE(MMS_EPI_GATE) CASE(MMS_EPI_RELU_DROP_BWD) CASE(MMS_EPI_F16_ACC) CASE(MMS_EPI_GELU_DROP) CASE(MMS_EPI_GELU_DROP_BWD)

}  // namespace
