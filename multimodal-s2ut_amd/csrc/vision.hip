// Image front end of the ViT feature extractor (multimodal-s2ut_amd/vision.py): decoded RGB images in,
// fp16 patch rows for the patch-embedding GEMM out, one launch for the whole batch.  It restates timm's
// eval transform for the vit_*_patch16_384 models -- torchvision Resize(S, bicubic) on a PIL image,
// CenterCrop(S), ToTensor, Normalize -- whose resample is Pillow's 8-bit Image.resize(BICUBIC): a
// horizontal pass, then a vertical pass, integer coefficients of 22 fractional bits, the intermediate
// rounded to uint8.
//
// Nothing here does float arithmetic.  The host computes, in double as Pillow does, the coefficient rows
// of the cropped S x S window only ((first source index, taps) per output index and `taps` int32
// coefficients), and the 3 x 256 fp16 table of the normalisation; a pixel of either pass is
// clamp((2^21 + sum pix * k) >> 22, 0, 255), the sum in int32 as in Pillow.
//
// vision_patch_kernel, grid ((S/P)^2, B), one block per output patch:
//   1. the horizontal pass for the patch's P columns over the source rows its P output rows read,
//      into a uint8 LDS tile [rows][P][3] (no HBM intermediate; vertically adjacent patches redo the
//      2 x support rows they share);
//   2. the vertical pass from the tile, the table lookup, and the store of the patch's row
//      [3 P P] in (c, py, px) order, the order of conv.weight.reshape(d, -1).
// Sources lie at arbitrary byte offsets in one buffer and are read bytewise (every source byte is read
// by about taps x 1.25 threads of neighbouring blocks, out of L1/L2); stores are 2-byte, coalesced.
// A block whose descriptor or table offsets do not fit the buffers, or whose rows exceed the tile,
// writes nothing: the kernel cannot read or write out of bounds whatever the tables hold.
#include <limits.h>

#include "common.h"
#include "../../include/mms2ut.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int VIS_BITS = 22;                     // Pillow's PRECISION_BITS for 8-bit images: 32 - 8 - 2

MMS_DEV int vis_clip8(int acc) {
  const int v = acc >> VIS_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one axis of one image: S (first, taps) pairs at tab + b, S rows of `stride` coefficients at tab + k
MMS_DEV bool vis_axis_ok(int b, int k, int stride, int S, long tab_len) {
  return stride >= 1 && b >= 0 && k >= 0 && (long)b + 2L * S <= tab_len && (long)k + (long)S * stride <= tab_len;
}

__global__ void __launch_bounds__(VIS_THREADS) vision_patch_kernel(
    const uint8_t* __restrict__ img, long img_bytes, const mms2ut_image_desc* __restrict__ desc,
    const int32_t* __restrict__ tab, long tab_len, const h16* __restrict__ norm, h16* __restrict__ out, int S, int P,
    int max_rows) {
  extern __shared__ uint8_t s_tile[];            // [rows][P][3]
  __shared__ h16 s_norm[3 * 256];
  const int np = S / P, patch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int py0 = (patch / np) * P, px0 = (patch % np) * P;
  const mms2ut_image_desc D = desc[b];
  if (D.w < 1 || D.h < 1 || D.w > MMS_VISION_MAX_SIDE || D.h > MMS_VISION_MAX_SIDE || D.src < 0 ||
      D.src + 3L * D.w * D.h > img_bytes) return;
  if (!vis_axis_ok(D.hb, D.hk, D.hn, S, tab_len) || !vis_axis_ok(D.vb, D.vk, D.vn, S, tab_len)) return;
  const int32_t* hb = tab + D.hb + 2 * px0;
  const int32_t* hk = tab + D.hk + (long)px0 * D.hn;
  const int32_t* vb = tab + D.vb + 2 * py0;
  const int32_t* vk = tab + D.vk + (long)py0 * D.vn;
  int r0 = INT_MAX, r1 = 0;
  for (int i = 0; i < P; ++i) {
    const int f = vb[2 * i], n = min(vb[2 * i + 1], D.vn);
    r0 = min(r0, f);
    r1 = max(r1, f + n);
  }
  r0 = max(r0, 0);
  r1 = min(r1, D.h);
  const int rows = r1 - r0;
  if (rows <= 0 || rows > max_rows) return;      // block-uniform, before the barrier
  for (int i = tid; i < 3 * 256; i += VIS_THREADS) s_norm[i] = norm[i];
  const uint8_t* src = img + D.src;
  const int n1 = rows * P * 3;
  for (int i = tid; i < n1; i += VIS_THREADS) {
    const int c = i % 3, x = (i / 3) % P, r = i / (3 * P);
    const int x0 = hb[2 * x], n = min(hb[2 * x + 1], D.hn);
    const int32_t* k = hk + (long)x * D.hn;
    const uint8_t* p = src + (long)(r0 + r) * D.w * 3 + c;
    int acc = 1 << (VIS_BITS - 1);
    for (int t = 0; t < n; ++t) {
      const int xs = x0 + t;
      if (xs >= 0 && xs < D.w) acc += (int)p[3L * xs] * k[t];
    }
    s_tile[i] = (uint8_t)vis_clip8(acc);
  }
  __syncthreads();
  const int n2 = 3 * P * P;
  h16* o = out + ((long)b * np * np + patch) * n2;
  for (int i = tid; i < n2; i += VIS_THREADS) {
    const int px = i % P, py = (i / P) % P, c = i / (P * P);
    const int y0 = vb[2 * py] - r0, n = min(vb[2 * py + 1], D.vn);
    const int32_t* k = vk + (long)py * D.vn;
    int acc = 1 << (VIS_BITS - 1);
    for (int t = 0; t < n; ++t) {
      const int r = y0 + t;
      if (r >= 0 && r < rows) acc += (int)s_tile[(r * P + px) * 3 + c] * k[t];
    }
    o[i] = s_norm[c * 256 + vis_clip8(acc)];
  }
}

// bad[b] = 1 where row b of x holds an fp16 inf or NaN (exponent bits all ones); rows stay untouched
__global__ void __launch_bounds__(VIS_THREADS) nonfinite_rows_kernel(const h16* __restrict__ x, long ld, long n8,
                                                                     int32_t* __restrict__ bad) {
  const s16x8* row = reinterpret_cast<const s16x8*>(x + (long)blockIdx.y * ld);
  bool found = false;
  for (long i = (long)blockIdx.x * VIS_THREADS + threadIdx.x; i < n8; i += (long)gridDim.x * VIS_THREADS) {
    const s16x8 v = row[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) found |= (v[e] & 0x7c00) == 0x7c00;
  }
  if (found) bad[blockIdx.y] = 1;                // every writer stores the same value
}

}  // namespace

extern "C" int mms2ut_vision_patches(const uint8_t* img, int64_t img_bytes, const mms2ut_image_desc* desc, int B,
                                     const int32_t* tab, int64_t tab_len, const mms2ut_half* norm,
                                     mms2ut_half* out, int S, int P, int max_rows, hipStream_t s) {
  MMS_REQUIRE(B >= 0 && B <= 65535, "vision_patches: B must be in [0, 65535] (got %d)", B);
  MMS_REQUIRE(P >= 1 && S >= P && S % P == 0, "vision_patches: the patch size %d must divide the image size %d", P, S);
  MMS_REQUIRE(max_rows >= 1 && (long)max_rows * P * 3 <= MMS_VISION_TILE_BYTES,
              "vision_patches: a tile of %d rows x %d columns exceeds %d bytes of LDS", max_rows, P, MMS_VISION_TILE_BYTES);
  if (B == 0) return 0;
  MMS_REQUIRE(img && desc && tab && norm && out && img_bytes > 0 && tab_len > 0, "vision_patches: null or empty buffer");
  MMS_REQUIRE(((uintptr_t)desc & 7) == 0 && ((uintptr_t)tab & 3) == 0 && ((uintptr_t)norm & 1) == 0 &&
              ((uintptr_t)out & 1) == 0, "vision_patches: misaligned buffer");
  const int np = S / P;
  hipLaunchKernelGGL(vision_patch_kernel, dim3(np * np, B), dim3(VIS_THREADS), (size_t)max_rows * P * 3, s, img,
                     (long)img_bytes, desc, tab, (long)tab_len, norm, out, S, P, max_rows);
  return mms::check_launch("vision_patches");
}

extern "C" int mms2ut_nonfinite_rows_f16(const mms2ut_half* x, int64_t ld, int B, int64_t n, int32_t* bad,
                                         hipStream_t s) {
  MMS_REQUIRE(B >= 0 && B <= 65535 && n >= 0, "nonfinite_rows: B in [0, 65535] and n >= 0 required");
  if (B == 0 || n == 0) return 0;
  MMS_REQUIRE(x && bad, "nonfinite_rows: null buffer");
  MMS_REQUIRE(((uintptr_t)x & 15) == 0 && ld % 8 == 0 && n % 8 == 0 && (B == 1 || ld >= n),
              "nonfinite_rows: rows must be 16-byte aligned runs of a multiple of 8 elements");
  const long n8 = n / 8;
  const int gx = (int)((n8 + VIS_THREADS - 1) / VIS_THREADS < 64 ? (n8 + VIS_THREADS - 1) / VIS_THREADS : 64);
  hipLaunchKernelGGL(nonfinite_rows_kernel, dim3(gx, B), dim3(VIS_THREADS), 0, s, x, (long)ld, n8, bad);
  return mms::check_launch("nonfinite_rows");
}
