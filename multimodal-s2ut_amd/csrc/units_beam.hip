// Beam decode of speech units: the reference's scripts/speech_to_speech_translation/mhubert.py
// HubertCode.decode(beamsearch=True) (lines 70-85) over the frames' top_k nearest centroids and their
// distances (units.hip kmeans_topk), as it evaluates in float32 (NumPy >= 2), host restatement
// units.beam_decode_host.  The reference rebuilds and re-groups every candidate's token list at every
// frame; here a kept sequence is (score, run count, last token) in LDS and a frame costs one sort.
//
//   units_beam   one block per utterance of T = lens[b] frames.  Frame t: the n_seq * top_k <= 2048
//                candidates (sequence seq, j-th nearest centroid) are scored
//                  f32(score + f32(f32(m / T) * f32(dist[t, j] / s)))
//                with m the candidate's run count (the parent's, plus 1 where the token differs from the
//                parent's last), m / T formed in double, s the frame's distances summed in numpy's
//                pairwise order.  The reference's sort is stable over (sequence, j) order, so a
//                candidate's key is its score's bits (positive floats order as their bits) above its
//                index seq * top_k + j: all keys differ, and a bitonic sort of them in LDS gives the
//                reference's order.  The first beamsize are kept; each writes a (parent, token)
//                back-pointer to the workspace.  After the last frame one thread walks sequence 0 back:
//                beam_code, and merged filled from its end (the run count is known from the state).
//
// Integer and fp32 work on fixed orders, no atomics: every run gives the same bits.
#include "common.h"
#include "../../include/mms2ut.h"

// Every operation of the score rounds on its own in the reference (see noise.hip on hipcc's default
// contraction); a / b is IEEE-rounded (hipcc's default, no fast-math in this build).
#pragma clang fp contract(off)

namespace {

constexpr int UB_THREADS = 1024;
constexpr int UB_MAX_CAND = MMS_UNITS_BEAM_MAX_CAND;
constexpr int UB_SLOTS = UB_MAX_CAND / UB_THREADS;        // kept sequences per thread
constexpr int UB_MAX_K = MMS_KMEANS_TOPK_MAX;
static_assert(UB_SLOTS * UB_THREADS == UB_MAX_CAND && (UB_MAX_CAND & (UB_MAX_CAND - 1)) == 0, "candidate limit");

// numpy.sum of k <= 32 contiguous float32 (its pairwise_sum below the 128-element block)
MMS_DEV float ub_pairwise(const float* a, int k) {
  if (k < 8) {
    float r = a[0];
    for (int i = 1; i < k; ++i) r = r + a[i];
    return r;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  const int n8 = k - (k & 7);
  for (int i = 8; i < n8; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
  }
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (int i = n8; i < k; ++i) res = res + a[i];
  return res;
}

__global__ void __launch_bounds__(UB_THREADS) units_beam_kernel(
    const int* __restrict__ idx, const float* __restrict__ dist, int Tmax, const int* __restrict__ lens, int k,
    int beamsize, int2* __restrict__ bp, int* __restrict__ code, int* __restrict__ merged, int* __restrict__ count,
    int* __restrict__ bad) {
  __shared__ unsigned long long keys[UB_MAX_CAND];
  __shared__ float sc[UB_MAX_CAND];                       // the kept sequences: score, run count, last token
  __shared__ int rn[UB_MAX_CAND], lt[UB_MAX_CAND];
  __shared__ int fi[UB_MAX_K];                            // the frame's candidates
  __shared__ float fv[UB_MAX_K];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int T = lens ? min(max(lens[b], 0), Tmax) : Tmax;
  const long row0 = (long)b * Tmax;
  if (tid == 0) {
    sc[0] = 1.f;
    rn[0] = 0;
    lt[0] = 0;
  }
  int nseq = 1, sbad = 0;
  for (int t = 0; t < T; ++t) {
    if (tid < k) {
      fi[tid] = idx[(row0 + t) * k + tid];
      fv[tid] = dist[(row0 + t) * k + tid];
    }
    __syncthreads();                                      // also orders the state written by the last frame
    const float s = ub_pairwise(fv, k);
    if (!(s > 0.f && isfinite(s))) sbad = 1;
    const int ncand = nseq * k;
    int N = 1;
    while (N < ncand) N <<= 1;
    for (int c = tid; c < N; c += UB_THREADS) {
      unsigned long long key = ~0ull;                     // the padding sorts behind every candidate
      if (c < ncand) {
        const int seq = c / k, j = c - seq * k;
        const int m = rn[seq] + ((t == 0 || fi[j] != lt[seq]) ? 1 : 0);
        const float rate = (float)((double)m / (double)T);
        const float r = fv[j] / s;
        const float inc = rate * r;
        const float ns = sc[seq] + inc;
        key = ((unsigned long long)__float_as_uint(ns) << 32) | (unsigned)c;
      }
      keys[c] = key;
    }
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int p = tid; p < (N >> 1); p += UB_THREADS) {
          const int i = 2 * p - (p & (stride - 1)), j = i + stride;
          const unsigned long long a = keys[i], c = keys[j];
          if ((a > c) == ((i & size) == 0)) {
            keys[i] = c;
            keys[j] = a;
          }
        }
        __syncthreads();
      }
    const int nnew = min(beamsize, ncand);
    float ns[UB_SLOTS];
    int nr[UB_SLOTS], nl[UB_SLOTS];
#pragma unroll
    for (int u = 0; u < UB_SLOTS; ++u) {
      const int i = tid + u * UB_THREADS;
      ns[u] = 0.f;
      nr[u] = nl[u] = 0;
      if (i < nnew) {
        const unsigned long long key = keys[i];
        const int c = (int)(unsigned)key, seq = c / k, j = c - seq * k;   // c < ncand: a candidate, never padding
        nl[u] = fi[j];
        ns[u] = __uint_as_float((unsigned)(key >> 32));
        nr[u] = rn[seq] + ((t == 0 || nl[u] != lt[seq]) ? 1 : 0);
        bp[(row0 + t) * beamsize + i] = make_int2(seq, nl[u]);
      }
    }
    __syncthreads();                                      // every read of the old state is done
#pragma unroll
    for (int u = 0; u < UB_SLOTS; ++u) {
      const int i = tid + u * UB_THREADS;
      if (i < nnew) {
        sc[i] = ns[u];
        rn[i] = nr[u];
        lt[i] = nl[u];
      }
    }
    nseq = nnew;
  }
  __syncthreads();                                        // the state and the block's back-pointers are visible
  if (tid != 0) return;
  const int runs = T > 0 ? rn[0] : 0;
  int p = 0, rem = 0, prev = 0;
  for (int t = T - 1; t >= 0; --t) {
    const int2 e = bp[(row0 + t) * beamsize + p];
    code[row0 + t] = e.y;
    if (t == T - 1 || e.y != prev) {                      // a run starts here, seen from the end
      ++rem;
      if (rem <= runs) merged[row0 + runs - rem] = e.y;
    }
    prev = e.y;
    p = e.x;
  }
  count[b] = runs;
  bad[b] = sbad;
}

}  // namespace

extern "C" int mms2ut_units_beam_ws(int B, int Tmax, int beamsize, int64_t* bytes) {
  MMS_REQUIRE(bytes && B >= 1 && Tmax >= 1 && beamsize >= 1 && beamsize <= UB_MAX_CAND,
              "units_beam_ws: B %d, Tmax %d, beamsize %d", B, Tmax, beamsize);
  *bytes = (int64_t)B * Tmax * beamsize * (int64_t)sizeof(int2);
  return 0;
}

extern "C" int mms2ut_units_beam(const int32_t* idx, const float* dist, int B, int Tmax, const int32_t* lens, int top_k,
                                 int beamsize, void* ws, int32_t* beam_code, int32_t* merged, int32_t* count,
                                 int32_t* bad, hipStream_t s) {
  MMS_REQUIRE(idx && dist && ws && beam_code && merged && count && bad, "units_beam: null buffer");
  MMS_REQUIRE(((uintptr_t)ws & 7) == 0, "units_beam: misaligned workspace");
  MMS_REQUIRE(B >= 1 && B <= 65535 && Tmax >= 1 && (long)B * Tmax < (1L << 31), "units_beam: B %d, Tmax %d", B, Tmax);
  MMS_REQUIRE(top_k >= 1 && top_k <= UB_MAX_K, "units_beam: top_k must be in [1, %d] (got %d)", UB_MAX_K, top_k);
  MMS_REQUIRE(beamsize >= 1 && (long)beamsize * top_k <= UB_MAX_CAND,
              "units_beam: beamsize * top_k must be in [1, %d] (got %d x %d)", UB_MAX_CAND, beamsize, top_k);
  hipLaunchKernelGGL(units_beam_kernel, dim3(B), dim3(UB_THREADS), 0, s, idx, dist, Tmax, lens, top_k, beamsize,
                     reinterpret_cast<int2*>(ws), beam_code, merged, count, bad);
  return mms::check_launch("units_beam");
}
