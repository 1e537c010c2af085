// Host build of the dropout stream in csrc/common.h.  tests/test_rng_ref.py cuts the hash functions
// (mms_mix32 .. mms_keep_site, mms_drop_thresh) out of the header into mms_rng_host.inc, compiles this
// file with the system compiler and compares what it prints with the known-answer table and with
// tests/rng_ref.py.  No HIP header and no runtime call: MMS_DEV becomes a plain host inline.
#include <stdint.h>
#include <stdio.h>

#define MMS_DEV static inline
#include "mms_rng_host.inc"

int main() {
  const uint64_t seeds[8] = {0, 0, 0, 0, 77, 77, (1ull << 63) - 1, 0x0123456789abcdefull};
  const uint64_t ctr0[8] = {0, 4097, (1ull << 33) - 3, (1ull << 40) + 1, 0, (1ull << 33) - 3, 0, (1ull << 33) - 3};
  for (int r = 0; r < 8; ++r) {
    printf("u16 %llu %llu", (unsigned long long)seeds[r], (unsigned long long)ctr0[r]);
    for (int i = 0; i < 6; ++i) printf(" %u", mms_hash(seeds[r], ctr0[r] + i));
    printf("\n");
  }
  const float ps[9] = {-1.f, 0.f, 1e-6f, 0.1f, 0.25f, 0.3f, 0.5f, 0.999f, 1.f};
  for (int i = 0; i < 9; ++i) printf("thresh %.9g %u\n", ps[i], mms_drop_thresh(ps[i]));
  // every fast form equals mms_keep on runs inside one high word and across a 2^33 boundary, from
  // even and odd first counters
  const uint64_t starts[6] = {0, 4097, (1ull << 33) - 600, (1ull << 33) - 601, (1ull << 33), (1ull << 40) + 1};
  const uint32_t th = mms_drop_thresh(0.25f);
  long bad = 0;
  for (int s = 0; s < 6; ++s) {
    const uint64_t c0 = starts[s], last = c0 + 1199, seed = 77 + s;
    const MmsSite site = mms_site(seed, c0, last);
    const bool same = mms_same_hi(c0, last);
    const uint32_t hm = mms_hi_mix(seed, c0);
    for (uint64_t c = c0; c + 3 <= last; ++c) {
      bool k[4], ks[4], kh[4];
      mms_keep4(seed, c, th, k);
      mms_keep4_site(site, seed, c, th, ks);
      if (same) mms_keep4_hi(hm, c, th, kh);
      for (int e = 0; e < 4; ++e) {
        const bool ref = mms_keep(seed, c + e, th);
        bad += k[e] != ref;
        bad += ks[e] != ref;
        if (same) bad += kh[e] != ref;
      }
      bad += mms_keep_site(site, seed, c, th) != mms_keep(seed, c, th);
      if (same) bad += mms_keep_hi(hm, c, th) != mms_keep(seed, c, th);
    }
    printf("site %llu same_hi %d\n", (unsigned long long)c0, (int)same);
  }
  printf("fast_path_mismatches %ld\n", bad);
  return bad ? 1 : 0;
}
