// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
// generator of every dropout keep-bit drawn on the device (si_base.hip sites 0 and 1, od_bwd.hip site 2).
// A keep-bit is one word of the block keyed by the two halves of the fit's seed and counted by
// (element / 4, sample id, epoch, site); word = element % 4.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct U4 {
  uint32_t v[4];
};

__device__ inline U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                   uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{{c0, c1, c2, c3}};
}

// the four words of elements 4 q .. 4 q + 3 of the sample with id `sid` at one site
__device__ inline U4 philox_drop_words(uint64_t seed, uint32_t epoch, uint32_t sid, uint32_t q, uint32_t site) {
  return philox4x32_10(q, sid, epoch, site, (uint32_t)seed, (uint32_t)(seed >> 32));
}
