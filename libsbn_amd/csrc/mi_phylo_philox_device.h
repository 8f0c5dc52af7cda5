// Philox4x32-10 (Salmon et al. 2011) for the kernels that draw random numbers: the topology
// sampler (kernels_sbn_vi.hip) and the branch-length models (kernels_branch_model.hip).  Multipliers
// D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85.  Inline: each .hip file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace miphylo {
namespace dev {

__device__ __forceinline__ void philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1;
  c[3] = (uint32_t)p0;
  c[0] = n0;
  c[2] = n2;
}

// the ten rounds: c holds the counter on entry and the four output words on return
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint64_t key) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the standard normal of edge v of sample s (mi_engine_branch_model_sample): counter (v, 1, s lo, s hi),
// the Box-Muller form of the first two and the last two output words
__device__ __forceinline__ double philox_normal(uint64_t seed, uint64_t s, uint32_t v) {
  uint32_t c[4] = {v, 1u, (uint32_t)s, (uint32_t)(s >> 32)};
  philox4x32_10(c, seed);
  const uint64_t b1 = ((uint64_t)c[0] << 32) | c[1], b2 = ((uint64_t)c[2] << 32) | c[3];
  const double u1 = (double)((b1 >> 11) + 1) * 0x1.0p-53, u2 = (double)(b2 >> 11) * 0x1.0p-53;
  return sqrt(-2.0 * log(u1)) * cos((2.0 * M_PI) * u2);
}

}  // namespace dev
}  // namespace miphylo
