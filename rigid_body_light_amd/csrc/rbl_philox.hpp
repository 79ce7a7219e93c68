// rbl_philox.hpp -- Philox-4x32-10, the counter-based generator of k_normal (rbl_kernels.hip) and of the Metropolis sampler
// (rbl_ens_mc.hip): ONE copy of the rounds.  c: the 128-bit counter, replaced by the block's four output words; (k0, k1): the key.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
