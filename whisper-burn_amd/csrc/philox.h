// The counter-based generator of the device-side draws (sample.hip, tsrules.hip): Philox4x32-10 and the Gumbel variate of
// one of its output words.  One definition, so that both draws produce the same key for the same (id, counters).
#pragma once
#include <hip/hip_runtime.h>

namespace wb {

struct U4 { uint32_t w[4]; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  U4 r;
  r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
  return r;
}

// u = ((word >> 9) + 0.5) 2^-23: exact in f32, inside [2^-24, 1 - 2^-24], so both logarithms are finite
__device__ __forceinline__ float gumbel_of(uint32_t word) {
  const float u = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

}  // namespace wb
