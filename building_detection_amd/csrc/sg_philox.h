// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the engine's only
// random number generator: a pure function of a 128-bit counter and a 64-bit key, so a kernel needs no state and no launch
// geometry to say which numbers an element gets.  Plain integer C++, host and device (the host form serves stand-alone checks
// of the known answers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t SG_PHILOX_M0 = 0xD2511F53u, SG_PHILOX_M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t SG_PHILOX_W0 = 0x9E3779B9u, SG_PHILOX_W1 = 0xBB67AE85u;   // Weyl constants of the key schedule

struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 sg_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)SG_PHILOX_M0 * c0, p1 = (uint64_t)SG_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += SG_PHILOX_W0;   // (the bump after the last round is dead code)
    k1 += SG_PHILOX_W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four words of mask indices 4q .. 4q + 3: counter (q mod 2^32, q >> 32, stream, step), key (k0, k1)
__host__ __device__ __forceinline__ Philox4 sg_mask_words(uint64_t q, uint32_t stream, uint32_t step, uint32_t k0, uint32_t k1) {
  return sg_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), stream, step, k0, k1);
}
