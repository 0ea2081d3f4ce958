// What the two lossless occupancy coders share (occ_rans.hip, occ_hier.hip): the context of a probability, the input
// error rule and the rANS step's division.  include/nvf_hip.h, "lossless geometry", is the contract.
#pragma once
#include "nvf_common.h"

#define OCC_CTX 256
#define OCC_KEY_ONE 0x3F800000u
#define OCC_RANS_L (1ull << 31)

namespace {

// the context of a probability, from its bits alone: which side of 0.5, and the exponent + 2 mantissa bits of the
// distance to the nearer end.  Any bit pattern (NaN, negative, > 1) lands inside [0, 256).
__device__ __forceinline__ int occ_ctx(float p) {
  const int side = p > 0.5f ? 1 : 0;
  const float q = side ? 1.0f - p : p;
  const int key = (int)(__float_as_uint(q) >> 21);
  int idx = (int)(0x3F000000u >> 21) - key;
  idx = idx < 0 ? 0 : (idx > 127 ? 127 : idx);
  return 2 * idx + side;
}

__device__ __forceinline__ bool occ_bad(float p) {
  uint32_t key = __float_as_uint(p);
  if (key == 0x80000000u) key = 0u;
  return key > OCC_KEY_ONE;
}

// x / f and x % f for x < 2^63 and 1 <= f < 2^16, in three 32-bit divisions (long division in base 2^16 below the top)
__device__ __forceinline__ void occ_divmod(unsigned long long x, uint32_t f, unsigned long long& quot, uint32_t& rem) {
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  const uint32_t q1 = hi / f, r1 = hi - q1 * f;
  const uint32_t n2 = (r1 << 16) | (lo >> 16);         // r1 < f < 2^16
  const uint32_t q2 = n2 / f, r2 = n2 - q2 * f;        // q2 < 2^16
  const uint32_t n3 = (r2 << 16) | (lo & 0xFFFFu);
  const uint32_t q3 = n3 / f;
  rem = n3 - q3 * f;
  quot = ((unsigned long long)q1 << 32) | ((unsigned long long)q2 << 16) | q3;
}

}  // namespace
