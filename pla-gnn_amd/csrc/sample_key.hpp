// The neighbour sampler's key function, shared by the device kernels (sample.hip) and the
// host twin (cpu_backend.cpp) so both select the same entries bit for bit.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif

namespace pg {

// splitmix64's finaliser (Steele, Lea, Flood 2014; public domain constants)
PG_HD inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// key(seed64, edge id): stateless and counter-based: the seed is mixed on its own first, so
// consecutive seeds and consecutive edge ids do not meet on one Weyl sequence
PG_HD inline uint32_t sample_key(uint64_t seed64, int32_t edge_id) {
  const uint64_t s = mix64(seed64 + 0x9E3779B97F4A7C15ull);
  const uint64_t z = mix64(s ^ (((uint64_t)(uint32_t)edge_id + 1) * 0x9E3779B97F4A7C15ull));
  return (uint32_t)(z >> 32);
}

// bits needed for the positions 0 .. deg-1 of a row (deg >= 1)
PG_HD inline int pos_bits(int32_t deg) {
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < (int64_t)deg) ++b;
  return b;
}

}  // namespace pg
