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

// the negative sampler's draw (linkpred.hip, cpu_backend.cpp): key(seed64, id of the positive
// edge, j-th negative of that edge, attempt t, end 0 = source / 1 = destination). The seed is
// mixed with a constant of its own (sample_key adds the Weyl constant instead), so one seed
// does not tie neighbour keys to negatives; (j, t, end) pack into one word: t < 64
PG_HD inline uint32_t negative_key(uint64_t seed64, int32_t id, int32_t j, int32_t t, int end) {
  const uint64_t s = mix64(seed64 ^ 0xD6E8FEB86659FD93ull);
  const uint64_t a = mix64(s ^ (((uint64_t)(uint32_t)id + 1) * 0x9E3779B97F4A7C15ull));
  const uint64_t c = ((uint64_t)(uint32_t)j << 7) | ((uint64_t)(uint32_t)t << 1) | (uint64_t)(end & 1);
  const uint64_t z = mix64(a ^ ((c + 1) * 0xC2B2AE3D27D4EB4Full));
  return (uint32_t)(z >> 32);
}

// a 32-bit key -> [0, n), n < 2^32
PG_HD inline int32_t key_to_range(uint32_t key, int64_t n) { return (int32_t)(((uint64_t)key * (uint64_t)n) >> 32); }

// bits needed for the positions 0 .. deg-1 of a row (deg >= 1)
PG_HD inline int pos_bits(int32_t deg) {
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < (int64_t)deg) ++b;
  return b;
}

}  // namespace pg
