// Prefix sums shared by sample.hip and graph_dev.hip: 1024 elements per workgroup
// (kBlock threads x kPerThread), the workgroup totals scanned by one workgroup that walks
// them kBlock at a time. Integer adds only: the result is a function of the input.
//   a kernel of the caller's   loads kPerThread values per thread, tile_scan_store
//   scan_tiles_kernel          tile_sums -> their exclusive scan in place (+ the grand total)
//   add_tile_offsets_kernel    out[i] += its tile's offset
// Everything sits in an unnamed namespace: each translation unit gets kernels of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kPerThread = 4;
constexpr int kTile = kBlock * kPerThread;  // elements of one workgroup's local scan

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// exclusive scan of one value per thread over the workgroup; *total = the workgroup's sum
__device__ inline int block_excl_scan(int v, int* lds, int* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const int add = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const int incl = lds[t];
  *total = lds[kBlock - 1];
  __syncthreads();
  return incl - v;
}

// v[0..4) of this thread -> local exclusive offsets written to out[i0 .. i0+4), tile total
__device__ inline void tile_scan_store(const int (&v)[kPerThread], int64_t i0, int64_t n, int32_t* out,
                                       int32_t* tile_sums, int* lds) {
  int sum = 0;
  for (int q = 0; q < kPerThread; ++q) sum += v[q];
  int total;
  int run = block_excl_scan(sum, lds, &total);
  for (int q = 0; q < kPerThread; ++q) {
    if (i0 + q < n) out[i0 + q] = run;
    run += v[q];
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums -> their exclusive scan in place; the grand total to total_out[0]
// (or, with status: a negative status instead of the total)
__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(int32_t* tile_sums, int64_t n_tiles, int32_t* total_out,
                                                            const int32_t* status) {
  __shared__ int lds[kBlock];
  int carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const int v = i < n_tiles ? tile_sums[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < n_tiles) tile_sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const int32_t st = status ? status[0] : 0;
    total_out[0] = st < 0 ? st : carry;
  }
}

__global__ __launch_bounds__(kBlock) void add_tile_offsets_kernel(int32_t* out, int64_t n, const int32_t* tile_offs) {
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  const int32_t off = tile_offs[blockIdx.x];
  for (int q = 0; q < kPerThread; ++q)
    if (i0 + q < n) out[i0 + q] += off;
}

}  // namespace
