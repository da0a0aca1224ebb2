// Device twins of graph.cpp's pg_csr_transpose / pg_schedule_count / pg_schedule_build: a sampled
// block's transpose and both work schedules without moving an index array across the bus. The
// results are integers and equal the host functions' bit for bit (the host functions are the
// specification). Not used by the reference (full-graph training only): reference-unpinned.
//
// Core: a stable LSD radix sort of (key u32, value u32) pairs over a caller-given number of key
// bits, 8-bit digits, kTile elements per workgroup. One pass =
//   radix_hist_kernel     per-tile digit counts into a (digit-major, tile-minor) table
//   a scan of that table  one workgroup while the table is short (scan_tiles_kernel), else the
//                         three-kernel tile scan of scan.hpp
//   radix_scatter_kernel  an entry's place = its digit's scanned table cell + its rank among the
//                         equal digits before it in its tile: wave ballots (one per digit bit,
//                         popcount(mask & lanes_below)), a cross-wave prefix and a running count
//                         over the tile's four rounds in LDS
// No atomics anywhere in this file: every result is a function of the arguments.
//
// pg_csr_transpose_dev   tslot = the slots stably sorted by column; tptr[c] = the first sorted position
//                        whose key is >= c (a binary search per column over the sorted keys: no
//                        histogram, no scan); tcol = the slot's row (a binary search in ptr)
// pg_schedule_count_dev  per-workgroup partial sums / extrema, reduced by one workgroup
// pg_schedule_build_dev  exclusive scans over the rows give every row's first raw item and first
//                        slot; items are keyed chunk - len, merges bound - n, both sorted by the
//                        radix primitive with the raw index as value, then written out
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "scan.hpp"

namespace {

constexpr int kDigits = 256;              // 8-bit digits
constexpr int64_t kOneGroupScan = 8192;   // table cells up to which one workgroup scans the table
constexpr int kCountGroups = 256;         // most workgroups of the count's partial pass

inline int bits_of(int64_t x) {  // bits needed to write x (0 for x <= 0)
  int b = 0;
  while (x > 0) {
    ++b;
    x >>= 1;
  }
  return b;
}
inline int passes_of(int bits) { return (bits + 7) / 8; }

inline unsigned grid_for(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, 256 * 8));
}

inline int launch_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pg::set_error((int)e, "%s: launch failed: %s", who, hipGetErrorString(e));
  return pg::ok();
}

// bump allocator over the caller's workspace
struct Carver {
  char* p;
  size_t used = 0;
  explicit Carver(void* ws) : p((char*)ws) {}
  template <typename T>
  T* take(int64_t n) {
    T* r = (T*)(p + used);
    used += align256((size_t)std::max<int64_t>(1, n) * sizeof(T));
    return r;
  }
};

// ---------------------------------------------------------------- generic scan of an int32 array
__global__ __launch_bounds__(kBlock) void scan_local_kernel(const int32_t* in, int64_t n, int32_t* out,
                                                            int32_t* tile_sums) {
  __shared__ int lds[kBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  int v[kPerThread];
  for (int q = 0; q < kPerThread; ++q) v[q] = i0 + q < n ? in[i0 + q] : 0;
  tile_scan_store(v, i0, n, out, tile_sums, lds);
}

// ---------------------------------------------------------------- radix sort
// lanes of this wave that are valid and hold digit d (d = 0 on invalid lanes, which ignore it)
__device__ inline uint64_t match_digit(int d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool one = (d >> b) & 1;
    const uint64_t bal = __ballot(one);
    m &= one ? bal : ~bal;
  }
  return m;
}

__device__ inline uint64_t lanes_below() {
  const int lane = threadIdx.x & (kWave - 1);
  return lane == 0 ? 0ull : (~0ull >> (kWave - lane));
}

// table[d * n_tiles + tile] = entries of the tile whose digit is d
__global__ __launch_bounds__(kBlock) void radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                            int32_t* __restrict__ table, int64_t n_tiles) {
  __shared__ int wcnt[kWavesPerBlock][kDigits];
  const int t = threadIdx.x;
  const int wave = t / kWave;
  const uint64_t below = lanes_below();
  for (int w = 0; w < kWavesPerBlock; ++w) wcnt[w][t] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t i = base + q * kBlock + t;
    const bool valid = i < n;
    const int d = valid ? (int)((keys[i] >> shift) & (kDigits - 1)) : 0;
    const uint64_t m = match_digit(d, valid);
    if (valid && (m & below) == 0) wcnt[wave][d] += __popcll(m);  // one lane per (wave, digit)
    __syncthreads();
  }
  int s = 0;
  for (int w = 0; w < kWavesPerBlock; ++w) s += wcnt[w][t];
  table[(int64_t)t * n_tiles + blockIdx.x] = s;
}

// table: the exclusive scan of radix_hist_kernel's. Stable: a tile's entries keep their order
// among equal digits (round q holds entries base + q * kBlock + t: ascending with (q, wave, lane))
__global__ __launch_bounds__(kBlock) void radix_scatter_kernel(const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ vals, int64_t n, int shift,
                                                               const int32_t* __restrict__ table, int64_t n_tiles,
                                                               uint32_t* __restrict__ keys_out,
                                                               uint32_t* __restrict__ vals_out) {
  __shared__ int wcnt[kWavesPerBlock][kDigits];
  __shared__ int running[kDigits];
  const int t = threadIdx.x;
  const int wave = t / kWave;
  const uint64_t below = lanes_below();
  running[t] = table[(int64_t)t * n_tiles + blockIdx.x];
  for (int w = 0; w < kWavesPerBlock; ++w) wcnt[w][t] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t i = base + q * kBlock + t;
    const bool valid = i < n;
    const uint32_t k = valid ? keys[i] : 0u;
    const uint32_t v = valid ? vals[i] : 0u;
    const int d = (int)((k >> shift) & (kDigits - 1));
    const uint64_t m = match_digit(d, valid);
    if (valid && (m & below) == 0) wcnt[wave][d] = __popcll(m);
    __syncthreads();
    if (valid) {
      int64_t at = running[d] + __popcll(m & below);
      for (int w = 0; w < wave; ++w) at += wcnt[w][d];
      if (at >= 0 && at < n) {  // holds for a table that matches the keys; a guard all the same
        keys_out[at] = k;
        vals_out[at] = v;
      }
    }
    __syncthreads();
    int s = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) {
      s += wcnt[w][t];
      wcnt[w][t] = 0;
    }
    running[t] += s;
    __syncthreads();
  }
}

// workspace of one sort of n pairs: the table, the tile sums of its scan, one total
inline int64_t sort_table_cells(int64_t n) { return kDigits * tiles_of(n); }
inline size_t sort_ws_bytes(int64_t n) {
  const int64_t cells = sort_table_cells(n);
  return align256((size_t)std::max<int64_t>(1, cells) * 4) + align256((size_t)std::max<int64_t>(1, tiles_of(cells)) * 4) +
         256;
}

// Sorts the n pairs of (k0, v0) by the low `bits` key bits, stably, ping-ponging with (k1, v1).
// Returns 0 when the result lies in (k0, v0), 1 when in (k1, v1).
inline int radix_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, int64_t n, int bits, Carver ws,
                      hipStream_t st) {
  if (n <= 1) return 0;
  const int64_t nt = tiles_of(n);
  const int64_t cells = sort_table_cells(n);
  const int64_t ct = tiles_of(cells);
  int32_t* table = ws.take<int32_t>(cells);
  int32_t* sums = ws.take<int32_t>(ct);
  int32_t* total = ws.take<int32_t>(1);
  uint32_t *ki = k0, *vi = v0, *ko = k1, *vo = v1;
  int where = 0;
  for (int pass = 0; pass < passes_of(bits); ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, (const uint32_t*)ki, n, shift,
                       table, nt);
    if (cells <= kOneGroupScan) {
      hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, table, cells, total,
                         (const int32_t*)nullptr);
    } else {
      hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)ct), dim3(kBlock), 0, st, (const int32_t*)table, cells,
                         table, sums);
      hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, sums, ct, total, (const int32_t*)nullptr);
      hipLaunchKernelGGL(add_tile_offsets_kernel, dim3((unsigned)ct), dim3(kBlock), 0, st, table, cells,
                         (const int32_t*)sums);
    }
    hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, (const uint32_t*)ki,
                       (const uint32_t*)vi, n, shift, (const int32_t*)table, nt, ko, vo);
    std::swap(ki, ko);
    std::swap(vi, vo);
    where ^= 1;
  }
  return where;
}

// ---------------------------------------------------------------- transpose
// largest r in [0, n_rows) with ptr[r] <= s (rows without entries are stepped over); n_rows >= 1.
// Every index read lies in [0, n_rows], whatever ptr holds.
__device__ inline int32_t row_of_slot(const int32_t* __restrict__ ptr, int64_t n_rows, int32_t s) {
  int64_t lo = 0, hi = n_rows;  // ptr[lo] <= s assumed (ptr[0] = 0), answer in [lo, hi)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= s)
      lo = mid;
    else
      hi = mid;
  }
  return (int32_t)lo;
}

// keys = the columns (0 for one outside [0, n_cols), which sets the status), values = the slots
__global__ __launch_bounds__(kBlock) void transpose_keys_kernel(const int32_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ col, int64_t n_rows,
                                                                int64_t n_cols, int64_t nnz, uint32_t* __restrict__ keys,
                                                                uint32_t* __restrict__ vals, int32_t* status) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
    int32_t c = col[k];
    if (c < 0 || c >= n_cols) {
      status[0] = -2;  // every writer of one code stores the same value
      c = 0;
    }
    keys[k] = (uint32_t)c;
    vals[k] = (uint32_t)k;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (ptr[0] != 0 || ptr[n_rows] != nnz)) status[0] = -3;
}

__global__ __launch_bounds__(kBlock) void set_status_kernel(int32_t* status, int32_t v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = v;
}

// tptr[c] = the number of sorted keys below c = the first sorted position whose key is >= c
__global__ __launch_bounds__(kBlock) void transpose_ptr_kernel(const uint32_t* __restrict__ keys, int64_t nnz,
                                                               int64_t n_cols, int32_t* __restrict__ tptr) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c <= n_cols; c += stride) {
    int64_t lo = 0, hi = nnz;  // first position in [0, nnz] whose key is >= c
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)keys[mid] < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    tptr[c] = (int32_t)lo;
  }
}

__global__ __launch_bounds__(kBlock) void fill_zero_kernel(int32_t* a, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) a[i] = 0;
}

__global__ __launch_bounds__(kBlock) void transpose_finish_kernel(const int32_t* __restrict__ ptr, int64_t n_rows,
                                                                  int64_t nnz, const uint32_t* __restrict__ vals,
                                                                  int32_t* __restrict__ tcol, int32_t* __restrict__ tslot,
                                                                  int32_t* __restrict__ tpos) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nnz; t += stride) {
    const int32_t s = (int32_t)vals[t];
    const int32_t r = row_of_slot(ptr, n_rows, s);
    tcol[t] = r;
    if (tslot) tslot[t] = s;
    if (tpos) tpos[t] = s - ptr[r];
  }
}

// ---------------------------------------------------------------- schedule count
struct Counts {
  long long items, merges, slots;
  int max_deg, min_deg, bad;
};

__device__ inline Counts counts_join(const Counts& a, const Counts& b) {
  return {a.items + b.items, a.merges + b.merges, a.slots + b.slots, a.max_deg > b.max_deg ? a.max_deg : b.max_deg,
          a.min_deg < b.min_deg ? a.min_deg : b.min_deg, a.bad | b.bad};
}

// the workgroup's join in thread 0 (sums, extrema and an OR: any order gives the same value)
__device__ inline Counts counts_reduce(Counts c, Counts* lds) {
  lds[threadIdx.x] = c;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) lds[threadIdx.x] = counts_join(lds[threadIdx.x], lds[threadIdx.x + off]);
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(kBlock) void count_partial_kernel(const int32_t* __restrict__ ptr, int64_t n_rows,
                                                               int32_t chunk, Counts* __restrict__ partial) {
  __shared__ Counts lds[kBlock];
  Counts c = {0, 0, 0, 0, INT32_MAX, 0};
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_rows; r += stride) {
    const int32_t d = ptr[r + 1] - ptr[r];
    if (d < 0) {
      c.bad = 1;
      continue;
    }
    c.max_deg = d > c.max_deg ? d : c.max_deg;
    c.min_deg = d < c.min_deg ? d : c.min_deg;
    if (d <= chunk) {
      c.items += 1;
    } else {
      const long long n = ((long long)d + chunk - 1) / chunk;
      c.items += n;
      c.merges += 1;
      c.slots += n;
    }
  }
  c = counts_reduce(c, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = c;
}

// counts[6] = n_items, n_merges, n_slots, max_deg, min_deg (0 without rows), status
__global__ __launch_bounds__(kBlock) void count_final_kernel(const Counts* __restrict__ partial, int n_partial,
                                                             int64_t* __restrict__ counts) {
  __shared__ Counts lds[kBlock];
  Counts c = {0, 0, 0, 0, INT32_MAX, 0};
  for (int i = threadIdx.x; i < n_partial; i += kBlock) c = counts_join(c, partial[i]);
  c = counts_reduce(c, lds);
  if (threadIdx.x == 0) {
    counts[0] = c.items;
    counts[1] = c.merges;
    counts[2] = c.slots;
    counts[3] = c.max_deg;
    counts[4] = c.min_deg == INT32_MAX ? 0 : c.min_deg;
    counts[5] = c.bad ? -1 : (c.items > INT32_MAX || c.slots > INT32_MAX) ? -2 : 0;
  }
}

// ---------------------------------------------------------------- schedule build
__device__ inline int32_t row_len(const int32_t* __restrict__ ptr, int64_t r) {
  const int32_t d = ptr[r + 1] - ptr[r];
  return d < 0 ? 0 : d;  // a ptr that is not monotone fails the count; here it only must not run away
}
__device__ inline int32_t pieces_of(int32_t d, int32_t chunk) {
  return (int32_t)(((int64_t)d + chunk - 1) / chunk);
}

// local scans over the rows of: split flag (-> merge index), pieces of split rows (-> first slot)
__global__ __launch_bounds__(kBlock) void build_rows_kernel(const int32_t* __restrict__ ptr, int64_t n_rows,
                                                            int32_t chunk, int32_t* __restrict__ mloc,
                                                            int32_t* __restrict__ sloc, int32_t* __restrict__ msums,
                                                            int32_t* __restrict__ ssums) {
  __shared__ int lds[kBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  int f[kPerThread], p[kPerThread];
  for (int q = 0; q < kPerThread; ++q) {
    const int32_t d = i0 + q < n_rows ? row_len(ptr, i0 + q) : 0;
    f[q] = d > chunk;
    p[q] = f[q] ? pieces_of(d, chunk) : 0;
  }
  tile_scan_store(f, i0, n_rows, mloc, msums, lds);
  tile_scan_store(p, i0, n_rows, sloc, ssums, lds);
}

// workgroup b scans the tile sums of array b (two arrays of n_tiles cells, `stride` apart)
__global__ __launch_bounds__(kBlock) void scan_tiles_pair_kernel(int32_t* sums, int64_t stride, int64_t n_tiles) {
  __shared__ int lds[kBlock];
  int32_t* a = sums + blockIdx.x * stride;
  int carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const int v = i < n_tiles ? a[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < n_tiles) a[i] = carry + ex;
    carry += total;
  }
}

// global offsets per row: mloc -> merge index, sloc -> first slot, first[r] = the row's first raw
// item = (rows before r that are not split) + (pieces of the split rows before r); first[n_rows] =
// the item count. The raw merge list (row order): keys bound - n, values the merge index.
__global__ __launch_bounds__(kBlock) void build_offsets_kernel(const int32_t* __restrict__ ptr, int64_t n_rows,
                                                               int32_t chunk, int32_t* __restrict__ mloc,
                                                               int32_t* __restrict__ sloc,
                                                               const int32_t* __restrict__ moffs,
                                                               const int32_t* __restrict__ soffs,
                                                               int32_t* __restrict__ first, int64_t n_merges,
                                                               int32_t bound, uint32_t* __restrict__ mkeys,
                                                               uint32_t* __restrict__ mvals, int32_t* __restrict__ mrow) {
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  const int32_t mo = moffs[blockIdx.x], so = soffs[blockIdx.x];
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t r = i0 + q;
    if (r >= n_rows) continue;
    const int32_t m = mloc[r] + mo, s = sloc[r] + so;
    mloc[r] = m;
    sloc[r] = s;
    first[r] = (int32_t)(r - m) + s;
    const int32_t d = row_len(ptr, r);
    if (d > chunk) {
      const int32_t n = pieces_of(d, chunk);
      if (m < n_merges) {
        mkeys[m] = (uint32_t)(n <= bound ? bound - n : 0);
        mvals[m] = (uint32_t)m;
        mrow[m] = (int32_t)r;
      }
      if (r == n_rows - 1) first[n_rows] = (int32_t)(r - m) + s + n;
    } else if (r == n_rows - 1) {
      first[n_rows] = (int32_t)(r - m) + s + 1;
    }
  }
}

// the row of raw item i: the largest r with first[r] <= i (first ascends strictly: a row has >= 1 item)
__device__ inline int32_t row_of_item(const int32_t* __restrict__ first, int64_t n_rows, int32_t i) {
  int64_t lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (first[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return (int32_t)lo;
}

__device__ inline void item_of(const int32_t* __restrict__ ptr, const int32_t* __restrict__ first,
                               const int32_t* __restrict__ slot0, int32_t chunk, int32_t r, int32_t i, int32_t out[4]) {
  const int32_t b = ptr[r], d = row_len(ptr, r), e = b + d;
  out[0] = r;
  if (d <= chunk) {
    out[1] = b;
    out[2] = e;
    out[3] = -1;
  } else {
    const int32_t j = i - first[r];
    const int64_t k0 = (int64_t)b + (int64_t)j * chunk;
    const int64_t k1 = k0 + chunk < e ? k0 + chunk : e;
    out[1] = (int32_t)k0;
    out[2] = (int32_t)k1;
    out[3] = slot0[r] + j;
  }
}

// raw items in row order: keys chunk - len, values the raw index, the item's row beside them
__global__ __launch_bounds__(kBlock) void build_item_keys_kernel(const int32_t* __restrict__ ptr, int64_t n_rows,
                                                                 int32_t chunk, const int32_t* __restrict__ first,
                                                                 const int32_t* __restrict__ slot0, int64_t n_items,
                                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                 int32_t* __restrict__ irow) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_items; i += stride) {
    const int32_t r = row_of_item(first, n_rows, (int32_t)i);
    int32_t it[4];
    item_of(ptr, first, slot0, chunk, r, (int32_t)i, it);
    const int32_t len = it[2] - it[1];
    keys[i] = (uint32_t)(len >= 0 && len <= chunk ? chunk - len : 0);
    vals[i] = (uint32_t)i;
    irow[i] = r;
  }
}

__global__ __launch_bounds__(kBlock) void build_items_kernel(const int32_t* __restrict__ ptr, int32_t chunk,
                                                             const int32_t* __restrict__ first,
                                                             const int32_t* __restrict__ slot0, int64_t n_items,
                                                             const uint32_t* __restrict__ vals,
                                                             const int32_t* __restrict__ irow, int32_t* __restrict__ items) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < n_items; at += stride) {
    const uint32_t i = vals[at];
    if (i >= (uint64_t)n_items) continue;
    int32_t it[4];
    item_of(ptr, first, slot0, chunk, irow[i], (int32_t)i, it);
    for (int q = 0; q < 4; ++q) items[4 * at + q] = it[q];
  }
}

__global__ __launch_bounds__(kBlock) void build_merges_kernel(const int32_t* __restrict__ ptr, int32_t chunk,
                                                              const int32_t* __restrict__ slot0, int64_t n_merges,
                                                              const uint32_t* __restrict__ vals,
                                                              const int32_t* __restrict__ mrow,
                                                              int32_t* __restrict__ merges) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < n_merges; at += stride) {
    const uint32_t m = vals[at];
    if (m >= (uint64_t)n_merges) continue;
    const int32_t r = mrow[m];
    merges[4 * at + 0] = r;
    merges[4 * at + 1] = slot0[r];
    merges[4 * at + 2] = pieces_of(row_len(ptr, r), chunk);
    merges[4 * at + 3] = 0;
  }
}

inline int32_t merge_bound(int32_t max_deg, int32_t chunk) {
  return max_deg <= 0 ? 0 : (int32_t)(((int64_t)max_deg + chunk - 1) / chunk);
}

}  // namespace

extern "C" {

// workspace: keys / values twice over nnz | the sort's
size_t pg_csr_transpose_dev_workspace(int64_t n_rows, int64_t n_cols, int64_t nnz) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0) return 0;
  return 4 * align256((size_t)std::max<int64_t>(1, nnz) * 4) + sort_ws_bytes(nnz);
}

int pg_csr_transpose_dev(const int32_t* ptr, const int32_t* col, int64_t n_rows, int64_t n_cols, int64_t nnz,
                         int32_t* tptr, int32_t* tcol, int32_t* tslot, int32_t* tpos, int32_t* status_dev, void* ws,
                         size_t ws_bytes, pg_stream_t stream) {
  const char* who = "pg_csr_transpose_dev";
  if (n_rows < 0 || n_cols < 0 || nnz < 0) return pg::set_error(PG_ERR_INVALID, "%s: negative size", who);
  if (n_rows > INT32_MAX - 1 || n_cols > INT32_MAX - 1 || nnz > INT32_MAX - kTile)
    return pg::set_error(PG_ERR_UNSUPPORTED, "%s: graph exceeds int32 ids", who);
  if (!tptr || !status_dev || (nnz > 0 && (!ptr || !col || !tcol)))
    return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  if (nnz > 0 && (n_rows == 0 || n_cols == 0)) return pg::set_error(PG_ERR_INVALID, "%s: entries without rows or columns", who);
  if (!ws || ws_bytes < pg_csr_transpose_dev_workspace(n_rows, n_cols, nnz))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(kBlock), 0, st, status_dev, 0);
  if (nnz == 0) {  // no input buffer is read
    hipLaunchKernelGGL(fill_zero_kernel, dim3(grid_for(n_cols + 1)), dim3(kBlock), 0, st, tptr, n_cols + 1);
    return launch_status(who);
  }
  Carver w(ws);
  uint32_t* k0 = w.take<uint32_t>(nnz);
  uint32_t* v0 = w.take<uint32_t>(nnz);
  uint32_t* k1 = w.take<uint32_t>(nnz);
  uint32_t* v1 = w.take<uint32_t>(nnz);
  hipLaunchKernelGGL(transpose_keys_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, st, ptr, col, n_rows, n_cols, nnz, k0,
                     v0, status_dev);
  const int where = radix_sort(k0, v0, k1, v1, nnz, bits_of(n_cols - 1), w, st);
  const uint32_t* ks = where ? k1 : k0;
  const uint32_t* vs = where ? v1 : v0;
  hipLaunchKernelGGL(transpose_ptr_kernel, dim3(grid_for(n_cols + 1)), dim3(kBlock), 0, st, ks, nnz, n_cols, tptr);
  hipLaunchKernelGGL(transpose_finish_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, st, ptr, n_rows, nnz, vs, tcol,
                     tslot, tpos);
  return launch_status(who);
}

size_t pg_schedule_count_dev_workspace(int64_t n_rows) {
  return n_rows < 0 ? 0 : align256((size_t)kCountGroups * sizeof(Counts));
}

int pg_schedule_count_dev(const int32_t* ptr, int64_t n_rows, int32_t chunk, int64_t* counts_dev, void* ws,
                          size_t ws_bytes, pg_stream_t stream) {
  const char* who = "pg_schedule_count_dev";
  if (n_rows < 0 || n_rows > INT32_MAX - 1 || chunk <= 0 || !counts_dev || (n_rows > 0 && !ptr))
    return pg::set_error(PG_ERR_INVALID, "%s: bad arguments", who);
  if (!ws || ws_bytes < pg_schedule_count_dev_workspace(n_rows))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  Counts* partial = (Counts*)ws;
  const int groups = n_rows == 0 ? 0 : (int)std::min<int64_t>(kCountGroups, (n_rows + kBlock - 1) / kBlock);
  if (groups > 0)
    hipLaunchKernelGGL(count_partial_kernel, dim3((unsigned)groups), dim3(kBlock), 0, st, ptr, n_rows, chunk, partial);
  hipLaunchKernelGGL(count_final_kernel, dim3(1), dim3(kBlock), 0, st, (const Counts*)partial, groups, counts_dev);
  return launch_status(who);
}

// workspace: merge index, first slot, first raw item per row | two arrays of tile sums | items'
// keys / values twice and rows | merges' keys / values twice and rows | the sort's
size_t pg_schedule_build_dev_workspace(int64_t n_rows, int64_t n_items, int64_t n_merges) {
  if (n_rows < 0 || n_items < 0 || n_merges < 0) return 0;
  auto a = [](int64_t n) { return align256((size_t)std::max<int64_t>(1, n) * 4); };
  return 2 * a(n_rows) + a(n_rows + 1) + a(2 * std::max<int64_t>(1, tiles_of(n_rows))) + 5 * a(n_items) +
         5 * a(n_merges) + sort_ws_bytes(std::max(n_items, n_merges));
}

int pg_schedule_build_dev(const int32_t* ptr, int64_t n_rows, int32_t chunk, int64_t n_items, int64_t n_merges,
                          int32_t max_deg, int32_t* items, int32_t* merges, void* ws, size_t ws_bytes,
                          pg_stream_t stream) {
  const char* who = "pg_schedule_build_dev";
  if (n_rows < 0 || n_rows > INT32_MAX - 1 || chunk <= 0 || n_items < 0 || n_merges < 0 || max_deg < 0 ||
      n_items > INT32_MAX - kTile || (n_rows > 0 && (!ptr || !items)) || (n_merges > 0 && !merges))
    return pg::set_error(PG_ERR_INVALID, "%s: bad arguments", who);
  if (n_items < n_rows || n_merges > n_rows)
    return pg::set_error(PG_ERR_INVALID, "%s: counts do not fit the rows", who);
  if (!ws || ws_bytes < pg_schedule_build_dev_workspace(n_rows, n_items, n_merges))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  if (n_rows == 0) return pg::ok();
  hipStream_t st = (hipStream_t)stream;
  const int64_t nt = tiles_of(n_rows);
  Carver w(ws);
  int32_t* mloc = w.take<int32_t>(n_rows);
  int32_t* sloc = w.take<int32_t>(n_rows);
  int32_t* first = w.take<int32_t>(n_rows + 1);
  int32_t* sums = w.take<int32_t>(2 * nt);
  uint32_t* ik0 = w.take<uint32_t>(n_items);
  uint32_t* iv0 = w.take<uint32_t>(n_items);
  uint32_t* ik1 = w.take<uint32_t>(n_items);
  uint32_t* iv1 = w.take<uint32_t>(n_items);
  int32_t* irow = w.take<int32_t>(n_items);
  uint32_t* mk0 = w.take<uint32_t>(n_merges);
  uint32_t* mv0 = w.take<uint32_t>(n_merges);
  uint32_t* mk1 = w.take<uint32_t>(n_merges);
  uint32_t* mv1 = w.take<uint32_t>(n_merges);
  int32_t* mrow = w.take<int32_t>(n_merges);
  const int32_t bound = merge_bound(max_deg, chunk);
  hipLaunchKernelGGL(build_rows_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, ptr, n_rows, chunk, mloc, sloc, sums,
                     sums + nt);
  hipLaunchKernelGGL(scan_tiles_pair_kernel, dim3(2), dim3(kBlock), 0, st, sums, nt, nt);
  hipLaunchKernelGGL(build_offsets_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, ptr, n_rows, chunk, mloc, sloc,
                     (const int32_t*)sums, (const int32_t*)(sums + nt), first, n_merges, bound, mk0, mv0, mrow);
  hipLaunchKernelGGL(build_item_keys_kernel, dim3(grid_for(n_items)), dim3(kBlock), 0, st, ptr, n_rows, chunk,
                     (const int32_t*)first, (const int32_t*)sloc, n_items, ik0, iv0, irow);
  // the items' sort and the merges' share the sort's workspace: one stream, one after the other
  const int iw = radix_sort(ik0, iv0, ik1, iv1, n_items, bits_of(chunk), w, st);
  hipLaunchKernelGGL(build_items_kernel, dim3(grid_for(n_items)), dim3(kBlock), 0, st, ptr, chunk,
                     (const int32_t*)first, (const int32_t*)sloc, n_items, (const uint32_t*)(iw ? iv1 : iv0),
                     (const int32_t*)irow, items);
  if (n_merges > 0) {
    const int mw = radix_sort(mk0, mv0, mk1, mv1, n_merges, bits_of(bound), w, st);
    hipLaunchKernelGGL(build_merges_kernel, dim3(grid_for(n_merges)), dim3(kBlock), 0, st, ptr, chunk,
                       (const int32_t*)sloc, n_merges, (const uint32_t*)(mw ? mv1 : mv0), (const int32_t*)mrow, merges);
  }
  return launch_status(who);
}

}  // extern "C"
