// Neighbour sampling and block compaction for mini-batch training (dgl.sampling.
// sample_neighbors / dgl.to_block): the per-batch work of a sampled training loop, on the
// device. Not used by the reference (full-graph training only): reference-unpinned.
//
// pg_sample_count  per-seed min(deg, fanout) and its exclusive prefix sum
// pg_sample_fill   one wave per sampled row: keys (sample_key.hpp) of the row's entries in
//                  LDS while the row fits (PG_SAMPLE_LDS_KEYS), recomputed per pass for longer
//                  rows, which first narrow the row to the (key, position) pairs below a key
//                  threshold (two passes over the row) and keep those in LDS; the fanout smallest
//                  (key, position) composites are found by a bitwise threshold search with a
//                  fixed number of passes (32 + position bits), counted with wave ballots; the
//                  kept entries are written in row order through ballot prefix counts. No
//                  atomics: the result is a function of the arguments.
// pg_block_compact dense first-position map over the parent's ids (int32 atomicMin: the minimum
//                  of a set of integers does not depend on the order they arrive in), flags of
//                  the first appearances, one prefix sum, two gathers.
// Prefix sums: scan.hpp (1024 elements per workgroup, the workgroup totals scanned by one workgroup).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "sample_key.hpp"
#include "scan.hpp"

namespace {

constexpr int kCap = PG_SAMPLE_LDS_KEYS;
constexpr int kCand = kCap / 2;  // (key, position) candidates of a hub row in the same LDS
constexpr int32_t kNever = INT32_MAX;

__device__ inline int32_t row_degree(const int32_t* ptr, int64_t n_rows, int32_t s) {
  if (s < 0 || s >= n_rows) return 0;
  return ptr[s + 1] - ptr[s];
}

__global__ __launch_bounds__(kBlock) void sample_count_kernel(const int32_t* ptr, int64_t n_rows, const int32_t* seeds,
                                                              int64_t n_seeds, int32_t fanout, int32_t* out_ptr,
                                                              int32_t* tile_sums) {
  __shared__ int lds[kBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  int v[kPerThread];
  for (int q = 0; q < kPerThread; ++q) {
    int32_t d = 0;
    if (i0 + q < n_seeds) {
      d = row_degree(ptr, n_rows, seeds[i0 + q]);
      d = d < 0 ? 0 : d;
      if (fanout >= 0 && d > fanout) d = fanout;
    }
    v[q] = d;
  }
  tile_scan_store(v, i0, n_seeds, out_ptr, tile_sums, lds);
}

__global__ __launch_bounds__(kBlock) void sample_fill_kernel(const int32_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ col,
                                                             const int32_t* __restrict__ eid, int64_t n_rows,
                                                             const int32_t* __restrict__ seeds, int64_t n_seeds,
                                                             int32_t fanout, uint64_t seed64,
                                                             const int32_t* __restrict__ out_ptr,
                                                             int32_t* __restrict__ out_col,
                                                             int32_t* __restrict__ out_eid) {
  __shared__ uint32_t keys_lds[kWavesPerBlock][kCap];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  uint32_t* keys = keys_lds[wave];
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));  // lanes before this one
  for (int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave; row < n_seeds;
       row += (int64_t)gridDim.x * kWavesPerBlock) {
    const int32_t s = seeds[row];
    if (s < 0 || s >= n_rows) continue;
    const int32_t b = ptr[s];
    const int32_t deg = ptr[s + 1] - b;
    if (deg <= 0 || fanout == 0) continue;
    const int64_t o = out_ptr[row];
    if (fanout < 0 || deg <= fanout) {
      for (int32_t j = lane; j < deg; j += kWave) {
        out_col[o + j] = col[b + j];
        out_eid[o + j] = eid ? eid[b + j] : b + j;
      }
      continue;
    }
    const int pb = pg::pos_bits(deg);
    const int32_t rank = fanout - 1;
    auto key_at = [&](int32_t j) -> uint32_t { return pg::sample_key(seed64, eid ? eid[b + j] : b + j); };
    // n candidates with composites comp(i), distinct and in ascending position: find the
    // composite V of rank fanout - 1 bit by bit from the top (V keeps a bit when at most rank
    // composites lie below V with that bit set), then write the candidates <= V in order
    auto select = [&](int32_t n, auto comp, auto pos_of) {
      uint64_t V = 0;
      for (int bit = 31 + pb; bit >= 0; --bit) {
        const uint64_t trial = V | (1ull << bit);
        int32_t cnt = 0;
        for (int32_t i0 = 0; i0 < n && cnt <= rank; i0 += kWave) {
          const int32_t i = i0 + lane;
          const bool p = i < n && comp(i) < trial;
          cnt += __popcll(__ballot(p));
        }
        if (cnt <= rank) V = trial;
      }
      int32_t base = 0;
      for (int32_t i0 = 0; i0 < n; i0 += kWave) {
        const int32_t i = i0 + lane;
        const bool p = i < n && comp(i) <= V;
        const uint64_t m = __ballot(p);
        if (p) {
          const int64_t at = o + base + __popcll(m & below);
          const int32_t j = pos_of(i);
          out_col[at] = col[b + j];
          out_eid[at] = eid ? eid[b + j] : b + j;
        }
        base += __popcll(m);
      }
    };
    if (deg <= kCap) {  // keys in LDS; every lane reads back only the keys it wrote itself
      for (int32_t j = lane; j < deg; j += kWave) keys[j] = key_at(j);
      select(deg, [&](int32_t i) { return ((uint64_t)keys[i] << pb) | (uint64_t)(uint32_t)i; },
             [&](int32_t i) { return i; });
      continue;
    }
    // a hub row: the keys do not fit and are recomputed in every pass over the row. Two such
    // passes, whose loads do not wait on one another: count the keys below a threshold t0 set
    // for an expected 2 fanout + 64 of them (doubled / halved until between fanout and kCand
    // keys pass: a function of the row's keys only), then gather those (key, position) pairs
    // into LDS, where the search runs. The fanout smallest composites are all among them.
    bool done = false;
    if (2 * (int64_t)fanout + 64 <= kCand) {
      uint32_t* ckey = keys;
      int32_t* cpos = (int32_t*)(keys + kCand);
      uint64_t t0 = ((uint64_t)(2 * fanout + 64) << 32) / (uint64_t)deg;  // < 2^32: deg > kCap
      bool ok = false;
      for (int tries = 0; tries < 40 && !ok; ++tries) {
        int32_t mine = 0;
#pragma unroll 4
        for (int32_t j = lane; j < deg; j += kWave) mine += (uint64_t)key_at(j) < t0;
        for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if (mine < fanout)
          t0 = t0 * 2 < (1ull << 32) ? t0 * 2 : (1ull << 32);
        else if (mine > kCand)
          t0 >>= 1;
        else
          ok = true;
      }
      if (ok) {
        int32_t nc = 0;
        for (int32_t j0 = 0; j0 < deg; j0 += kWave) {
          const int32_t j = j0 + lane;
          const uint32_t k = j < deg ? key_at(j) : 0u;
          const bool p = j < deg && (uint64_t)k < t0;
          const uint64_t m = __ballot(p);
          if (p) {
            const int32_t at = nc + __popcll(m & below);
            ckey[at] = k;
            cpos[at] = j;
          }
          nc += __popcll(m);
        }
        // the candidates were written by other lanes of this wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        select(nc, [&](int32_t i) { return ((uint64_t)ckey[i] << pb) | (uint64_t)(uint32_t)cpos[i]; },
               [&](int32_t i) { return cpos[i]; });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        done = true;
      }
    }
    if (!done)  // a fanout too large for the candidate buffer: every pass of the search walks the row
      select(deg, [&](int32_t i) { return ((uint64_t)key_at(i) << pb) | (uint64_t)(uint32_t)i; },
             [&](int32_t i) { return i; });
  }
}

// ---- block compaction
__global__ __launch_bounds__(kBlock) void compact_init_kernel(int32_t* first, int64_t n_parent, int32_t* status) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_parent; i += stride) first[i] = kNever;
  if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = 0;
}

__device__ inline int32_t compact_id(const int32_t* dst_ids, int64_t n_dst, const int32_t* col, int64_t p) {
  return p < n_dst ? dst_ids[p] : col[p - n_dst];
}

__global__ __launch_bounds__(kBlock) void compact_min_kernel(const int32_t* dst_ids, int64_t n_dst, const int32_t* col,
                                                             int64_t n_all, int64_t n_parent, int32_t* first,
                                                             int32_t* status) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n_all; p += stride) {
    const int32_t id = compact_id(dst_ids, n_dst, col, p);
    if (id < 0 || id >= n_parent)
      status[0] = -2;  // every writer stores the same value
    else
      atomicMin(&first[id], (int32_t)p);
  }
}

// flag[p] = position p is the first appearance of its id; local scan of the flags
__global__ __launch_bounds__(kBlock) void compact_flag_kernel(const int32_t* dst_ids, int64_t n_dst, const int32_t* col,
                                                              int64_t n_all, int64_t n_parent, const int32_t* first,
                                                              int32_t* rank, int32_t* tile_sums, int32_t* status) {
  __shared__ int lds[kBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  int v[kPerThread];
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t p = i0 + q;
    v[q] = 0;
    if (p < n_all) {
      const int32_t id = compact_id(dst_ids, n_dst, col, p);
      if (id >= 0 && id < n_parent) {
        v[q] = first[id] == (int32_t)p;
        if (p < n_dst && !v[q] && status[0] == 0) status[0] = -1;  // a duplicate among dst_ids
      }
    }
  }
  tile_scan_store(v, i0, n_all, rank, tile_sums, lds);
}

// rank[p] += its tile's offset; src_ids[rank[p]] = id at the first appearances
__global__ __launch_bounds__(kBlock) void compact_src_kernel(const int32_t* dst_ids, int64_t n_dst, const int32_t* col,
                                                             int64_t n_all, int64_t n_parent, const int32_t* first,
                                                             int32_t* rank, const int32_t* tile_offs, int32_t* src_ids) {
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  const int32_t off = tile_offs[blockIdx.x];
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t p = i0 + q;
    if (p >= n_all) continue;
    const int32_t r = rank[p] + off;
    rank[p] = r;
    const int32_t id = compact_id(dst_ids, n_dst, col, p);
    if (id >= 0 && id < n_parent && first[id] == (int32_t)p) src_ids[r] = id;
  }
}

__global__ __launch_bounds__(kBlock) void compact_local_kernel(const int32_t* col, int64_t nnz, int64_t n_parent,
                                                               const int32_t* first, const int32_t* rank,
                                                               int32_t* col_local) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
    const int32_t id = col[k];
    col_local[k] = (id >= 0 && id < n_parent) ? rank[first[id]] : -1;
  }
}

inline int launch_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pg::set_error((int)e, "%s: launch failed: %s", who, hipGetErrorString(e));
  return pg::ok();
}

inline unsigned grid_for(int64_t n, int per_block) {
  const int64_t b = (n + per_block - 1) / per_block;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, 256 * 8));
}

}  // namespace

extern "C" {

size_t pg_sample_count_workspace(int64_t n_seeds) {
  return n_seeds < 0 ? 0 : align256((size_t)std::max<int64_t>(1, tiles_of(n_seeds)) * sizeof(int32_t));
}

int pg_sample_count(const pg_csr_t* g, const int32_t* seeds, int64_t n_seeds, int32_t fanout, int32_t* out_ptr,
                    void* ws, size_t ws_bytes, pg_stream_t stream) {
  const char* who = "pg_sample_count";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  if (!ws || ws_bytes < pg_sample_count_workspace(n_seeds))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  int32_t* tile_sums = (int32_t*)ws;
  const int64_t nt = tiles_of(n_seeds);
  if (nt > 0)
    hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, g->ptr, g->n_rows, seeds, n_seeds,
                       fanout, out_ptr, tile_sums);
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, tile_sums, nt, out_ptr + n_seeds,
                     (const int32_t*)nullptr);
  if (nt > 1)
    hipLaunchKernelGGL(add_tile_offsets_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, out_ptr, n_seeds, tile_sums);
  return launch_status(who);
}

int pg_sample_fill(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds, int32_t fanout,
                   uint64_t seed64, const int32_t* out_ptr, int32_t* out_col, int32_t* out_eid,
                   pg_stream_t stream) {
  const char* who = "pg_sample_fill";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  if (n_seeds == 0 || g->nnz == 0 || fanout == 0) return pg::ok();
  if (!out_col || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  hipLaunchKernelGGL(sample_fill_kernel, dim3(grid_for(n_seeds, kWavesPerBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, g->ptr, g->col, eid, g->n_rows, seeds, n_seeds, fanout, seed64, out_ptr,
                     out_col, out_eid);
  return launch_status(who);
}

// workspace layout: first[n_parent] | rank[n_dst + nnz] | tile_sums[tiles] | status[1]
size_t pg_block_compact_workspace(int64_t n_dst, int64_t nnz, int64_t n_parent) {
  if (n_dst < 0 || nnz < 0 || n_parent < 0) return 0;
  const int64_t n_all = n_dst + nnz;
  return align256((size_t)n_parent * 4) + align256((size_t)n_all * 4) +
         align256((size_t)std::max<int64_t>(1, tiles_of(n_all)) * 4) + 256;
}

int pg_block_compact(const int32_t* dst_ids, int64_t n_dst, const int32_t* col, int64_t nnz, int64_t n_parent,
                     int32_t* src_ids, int32_t* col_local, int32_t* n_src_dev, void* ws, size_t ws_bytes,
                     pg_stream_t stream) {
  const char* who = "pg_block_compact";
  if (n_dst < 0 || nnz < 0 || n_parent < 0 || n_dst + nnz > INT32_MAX - 1 || n_parent > INT32_MAX)
    return pg::set_error(PG_ERR_INVALID, "%s: bad sizes", who);
  if (!n_src_dev || (n_dst > 0 && !dst_ids) || (nnz > 0 && (!col || !col_local)) || (n_dst + nnz > 0 && !src_ids))
    return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  if (!ws || ws_bytes < pg_block_compact_workspace(n_dst, nnz, n_parent))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_all = n_dst + nnz;
  const int64_t nt = tiles_of(n_all);
  char* w = (char*)ws;
  int32_t* first = (int32_t*)w;
  w += align256((size_t)n_parent * 4);
  int32_t* rank = (int32_t*)w;
  w += align256((size_t)n_all * 4);
  int32_t* tile_sums = (int32_t*)w;
  w += align256((size_t)std::max<int64_t>(1, nt) * 4);
  int32_t* status = (int32_t*)w;
  hipLaunchKernelGGL(compact_init_kernel, dim3(grid_for(n_parent, kBlock)), dim3(kBlock), 0, st, first, n_parent,
                     status);
  if (n_all > 0) {
    hipLaunchKernelGGL(compact_min_kernel, dim3(grid_for(n_all, kBlock)), dim3(kBlock), 0, st, dst_ids, n_dst, col,
                       n_all, n_parent, first, status);
    hipLaunchKernelGGL(compact_flag_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, dst_ids, n_dst, col, n_all,
                       n_parent, (const int32_t*)first, rank, tile_sums, status);
  }
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, tile_sums, nt, n_src_dev,
                     (const int32_t*)status);
  if (n_all > 0) {
    hipLaunchKernelGGL(compact_src_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, dst_ids, n_dst, col, n_all,
                       n_parent, (const int32_t*)first, rank, (const int32_t*)tile_sums, src_ids);
    if (nnz > 0)
      hipLaunchKernelGGL(compact_local_kernel, dim3(grid_for(nnz, kBlock)), dim3(kBlock), 0, st, col, nnz, n_parent,
                         (const int32_t*)first, (const int32_t*)rank, col_local);
  }
  return launch_status(who);
}

}  // extern "C"
