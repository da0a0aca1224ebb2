// Link-prediction mini-batches (dgl.dataloading.as_edge_prediction_sampler): the per-batch work
// an edge-seeded loop adds to sample.hip's. Not used by the reference (node classification on
// the full graph): reference-unpinned. Integer only; every result equals its _cpu twin
// (cpu_backend.cpp) bit for bit.
//
// pg_edge_bits_update   a bit set over edge ids: atomicOr / atomicAnd of one word per id
//                       (order-independent on integers).
// pg_sample_count_excl  one wave per seed row: the row's entries whose bit is clear, capped at
//                       fanout; then scan.hpp's tile scan as pg_sample_count.
// pg_sample_fill_excl   sample_fill_kernel's structure (one wave per row, the bitwise threshold
//                       search over (key, position) composites counted with ballots) on the rows
//                       with the excluded entries left out. A row that fits LDS reads the bit
//                       set once, into kCap / 32 flag words beside its keys; an excluded entry's
//                       composite is all ones, above every searched bit (32 + position bits
//                       <= 63), so no `comp < trial` counts it and the final `comp <= V` skips
//                       it. A hub row gathers only surviving (key, position) pairs, under a
//                       threshold estimated from the row's remaining count.
// pg_edge_lookup        one wave per (u, v) pair scans row v for column u; the first match of a
//                       ballot is the smallest edge id (rows ascend in edge id).
// pg_negative_sample    one wave per slot: every lane computes the slot's draws (sample_key.hpp),
//                       the wave looks each candidate up as pg_edge_lookup does. Failures are
//                       counted with an int32 atomicAdd.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "sample_key.hpp"
#include "scan.hpp"

namespace {

constexpr int kCap = PG_SAMPLE_LDS_KEYS;
constexpr int kCand = kCap / 2;        // (key, position) candidates of a hub row in the same LDS
constexpr int kFlagWords = kCap / 32;  // exclusion flags of an LDS-resident row
constexpr uint64_t kExcluded = ~0ull;  // a composite no pass of the search reaches

// the bit of edge id e; an id outside the bit set's range counts as not excluded
__device__ inline bool excluded(const uint32_t* __restrict__ bits, int64_t n_ids, int32_t e) {
  return bits && e >= 0 && e < n_ids && ((bits[e >> 5] >> (e & 31)) & 1u);
}

__global__ __launch_bounds__(kBlock) void edge_bits_kernel(uint32_t* bits, int64_t n_ids, const int32_t* eids, int64_t n,
                                                           int set, int32_t* status) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int32_t e = eids[i];
    if (e < 0 || e >= n_ids) {
      if (status) status[0] = -2;  // every writer stores the same value
      continue;
    }
    const uint32_t m = 1u << (e & 31);
    if (set)
      atomicOr(&bits[e >> 5], m);
    else
      atomicAnd(&bits[e >> 5], ~m);
  }
}

// counts[row] = min(entries of the seed's row whose bit is clear, fanout); one wave per row
__global__ __launch_bounds__(kBlock) void sample_count_excl_kernel(const int32_t* __restrict__ ptr,
                                                                   const int32_t* __restrict__ eid, int64_t n_rows,
                                                                   int64_t n_ids, const int32_t* __restrict__ seeds,
                                                                   int64_t n_seeds, int32_t fanout,
                                                                   const uint32_t* __restrict__ bits,
                                                                   int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave; row < n_seeds;
       row += (int64_t)gridDim.x * kWavesPerBlock) {
    const int32_t s = seeds[row];
    int32_t rem = 0;
    if (s >= 0 && s < n_rows) {
      const int32_t b = ptr[s];
      const int32_t deg = ptr[s + 1] - b;
      if (deg > 0 && !bits) rem = deg;
      if (deg > 0 && bits) {
        for (int32_t j = lane; j < deg; j += kWave) rem += !excluded(bits, n_ids, eid ? eid[b + j] : b + j);
        for (int off = kWave / 2; off > 0; off >>= 1) rem += __shfl_xor(rem, off);
      }
    }
    if (fanout >= 0 && rem > fanout) rem = fanout;
    if (lane == 0) counts[row] = rem;
  }
}

__global__ __launch_bounds__(kBlock) void scan_counts_kernel(const int32_t* counts, int64_t n, int32_t* out_ptr,
                                                             int32_t* tile_sums) {
  __shared__ int lds[kBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread;
  int v[kPerThread];
  for (int q = 0; q < kPerThread; ++q) v[q] = i0 + q < n ? counts[i0 + q] : 0;
  tile_scan_store(v, i0, n, out_ptr, tile_sums, lds);
}

__global__ __launch_bounds__(kBlock) void sample_fill_excl_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid, int64_t n_rows,
    int64_t n_ids, const int32_t* __restrict__ seeds, int64_t n_seeds, int32_t fanout, uint64_t seed64,
    const uint32_t* __restrict__ bits, const int32_t* __restrict__ out_ptr, int32_t* __restrict__ out_col,
    int32_t* __restrict__ out_eid) {
  __shared__ uint32_t keys_lds[kWavesPerBlock][kCap];
  __shared__ uint32_t flags_lds[kWavesPerBlock][kFlagWords];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  uint32_t* keys = keys_lds[wave];
  uint32_t* flags = flags_lds[wave];
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));  // lanes before this one
  for (int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave; row < n_seeds;
       row += (int64_t)gridDim.x * kWavesPerBlock) {
    // the previous row's reads of this wave's LDS come before this row's writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int32_t s = seeds[row];
    if (s < 0 || s >= n_rows) continue;
    const int32_t b = ptr[s];
    const int32_t deg = ptr[s + 1] - b;
    if (deg <= 0 || fanout == 0) continue;
    const int64_t o = out_ptr[row];
    const bool in_lds = deg <= kCap;
    auto eid_at = [&](int32_t j) -> int32_t { return eid ? eid[b + j] : b + j; };
    // the row's remaining count; an LDS-resident row keeps the flags (word w of lane 0's two
    // stores covers positions 32 w .. 32 w + 31; j0 <= kCap - 64, so both fit kFlagWords)
    int32_t rem = deg;
    for (int32_t j0 = 0; j0 < deg; j0 += kWave) {
      const int32_t j = j0 + lane;
      const uint64_t m = __ballot(j < deg && excluded(bits, n_ids, eid_at(j)));
      rem -= __popcll(m);
      if (in_lds && lane == 0) {
        flags[j0 >> 5] = (uint32_t)m;
        flags[(j0 >> 5) + 1] = (uint32_t)(m >> 32);
      }
    }
    // the flags were written by lane 0
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (rem <= 0) continue;
    auto out_of = [&](int32_t j) -> bool {  // j < deg
      return in_lds ? ((flags[j >> 5] >> (j & 31)) & 1u) != 0 : excluded(bits, n_ids, eid_at(j));
    };
    if (fanout < 0 || rem <= fanout) {  // every remaining entry, in order
      int32_t base = 0;
      for (int32_t j0 = 0; j0 < deg; j0 += kWave) {
        const int32_t j = j0 + lane;
        const bool p = j < deg && !out_of(j);
        const uint64_t m = __ballot(p);
        if (p) {
          const int64_t at = o + base + __popcll(m & below);
          out_col[at] = col[b + j];
          out_eid[at] = eid_at(j);
        }
        base += __popcll(m);
      }
      continue;
    }
    const int pb = pg::pos_bits(deg);
    const int32_t rank = fanout - 1;
    auto key_at = [&](int32_t j) -> uint32_t { return pg::sample_key(seed64, eid_at(j)); };
    // sample_fill_kernel's search: the composite V of rank fanout - 1 among the n candidates,
    // bit by bit from the top, then the candidates <= V in order. kExcluded is never below a
    // trial (trial < 2^(32 + pb)) and never <= V
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
          out_eid[at] = eid_at(j);
        }
        base += __popcll(m);
      }
    };
    if (in_lds) {  // keys in LDS; every lane reads back only the keys it wrote itself
      for (int32_t j = lane; j < deg; j += kWave) keys[j] = key_at(j);
      select(deg,
             [&](int32_t i) { return out_of(i) ? kExcluded : (((uint64_t)keys[i] << pb) | (uint64_t)(uint32_t)i); },
             [&](int32_t i) { return i; });
      continue;
    }
    // a hub row, narrowed as in sample_fill_kernel; the threshold is set for an expected
    // 2 fanout + 64 of the rem remaining keys (rem > fanout; at most 2^32: every key passes)
    bool done = false;
    if (2 * (int64_t)fanout + 64 <= kCand) {
      uint32_t* ckey = keys;
      int32_t* cpos = (int32_t*)(keys + kCand);
      uint64_t t0 = ((uint64_t)(2 * fanout + 64) << 32) / (uint64_t)rem;
      if (t0 > (1ull << 32)) t0 = 1ull << 32;
      bool ok = false;
      for (int tries = 0; tries < 40 && !ok; ++tries) {
        int32_t mine = 0;
        for (int32_t j = lane; j < deg; j += kWave) mine += !out_of(j) && (uint64_t)key_at(j) < t0;
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
          const bool p = j < deg && (uint64_t)k < t0 && !out_of(j);
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
        done = true;
      }
    }
    if (!done)  // a fanout too large for the candidate buffer: every pass of the search walks the row
      select(deg,
             [&](int32_t i) { return out_of(i) ? kExcluded : (((uint64_t)key_at(i) << pb) | (uint64_t)(uint32_t)i); },
             [&](int32_t i) { return i; });
  }
}

// first position of column u in row v (both in range, the same for every lane), -1: none
__device__ inline int32_t wave_row_find(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, int32_t v,
                                        int32_t u, int lane) {
  const int32_t b = ptr[v];
  const int32_t deg = ptr[v + 1] - b;
  for (int32_t j0 = 0; j0 < deg; j0 += kWave) {
    const int32_t j = j0 + lane;
    const uint64_t m = __ballot(j < deg && col[b + j] == u);
    if (m) return b + j0 + __ffsll((unsigned long long)m) - 1;
  }
  return -1;
}

__global__ __launch_bounds__(kBlock) void edge_lookup_kernel(const int32_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ col,
                                                             const int32_t* __restrict__ eid, int64_t n_rows,
                                                             int64_t n_cols, const int32_t* __restrict__ u,
                                                             const int32_t* __restrict__ v, int64_t n,
                                                             int32_t* __restrict__ out_eid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wave; i < n; i += (int64_t)gridDim.x * kWavesPerBlock) {
    const int32_t uu = u[i], vv = v[i];
    int32_t slot = -1;
    if (uu >= 0 && uu < n_cols && vv >= 0 && vv < n_rows) slot = wave_row_find(ptr, col, vv, uu, lane);
    if (lane == 0) out_eid[i] = slot < 0 ? -1 : (eid ? eid[slot] : slot);
  }
}

__global__ void zero_one_kernel(int32_t* p) { p[0] = 0; }

__global__ __launch_bounds__(kBlock) void negative_sample_kernel(const int32_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ col, int64_t n_rows,
                                                                 int64_t n_cols, const int32_t* __restrict__ pos_src,
                                                                 const int32_t* __restrict__ pos_id, int64_t n_pos,
                                                                 int32_t k, int32_t tries, int flags, uint64_t seed64,
                                                                 int32_t* __restrict__ neg_src,
                                                                 int32_t* __restrict__ neg_dst, int32_t* n_fail) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t n_slots = n_pos * k;
  for (int64_t slot = (int64_t)blockIdx.x * kWavesPerBlock + wave; slot < n_slots;
       slot += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t i = slot / k;
    const int32_t j = (int32_t)(slot - i * k);
    const int32_t id = pos_id ? pos_id[i] : (int32_t)i;
    const int32_t fixed = pos_src ? pos_src[i] : 0;
    int32_t ru = -1, rv = -1;
    const bool can = n_rows > 0 && n_cols > 0 && fixed >= 0 && fixed < n_cols;
    for (int32_t t = 0; can && t < tries; ++t) {
      const int32_t uu = pos_src ? fixed : pg::key_to_range(pg::negative_key(seed64, id, j, t, 0), n_cols);
      const int32_t vv = pg::key_to_range(pg::negative_key(seed64, id, j, t, 1), n_rows);
      if ((flags & PG_NEG_REJECT_SELF) && uu == vv) continue;
      if ((flags & PG_NEG_REJECT_EDGE) && wave_row_find(ptr, col, vv, uu, lane) >= 0) continue;
      ru = uu;
      rv = vv;
      break;
    }
    if (lane == 0) {
      neg_src[slot] = ru;
      neg_dst[slot] = rv;
      if (ru < 0) atomicAdd(n_fail, 1);
    }
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

inline int check_seeds(const char* who, const int32_t* seeds, int64_t n_seeds, const int32_t* out_ptr) {
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  return PG_OK;
}

}  // namespace

extern "C" {

int pg_edge_bits_update(uint32_t* bits, int64_t n_edge_ids, const int32_t* eids, int64_t n, int set,
                        int32_t* status_dev, pg_stream_t stream) {
  const char* who = "pg_edge_bits_update";
  if (n_edge_ids < 0 || n_edge_ids > INT32_MAX || n < 0 || n > INT32_MAX)
    return pg::set_error(PG_ERR_INVALID, "%s: bad sizes", who);
  if (n == 0) return pg::ok();
  if (!eids || (n_edge_ids > 0 && !bits)) return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  hipLaunchKernelGGL(edge_bits_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, bits,
                     n_edge_ids, eids, n, set, status_dev);
  return launch_status(who);
}

// workspace layout: counts[n_seeds] | tile_sums[tiles]
size_t pg_sample_count_excl_workspace(int64_t n_seeds) {
  if (n_seeds < 0) return 0;
  return align256((size_t)std::max<int64_t>(1, n_seeds) * sizeof(int32_t)) +
         align256((size_t)std::max<int64_t>(1, tiles_of(n_seeds)) * sizeof(int32_t));
}

int pg_sample_count_excl(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                         int32_t fanout, const uint32_t* excl_bits, int32_t* out_ptr, void* ws, size_t ws_bytes,
                         pg_stream_t stream) {
  const char* who = "pg_sample_count_excl";
  PG_TRY(pg::check_csr(g, who, false));
  PG_TRY(check_seeds(who, seeds, n_seeds, out_ptr));
  if (!ws || ws_bytes < pg_sample_count_excl_workspace(n_seeds))
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  int32_t* counts = (int32_t*)ws;
  int32_t* tile_sums = (int32_t*)((char*)ws + align256((size_t)std::max<int64_t>(1, n_seeds) * sizeof(int32_t)));
  const int64_t nt = tiles_of(n_seeds);
  if (nt > 0) {
    hipLaunchKernelGGL(sample_count_excl_kernel, dim3(grid_for(n_seeds, kWavesPerBlock)), dim3(kBlock), 0, st, g->ptr,
                       eid, g->n_rows, g->nnz, seeds, n_seeds, fanout, excl_bits, counts);
    hipLaunchKernelGGL(scan_counts_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, (const int32_t*)counts, n_seeds,
                       out_ptr, tile_sums);
  }
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, tile_sums, nt, out_ptr + n_seeds,
                     (const int32_t*)nullptr);
  if (nt > 1)
    hipLaunchKernelGGL(add_tile_offsets_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, out_ptr, n_seeds, tile_sums);
  return launch_status(who);
}

int pg_sample_fill_excl(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds, int32_t fanout,
                        uint64_t seed64, const uint32_t* excl_bits, const int32_t* out_ptr, int32_t* out_col,
                        int32_t* out_eid, pg_stream_t stream) {
  const char* who = "pg_sample_fill_excl";
  if (!excl_bits) return pg_sample_fill(g, eid, seeds, n_seeds, fanout, seed64, out_ptr, out_col, out_eid, stream);
  PG_TRY(pg::check_csr(g, who, false));
  PG_TRY(check_seeds(who, seeds, n_seeds, out_ptr));
  if (n_seeds == 0 || g->nnz == 0 || fanout == 0) return pg::ok();
  if (!out_col || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  hipLaunchKernelGGL(sample_fill_excl_kernel, dim3(grid_for(n_seeds, kWavesPerBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, g->ptr, g->col, eid, g->n_rows, g->nnz, seeds, n_seeds, fanout, seed64,
                     excl_bits, out_ptr, out_col, out_eid);
  return launch_status(who);
}

int pg_edge_lookup(const pg_csr_t* g, const int32_t* eid, const int32_t* u, const int32_t* v, int64_t n,
                   int32_t* out_eid, pg_stream_t stream) {
  const char* who = "pg_edge_lookup";
  PG_TRY(pg::check_csr(g, who, false));
  if (n < 0 || n > INT32_MAX) return pg::set_error(PG_ERR_INVALID, "%s: bad n", who);
  if (n == 0) return pg::ok();
  if (!u || !v || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  hipLaunchKernelGGL(edge_lookup_kernel, dim3(grid_for(n, kWavesPerBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     g->ptr, g->col, eid, g->n_rows, g->n_cols, u, v, n, out_eid);
  return launch_status(who);
}

int pg_negative_sample(const pg_csr_t* g, const int32_t* pos_src, const int32_t* pos_id, int64_t n_pos, int32_t k,
                       int32_t tries, int flags, uint64_t seed64, int32_t* neg_src, int32_t* neg_dst,
                       int32_t* n_fail_dev, pg_stream_t stream) {
  const char* who = "pg_negative_sample";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_pos < 0 || k < 1 || tries < 1 || tries > 64 || n_pos * (int64_t)k > INT32_MAX ||
      (flags & ~(PG_NEG_REJECT_EDGE | PG_NEG_REJECT_SELF)))
    return pg::set_error(PG_ERR_INVALID, "%s: n_pos >= 0, k >= 1, 1 <= tries <= 64, n_pos k < 2^31, known flags", who);
  if (!n_fail_dev || (n_pos > 0 && (!neg_src || !neg_dst)))
    return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_one_kernel, dim3(1), dim3(1), 0, st, n_fail_dev);
  if (n_pos > 0)
    hipLaunchKernelGGL(negative_sample_kernel, dim3(grid_for(n_pos * k, kWavesPerBlock)), dim3(kBlock), 0, st, g->ptr,
                       g->col, g->n_rows, g->n_cols, pos_src, pos_id, n_pos, k, tries, flags, seed64, neg_src,
                       neg_dst, n_fail_dev);
  return launch_status(who);
}

}  // extern "C"
