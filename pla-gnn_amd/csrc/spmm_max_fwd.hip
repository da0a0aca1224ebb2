// Max forward: CSR SpMM with max / argmax (DGL SpMMCmpCsr<copy_lhs|u_mul_e, Max>), whole-row
// tiles and XCD column slices. Work decomposition and numerics: spmm_common.hpp.
#include "spmm_common.hpp"
#include "x3_split.hpp"

namespace {

// ---- max forward ---------------------------------------------------------------------
// In-launch combine of split rows for the whole-row forward (MERGE; replaces
// max_merge_kernel's launch), the max backward's hand-off (max_bwd_pull_kernel): every piece
// stores its partial maxima and positions write-through (sc1), drains them and draws a
// ticket from its (row, feature tile) counter (zeroed by a clear launch ahead); the piece
// that draws the last ticket reads the row's slots with sc1 loads and takes the maximum in
// slot order with strict > (the earliest maximal edge wins, as in max_merge_kernel).
struct FwdMerge {
  int chunk;            // the schedule's chunk
  uint32_t* tickets;    // [n_slots x n_ftiles]
  uint32_t val_bytes;   // the slot regions (< 2 GiB each, checked on the host)
  uint32_t arg_bytes;
};

template <int W, int NC, bool HAS_W, typename A, typename T = float, bool MERGE = false>
__global__ __launch_bounds__(kBlock) void max_fwd_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ eslot, const float* __restrict__ ew,
    const int4* __restrict__ items, int n_items, const T* __restrict__ X, int64_t ldx, int F,
    T* __restrict__ out, int64_t ldo, A* __restrict__ arg, int64_t lda,
    float* __restrict__ ws_val, A* __restrict__ ws_arg, int64_t ldw, int n_ftiles, int ftile, int dead_none,
    FwdMerge fm = {}) {
  constexpr int U = EdgeU<W, NC>::value;
  float* const val_base = ws_val;
  A* const arg_base = ws_arg;
  int ft = 0, f0 = 0;
  // n_ftiles > 1: all feature tiles of F in one launch, block b -> (item block b / n_ftiles,
  // tile b % n_ftiles), so every tile's longest items start first
  int bx = blockIdx.x;
  if (n_ftiles > 1) {
    const int t = bx % n_ftiles;
    ft = t;
    bx /= n_ftiles;
    f0 = t * ftile;
    X += f0;
    out += f0;
    arg += f0;
    if (ws_val) ws_val += f0;
    if (ws_arg) ws_arg += f0;
    F = min(ftile, F - f0);
  }
  const int it = bx * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z, slot = item.w;
  const int rs = ptr[row];
  const int lane = lane_id();
  const float ninf = -std::numeric_limits<float>::infinity();

  float best[NC][W];
  int bpos[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < W; ++i) {
      best[c][i] = ninf;
      bpos[c][i] = arg_none<A>();
    }

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int kl = kw + min(lane, nw - 1);
    const int idxv = col[kl];
    float wv = 1.f;
    if constexpr (HAS_W) wv = ew[eslot ? eslot[kl] : kl];
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float v[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const T* xr = X + (int64_t)bcast(idxv, j + min(e, nv - 1)) * ldx;
#pragma unroll
        for (int c = 0; c < NC; ++c) load_tile<W, T>(xr, (c * kWave + lane) * W, F, v[e][c], ninf);
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
          const int pos = kw + j + e - rs;
          float w = 1.f;
          if constexpr (HAS_W) w = bcastf(wv, j + e);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i) {
              const float m = HAS_W ? v[e][c][i] * w : v[e][c][i];
              if (m > best[c][i]) {
                best[c][i] = m;
                bpos[c][i] = pos;
              }
            }
        }
      }
    }
  }

  if (slot < 0) {
    // whole row: finalise (+-inf -> 0, empty row -> 0 / none)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < W; ++i)
        if (__builtin_isinf(best[c][i])) best[c][i] = 0.f;
    if (dead_none) {  // PG_ARG_DEAD_NONE: a zero maximum records no winner
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (best[c][i] == 0.f) bpos[c][i] = arg_none<A>();
    }
    T* orow = out + (int64_t)row * ldo;
    A* arow = arg + (int64_t)row * lda;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * kWave + lane) * W;
      store_tile<W, T>(orow, f, F, best[c]);
      store_arg<W, A>(arow, f, F, bpos[c]);
    }
  } else if constexpr (MERGE && W == 4) {
    const __amdgpu_buffer_rsrc_t rv = pg_x3::rsrc(val_base, fm.val_bytes);
    const __amdgpu_buffer_rsrc_t ra = pg_x3::rsrc(arg_base, fm.arg_bytes);
    auto voff = [&](int sl, int f) { return ((uint32_t)sl * (uint32_t)ldw + (uint32_t)(f0 + f)) * 4u; };
    auto aoff = [&](int sl, int f) { return ((uint32_t)sl * (uint32_t)ldw + (uint32_t)(f0 + f)) * (uint32_t)sizeof(A); };
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * kWave + lane) * W;
      if (f < F) {
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(pg_u32x4, make_float4(best[c][0], best[c][1], best[c][2], best[c][3])), rv,
            voff(slot, f), 0, 16);
        if constexpr (sizeof(A) == 2) {
          const pg_u32x2 a2 = {(uint32_t)(bpos[c][0] & 0xFFFF) | ((uint32_t)bpos[c][1] << 16),
                               (uint32_t)(bpos[c][2] & 0xFFFF) | ((uint32_t)bpos[c][3] << 16)};
          __builtin_amdgcn_raw_buffer_store_b64(a2, ra, aoff(slot, f), 0, 16);
        } else {
          const pg_u32x4 a4 = {(uint32_t)bpos[c][0], (uint32_t)bpos[c][1], (uint32_t)bpos[c][2], (uint32_t)bpos[c][3]};
          __builtin_amdgcn_raw_buffer_store_b128(a4, ra, aoff(slot, f), 0, 16);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every payload store drained before the ticket
    const int re = ptr[row + 1];
    const int s0 = slot - (k0 - rs) / fm.chunk;
    const int ns = (re - rs + fm.chunk - 1) / fm.chunk;
    uint32_t ticket = 0;
    if (lane == 0)
      ticket = __hip_atomic_fetch_add((pg_gu32*)(fm.tickets + (int64_t)s0 * n_ftiles + ft), 1u, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    if ((int)ticket != ns - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // keeps the loads below the ticket
    T* orow = out + (int64_t)row * ldo;
    A* arow = arg + (int64_t)row * lda;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * kWave + lane) * W;
      float bv[4] = {ninf, ninf, ninf, ninf};
      int bp[4] = {arg_none<A>(), arg_none<A>(), arg_none<A>(), arg_none<A>()};
      // 4 slots in flight, positions kept packed: the tail stays inside the main loop's
      // registers (8 slots and unpacked positions took the kernel from 46 to 68 VGPRs and
      // one wave per SIMD less for every item)
      constexpr int kS = 4;
      using AV = std::conditional_t<sizeof(A) == 2, pg_u32x2, pg_u32x4>;
      for (int sb = s0; sb < s0 + ns; sb += kS) {
        float4 v[kS];
        AV a[kS];
#pragma unroll
        for (int e = 0; e < kS; ++e) {
          const int sl = min(sb + e, s0 + ns - 1);
          v[e] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rv, voff(sl, f), 0, 16));
          if constexpr (sizeof(A) == 2) a[e] = __builtin_amdgcn_raw_buffer_load_b64(ra, aoff(sl, f), 0, 16);
          else a[e] = __builtin_amdgcn_raw_buffer_load_b128(ra, aoff(sl, f), 0, 16);
        }
#pragma unroll
        for (int e = 0; e < kS; ++e)
          if (sb + e < s0 + ns) {
            const float ve[4] = {v[e].x, v[e].y, v[e].z, v[e].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              int ai;
              if constexpr (sizeof(A) == 2) ai = (int)((a[e][i >> 1] >> (16 * (i & 1))) & 0xFFFF);
              else ai = (int)a[e][i];
              if (ve[i] > bv[i]) {
                bv[i] = ve[i];
                bp[i] = ai;
              }
            }
          }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (__builtin_isinf(bv[i])) bv[i] = 0.f;
        if (dead_none && bv[i] == 0.f) bp[i] = arg_none<A>();
      }
      store_tile<4, T>(orow, f, F, bv);
      store_arg<4, A>(arow, f, F, bp);
    }
  } else {
    float* orow = ws_val + (int64_t)slot * ldw;
    A* arow = ws_arg + (int64_t)slot * ldw;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * kWave + lane) * W;
      store_tile<W>(orow, f, F, best[c]);
      store_arg<W, A>(arow, f, F, bpos[c]);
    }
  }
}

// ---- max forward over XCD column slices ---------------------------------------------
// The feature columns are cut into slices of LPR * 4 columns; every workgroup of one XCD
// (blockIdx % 8 labels the XCD) works on the same slice, so the part of X that XCD gathers
// (N rows x one slice) is small enough to stay in its 4 MiB L2 instead of crossing the
// fabric to the Infinity Cache for every edge. A wave holds 64 / LPR items side by side
// (LPR lanes each; neighbouring items have similar lengths: the schedule is longest-first)
// and walks each item's edges in order, U row pieces in flight, so ties keep the first
// maximal edge exactly as max_fwd_kernel. Slice s of item block i: s = g + 8 * pass,
// i = blockIdx / 8 within the pass (n_slices >= 8), or the n_slices < 8 slices shared out
// over the eight XCD labels.
// Measured in the cfg2 step: 256-B slices take F = 256 from 96 to 82 us and F = 504 from
// 184 to 156 us (about 16 TB/s of gathered row bytes, close to the 17-19 TB/s the
// microarchitecture guide measures for gathers served by L2); 128-B slices, whose part of X
// fits an L2 whole, are no faster; on cfg5's 384 656-row bf16 graph slicing loses (8.1 ->
// 12.1 ms per step), hence the size gate. The XCD mapping is what pays: the same kernel
// with each slice spread over all XCDs (slice-major block order: slice = b / n_iblk) takes
// 113 us at F = 256.
#ifndef PG_FWD_SLICE
#define PG_FWD_SLICE 256  // bytes of a row per slice (0: whole-row tiles only)
#endif
#ifndef PG_FWD_SLICE_MAXTAB
#define PG_FWD_SLICE_MAXTAB (32ll << 20)  // largest slice of X (rows x slice bytes) sliced
#endif
// (slice, item block) of workgroup b over n_iblk item blocks, XCD-affine (see above)
__device__ __forceinline__ void slice_of_block(int b, int n_slices, int n_iblk, int& slice, int& iblk) {
  const int g = b % 8, v = b / 8;
  if (n_slices >= 8) {
    slice = g + 8 * (v / n_iblk);
    iblk = v % n_iblk;
  } else {
    const int rep = 8 / n_slices;
    slice = g % n_slices;
    iblk = v * rep + g / n_slices;
  }
}

// One lane group's running maximum over `len` edges from in-CSR slot k0 (positions
// relative to rs), LPR edges' ids per load, UE row pieces in flight. (A macro, not a
// function: passed by reference the running maxima took 109-126 registers against 72-75
// written out in the kernel.) It reads the enclosing kernel's `lane`, `col`, `eslot`, `ew`,
// `X`, `ldx`, `f`, `F`, `ninf` and updates its `best[4]` / `bpos[4]`.
#define PG_SLICE_RUN(LPR, UE, HAS_W, T, k0_, len_, rs_)                                              \
  do {                                                                                               \
    constexpr int U_ = (UE) < (LPR) ? (UE) : (LPR);                                                  \
    static_assert((LPR) <= 32 && (LPR) % U_ == 0, "slice lanes");                                    \
    const int sk0 = (k0_), slen = (len_), srs = (rs_);                                               \
    const int q_ = lane % (LPR);                                                                     \
    const int gbase = 4 * (lane - q_);                                                               \
    for (int j = 0; j < slen; j += (LPR)) {                                                          \
      const int kq = sk0 + j + min(q_, slen - j - 1);                                                \
      const int idv = col[kq];                                                                       \
      float wv = 1.f;                                                                                \
      if constexpr (HAS_W) wv = ew[eslot ? eslot[kq] : kq];                                          \
      _Pragma("unroll") for (int e0 = 0; e0 < (LPR); e0 += U_) {                                     \
        if (j + e0 >= slen) break;                                                                   \
        float x[U_][4];                                                                              \
        _Pragma("unroll") for (int e = 0; e < U_; ++e) {                                             \
          const int id = __builtin_amdgcn_ds_bpermute(gbase + 4 * (e0 + e), idv);                    \
          load_tile<4, T>(X + (int64_t)id * ldx, f, F, x[e], ninf);                                  \
        }                                                                                            \
        _Pragma("unroll") for (int e = 0; e < U_; ++e) {                                             \
          if (j + e0 + e < slen) {                                                                   \
            const int pos = sk0 + j + e0 + e - srs;                                                  \
            float w = 1.f;                                                                           \
            if constexpr (HAS_W)                                                                     \
              w = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(gbase + 4 * (e0 + e),       \
                                                                          __builtin_bit_cast(int, wv))); \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                          \
              const float m = HAS_W ? x[e][i] * w : x[e][i];                                         \
              if (m > best[i]) {                                                                     \
                best[i] = m;                                                                         \
                bpos[i] = pos;                                                                       \
              }                                                                                      \
            }                                                                                        \
          }                                                                                          \
        }                                                                                            \
      }                                                                                              \
    }                                                                                                \
  } while (0)

template <int LPR, typename A, typename T>
__device__ __forceinline__ void slice_store(T* __restrict__ out, int64_t ldo, A* __restrict__ arg, int64_t lda,
                                            int row, int f, int F, float (&best)[4], int (&bpos)[4],
                                            int dead_none) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (__builtin_isinf(best[i])) best[i] = 0.f;
    if (dead_none && best[i] == 0.f) bpos[i] = arg_none<A>();
  }
  store_tile<4, T>(out + (int64_t)row * ldo, f, F, best);
  store_arg<4, A>(arg + (int64_t)row * lda, f, F, bpos);
}

// Rows longer than the schedule's chunk (its split rows, `merges`, longest first) take the
// first hub_grid workgroups of the launch, one workgroup per (row, slice): its lane groups
// take contiguous runs of the row's edges, in order, and combine their maxima through LDS
// in run order (strict >: the earliest maximal edge wins, as in one sequential pass), so
// no partial slots and no merge launch. The other workgroups take the schedule's items and
// skip its pieces of those rows. (As a launch of its own before the other rows, the split
// rows' tail ran alone: 0.350 vs 0.301 ms per cfg2 step.)
template <int LPR, int UE, bool HAS_W, typename A, typename T = float>
__global__ __launch_bounds__(kBlock) void max_fwd_slice_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ eslot, const float* __restrict__ ew,
    const int4* __restrict__ items, int n_items, const int4* __restrict__ hubs, int n_hub, int hub_grid,
    const T* __restrict__ X, int64_t ldx, int F, T* __restrict__ out, int64_t ldo, A* __restrict__ arg,
    int64_t lda, int n_slices, int n_iblk, int dead_none) {
  constexpr int RPW = kWave / LPR;
  constexpr int CS = LPR * 4;
  constexpr int NG = RPW * kWavesPerBlock;  // lane groups per workgroup
  __shared__ float hv[NG][CS];
  __shared__ int hp[NG][CS];
  const int lane = lane_id();
  const float ninf = -std::numeric_limits<float>::infinity();
  float best[4] = {ninf, ninf, ninf, ninf};
  int bpos[4] = {arg_none<A>(), arg_none<A>(), arg_none<A>(), arg_none<A>()};
  int b = blockIdx.x;
  int slice, iblk;
  if (b < hub_grid) {
    // a split row, whole: the workgroup's lane groups take contiguous runs of its edges
    slice_of_block(b, n_slices, n_hub, slice, iblk);
    if (slice >= n_slices || iblk >= n_hub) return;  // uniform over the workgroup
    const int row = hubs[iblk].x;
    const int rs = ptr[row], deg = ptr[row + 1] - rs;
    const int grp = wave_id_uniform() * RPW + lane / LPR;
    const int run = (deg + NG - 1) / NG;
    const int k0 = min(deg, grp * run);
    const int len = min(deg, k0 + run) - k0;
    const int c = (lane % LPR) * 4;
    const int f = slice * CS + c;
    PG_SLICE_RUN(LPR, UE, HAS_W, T, rs + k0, len, rs);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[grp][c + i] = best[i];
      hp[grp][c + i] = bpos[i];
    }
    __syncthreads();
    if (grp == 0) {
      for (int r = 1; r < NG; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (hv[r][c + i] > best[i]) {
            best[i] = hv[r][c + i];
            bpos[i] = hp[r][c + i];
          }
      slice_store<LPR, A, T>(out, ldo, arg, lda, row, f, F, best, bpos, dead_none);
    }
    return;
  }
  slice_of_block(b - hub_grid, n_slices, n_iblk, slice, iblk);
  if (slice >= n_slices || iblk >= n_iblk) return;
  const int it = (iblk * kWavesPerBlock + wave_id_uniform()) * RPW + lane / LPR;
  if (it >= n_items) return;
  const int4 item = items[it];
  if (item.w >= 0) return;  // a piece of a split row: taken whole above
  const int row = item.x;
  const int f = slice * CS + (lane % LPR) * 4;
  PG_SLICE_RUN(LPR, UE, HAS_W, T, item.y, item.z - item.y, ptr[row]);
  slice_store<LPR, A, T>(out, ldo, arg, lda, row, f, F, best, bpos, dead_none);
}

// Combine the partial maxima of split rows in chunk order (earlier chunk wins ties).
// One workgroup per split row, one thread per feature; slot loads batched.
template <typename A, typename T = float>
__global__ __launch_bounds__(kBlock) void max_merge_kernel(const int4* __restrict__ merges,
                                                           int n_merges, int F,
                                                           const float* __restrict__ ws_val,
                                                           const A* __restrict__ ws_arg,
                                                           int64_t ldw, T* __restrict__ out,
                                                           int64_t ldo, A* __restrict__ arg,
                                                           int64_t lda, int dead_none) {
  const int4 m = merges[blockIdx.x];
  const int row = m.x, s0 = m.y, ns = m.z;
  for (int f = threadIdx.x; f < F; f += kBlock) {
    float best = -std::numeric_limits<float>::infinity();
    int bp = arg_none<A>();
    for (int s = s0; s < s0 + ns; s += 8) {
      float v[8];
      int a[8];  // loaded with the values: no dependent load behind each compare
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t o = (int64_t)min(s + e, s0 + ns - 1) * ldw + f;
        v[e] = ws_val[o];
        a[e] = (int)ws_arg[o];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (s + e < s0 + ns && v[e] > best) {
          best = v[e];
          bp = a[e];
        }
    }
    if (__builtin_isinf(best)) best = 0.f;
    if (dead_none && best == 0.f) bp = arg_none<A>();
    out[(int64_t)row * ldo + f] = from_f<T>(best);
    arg[(int64_t)row * lda + f] = (A)bp;
  }
}

#ifndef PG_FWD_MERGE
#define PG_FWD_MERGE 1  // split rows combined inside the whole-row forward (0: the max_merge_kernel launch)
#endif

template <typename A, typename T>
int launch_max_fwd(const pg_csr_t* g, const T* X, int64_t ldx, int64_t F, T* out,
                   int64_t ldo, A* arg, int64_t lda, float* ws_val, A* ws_arg, int64_t ldw,
                   int dead_none, hipStream_t st, uint32_t* tickets) {
  // argpos rows: u16 x4 = 8 B -> need 8-B alignment only; treat via the same 16-B check on
  // the float operands and an 8-B check on arg.
  TilePlan tp = plan_tiles(F, {ldx, ldo, lda}, {X, out, ws_val});
  if (tp.vec && (((uintptr_t)arg & (4 * sizeof(A) - 1)) != 0 ||
                 ((uintptr_t)ws_arg & (4 * sizeof(A) - 1)) != 0))
    tp.vec = false;
  if (!tp.vec) tp.tile = kFTileScalar;
  const bool has_w = g->ew != nullptr;
  const int blocks = grid_for(g->n_items);
  // every feature tile in one launch (blocks interleaved over the tiles), one merge launch
  // over the whole F
  const int n_ft = (int)((F + tp.tile - 1) / tp.tile);
  if constexpr (PG_FWD_SLICE > 0) if (tp.vec && g->n_items > 0 && (g->n_merges == 0 || g->merges)) {
    // XCD column slices (max_fwd_slice_kernel); split rows whole, first. The slices must share
    // out over the 8 XCDs (1, 2, 4 or a multiple of 8 of them): a width whose PG_FWD_SLICE-byte
    // slices do not (F = 400 f32: 7 of 64 columns) tries slices twice as wide (4 of 128).
    auto try_slices = [&](auto lpr_c) -> bool {
      constexpr int LPR = decltype(lpr_c)::value;
      constexpr int RPW = kWave / LPR;
      const int n_sl = (int)((F + 4 * LPR - 1) / (4 * LPR));
      if (!(n_sl % 8 == 0 || n_sl == 1 || n_sl == 2 || n_sl == 4) ||
          g->n_cols * (int64_t)(4 * LPR * sizeof(T)) > PG_FWD_SLICE_MAXTAB)
        return false;
      auto grid_of = [&](int64_t n_iblk) -> int64_t {
        if (n_iblk == 0) return 0;
        return n_sl >= 8 ? n_iblk * n_sl : 8 * ((n_iblk + 8 / n_sl - 1) / (8 / n_sl));
      };
      const int n_iblk = (int)((g->n_items + RPW * kWavesPerBlock - 1) / (RPW * kWavesPerBlock));
      const int n_hub = (int)g->n_merges;
      // row pieces in flight per lane group: 4 with one slice per XCD and no edge weights
      // (cfg2's F = 512: 147.8-148.2 vs 151.8 us), else 8 (F = 256: 81.6 vs 88.5 us; cfg3's
      // weighted F = 512: 169-171 vs 177-180 us)
      auto go = [&](auto hw_c, auto ue_c) {
        constexpr bool HW = decltype(hw_c)::value;
        constexpr int UE = decltype(ue_c)::value;
        const int64_t hub_grid = grid_of(n_hub);
        hipLaunchKernelGGL((max_fwd_slice_kernel<LPR, UE, HW, A, T>), dim3((unsigned)(hub_grid + grid_of(n_iblk))),
                           dim3(kBlock), 0, st, g->ptr, g->col, g->eslot, g->ew, (const int4*)g->items,
                           (int)g->n_items, (const int4*)g->merges, n_hub, (int)hub_grid, X, ldx, (int)F, out, ldo,
                           arg, lda, n_sl, n_iblk, dead_none);
      };
      using U4 = std::integral_constant<int, 4>;
      using U8 = std::integral_constant<int, 8>;
      if (n_sl >= 8 && !has_w) {
        go(std::false_type{}, U4{});
      } else {
        if (has_w) go(std::true_type{}, U8{}); else go(std::false_type{}, U8{});
      }
      return true;
    };
    constexpr int LPR0 = std::min(32, PG_FWD_SLICE / (4 * (int)sizeof(T)));
    bool done = try_slices(std::integral_constant<int, LPR0>{});
    if constexpr (2 * LPR0 <= 32)
      if (!done) done = try_slices(std::integral_constant<int, 2 * LPR0>{});
    if (done) return hip_status("pg_spmm_max_fwd");
  }
  {
    const int64_t f0 = 0;
    const int Ft = (int)std::min<int64_t>(tp.tile, F);
    // split rows combined inside the launch (max_merge_kernel's launch otherwise): the vector
    // path, the schedule's chunk known, slot regions a 32-bit buffer offset covers
    const size_t vbytes = round_up(g->n_slots * ldw * 4, 256), abytes = round_up(g->n_slots * ldw * (int64_t)sizeof(A), 256);
    const bool merge_in = PG_FWD_MERGE && tp.vec && g->n_merges > 0 && g->chunk > 0 && tickets &&
                          vbytes < ((size_t)1 << 31) && abytes < ((size_t)1 << 31);
    if (merge_in) {  // the tickets start at zero: [n_slots x n_ft] words, a 256-B padded block
      const int64_t n4 = round_up(g->n_slots * n_ft * 4, 256) / 16;
      hipLaunchKernelGGL(clear_u4_kernel, dim3((unsigned)std::min<int64_t>(2048, (n4 + kBlock - 1) / kBlock)),
                         dim3(kBlock), 0, st, reinterpret_cast<uint4*>(tickets), n4);
    }
    const FwdMerge fm{g->chunk, tickets, (uint32_t)vbytes, (uint32_t)abytes};
    auto go = [&](auto nc_c, auto w_c, auto hw_c) -> int {
      constexpr int NC = decltype(nc_c)::value;
      constexpr int W = decltype(w_c)::value;
      constexpr bool HW = decltype(hw_c)::value;
      auto launch = [&](auto merge_c) {
        hipLaunchKernelGGL((max_fwd_kernel<W, NC, HW, A, T, decltype(merge_c)::value>), dim3((unsigned)blocks * n_ft),
                           dim3(kBlock), 0, st, g->ptr, g->col, g->eslot, g->ew, (const int4*)g->items,
                           (int)g->n_items, X, ldx, n_ft > 1 ? (int)F : Ft, out, ldo, arg, lda, ws_val, ws_arg, ldw,
                           n_ft, (int)tp.tile, dead_none, fm);
        return PG_OK;
      };
      if constexpr (W == 4)  // merge_in needs the vector path: the scalar kernels have no MERGE form
        if (merge_in) return launch(std::true_type{});
      return launch(std::false_type{});
    };
    const int rc = dispatch_tile(tp, Ft, has_w, go);
    if (rc != PG_OK) return pg::set_error(rc, "pg_spmm_max_fwd: unsupported feature tile");
    if (g->n_merges > 0 && !merge_in) {
      hipLaunchKernelGGL((max_merge_kernel<A, T>), dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)g->n_merges, (int)F, ws_val + f0, ws_arg + f0,
                         ldw, out + f0, ldo, arg + f0, lda, dead_none);
    }
  }
  return hip_status("pg_spmm_max_fwd");
}

template <typename T>
int max_fwd_entry(const pg_csr_t* g, const T* X, int64_t ldx, int64_t F, T* out, int64_t ldo,
                  void* argpos, int64_t lda, int arg_kind, void* ws, size_t ws_bytes,
                  pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_spmm_max_fwd", true));
  const int dead_none = (arg_kind & PG_ARG_DEAD_NONE) != 0;
  arg_kind &= ~PG_ARG_DEAD_NONE;
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd: bad arg_kind %d", arg_kind);
  if (F < 0 || ldx < F || ldo < F || lda < F)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd: bad F/leading dims");
  if (arg_kind == PG_ARG_U16 && g->max_deg >= 0xFFFF)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd: max degree %d needs PG_ARG_I32",
                         g->max_deg);
  if (F == 0 || g->n_rows == 0) return pg::ok();
  if (!X || !out || !argpos) return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd: NULL buffer");
  const size_t need = pg_spmm_max_fwd_workspace(g, F, arg_kind);
  PG_TRY(check_ws(ws_bytes, need, "pg_spmm_max_fwd"));
  const int64_t ldw = ws_ld(F);
  float* ws_val = need ? (float*)ws : nullptr;
  void* ws_arg = need ? (char*)ws + round_up(g->n_slots * ldw * 4, 256) : nullptr;
  // [slot values | slot positions | split-row tickets]
  uint32_t* tickets = need ? (uint32_t*)((char*)ws_arg + round_up(g->n_slots * ldw * (int64_t)pg::arg_bytes(arg_kind), 256))
                           : nullptr;
  if (((uintptr_t)ws & 255) != 0) tickets = nullptr;  // (the in-launch combine wants aligned regions)
  hipStream_t st = (hipStream_t)stream;
  if (arg_kind == PG_ARG_U16)
    return launch_max_fwd<uint16_t, T>(g, X, ldx, F, out, ldo, (uint16_t*)argpos, lda, ws_val,
                                       (uint16_t*)ws_arg, ldw, dead_none, st, tickets);
  return launch_max_fwd<int32_t, T>(g, X, ldx, F, out, ldo, (int32_t*)argpos, lda, ws_val,
                                    (int32_t*)ws_arg, ldw, dead_none, st, tickets);
}

}  // namespace

extern "C" {

size_t pg_spmm_max_fwd_workspace(const pg_csr_t* g, int64_t F, int arg_kind) {
  if (!g || g->n_slots <= 0 || F <= 0) return 0;
  const int64_t ldw = ws_ld(F);
  const size_t vals = round_up(g->n_slots * ldw * 4, 256);
  const size_t args = round_up(g->n_slots * ldw * (int64_t)pg::arg_bytes(arg_kind & ~PG_ARG_DEAD_NONE), 256);
  // the whole-row kernel's split-row tickets: one word per slot and 256-column feature tile
  const size_t tickets = round_up(g->n_slots * ((F + 255) / 256) * 4, 256);
  return vals + args + tickets;
}

int pg_spmm_max_fwd(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, float* out,
                    int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
                    size_t ws_bytes, pg_stream_t stream) {
  return max_fwd_entry<float>(g, X, ldx, F, out, ldo, argpos, lda, arg_kind, ws, ws_bytes, stream);
}

int pg_spmm_max_fwd_bf16(const pg_csr_t* g, const void* X, int64_t ldx, int64_t F, void* out,
                         int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
                         size_t ws_bytes, pg_stream_t stream) {
  return max_fwd_entry<uint16_t>(g, (const uint16_t*)X, ldx, F, (uint16_t*)out, ldo, argpos, lda,
                                 arg_kind, ws, ws_bytes, stream);
}

}  // extern "C"
