// Message-passing kernels for gfx950 (MI355X): CSR SpMM with max/argmax (DGL
// SpMMCmpCsr<copy_lhs|u_mul_e, Max>, reached from SAGEConv('pool') at
// code/model.py:20/22/24), its backward (DGL GSpMM.backward scatter_add_ through argX,
// reached from code/train.py:204), the sum/mean variants, SDDMM, multi-head attention and
// g-SpMM / g-SDDMM for vector edge features (DGL's gspmm / gsddmm) and the fused GATv2
// attention scores. This header holds what two or more of the families share; one source
// per family: spmm_max_fwd.hip, spmm_max_bwd.hip, spmm_sum.hip (sum / mean, SDDMM),
// attention.hip (edge softmax, per-head sum and SDDMM, GATv2 scores) and gspmm.hip.
// Everything here has internal linkage: each source gets its own copy of what it uses.
//
// Work decomposition: one 64-lane wave per schedule item {row, k0, k1, slot}. A row
// longer than the schedule's chunk is cut into several items whose partial results go
// to workspace slots and are combined in chunk order by a merge kernel, so hub rows do
// not serialise on one wave. Items are ordered longest first (pg_schedule_build).
// Inside a wave each lane owns W consecutive features (W = 4: float4 loads, 1 KiB per
// wave-instruction; W = 1: scalar path for unaligned rows) in NC chunks of 64*W.
// Row indices and weights are wave-uniform and come through the scalar cache.
//
// Numerics: the max is a selection (bit-exact); ties keep the earlier entry (strict >),
// matching DGL's in-order loop. Backward sums run in ascending destination order, the
// same order as a sequential scatter_add_, so unsplit rows are bit-exact against it.
// Build with -ffp-contract=off (no silent FMA contraction).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <type_traits>

#include "common.hpp"

namespace {

// global agent-scope words (split-row tickets) and the buffer builtins' vector types
typedef __attribute__((address_space(1))) uint32_t pg_gu32;
typedef uint32_t pg_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pg_u32x2 __attribute__((ext_vector_type(2)));

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

template <typename A>
__device__ __forceinline__ int arg_none();
template <>
__device__ __forceinline__ int arg_none<uint16_t>() { return 0xFFFF; }
template <>
__device__ __forceinline__ int arg_none<int32_t>() { return -1; }

__device__ __forceinline__ int wave_id_uniform() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// ---- element types: float, or bf16 storage (uint16_t bits) computed in f32 ------------
__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
template <typename T>
__device__ __forceinline__ T from_f(float x);
template <>
__device__ __forceinline__ float from_f<float>(float x) { return x; }
template <>
__device__ __forceinline__ uint16_t from_f<uint16_t>(float x) {  // round to nearest even
  return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x));
}

// ---- per-lane feature tile access ----------------------------------------------------
template <int W, typename T = float>
__device__ __forceinline__ void load_tile(const T* __restrict__ row, int f, int F,
                                          float (&r)[W], float fill) {
  if constexpr (W == 4) {
    if (f < F) {
      if constexpr (sizeof(T) == 4) {
        const float4 t = *reinterpret_cast<const float4*>(row + f);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
      } else {
        const uint2 t = *reinterpret_cast<const uint2*>(row + f);
        r[0] = to_f((uint16_t)(t.x & 0xFFFF)); r[1] = to_f((uint16_t)(t.x >> 16));
        r[2] = to_f((uint16_t)(t.y & 0xFFFF)); r[3] = to_f((uint16_t)(t.y >> 16));
      }
    } else {
      r[0] = r[1] = r[2] = r[3] = fill;
    }
  } else {
    r[0] = f < F ? to_f(row[f]) : fill;
  }
}

template <int W, typename T = float>
__device__ __forceinline__ void store_tile(T* __restrict__ row, int f, int F,
                                           const float (&r)[W]) {
  if constexpr (W == 4) {
    if (f < F) {
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(row + f) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
        uint2 t;
        t.x = (uint32_t)from_f<uint16_t>(r[0]) | ((uint32_t)from_f<uint16_t>(r[1]) << 16);
        t.y = (uint32_t)from_f<uint16_t>(r[2]) | ((uint32_t)from_f<uint16_t>(r[3]) << 16);
        *reinterpret_cast<uint2*>(row + f) = t;
      }
    }
  } else {
    if (f < F) row[f] = from_f<T>(r[0]);
  }
}

template <int W, typename A>
__device__ __forceinline__ void load_arg(const A* __restrict__ row, int f, int F, int (&r)[W]) {
  if constexpr (W == 4) {
    if (f < F) {
      if constexpr (sizeof(A) == 2) {
        const uint2 t = *reinterpret_cast<const uint2*>(row + f);
        r[0] = t.x & 0xFFFF; r[1] = t.x >> 16; r[2] = t.y & 0xFFFF; r[3] = t.y >> 16;
      } else {
        const int4 t = *reinterpret_cast<const int4*>(row + f);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
      }
    } else {
      r[0] = r[1] = r[2] = r[3] = arg_none<A>();
    }
  } else {
    r[0] = f < F ? (int)row[f] : arg_none<A>();
  }
}

template <int W, typename A>
__device__ __forceinline__ void store_arg(A* __restrict__ row, int f, int F, const int (&r)[W]) {
  if constexpr (W == 4) {
    if (f < F) {
      if constexpr (sizeof(A) == 2) {
        uint2 t;
        t.x = (uint32_t)(r[0] & 0xFFFF) | ((uint32_t)r[1] << 16);
        t.y = (uint32_t)(r[2] & 0xFFFF) | ((uint32_t)r[3] << 16);
        *reinterpret_cast<uint2*>(row + f) = t;
      } else {
        *reinterpret_cast<int4*>(row + f) = make_int4(r[0], r[1], r[2], r[3]);
      }
    }
  } else {
    if (f < F) row[f] = (A)r[0];
  }
}

// ---- edge windows ---------------------------------------------------------------------
// A wave walks its item's entries in windows of 64: one coalesced vector load brings 64
// column ids (and per-entry scalars) into a VGPR, and each edge's id is broadcast with
// v_readlane (a uniform lane select), so no per-edge scalar-load round trip sits in front
// of the row loads. Inside a window, U edges are in flight at once: all their row loads
// are issued before any is consumed. The last batch of a window is padded by repeating
// its last valid edge for the loads; its compute is skipped by a uniform branch.
__device__ __forceinline__ int bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float bcastf(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

#ifndef PG_EDGE_U
#define PG_EDGE_U 8  // edges in flight per wave for feature tiles of <= 8 values per lane
#endif
template <int W, int NC>
struct EdgeU {
  static constexpr int value = (NC * W <= 8) ? PG_EDGE_U : 4;
};

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum partial slots in order; optional relu' mask (bwd) or 1/deg (mean fwd).
// One workgroup per split row, one thread per feature.
template <typename T = float>
__global__ __launch_bounds__(kBlock) void sum_merge_kernel(
    const int4* __restrict__ merges, int n_merges, int F, const float* __restrict__ ws,
    int64_t ldw, const int32_t* __restrict__ ptr, int divide_by_deg,
    const T* __restrict__ mask, int64_t ldm, T* __restrict__ out, int64_t ldo) {
  const int4 m = merges[blockIdx.x];
  const int row = m.x, s0 = m.y, ns = m.z;
  const float deg = divide_by_deg ? (float)(ptr[row + 1] - ptr[row]) : 1.f;
  // 4 features per thread (float4 slot loads) when every row is 4-aligned: the same
  // per-feature order, bitwise the same result
  constexpr uintptr_t kTa = 4 * sizeof(T) - 1;
  const bool vec = (F % 4) == 0 && (ldw % 4) == 0 && (ldo % 4) == 0 && ((uintptr_t)ws & 15) == 0 &&
                   ((uintptr_t)out & kTa) == 0 && (!mask || ((ldm % 4) == 0 && ((uintptr_t)mask & kTa) == 0));
  if (vec) {
    for (int f = threadIdx.x * 4; f < F; f += kBlock * 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int s = s0; s < s0 + ns; s += 8) {
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          v[e] = *reinterpret_cast<const float4*>(ws + (int64_t)min(s + e, s0 + ns - 1) * ldw + f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (s + e < s0 + ns) {
            acc[0] += v[e].x; acc[1] += v[e].y; acc[2] += v[e].z; acc[3] += v[e].w;
          }
      }
      if (divide_by_deg)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = acc[i] / deg;
      if (mask) {
        float mk[4];
        load_tile<4, T>(mask + (int64_t)row * ldm, f, F, mk, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!(mk[i] > 0.f)) acc[i] = 0.f;
      }
      store_tile<4, T>(out + (int64_t)row * ldo, f, F, acc);
    }
    return;
  }
  for (int f = threadIdx.x; f < F; f += kBlock) {
    float acc = 0.f;
    for (int s = s0; s < s0 + ns; s += 8) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ws[(int64_t)min(s + e, s0 + ns - 1) * ldw + f];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (s + e < s0 + ns) acc += v[e];
    }
    if (divide_by_deg) acc = acc / deg;
    if (mask && !(to_f(mask[(int64_t)row * ldm + f]) > 0.f)) acc = 0.f;
    out[(int64_t)row * ldo + f] = from_f<T>(acc);
  }
}

// zero / constant fills by kernels of this library (ticket words, descriptor arrays, dx)
__global__ __launch_bounds__(kBlock) void clear_u4_kernel(uint4* __restrict__ x, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock)
    x[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kBlock) void fill2d_kernel(float* __restrict__ x, int64_t ldx,
                                                        int64_t rows, int cols, float val) {
  const int64_t n = rows * (int64_t)cols;
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    x[r * ldx + c] = val;
  }
}

constexpr int kGTile = 256;  // feature columns per wave (g-SpMM / g-SDDMM, GATv2 backward)

// ---- host-side dispatch helpers --------------------------------------------------------
inline int grid_for(int64_t n_work) {
  return (int)((n_work + kWavesPerBlock - 1) / kWavesPerBlock);
}

inline int hip_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pg::set_error((int)e, "%s: launch failed: %s", who, hipGetErrorString(e));
  return pg::ok();
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// workspace layout: [values: n_slots x ldw floats][args: n_slots x ldw A], 256-B aligned
inline int64_t ws_ld(int64_t F) { return round_up(F, 4); }

// Feature tiles per launch: a kernel is instantiated for NC = 1 ... MAXNC chunks of 64 * W
// columns; wider F is processed in tiles by offsetting the feature pointers.
constexpr int kMaxNCScalar = 16;                    // scalar path: F <= 16 * 64 per launch
constexpr int kFTileVec = 4 * kWave * 4;            // 1024: the widest vector tile (4 chunks of 256)
constexpr int kFTileScalar = kMaxNCScalar * kWave;  // 1024

// fn(integral_constant<int, nc>) for 1 <= nc <= MAXNC
template <int MAXNC, int NC = 1, typename Fn>
int dispatch_nc(int nc, Fn&& fn) {
  if (nc == NC) return fn(std::integral_constant<int, NC>{});
  if constexpr (NC < MAXNC) return dispatch_nc<MAXNC, NC + 1>(nc, fn);
  else return PG_ERR_UNSUPPORTED;
}

template <typename T>
struct TypeTag {
  using type = T;
};

struct TilePlan {
  bool vec;
  int64_t tile;
};

// Feature columns per launch on the vector path (a multiple of 256 up to 1024; variant
// builds: -DPG_SPMM_FTILE=...): narrower tiles mean fewer registers per wave (higher
// occupancy) at the price of re-reading the column ids once per tile. 256 measured best.
#ifndef PG_SPMM_FTILE
#define PG_SPMM_FTILE 256
#endif
static_assert(PG_SPMM_FTILE >= 256 && PG_SPMM_FTILE <= kFTileVec && PG_SPMM_FTILE % 256 == 0, "feature tile");
constexpr int64_t vec_ftile() { return PG_SPMM_FTILE; }

inline TilePlan plan_tiles(int64_t F, std::initializer_list<int64_t> lds,
                           std::initializer_list<const void*> ptrs) {
  bool vec = (F % 4) == 0;
  for (int64_t l : lds) vec = vec && (l % 4) == 0;
  for (const void* p : ptrs) vec = vec && (p == nullptr || aligned16(p));
  return {vec, vec ? vec_ftile() : (int64_t)kFTileScalar};
}

// The kernel shape for a feature tile of Ft columns under the plan: fn(NC, W) as
// integral_constants. Vector path: W = 4, NC chunks of 256 columns, at most the vector tile's
// (one in the product build; a build with a wider PG_SPMM_FTILE instantiates its own).
// Scalar path: W = 1, NC chunks of 64 columns.
template <typename Fn>
int dispatch_tile(const TilePlan& tp, int Ft, Fn&& fn) {
  if (tp.vec)
    return dispatch_nc<PG_SPMM_FTILE / 256>((Ft + 255) / 256,
                                            [&](auto nc) { return fn(nc, std::integral_constant<int, 4>{}); });
  return dispatch_nc<kMaxNCScalar>((Ft + 63) / 64, [&](auto nc) { return fn(nc, std::integral_constant<int, 1>{}); });
}

// ... and fn(NC, W, HAS_W) for the kernels with an edge-weight form
template <typename Fn>
int dispatch_tile(const TilePlan& tp, int Ft, bool has_w, Fn&& fn) {
  return dispatch_tile(tp, Ft, [&](auto nc, auto w) {
    return has_w ? fn(nc, w, std::true_type{}) : fn(nc, w, std::false_type{});
  });
}

inline int check_ws(size_t have, size_t need, const char* who) {
  if (have < need)
    return pg::set_error(PG_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", who, have, need);
  return PG_OK;
}

}  // namespace
