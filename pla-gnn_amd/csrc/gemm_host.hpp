// Host front end shared by the GEMM families (gemm.hip, gemm_x3.hip, gemm_bf16.hip): the
// argument checks, the epilogue code, K slicing, the split-K combine launch, the dispatch
// helpers that turn runtime (tile, transposition, epilogue) values into template arguments,
// and the grouped launches' part check, slab layout and part / job fill. Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "gemm_common.hpp"

namespace pg_gemm {

inline constexpr pg_gemm_epilogue_t kNoEpilogue{nullptr, PG_ACT_NONE, 0.f, nullptr, 0, nullptr};

// ---- argument checks ---------------------------------------------------------------------
// What every product entry point checks before it looks at its operands' layout; `who`
// names the entry point in the message, `split_rule` states its split-K restriction
// (split_barred: a reason of the caller's own, such as a bf16 C). `type_error`, when not
// null, is the caller's finding about its storage types; it ranks after the sizes.
inline int check_product(const char* who, int transa, int transb, int64_t M, int64_t N, int64_t K, int64_t lda,
                         int64_t ldb, int64_t ldc, const pg_gemm_epilogue_t& ep, float beta, int split_k,
                         bool split_barred, const char* split_rule, const char* type_error = nullptr) {
  if (M < 0 || N < 0 || K < 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    return pg::set_error(PG_ERR_INVALID, "%s: bad sizes", who);
  if (type_error) return pg::set_error(PG_ERR_INVALID, "%s: %s", who, type_error);
  if (ldc < N || (!transa && lda < K) || (transa && lda < M) || (!transb && ldb < N) || (transb && ldb < K))
    return pg::set_error(PG_ERR_INVALID, "%s: leading dimension too small", who);
  if (ep.act != PG_ACT_NONE && ep.act != PG_ACT_RELU && ep.act != PG_ACT_LEAKY)
    return pg::set_error(PG_ERR_INVALID, "%s: bad act %d", who, ep.act);
  if (split_k > 1 &&
      (split_barred || ep.bias || ep.act != PG_ACT_NONE || ep.dact || (beta != 0.f && beta != 1.f)))
    return pg::set_error(PG_ERR_INVALID, "%s: split_k > 1 %s", who, split_rule);
  if (ep.dact && (ep.act == PG_ACT_NONE || ep.lddact < N))
    return pg::set_error(PG_ERR_INVALID, "%s: dact needs act relu|leaky and lddact >= N", who);
  return PG_OK;
}

inline int epi_code(const pg_gemm_epilogue_t& ep, bool split) {
  if (split) return EPI_SPLIT;
  if (ep.dact) return ep.act == PG_ACT_RELU ? EPI_DRELU : EPI_DLEAKY;
  return ep.act == PG_ACT_RELU ? EPI_RELU : ep.act == PG_ACT_LEAKY ? EPI_LEAKY : EPI_NONE;
}

// K slicing: slices of equal length, a multiple of the K step bk; returns the slice length
// and lowers split_k to the slices that are not empty.
inline int k_slices(int64_t K, int bk, int& split_k) {
  if (split_k <= 1) return (int)K;
  int kps = (int)((K + split_k - 1) / split_k);
  kps = (kps + bk - 1) / bk * bk;
  split_k = (int)((K + kps - 1) / kps);
  if (split_k < 1) split_k = 1;
  return kps;
}

inline void tile_grid(int64_t M, int64_t N, int bm, int bn, int& tiles_n, int& tiles) {
  tiles_n = (int)((N + bn - 1) / bn);
  tiles = tiles_n * (int)((M + bm - 1) / bm);
}

// ---- dispatch: runtime value -> template argument ------------------------------------------
// Each calls f with the matching compile-time constant(s) and returns f's code, or `miss`
// when the value is not in the list.
template <int... Vs, class F>
int dispatch_int(int v, F&& f, int miss = PG_ERR_INVALID) {
  int rc = miss;
  (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return rc;
}

template <class F>
int dispatch_epi(int epi, F&& f) {
  return dispatch_int<EPI_NONE, EPI_RELU, EPI_LEAKY, EPI_DRELU, EPI_DLEAKY, EPI_SPLIT>(epi, f);
}

template <class F>
int dispatch_flag(bool a, F&& f) {
  return a ? f(std::true_type{}) : f(std::false_type{});
}

// two flags: (transa, transb), or the loaders' (va, vb)
template <class F>
int dispatch_flags(bool a, bool b, F&& f) {
  if (!a && !b) return f(std::false_type{}, std::false_type{});
  if (!a && b) return f(std::false_type{}, std::true_type{});
  if (a && !b) return f(std::true_type{}, std::false_type{});
  return f(std::true_type{}, std::true_type{});
}

template <int BM, int BN>
struct Tile {
  static constexpr int bm = BM, bn = BN;
};

template <class... Ts, class F>
int dispatch_tile(int bm, int bn, F&& f, int miss = PG_ERR_INVALID) {
  int rc = miss;
  (void)(((bm == Ts::bm && bn == Ts::bn) ? (rc = f(Ts{}), true) : false) || ...);
  return rc;
}

// ---- split-K combine -----------------------------------------------------------------------
// Blocks of one combine: a work unit is 4 consecutive outputs (N % 4 == 0) or one, then one
// per row sum; 256 / G units per block, at most 8192 blocks (the kernel strides).
inline int combine_blocks(int64_t M, int64_t N, bool rowsum, int G) {
  const int64_t n = (N % 4 == 0 ? M * N / 4 : M * N) + (rowsum ? M : 0);
  const int opb = 256 / G;
  return (int)std::min<int64_t>(8192, (n + opb - 1) / opb);
}

// (a template, so that only a file that launches the combine instantiates its kernels)
template <class Stream>
void launch_combine(const float* ws, int split_k, int64_t M, int64_t N, float alpha, float beta, float* C,
                    int64_t ldc, const float* ws_rowsum, float* rowsum, Stream st) {
  const int G = splitk_groups(split_k);
  const int blocks = combine_blocks(M, N, rowsum != nullptr, G);
  dispatch_int<1, 4, 16>(G, [&](auto g) {
    hipLaunchKernelGGL(splitk_reduce_kernel<decltype(g)::value>, dim3(blocks), dim3(256), 0, st, ws, split_k, (int)M,
                       (int)N, alpha, beta, C, ldc, ws_rowsum, rowsum);
    return PG_OK;
  });
}

// ---- the three-piece kernel's tile rule (gemm.hip picks, gemm_x3.hip builds) ---------------
#ifndef PG_X3_TILE_FORCE
#define PG_X3_TILE_FORCE 0  // variant builds: BM * 1000 + BN forces one tile
#endif
// A variant build that forces a tile passes the flag to BOTH files (VSRC="gemm gemm_x3"):
// gemm.hip picks the tile and gemm_x3.hip builds it. With the flag on gemm.hip alone the
// library links, but a product whose forced tile the other file did not build fails with
// "dispatch failed" (cat / rows: PG_ERR_UNSUPPORTED). Both functions have internal linkage,
// so the two files may hold different bodies.
// Measured per cfg2 shape with each tile forced, within 1-3 % of the best everywhere:
// 128 x 128 (4 waves of 64 x 64: 0.5 fragment reads per MFMA) wherever that gives >= 2
// workgroups per CU; else 128 x 64, else 64 x 64. (Round 6: a long-K product with 256-511
// 128 x 128 tiles, cfg2's fwd.cat.l1, runs 87.2 instead of 91.0 us on 128 x 64 tiles: 752
// tiles share out over 256 CUs, 376 leave 136 CUs one tile idle.) Split products: 128 x 128,
// ~2 workgroups per CU (512: 1.636 ms/step, 768: 1.667, 1024: 1.721).
static inline void pick_tile_x3(int64_t M, int64_t N, int64_t K, int split, int& bm, int& bn) {
  (void)K;
  if constexpr (PG_X3_TILE_FORCE != 0) {  // variant builds only
    bm = PG_X3_TILE_FORCE / 1000;
    bn = PG_X3_TILE_FORCE % 1000;
    return;
  }
  auto tiles = [&](int tm, int tn) { return ((M + tm - 1) / tm) * ((N + tn - 1) / tn); };
  if (split > 1) {
    bm = M > 64 ? 128 : 64;
    bn = N > 64 ? 128 : 64;
    return;
  }
  bm = bn = 64;
  if (tiles(128, 128) >= 512) bm = bn = 128;
  else if (tiles(128, 64) >= 512) bm = 128;
}
// the tiles pick_tile_x3 can return: split products all four, others never 64 x 128
template <int BM, int BN>
static constexpr bool x3_tile_built(bool split) {
  if (PG_X3_TILE_FORCE != 0) return BM * 1000 + BN == PG_X3_TILE_FORCE;
  return split || !(BM == 64 && BN == 128);
}

// ---- grouped split-K launches ----------------------------------------------------------------
inline bool part_ok(const pg_gemm_part_t& q) {
  const bool bufs = (q.M == 0 || q.N == 0 || q.C) && (q.M == 0 || q.N == 0 || q.K == 0 || (q.A && q.B));
  return bufs && q.M >= 0 && q.N >= 0 && q.K >= 0 && q.M <= INT32_MAX && q.N <= INT32_MAX && q.K <= INT32_MAX &&
         q.ldc >= q.N && (q.transa ? q.lda >= q.M : q.lda >= q.K) && (q.transb ? q.ldb >= q.K : q.ldb >= q.N) &&
         (q.beta == 0.f || q.beta == 1.f);
}

// A group's plan. The family's policy fills in[] (the part runs in the grouped launch) and
// split[] (the K slices it wants for it); group_layout then settles, per member, the slice
// length (a multiple of bk), the slices that are not empty, and the offset of its slabs
// ([split][M][N], then the [split][M] row-sum slices) in the workspace, 256-B aligned.
struct GroupPlan {
  bool in[kMaxParts];
  int split[kMaxParts];
  int kps[kMaxParts];
  size_t off[kMaxParts + 1];
};

inline void group_layout(const pg_gemm_part_t* parts, int n, int bk, GroupPlan& g) {
  size_t off = 0;
  for (int p = 0; p < n; ++p) {
    const pg_gemm_part_t& q = parts[p];
    g.off[p] = off;
    if (!g.in[p]) {
      g.split[p] = 1;
      g.kps[p] = bk;
      continue;
    }
    int64_t sp = g.split[p];
    int64_t kps = (q.K + sp - 1) / sp;
    kps = std::max<int64_t>(bk, (kps + bk - 1) / bk * bk);
    sp = std::max<int64_t>(1, (q.K + kps - 1) / kps);
    g.split[p] = (int)sp;
    g.kps[p] = (int)kps;
    off += ((size_t)sp * (size_t)std::max<int64_t>(q.M, 0) * (size_t)(std::max<int64_t>(q.N, 0) + 1) * 4 + 255) /
           256 * 256;
  }
  g.off[n] = off;
}

// The members with outputs as the kernel's parts (items = tiles x slices, laid end to end)
// and as the combine's jobs; returns how many.
template <class T>
int group_fill(const pg_gemm_part_t* parts, int n, const GroupPlan& g, int bm, int bn, void* ws, GemmGroup<T>& grp,
               pg_splitk_job_t* jobs) {
  int items = 0, nj = 0;
  for (int p = 0; p < n; ++p) {
    const pg_gemm_part_t& q = parts[p];
    if (!g.in[p] || q.M == 0 || q.N == 0) continue;
    float* w = (float*)((char*)ws + g.off[p]);
    GemmPart<T>& x = grp.p[nj];
    x.M = (int)q.M; x.N = (int)q.N; x.K = (int)q.K; x.kps = g.kps[p];
    tile_grid(q.M, q.N, bm, bn, x.tiles_n, x.tiles);
    x.first_item = items;
    x.A = (const T*)q.A; x.lda = q.lda; x.B = (const T*)q.B; x.ldb = q.ldb;
    x.ws = w;
    x.ws_rowsum = w + (int64_t)g.split[p] * q.M * q.N;
    x.rowsum = q.rowsum;
    items += x.tiles * g.split[p];
    pg_splitk_job_t& j = jobs[nj];
    j.ws = w; j.split_k = g.split[p]; j.M = q.M; j.N = q.N;
    j.alpha = 1.f; j.beta = q.beta; j.C = q.C; j.ldc = q.ldc; j.rowsum = q.rowsum;
    ++nj;
  }
  grp.n = nj;
  grp.items = items;
  return nj;
}

}  // namespace pg_gemm
