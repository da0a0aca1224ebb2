// Sum / mean / weighted CSR SpMM and the SDDMM dot products (the edge-weight gradient of
// u_mul_e; u_dot_v). Work decomposition and numerics: spmm_common.hpp.
#include "spmm_common.hpp"

namespace {

// ---- sum / mean / weighted SpMM ------------------------------------------------------
template <int W, int NC, bool HAS_W, int NORM>
__global__ __launch_bounds__(kBlock) void sum_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ eslot, const float* __restrict__ ew,
    const int32_t* __restrict__ norm_ptr, const int4* __restrict__ items, int n_items,
    const float* __restrict__ X, int64_t ldx, int F, float* __restrict__ out, int64_t ldo,
    float* __restrict__ ws, int64_t ldw) {
  constexpr int U = EdgeU<W, NC>::value;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z, slot = item.w;
  const int lane = lane_id();
  float acc[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < W; ++i) acc[c][i] = 0.f;

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int kl = kw + min(lane, nw - 1);
    const int idxv = col[kl];
    float wv = 1.f, dv = 1.f;
    if constexpr (HAS_W) wv = ew[eslot ? eslot[kl] : kl];
    if constexpr (NORM == 2) dv = (float)(norm_ptr[idxv + 1] - norm_ptr[idxv]);
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float v[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const float* xr = X + (int64_t)bcast(idxv, j + min(e, nv - 1)) * ldx;
#pragma unroll
        for (int c = 0; c < NC; ++c) load_tile<W>(xr, (c * kWave + lane) * W, F, v[e][c], 0.f);
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
          float w = 1.f, dc = 1.f;
          if constexpr (HAS_W) w = bcastf(wv, j + e);
          if constexpr (NORM == 2) dc = bcastf(dv, j + e);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i) {
              float tv = HAS_W ? v[e][c][i] * w : v[e][c][i];
              if constexpr (NORM == 2) tv = tv / dc;
              acc[c][i] += tv;
            }
        }
      }
    }
  }
  if (slot < 0) {
    if constexpr (NORM == 1) {
      const int d = ptr[row + 1] - ptr[row];
      if (d > 0) {
        const float fd = (float)d;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < W; ++i) acc[c][i] = acc[c][i] / fd;
      }
    }
    float* orow = out + (int64_t)row * ldo;
#pragma unroll
    for (int c = 0; c < NC; ++c) store_tile<W>(orow, (c * kWave + lane) * W, F, acc[c]);
  } else {
    float* wr = ws + (int64_t)slot * ldw;
#pragma unroll
    for (int c = 0; c < NC; ++c) store_tile<W>(wr, (c * kWave + lane) * W, F, acc[c]);
  }
}

// ---- SDDMM: per-edge dot products (the edge-weight gradient of u_mul_e; u_dot_v) --------
// One wave per schedule item, the same items as sum_kernel: every slot lies in exactly one
// item, so split rows need no merge. The item's D row tile (and, in the max form, its record
// tile) sits in registers; X rows are gathered U at a time and each lane forms U partial
// sums over its W features. A transposing butterfly then reduces them across the wave:
// log2(U) steps in which a lane keeps half of its values and hands the other half to its
// partner (U - 1 shuffles), after which lane l holds edge (l & (U - 1)) summed over U lanes,
// and 6 - log2(U) plain steps over the remaining lane bits: U + 2 shuffles per U edges
// instead of 6 U. The results of a 64-edge window collect in one register (lane j = edge j
// of the window) over every feature tile, tile after tile in a fixed order, and leave in one
// coalesced store. Max form: an edge no lane's records name skips its X row (wave-uniform).
template <int W, bool MAX, typename A, int NORM>
__global__ __launch_bounds__(kBlock) void sddmm_dot_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const int4* __restrict__ items, int n_items, const float* __restrict__ D, int64_t ldd,
    const float* __restrict__ X, int64_t ldx, int F, const A* __restrict__ arg, int64_t lda,
    float* __restrict__ de) {
  constexpr int U = 8;
  constexpr int T = kWave * W;  // feature columns per tile
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  const int lane = lane_id();
  const int rs = ptr[row];
  const float* drow = D + (int64_t)row * ldd;
  const A* arow = MAX ? arg + (int64_t)row * lda : nullptr;
  const bool one_tile = F <= T;  // the usual case: the row tiles are loaded once per item
  float d[W];
  int a[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { d[i] = 0.f; a[i] = arg_none<A>(); }
  if (one_tile) {
    load_tile<W>(drow, lane * W, F, d, 0.f);
    if constexpr (MAX) load_arg<W, A>(arow, lane * W, F, a);
  }
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int idxv = col[kw + min(lane, nw - 1)];
    float accw = 0.f;  // lane j: edge kw + j
    for (int f0 = 0; f0 < F; f0 += T) {
      const int f = f0 + lane * W;
      if (!one_tile) {
        load_tile<W>(drow, f, F, d, 0.f);
        if constexpr (MAX) load_arg<W, A>(arow, f, F, a);
      }
      for (int j = 0; j < nw; j += U) {
        const int nv = min(U, nw - j);
        float v[U][W];
#pragma unroll
        for (int e = 0; e < U; ++e) {  // a short last batch repeats its last edge (lanes >= nw: not stored)
          const int je = j + min(e, nv - 1);
          bool live = true;
          if constexpr (MAX) {
            const int pos = kw + je - rs;
            bool m = false;
#pragma unroll
            for (int i = 0; i < W; ++i) m = m || a[i] == pos;
            live = __any(m);
          }
          if (live) {
            load_tile<W>(X + (int64_t)bcast(idxv, je) * ldx, f, F, v[e], 0.f);
          } else {
#pragma unroll
            for (int i = 0; i < W; ++i) v[e][i] = 0.f;
          }
        }
        float p[U];
#pragma unroll
        for (int e = 0; e < U; ++e) {
          const int pos = kw + j + min(e, nv - 1) - rs;
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < W; ++i) {
            const float t = d[i] * v[e][i];
            s += (!MAX || a[i] == pos) ? t : 0.f;
          }
          p[e] = s;
        }
        // transpose-reduce: 8 -> 4 -> 2 -> 1 values per lane; lane l ends with edge l & 7
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float keep = b0 ? p[2 * i + 1] : p[2 * i], send = b0 ? p[2 * i] : p[2 * i + 1];
          p[i] = keep + __shfl_xor(send, 1);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float keep = b1 ? p[2 * i + 1] : p[2 * i], send = b1 ? p[2 * i] : p[2 * i + 1];
          p[i] = keep + __shfl_xor(send, 2);
        }
        {
          const float keep = b2 ? p[1] : p[0], send = b2 ? p[0] : p[1];
          p[0] = keep + __shfl_xor(send, 4);
        }
        p[0] += __shfl_xor(p[0], 8);
        p[0] += __shfl_xor(p[0], 16);
        p[0] += __shfl_xor(p[0], 32);
        if ((lane >> 3) == (j >> 3)) accw += p[0];
      }
    }
    if constexpr (NORM == 1) accw = accw / (float)(ptr[row + 1] - rs);
    if (lane < nw) de[kw + lane] = accw;
  }
}

}  // namespace

extern "C" {

size_t pg_spmm_sum_workspace(const pg_csr_t* g, int64_t F) {
  if (!g || g->n_slots <= 0 || F <= 0) return 0;
  return round_up(g->n_slots * ws_ld(F) * 4, 256);
}

int pg_spmm_sum(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, int norm_mode,
                const int32_t* norm_ptr, float* out, int64_t ldo, void* ws, size_t ws_bytes,
                pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_spmm_sum", true));
  if (F < 0 || ldx < F || ldo < F)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum: bad F/leading dims");
  if (norm_mode < 0 || norm_mode > 2 || (norm_mode == 2 && !norm_ptr))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum: bad norm_mode %d", norm_mode);
  if (F == 0 || g->n_rows == 0) return pg::ok();
  if (!X || !out) return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum: NULL buffer");
  const size_t need = pg_spmm_sum_workspace(g, F);
  PG_TRY(check_ws(ws_bytes, need, "pg_spmm_sum"));
  float* w = need ? (float*)ws : nullptr;
  const int64_t ldw = ws_ld(F);
  hipStream_t st = (hipStream_t)stream;
  TilePlan tp = plan_tiles(F, {ldx, ldo}, {X, out, w});
  const bool has_w = g->ew != nullptr;
  const int blocks = grid_for(g->n_items);
  for (int64_t f0 = 0; f0 < F; f0 += tp.tile) {
    const int Ft = (int)std::min<int64_t>(tp.tile, F - f0);
    auto go = [&](auto nc_c, auto w_c, auto hw_c, auto norm_c) -> int {
      constexpr int NC = decltype(nc_c)::value;
      constexpr int W = decltype(w_c)::value;
      constexpr bool HW = decltype(hw_c)::value;
      constexpr int NORM = decltype(norm_c)::value;
      hipLaunchKernelGGL((sum_kernel<W, NC, HW, NORM>), dim3(blocks), dim3(kBlock), 0, st, g->ptr,
                         g->col, g->eslot, g->ew, norm_ptr, (const int4*)g->items, (int)g->n_items,
                         X + f0, ldx, Ft, out + f0, ldo, w ? w + f0 : nullptr, ldw);
      return PG_OK;
    };
    auto by_norm = [&](auto nc_c, auto w_c, auto hw_c) -> int {
      switch (norm_mode) {
        case 0: return go(nc_c, w_c, hw_c, std::integral_constant<int, 0>{});
        case 1: return go(nc_c, w_c, hw_c, std::integral_constant<int, 1>{});
        default: return go(nc_c, w_c, hw_c, std::integral_constant<int, 2>{});
      }
    };
    const int rc = dispatch_tile(tp, Ft, has_w, by_norm);
    if (rc != PG_OK) return pg::set_error(rc, "pg_spmm_sum: unsupported feature tile");
    if (g->n_merges > 0)
      hipLaunchKernelGGL(sum_merge_kernel<float>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)g->n_merges, Ft, w + f0, ldw, g->ptr,
                         norm_mode == 1 ? 1 : 0, nullptr, 0, out + f0, ldo);
  }
  return hip_status("pg_spmm_sum");
}

int pg_sddmm_dot(const pg_csr_t* g, const float* D, int64_t ldd, const float* X, int64_t ldx,
                 int64_t F, int norm_mode, const void* argpos, int64_t lda, int arg_kind,
                 float* de, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_sddmm_dot", true));
  PG_TRY(pg::check_sddmm(g, "pg_sddmm_dot", ldd, ldx, F, norm_mode, argpos, lda, arg_kind));
  if (F > (1 << 30)) return pg::set_error(PG_ERR_UNSUPPORTED, "pg_sddmm_dot: F too large");
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!de || (F > 0 && (!D || !X))) return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot: NULL buffer");
  const TilePlan tp = plan_tiles(F, {ldd, ldx, argpos ? lda : 0}, {D, X, argpos});
  const int blocks = grid_for(g->n_items);
  hipStream_t st = (hipStream_t)stream;
  auto go = [&](auto w_c, auto max_c, auto a_c, auto norm_c) {
    constexpr int W = decltype(w_c)::value;
    constexpr bool MAX = decltype(max_c)::value;
    using A = typename decltype(a_c)::type;
    constexpr int NORM = decltype(norm_c)::value;
    hipLaunchKernelGGL((sddmm_dot_kernel<W, MAX, A, NORM>), dim3(blocks), dim3(kBlock), 0, st, g->ptr,
                       g->col, (const int4*)g->items, (int)g->n_items, D, ldd, X, ldx, (int)F,
                       (const A*)argpos, lda, de);
  };
  auto by_norm = [&](auto w_c, auto max_c, auto a_c) {
    if (norm_mode == 1) go(w_c, max_c, a_c, std::integral_constant<int, 1>{});
    else go(w_c, max_c, a_c, std::integral_constant<int, 0>{});
  };
  auto by_form = [&](auto w_c) {
    if (!argpos) by_norm(w_c, std::false_type{}, TypeTag<uint16_t>{});
    else if ((arg_kind & ~PG_ARG_DEAD_NONE) == PG_ARG_U16) by_norm(w_c, std::true_type{}, TypeTag<uint16_t>{});
    else by_norm(w_c, std::true_type{}, TypeTag<int32_t>{});
  };
  if (tp.vec) by_form(std::integral_constant<int, 4>{});
  else by_form(std::integral_constant<int, 1>{});
  return hip_status("pg_sddmm_dot");
}

}  // extern "C"
