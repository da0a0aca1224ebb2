// ---- g-SpMM / g-SDDMM: messages with vector edge features --------------------------------
// z = op(L[t_l(k)], R[t_r(k)]) per entry k, an operand row being the gathered node row
// col[k], the row that owns k (g-SDDMM) or the edge row e(k) = emap[k] (k without a map).
// One wave per schedule item, as sum_kernel; 256 feature columns per wave (one float4 per
// lane on the vector path, four floats 64 apart on the scalar path), wider F in feature
// tiles along gridDim.y. The item's col / emap values come 64 at a time and are broadcast;
// U entries are in flight per wave: all their operand rows are loaded before any is used
// (U = 4 with two operands, 8 with one: eight 16-byte loads per lane either way).
// Shared tile access, merge kernel and host helpers: spmm_common.hpp.
#include "spmm_common.hpp"

namespace {

template <int OP>
__device__ __forceinline__ float gop(float l, float r) {
  if constexpr (OP == PG_OP_ADD) return l + r;
  else if constexpr (OP == PG_OP_SUB) return l - r;
  else if constexpr (OP == PG_OP_MUL) return l * r;
  else if constexpr (OP == PG_OP_DIV) return l / r;
  else if constexpr (OP == PG_OP_COPY_LHS) return l;
  else return r;
}

template <int RED>
__device__ __forceinline__ bool gbetter(float m, float best) {
  if constexpr (RED == PG_RED_MIN) return m < best;
  else return m > best;
}

// records: int, -1 = none, stored as u16 (0xFFFF = none) or i32
template <int W>
__device__ __forceinline__ void gstore_arg(void* row, int a16, int f, int F, const int (&r)[W]) {
  if (a16) store_arg<W, uint16_t>((uint16_t*)row, f, F, r);
  else store_arg<W, int32_t>((int32_t*)row, f, F, r);
}
template <int W>
__device__ __forceinline__ void gload_arg(const void* row, int a16, int f, int F, int (&r)[W]) {
  if (a16) load_arg<W, uint16_t>((const uint16_t*)row, f, F, r);
  else load_arg<W, int32_t>((const int32_t*)row, f, F, r);
}

template <int W, int OP, int RED>
__global__ __launch_bounds__(kBlock) void gspmm_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const int32_t* __restrict__ emap,
    const int4* __restrict__ items, int n_items, const float* __restrict__ L, int64_t ldl, int lt_e,
    const float* __restrict__ R, int64_t ldr, int rt_e, int F, int norm, float* __restrict__ out,
    int64_t ldo, void* __restrict__ arg, int64_t lda, int a16, float* __restrict__ ws_val,
    int32_t* __restrict__ ws_arg, int64_t ldw) {
  constexpr int NC = W == 4 ? 1 : 4;
  constexpr bool UL = OP != PG_OP_COPY_RHS, UR = OP != PG_OP_COPY_LHS;
  constexpr int U = (UL && UR) ? 4 : 8;
  constexpr bool SUM = RED == PG_RED_SUM;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z, slot = item.w;
  const int lane = lane_id();
  const int f0 = (int)blockIdx.y * kGTile;
  const int Ft = min(kGTile, F - f0);
  const int rs = ptr[row];
  if (UL) L += f0;
  if (UR) R += f0;
  const float init = SUM ? 0.f
                         : (RED == PG_RED_MIN ? std::numeric_limits<float>::infinity()
                                              : -std::numeric_limits<float>::infinity());
  float acc[NC][W];
  int bp[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < W; ++i) { acc[c][i] = init; bp[c][i] = -1; }

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int kl = kw + min(lane, nw - 1);
    const int cv = col[kl];
    const int ev = emap ? emap[kl] : kl;
    const int lv = lt_e ? ev : cv, rv = rt_e ? ev : cv;
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float a[U][NC][W], b[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const int je = j + min(e, nv - 1);
        if constexpr (UL) {
          const float* lr = L + (int64_t)bcast(lv, je) * ldl;
#pragma unroll
          for (int c = 0; c < NC; ++c) load_tile<W>(lr, (c * kWave + lane) * W, Ft, a[e][c], 0.f);
        }
        if constexpr (UR) {
          const float* rr = R + (int64_t)bcast(rv, je) * ldr;
#pragma unroll
          for (int c = 0; c < NC; ++c) load_tile<W>(rr, (c * kWave + lane) * W, Ft, b[e][c], 0.f);
        }
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
          const int pos = kw + j + e - rs;
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i) {
              const float m = gop<OP>(UL ? a[e][c][i] : 0.f, UR ? b[e][c][i] : 0.f);
              if constexpr (SUM) {
                acc[c][i] += m;
              } else if (gbetter<RED>(m, acc[c][i])) {
                acc[c][i] = m;
                bp[c][i] = pos;
              }
            }
        }
      }
    }
  }
  if (slot < 0) {
    if constexpr (SUM) {
      const int d = ptr[row + 1] - rs;
      if (norm == 1 && d > 0) {
        const float fd = (float)d;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < W; ++i) acc[c][i] = acc[c][i] / fd;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (__builtin_isinf(acc[c][i])) acc[c][i] = 0.f;
    }
    float* orow = out + (int64_t)row * ldo + f0;
#pragma unroll
    for (int c = 0; c < NC; ++c) store_tile<W>(orow, (c * kWave + lane) * W, Ft, acc[c]);
    if constexpr (!SUM) {
      if (arg) {
        void* arow = (char*)arg + ((int64_t)row * lda + f0) * (a16 ? 2 : 4);
#pragma unroll
        for (int c = 0; c < NC; ++c) gstore_arg<W>(arow, a16, (c * kWave + lane) * W, Ft, bp[c]);
      }
    }
  } else {
    float* wr = ws_val + (int64_t)slot * ldw + f0;
#pragma unroll
    for (int c = 0; c < NC; ++c) store_tile<W>(wr, (c * kWave + lane) * W, Ft, acc[c]);
    if constexpr (!SUM) {
      int32_t* war = ws_arg + (int64_t)slot * ldw + f0;
#pragma unroll
      for (int c = 0; c < NC; ++c) store_arg<W, int32_t>(war, (c * kWave + lane) * W, Ft, bp[c]);
    }
  }
}

// The pieces of a split row in slot order, strict compare: the earliest extremal entry wins
// (max_merge_kernel's rule, for max and min, i32 slot records). One workgroup per split row.
template <int RED>
__global__ __launch_bounds__(kBlock) void gcmp_merge_kernel(
    const int4* __restrict__ merges, int F, const float* __restrict__ ws_val,
    const int32_t* __restrict__ ws_arg, int64_t ldw, float* __restrict__ out, int64_t ldo,
    void* __restrict__ arg, int64_t lda, int a16) {
  const int4 m = merges[blockIdx.x];
  const int row = m.x, s0 = m.y, ns = m.z;
  for (int f = threadIdx.x; f < F; f += kBlock) {
    float best = RED == PG_RED_MIN ? std::numeric_limits<float>::infinity()
                                   : -std::numeric_limits<float>::infinity();
    int bp = -1;
    for (int s = s0; s < s0 + ns; s += 8) {
      float v[8];
      int a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t o = (int64_t)min(s + e, s0 + ns - 1) * ldw + f;
        v[e] = ws_val[o];
        a[e] = ws_arg[o];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (s + e < s0 + ns && gbetter<RED>(v[e], best)) {
          best = v[e];
          bp = a[e];
        }
    }
    if (__builtin_isinf(best)) best = 0.f;
    out[(int64_t)row * ldo + f] = best;
    if (arg) {
      if (a16) ((uint16_t*)arg)[(int64_t)row * lda + f] = (uint16_t)bp;
      else ((int32_t*)arg)[(int64_t)row * lda + f] = bp;
    }
  }
}

// g-SDDMM: one output row per entry, written at e(k). An operand at V (the item's own row)
// is loaded once per item; MASK: the records of the row, loaded once per item, select the
// features whose winner is this entry, and an entry no lane's records name loads nothing.
template <int W, int OP, bool MASK>
__global__ __launch_bounds__(kBlock) void gsddmm_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const int32_t* __restrict__ emap,
    const int4* __restrict__ items, int n_items, const float* __restrict__ L, int64_t ldl, int lt,
    const float* __restrict__ R, int64_t ldr, int rt, int F, float* __restrict__ out, int64_t ldo,
    const void* __restrict__ arg, int64_t lda, int a16) {
  constexpr int NC = W == 4 ? 1 : 4;
  constexpr bool UL = OP != PG_OP_COPY_RHS, UR = OP != PG_OP_COPY_LHS;
  constexpr int U = 4;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  if (k0 >= k1) return;
  const int lane = lane_id();
  const int f0 = (int)blockIdx.y * kGTile;
  const int Ft = min(kGTile, F - f0);
  const int rs = ptr[row];
  if (UL) L += f0;
  if (UR) R += f0;
  out += f0;
  const bool l_own = UL && lt == PG_TGT_V, r_own = UR && rt == PG_TGT_V;
  float lo[NC][W], ro[NC][W];
  int rec[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * kWave + lane) * W;
#pragma unroll
    for (int i = 0; i < W; ++i) { lo[c][i] = 0.f; ro[c][i] = 0.f; rec[c][i] = -1; }
    if (l_own) load_tile<W>(L + (int64_t)row * ldl, f, Ft, lo[c], 0.f);
    if (r_own) load_tile<W>(R + (int64_t)row * ldr, f, Ft, ro[c], 0.f);
    if constexpr (MASK)
      gload_arg<W>((const char*)arg + ((int64_t)row * lda + f0) * (a16 ? 2 : 4), a16, f, Ft, rec[c]);
  }

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int kl = kw + min(lane, nw - 1);
    const int cv = col[kl];
    const int ev = emap ? emap[kl] : kl;
    const int lv = lt == PG_TGT_E ? ev : cv, rv = rt == PG_TGT_E ? ev : cv;
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float a[U][NC][W], b[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const int je = j + min(e, nv - 1);
        bool live = true;
        if constexpr (MASK) {
          const int pos = kw + je - rs;
          bool hit = false;
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i) hit = hit || rec[c][i] == pos;
          live = __any(hit);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int f = (c * kWave + lane) * W;
#pragma unroll
          for (int i = 0; i < W; ++i) { a[e][c][i] = lo[c][i]; b[e][c][i] = ro[c][i]; }
          if (live) {
            if (UL && !l_own) load_tile<W>(L + (int64_t)bcast(lv, je) * ldl, f, Ft, a[e][c], 0.f);
            if (UR && !r_own) load_tile<W>(R + (int64_t)bcast(rv, je) * ldr, f, Ft, b[e][c], 0.f);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
          const int pos = kw + j + e - rs;
          float* orow = out + (int64_t)bcast(ev, j + e) * ldo;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            float z[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
              const float m = gop<OP>(a[e][c][i], b[e][c][i]);
              z[i] = (!MASK || rec[c][i] == pos) ? m : 0.f;
            }
            store_tile<W>(orow, (c * kWave + lane) * W, Ft, z);
          }
        }
      }
    }
  }
}

template <typename Fn>
int dispatch_gop(int op, Fn&& fn) {
  switch (op) {
    case PG_OP_ADD: return fn(std::integral_constant<int, PG_OP_ADD>{});
    case PG_OP_SUB: return fn(std::integral_constant<int, PG_OP_SUB>{});
    case PG_OP_MUL: return fn(std::integral_constant<int, PG_OP_MUL>{});
    case PG_OP_DIV: return fn(std::integral_constant<int, PG_OP_DIV>{});
    case PG_OP_COPY_LHS: return fn(std::integral_constant<int, PG_OP_COPY_LHS>{});
    case PG_OP_COPY_RHS: return fn(std::integral_constant<int, PG_OP_COPY_RHS>{});
  }
  return PG_ERR_INVALID;
}

inline bool arg_aligned(const void* p, int arg_kind) {
  return ((uintptr_t)p & (arg_kind == PG_ARG_U16 ? 7 : 15)) == 0;
}

}  // namespace

extern "C" {

size_t pg_gspmm_workspace(const pg_csr_t* g, int64_t F, int reduce, int arg_kind) {
  (void)arg_kind;  // slot records are i32 for both kinds
  if (!g || g->n_slots <= 0 || F <= 0) return 0;
  const size_t vals = round_up(g->n_slots * ws_ld(F) * 4, 256);
  return reduce == PG_RED_SUM ? vals : 2 * vals;
}

int pg_gspmm(const pg_csr_t* g, int op, int reduce, const float* L, int64_t ldl, int lt,
             const float* R, int64_t ldr, int rt, const int32_t* eidx, int64_t F, int norm_mode,
             float* out, int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
             size_t ws_bytes, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_gspmm", true));
  if (reduce < PG_RED_SUM || reduce > PG_RED_MIN)
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm: bad reduce %d", reduce);
  const bool sum = reduce == PG_RED_SUM;
  if (sum) argpos = nullptr;
  PG_TRY(pg::check_gop(g, "pg_gspmm", op, ldl, lt, ldr, rt, F, ldo, false, argpos, lda, arg_kind));
  if (norm_mode < 0 || norm_mode > 1 || (norm_mode == 1 && !sum))
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm: bad norm_mode %d", norm_mode);
  if (F == 0 || g->n_rows == 0) return pg::ok();
  const bool ul = pg::gop_reads_lhs(op), ur = pg::gop_reads_rhs(op);
  if (!out || (g->nnz > 0 && ((ul && !L) || (ur && !R))))
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm: NULL buffer");
  const size_t need = pg_gspmm_workspace(g, F, reduce, arg_kind);
  PG_TRY(check_ws(ws_bytes, need, "pg_gspmm"));
  const int64_t ldw = ws_ld(F);
  float* ws_val = need ? (float*)ws : nullptr;
  int32_t* ws_arg = (need && !sum) ? (int32_t*)((char*)ws + need / 2) : nullptr;
  const int32_t* emap = eidx ? eidx : g->eslot;
  const int a16 = arg_kind == PG_ARG_U16;
  TilePlan tp = plan_tiles(F, {ul ? ldl : 4, ur ? ldr : 4, ldo, argpos ? lda : 4},
                           {ul ? L : nullptr, ur ? R : nullptr, out, ws_val});
  if (tp.vec && argpos && !arg_aligned(argpos, arg_kind)) tp.vec = false;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)grid_for(g->n_items), (unsigned)((F + kGTile - 1) / kGTile));
  auto go = [&](auto w_c, auto op_c, auto red_c) -> int {
    hipLaunchKernelGGL((gspmm_kernel<decltype(w_c)::value, decltype(op_c)::value, decltype(red_c)::value>), grid,
                       dim3(kBlock), 0, st, g->ptr, g->col, emap, (const int4*)g->items, (int)g->n_items, L,
                       ldl, (int)(lt == PG_TGT_E), R, ldr, (int)(rt == PG_TGT_E), (int)F, norm_mode, out, ldo,
                       argpos, lda, a16, ws_val, ws_arg, ldw);
    return PG_OK;
  };
  auto by_red = [&](auto w_c, auto op_c) -> int {
    switch (reduce) {
      case PG_RED_SUM: return go(w_c, op_c, std::integral_constant<int, PG_RED_SUM>{});
      case PG_RED_MAX: return go(w_c, op_c, std::integral_constant<int, PG_RED_MAX>{});
      default: return go(w_c, op_c, std::integral_constant<int, PG_RED_MIN>{});
    }
  };
  const int rc = tp.vec ? dispatch_gop(op, [&](auto o) { return by_red(std::integral_constant<int, 4>{}, o); })
                        : dispatch_gop(op, [&](auto o) { return by_red(std::integral_constant<int, 1>{}, o); });
  if (rc != PG_OK) return pg::set_error(rc, "pg_gspmm: bad op %d", op);
  if (g->n_merges > 0) {
    if (sum)
      hipLaunchKernelGGL(sum_merge_kernel<float>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)g->n_merges, (int)F, ws_val, ldw, g->ptr, norm_mode,
                         nullptr, 0, out, ldo);
    else if (reduce == PG_RED_MAX)
      hipLaunchKernelGGL(gcmp_merge_kernel<PG_RED_MAX>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)F, ws_val, ws_arg, ldw, out, ldo, argpos, lda, a16);
    else
      hipLaunchKernelGGL(gcmp_merge_kernel<PG_RED_MIN>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)F, ws_val, ws_arg, ldw, out, ldo, argpos, lda, a16);
  }
  return hip_status("pg_gspmm");
}

int pg_gsddmm(const pg_csr_t* g, int op, const float* L, int64_t ldl, int lt, const float* R,
              int64_t ldr, int rt, const int32_t* eidx, int64_t F, float* out, int64_t ldo,
              const void* argpos, int64_t lda, int arg_kind, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_gsddmm", true));
  PG_TRY(pg::check_gop(g, "pg_gsddmm", op, ldl, lt, ldr, rt, F, ldo, true, argpos, lda, arg_kind));
  if (F == 0 || g->n_rows == 0 || g->nnz == 0) return pg::ok();
  const bool ul = pg::gop_reads_lhs(op), ur = pg::gop_reads_rhs(op);
  if (!out || (ul && !L) || (ur && !R)) return pg::set_error(PG_ERR_INVALID, "pg_gsddmm: NULL buffer");
  if ((ul && out == L) || (ur && out == R))
    return pg::set_error(PG_ERR_INVALID, "pg_gsddmm: the output aliases an input");
  const int32_t* emap = eidx ? eidx : g->eslot;
  const int a16 = arg_kind == PG_ARG_U16;
  TilePlan tp = plan_tiles(F, {ul ? ldl : 4, ur ? ldr : 4, ldo, argpos ? lda : 4},
                           {ul ? L : nullptr, ur ? R : nullptr, out});
  if (tp.vec && argpos && !arg_aligned(argpos, arg_kind)) tp.vec = false;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)grid_for(g->n_items), (unsigned)((F + kGTile - 1) / kGTile));
  auto go = [&](auto w_c, auto op_c, auto mask_c) -> int {
    hipLaunchKernelGGL((gsddmm_kernel<decltype(w_c)::value, decltype(op_c)::value, decltype(mask_c)::value>), grid,
                       dim3(kBlock), 0, st, g->ptr, g->col, emap, (const int4*)g->items, (int)g->n_items, L,
                       ldl, lt, R, ldr, rt, (int)F, out, ldo, argpos, lda, a16);
    return PG_OK;
  };
  auto by_mask = [&](auto w_c, auto op_c) -> int {
    return argpos ? go(w_c, op_c, std::true_type{}) : go(w_c, op_c, std::false_type{});
  };
  const int rc = tp.vec ? dispatch_gop(op, [&](auto o) { return by_mask(std::integral_constant<int, 4>{}, o); })
                        : dispatch_gop(op, [&](auto o) { return by_mask(std::integral_constant<int, 1>{}, o); });
  if (rc != PG_OK) return pg::set_error(rc, "pg_gsddmm: bad op %d", op);
  return hip_status("pg_gsddmm");
}

}  // extern "C"
