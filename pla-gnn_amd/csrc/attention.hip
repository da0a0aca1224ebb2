// Attention kernels on the CSR schedule: edge softmax, per-head weighted sum and SDDMM (GAT),
// and the fused GATv2 scores with their backward. Work decomposition: spmm_common.hpp.
#include "spmm_common.hpp"

namespace {

// ---- multi-head attention: edge softmax, per-head weighted sum, per-head SDDMM ----------
// Edge features are [nnz][ld] in in-CSR slot order, H <= 64 heads per edge.
//
// Edge softmax (forward and backward): a row the schedule keeps whole takes one wave, a row
// it splits (exactly the rows of `merges`) one 256-thread workgroup, the first n_merges
// workgroups of the launch; the other workgroups walk the items and skip the pieces of split
// rows. With H a power of two (lg = log2 H) a thread covers the row's deg * H values at
// i = tid, tid + NT, ...: its head i & (H - 1) never changes (NT % H == 0), so a reduction
// over the row is a per-thread running value, xor-shuffles of stride H, 2H, ... 32 across the
// lanes of equal head and, in a workgroup, one pass over the four waves' results in LDS in
// wave order. Any other H goes one head at a time through the same code (lg = 0 on a base
// pointer moved to the head, values ld apart). A whole row of at most 64 * kSmR values stays
// in registers between the passes (read once, written once); longer rows re-read their
// values, in loops unrolled by 4 so that four loads per thread are in flight (the longest
// split row bounds the call: cfg2 forward 36 -> 27 us). No workspace, no
// atomics; the order of every reduction depends on (deg, H) only.
constexpr int kSmR = 4;

__device__ __forceinline__ int64_t esm_off(int i, int lg, int64_t ld) {
  return (int64_t)(i >> lg) * ld + (i & ((1 << lg) - 1));
}

// reduction over the threads of equal head: lanes `stride0` apart inside the wave, then (BLOCK)
// the four waves in order through red[wave][head]; every thread gets its head's result
template <bool MAX, bool BLOCK>
__device__ __forceinline__ float esm_reduce(float x, int stride0, float (*red)[kWave]) {
  for (int o = stride0; o < kWave; o <<= 1) {
    const float y = __shfl_xor(x, o);
    x = MAX ? fmaxf(x, y) : x + y;
  }
  if constexpr (BLOCK) {
    const int lane = lane_id();
    if (lane < stride0) red[threadIdx.x >> 6][lane] = x;
    __syncthreads();
    const int h = lane & (stride0 - 1);
    x = red[0][h];
#pragma unroll
    for (int q = 1; q < kWavesPerBlock; ++q) x = MAX ? fmaxf(x, red[q][h]) : x + red[q][h];
  }
  return x;
}

// a[i] = exp(s[i] - m) / sum over the n = deg << lg values of one row (s, a at its first slot)
template <bool BLOCK>
__device__ __forceinline__ void esm_fwd_row(const float* __restrict__ s, int64_t lds, float* __restrict__ a,
                                            int64_t lda, int n, int lg, float (*rmax)[kWave],
                                            float (*rsum)[kWave]) {
  constexpr int NT = BLOCK ? kBlock : kWave;
  const int tid = BLOCK ? (int)threadIdx.x : lane_id();
  const float ninf = -std::numeric_limits<float>::infinity();
  const bool in_regs = !BLOCK && n <= NT * kSmR;  // uniform
  float v[kSmR];
  float m = ninf;
  if (in_regs) {
#pragma unroll
    for (int t = 0; t < kSmR; ++t) {
      const int i = tid + t * NT;
      v[t] = i < n ? s[esm_off(i, lg, lds)] : ninf;
      m = fmaxf(m, v[t]);
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += NT) m = fmaxf(m, s[esm_off(i, lg, lds)]);
  }
  m = esm_reduce<true, BLOCK>(m, 1 << lg, rmax);
  float sum = 0.f;
  if (in_regs) {
#pragma unroll
    for (int t = 0; t < kSmR; ++t) {
      v[t] = expf(v[t] - m);  // -inf (a masked score, a lane past the row): exactly 0
      sum += v[t];
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += NT) sum += expf(s[esm_off(i, lg, lds)] - m);
  }
  sum = esm_reduce<false, BLOCK>(sum, 1 << lg, rsum);
  if (in_regs) {
#pragma unroll
    for (int t = 0; t < kSmR; ++t) {
      const int i = tid + t * NT;
      if (i < n) a[esm_off(i, lg, lda)] = v[t] / sum;
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += NT) a[esm_off(i, lg, lda)] = expf(s[esm_off(i, lg, lds)] - m) / sum;
  }
}

// ds[i] = a[i] * (da[i] - sum_row a * da)
template <bool BLOCK>
__device__ __forceinline__ void esm_bwd_row(const float* __restrict__ a, int64_t lda, const float* __restrict__ da,
                                            int64_t ldda, float* __restrict__ ds, int64_t ldds, int n, int lg,
                                            float (*rsum)[kWave]) {
  constexpr int NT = BLOCK ? kBlock : kWave;
  const int tid = BLOCK ? (int)threadIdx.x : lane_id();
  const bool in_regs = !BLOCK && n <= NT * kSmR;  // uniform
  float va[kSmR], vd[kSmR];
  float sum = 0.f;
  if (in_regs) {
#pragma unroll
    for (int t = 0; t < kSmR; ++t) {
      const int i = tid + t * NT;
      va[t] = i < n ? a[esm_off(i, lg, lda)] : 0.f;
      vd[t] = i < n ? da[esm_off(i, lg, ldda)] : 0.f;
      sum += va[t] * vd[t];
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += NT) sum += a[esm_off(i, lg, lda)] * da[esm_off(i, lg, ldda)];
  }
  sum = esm_reduce<false, BLOCK>(sum, 1 << lg, rsum);
  if (in_regs) {
#pragma unroll
    for (int t = 0; t < kSmR; ++t) {
      const int i = tid + t * NT;
      if (i < n) ds[esm_off(i, lg, ldds)] = va[t] * (vd[t] - sum);
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += NT)
      ds[esm_off(i, lg, ldds)] = a[esm_off(i, lg, lda)] * (da[esm_off(i, lg, ldda)] - sum);
  }
}

// The row of this wave (whole-row items) or workgroup (split rows): false = nothing to do.
// lg >= 0: H = 1 << lg; lg < 0: any H, one head at a time.
__device__ __forceinline__ bool esm_row(const int32_t* __restrict__ ptr, const int4* __restrict__ items, int n_items,
                                        const int4* __restrict__ merges, int n_merges, int& rs, int& deg) {
  if ((int)blockIdx.x < n_merges) {
    const int row = merges[blockIdx.x].x;
    rs = ptr[row];
    deg = ptr[row + 1] - rs;
    return true;
  }
  const int it = ((int)blockIdx.x - n_merges) * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return false;
  const int4 item = items[it];
  if (item.w >= 0) return false;  // a piece of a split row: taken whole by a workgroup
  rs = item.y;
  deg = item.z - item.y;
  return deg > 0;
}

__global__ __launch_bounds__(kBlock) void edge_softmax_fwd_kernel(
    const int32_t* __restrict__ ptr, const int4* __restrict__ items, int n_items, const int4* __restrict__ merges,
    int n_merges, const float* __restrict__ s, int64_t lds, float* __restrict__ a, int64_t lda, int H, int lg) {
  __shared__ float rmax[kWavesPerBlock][kWave], rsum[kWavesPerBlock][kWave];
  int rs, deg;
  if (!esm_row(ptr, items, n_items, merges, n_merges, rs, deg)) return;
  s += (int64_t)rs * lds;
  a += (int64_t)rs * lda;
  if ((int)blockIdx.x < n_merges) {  // uniform over the workgroup
    if (lg >= 0) {
      esm_fwd_row<true>(s, lds, a, lda, deg << lg, lg, rmax, rsum);
    } else {
      for (int h = 0; h < H; ++h) {
        esm_fwd_row<true>(s + h, lds, a + h, lda, deg, 0, rmax, rsum);
        __syncthreads();  // rmax / rsum are reused by the next head
      }
    }
  } else if (lg >= 0) {
    esm_fwd_row<false>(s, lds, a, lda, deg << lg, lg, rmax, rsum);
  } else {
    for (int h = 0; h < H; ++h) esm_fwd_row<false>(s + h, lds, a + h, lda, deg, 0, rmax, rsum);
  }
}

__global__ __launch_bounds__(kBlock) void edge_softmax_bwd_kernel(
    const int32_t* __restrict__ ptr, const int4* __restrict__ items, int n_items, const int4* __restrict__ merges,
    int n_merges, const float* __restrict__ a, int64_t lda, const float* __restrict__ da, int64_t ldda,
    float* __restrict__ ds, int64_t ldds, int H, int lg) {
  __shared__ float rsum[kWavesPerBlock][kWave];
  int rs, deg;
  if (!esm_row(ptr, items, n_items, merges, n_merges, rs, deg)) return;
  a += (int64_t)rs * lda;
  da += (int64_t)rs * ldda;
  ds += (int64_t)rs * ldds;
  if ((int)blockIdx.x < n_merges) {  // uniform over the workgroup
    if (lg >= 0) {
      esm_bwd_row<true>(a, lda, da, ldda, ds, ldds, deg << lg, lg, rsum);
    } else {
      for (int h = 0; h < H; ++h) {
        esm_bwd_row<true>(a + h, lda, da + h, ldda, ds + h, ldds, deg, 0, rsum);
        __syncthreads();  // rsum is reused by the next head
      }
    }
  } else if (lg >= 0) {
    esm_bwd_row<false>(a, lda, da, ldda, ds, ldds, deg << lg, lg, rsum);
  } else {
    for (int h = 0; h < H; ++h) esm_bwd_row<false>(a + h, lda, da + h, ldda, ds + h, ldds, deg, 0, rsum);
  }
}

// Per-head weighted sum: sum_kernel with the weight A[slot, head of the column] in place of
// ew[slot]. The launch covers the columns [f0, f0 + F) of the H * Fh (X, out, ws point at
// column f0): a lane's head comes from its absolute column, once per column chunk, so a head
// may straddle two launches' tiles. On the vector path (Fh % 4 == 0) a lane's four columns
// share one head. The U edges' weights are fetched beside their X rows (one 4-byte load per
// lane and chunk; the lanes of a head read one address), so the loads of a batch are all in
// flight together. Split rows leave partial sums in ws for sum_merge_kernel, as sum_kernel.
template <int W, int NC>
__global__ __launch_bounds__(kBlock) void sum_heads_kernel(
    const int32_t* __restrict__ col, const int32_t* __restrict__ eslot, const float* __restrict__ A,
    int64_t lda, int H, int Fh, int f0, const int4* __restrict__ items, int n_items,
    const float* __restrict__ X, int64_t ldx, int F, float* __restrict__ out, int64_t ldo,
    float* __restrict__ ws, int64_t ldw) {
  constexpr int U = EdgeU<W, NC>::value;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z, slot = item.w;
  const int lane = lane_id();
  float acc[NC][W];
  int hc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hc[c] = min((f0 + (c * kWave + lane) * W) / Fh, H - 1);  // lanes past F: a valid head, result not stored
#pragma unroll
    for (int i = 0; i < W; ++i) acc[c][i] = 0.f;
  }

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int kl = kw + min(lane, nw - 1);
    const int idxv = col[kl];
    const int sv = eslot ? eslot[kl] : kl;
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float v[U][NC][W];
      float w[U][NC];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const int je = j + min(e, nv - 1);
        const float* xr = X + (int64_t)bcast(idxv, je) * ldx;
        const float* ar = A + (int64_t)bcast(sv, je) * lda;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          load_tile<W>(xr, (c * kWave + lane) * W, F, v[e][c], 0.f);
          w[e][c] = ar[hc[c]];
        }
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i) acc[c][i] += v[e][c][i] * w[e][c];
        }
      }
    }
  }
  float* orow = slot < 0 ? out + (int64_t)row * ldo : ws + (int64_t)slot * ldw;
#pragma unroll
  for (int c = 0; c < NC; ++c) store_tile<W>(orow, (c * kWave + lane) * W, F, acc[c]);
}

// Per-head SDDMM, vector path with Fh / 4 = 1 << LGL lanes per head (Fh = 4 ... 256):
// sddmm_dot_kernel with the cross-lane reduction stopped at the head boundary. Of the
// transposing butterfly's three steps the first TS = min(3, LGL) stay inside a head; plain
// steps cover the head's remaining lane bits. A lane then holds 8 >> TS sums: those of the
// batch's edges (i << TS) + (lane & (2^TS - 1)) for the head of its columns. A head lies in
// exactly one 256-column tile, so nothing is carried between tiles; one lane per (edge, head)
// stores, a batch's H values per edge side by side.
template <int LGL>
__global__ __launch_bounds__(kBlock) void sddmm_heads_kernel(
    const int32_t* __restrict__ col, const int4* __restrict__ items, int n_items,
    const float* __restrict__ D, int64_t ldd, const float* __restrict__ X, int64_t ldx, int F,
    float* __restrict__ de, int64_t lde) {
  constexpr int U = 8, W = 4;
  constexpr int T = kWave * W;
  constexpr int TS = LGL < 3 ? LGL : 3;
  constexpr int LPH = 1 << LGL;  // lanes per head
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  const int lane = lane_id();
  const float* drow = D + (int64_t)row * ldd;
  const bool one_tile = F <= T;
  float d[W] = {0.f, 0.f, 0.f, 0.f};
  if (one_tile) load_tile<W>(drow, lane * W, F, d, 0.f);
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  const int esub = lane & ((1 << TS) - 1);        // the lane's edge inside a group of 1 << TS
  const bool writer = (lane & (LPH - 1)) == esub;  // one lane per (edge, head)

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int idxv = col[kw + min(lane, nw - 1)];
    for (int f0 = 0; f0 < F; f0 += T) {
      const int f = f0 + lane * W;
      if (!one_tile) load_tile<W>(drow, f, F, d, 0.f);
      const int head = f >> (LGL + 2);
      for (int j = 0; j < nw; j += U) {
        const int nv = min(U, nw - j);
        float v[U][W];
#pragma unroll
        for (int e = 0; e < U; ++e)
          load_tile<W>(X + (int64_t)bcast(idxv, j + min(e, nv - 1)) * ldx, f, F, v[e], 0.f);
        float p[U];
#pragma unroll
        for (int e = 0; e < U; ++e) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < W; ++i) s += d[i] * v[e][i];
          p[e] = s;
        }
        if constexpr (TS >= 1) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float keep = b0 ? p[2 * i + 1] : p[2 * i], send = b0 ? p[2 * i] : p[2 * i + 1];
            p[i] = keep + __shfl_xor(send, 1);
          }
        }
        if constexpr (TS >= 2) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const float keep = b1 ? p[2 * i + 1] : p[2 * i], send = b1 ? p[2 * i] : p[2 * i + 1];
            p[i] = keep + __shfl_xor(send, 2);
          }
        }
        if constexpr (TS >= 3) {
          const float keep = b2 ? p[1] : p[0], send = b2 ? p[0] : p[1];
          p[0] = keep + __shfl_xor(send, 4);
#pragma unroll
          for (int o = 8; o < LPH; o <<= 1) p[0] += __shfl_xor(p[0], o);
        }
        if (writer && f < F) {
#pragma unroll
          for (int i = 0; i < (U >> TS); ++i) {
            const int e = (i << TS) + esub;
            if (e < nv) de[(int64_t)(kw + j + e) * lde + head] = p[i];
          }
        }
      }
    }
  }
}

// Any other Fh, or unaligned operands: one (edge, head) pair per lane, Fh products in
// ascending j (the host entry point's order).
__global__ __launch_bounds__(kBlock) void sddmm_heads_generic_kernel(
    const int32_t* __restrict__ col, const int4* __restrict__ items, int n_items,
    const float* __restrict__ D, int64_t ldd, const float* __restrict__ X, int64_t ldx, int H, int Fh,
    float* __restrict__ de, int64_t lde) {
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  const float* drow = D + (int64_t)row * ldd;
  const int64_t n = (int64_t)(k1 - k0) * H;
  for (int64_t i = lane_id(); i < n; i += kWave) {
    const int k = k0 + (int)(i / H), h = (int)(i % H);
    const float* dh = drow + (int64_t)h * Fh;
    const float* xh = X + (int64_t)col[k] * ldx + (int64_t)h * Fh;
    float acc = 0.f;
    for (int j = 0; j < Fh; ++j) acc += dh[j] * xh[j];
    de[(int64_t)k * lde + h] = acc;
  }
}

}  // namespace

extern "C" {

int pg_edge_softmax_fwd(const pg_csr_t* g, const float* s, int64_t lds, int32_t H, float* a, int64_t lda,
                        pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_edge_softmax_fwd", true));
  PG_TRY(pg::check_heads(g, "pg_edge_softmax_fwd", H, {lds, lda}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!s || !a) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_fwd: NULL buffer");
  if (s == a) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_fwd: the output aliases an input");
  const int blocks = (int)g->n_merges + grid_for(g->n_items);
  hipLaunchKernelGGL(edge_softmax_fwd_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g->ptr,
                     (const int4*)g->items, (int)g->n_items, (const int4*)g->merges, (int)g->n_merges, s, lds, a,
                     lda, (int)H, pg::log2_exact(H));
  return hip_status("pg_edge_softmax_fwd");
}

int pg_edge_softmax_bwd(const pg_csr_t* g, const float* a, int64_t lda, const float* da, int64_t ldda, int32_t H,
                        float* ds, int64_t ldds, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_edge_softmax_bwd", true));
  PG_TRY(pg::check_heads(g, "pg_edge_softmax_bwd", H, {lda, ldda, ldds}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!a || !da || !ds) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_bwd: NULL buffer");
  if (ds == a || ds == da) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_bwd: the output aliases an input");
  const int blocks = (int)g->n_merges + grid_for(g->n_items);
  hipLaunchKernelGGL(edge_softmax_bwd_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g->ptr,
                     (const int4*)g->items, (int)g->n_items, (const int4*)g->merges, (int)g->n_merges, a, lda, da,
                     ldda, ds, ldds, (int)H, pg::log2_exact(H));
  return hip_status("pg_edge_softmax_bwd");
}

int pg_spmm_sum_heads(const pg_csr_t* g, const float* A, int64_t lda, int32_t H, const float* X, int64_t ldx,
                      int64_t Fh, float* out, int64_t ldo, void* ws, size_t ws_bytes, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_spmm_sum_heads", true));
  PG_TRY(pg::check_heads(g, "pg_spmm_sum_heads", H, {lda}));
  PG_TRY(pg::check_head_features("pg_spmm_sum_heads", H, Fh, {ldx, ldo}));
  if (g->n_rows == 0) return pg::ok();  // (nnz == 0 with rows: every row is empty, out = 0)
  const int64_t F = (int64_t)H * Fh;
  if (!X || !out || (g->nnz > 0 && !A)) return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_heads: NULL buffer");
  if (out == X || out == A) return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_heads: the output aliases an input");
  const size_t need = pg_spmm_sum_workspace(g, F);
  PG_TRY(check_ws(ws_bytes, need, "pg_spmm_sum_heads"));
  float* w = need ? (float*)ws : nullptr;
  const int64_t ldw = ws_ld(F);
  hipStream_t st = (hipStream_t)stream;
  TilePlan tp = plan_tiles(F, {ldx, ldo}, {X, out, w});
  if (Fh % 4 != 0) tp = {false, (int64_t)kFTileScalar};  // a lane's four columns must share a head
  const int blocks = grid_for(g->n_items);
  for (int64_t f0 = 0; f0 < F; f0 += tp.tile) {
    const int Ft = (int)std::min<int64_t>(tp.tile, F - f0);
    auto go = [&](auto nc_c, auto w_c) -> int {
      constexpr int NC = decltype(nc_c)::value;
      constexpr int W = decltype(w_c)::value;
      hipLaunchKernelGGL((sum_heads_kernel<W, NC>), dim3(blocks), dim3(kBlock), 0, st, g->col, g->eslot, A, lda,
                         (int)H, (int)Fh, (int)f0, (const int4*)g->items, (int)g->n_items, X + f0, ldx, Ft,
                         out + f0, ldo, w ? w + f0 : nullptr, ldw);
      return PG_OK;
    };
    const int rc = dispatch_tile(tp, Ft, go);
    if (rc != PG_OK) return pg::set_error(rc, "pg_spmm_sum_heads: unsupported feature tile");
    if (g->n_merges > 0)
      hipLaunchKernelGGL(sum_merge_kernel<float>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                         (const int4*)g->merges, (int)g->n_merges, Ft, w + f0, ldw, g->ptr, 0, nullptr, 0,
                         out + f0, ldo);
  }
  return hip_status("pg_spmm_sum_heads");
}

int pg_sddmm_dot_heads(const pg_csr_t* g, const float* Dm, int64_t ldd, const float* X, int64_t ldx, int32_t H,
                       int64_t Fh, float* de, int64_t lde, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_sddmm_dot_heads", true));
  PG_TRY(pg::check_heads(g, "pg_sddmm_dot_heads", H, {lde}));
  PG_TRY(pg::check_head_features("pg_sddmm_dot_heads", H, Fh, {ldd, ldx}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!de || !Dm || !X) return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot_heads: NULL buffer");
  if (de == Dm || de == X) return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot_heads: the output aliases an input");
  const int64_t F = (int64_t)H * Fh;
  const TilePlan tp = plan_tiles(F, {ldd, ldx}, {Dm, X});
  const int lgl = (Fh % 4 == 0) ? pg::log2_exact((int32_t)std::min<int64_t>(Fh / 4, 1 << 20)) : -1;
  const int blocks = grid_for(g->n_items);
  hipStream_t st = (hipStream_t)stream;
  auto go = [&](auto l_c) {
    constexpr int LGL = decltype(l_c)::value;
    hipLaunchKernelGGL((sddmm_heads_kernel<LGL>), dim3(blocks), dim3(kBlock), 0, st, g->col, (const int4*)g->items,
                       (int)g->n_items, Dm, ldd, X, ldx, (int)F, de, lde);
  };
  if (tp.vec && lgl >= 0 && lgl <= 6) {
    switch (lgl) {
      case 0: go(std::integral_constant<int, 0>{}); break;
      case 1: go(std::integral_constant<int, 1>{}); break;
      case 2: go(std::integral_constant<int, 2>{}); break;
      case 3: go(std::integral_constant<int, 3>{}); break;
      case 4: go(std::integral_constant<int, 4>{}); break;
      case 5: go(std::integral_constant<int, 5>{}); break;
      default: go(std::integral_constant<int, 6>{}); break;
    }
  } else {
    hipLaunchKernelGGL(sddmm_heads_generic_kernel, dim3(blocks), dim3(kBlock), 0, st, g->col,
                       (const int4*)g->items, (int)g->n_items, Dm, ldd, X, ldx, (int)H, (int)Fh, de, lde);
  }
  return hip_status("pg_sddmm_dot_heads");
}

}  // extern "C"

// ---- GATv2 attention scores, fused ----------------------------------------------------------
// s[k,h] = sum_d attn[h,d] * lrelu(XL[col[k],h,d] + XR[v,h,d]): the non-linearity sits between
// the add and the contraction, so the score does not factor into per-node scalars. Forward
// and backward recompute the pre-activation t_k from the two node rows; no [nnz][H*Fh] tensor
// is ever formed.
namespace {

__device__ __forceinline__ float lrelu(float x, float slope) { return x > 0.f ? x : slope * x; }

// Forward, vector path (Fh % 4 == 0): one wave per schedule item, 256 columns (one float4 per
// lane) per feature tile, a lane's four columns in one head. U gathered XL rows are in flight
// before any is used; the item's XR tile and the attn tile stay in registers when F fits one
// tile. The lanes of a head are consecutive, so a segmented shuffle reduction (offsets 1, 2,
// ... below the lanes a head can span) leaves each head's sum in its first lane. A head that
// runs past the tile's end is not stored: its partial sum is carried (wave-uniform) into the
// next tile, where lane 0 continues it. The tiles of a batch are walked inside the wave, so
// each s[k,h] is written once, by one lane, in a fixed order.
__global__ __launch_bounds__(kBlock) void gatv2_score_kernel(
    const int32_t* __restrict__ col, const int4* __restrict__ items, int n_items,
    const float* __restrict__ XL, int64_t ldl, const float* __restrict__ XR, int64_t ldr,
    const float* __restrict__ attn, int F, int Fh, float slope, float* __restrict__ s, int64_t lds) {
  constexpr int U = 8, W = 4;
  constexpr int T = kWave * W;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  const int lane = lane_id();
  const float* orow = XR + (int64_t)row * ldr;
  const bool one_tile = F <= T;
  const int seg = min(kWave, Fh / W);  // lanes a head can span inside a tile
  float own[W] = {0.f, 0.f, 0.f, 0.f}, at[W] = {0.f, 0.f, 0.f, 0.f};
  int head = -1;  // lanes past F: a segment of their own, never stored
  if (one_tile) {
    load_tile<W>(orow, lane * W, F, own, 0.f);
    load_tile<W>(attn, lane * W, F, at, 0.f);
    head = lane * W < F ? lane * W / Fh : -1;
  }

  for (int kw = k0; kw < k1; kw += kWave) {
    const int nw = min(kWave, k1 - kw);
    const int idxv = col[kw + min(lane, nw - 1)];
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      float carry[U];
#pragma unroll
      for (int e = 0; e < U; ++e) carry[e] = 0.f;
      int carry_h = -1;
      for (int f0 = 0; f0 < F; f0 += T) {
        const int f = f0 + lane * W;
        if (!one_tile) {
          load_tile<W>(orow, f, F, own, 0.f);
          load_tile<W>(attn, f, F, at, 0.f);
          head = f < F ? f / Fh : -1;
        }
        float v[U][W];
#pragma unroll
        for (int e = 0; e < U; ++e)
          load_tile<W>(XL + (int64_t)bcast(idxv, j + min(e, nv - 1)) * ldl, f, F, v[e], 0.f);
        float p[U];
#pragma unroll
        for (int e = 0; e < U; ++e) {
          float a = 0.f;
#pragma unroll
          for (int i = 0; i < W; ++i) a += at[i] * lrelu(v[e][i] + own[i], slope);
          p[e] = a;
        }
        for (int o = 1; o < seg; o <<= 1) {
          const int hn = __shfl_down(head, o);  // by every lane, before the lane test: a shuffle
          const bool same = (lane + o < kWave) & (hn == head);  // under a lane mask reads dead lanes
#pragma unroll
          for (int e = 0; e < U; ++e) {
            const float q = __shfl_down(p[e], o);
            if (same) p[e] += q;
          }
        }
        const int hprev = __shfl_up(head, 1);
        const bool first = head >= 0 && (lane == 0 || hprev != head);
        if (lane == 0 && head == carry_h) {
#pragma unroll
          for (int e = 0; e < U; ++e) p[e] = carry[e] + p[e];
        }
        const int fend = min(F, f0 + T);
        const int hl = (fend - 1) / Fh;               // the tile's last head
        const bool ends = (hl + 1) * Fh <= fend;      // ... is complete here
        if (first && (head != hl || ends)) {
#pragma unroll
          for (int e = 0; e < U; ++e)
            if (e < nv) s[(int64_t)(kw + j + e) * lds + head] = p[e];
        }
        if (!ends) {
          const int fl = max(0, (hl * Fh - f0) / W);  // first lane of the last head
#pragma unroll
          for (int e = 0; e < U; ++e) carry[e] = __shfl(p[e], fl);
          carry_h = hl;
        }
      }
    }
  }
}

// Forward, scalar path (any Fh, ld and alignment): one (entry, head) pair per lane, the Fh
// terms in ascending d (the host entry point's order).
__global__ __launch_bounds__(kBlock) void gatv2_score_generic_kernel(
    const int32_t* __restrict__ col, const int4* __restrict__ items, int n_items,
    const float* __restrict__ XL, int64_t ldl, const float* __restrict__ XR, int64_t ldr,
    const float* __restrict__ attn, int H, int Fh, float slope, float* __restrict__ s, int64_t lds) {
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, k0 = item.y, k1 = item.z;
  const float* orow = XR + (int64_t)row * ldr;
  const int64_t n = (int64_t)(k1 - k0) * H;
  for (int64_t i = lane_id(); i < n; i += kWave) {
    const int k = k0 + (int)(i / H), h = (int)(i % H);
    const float* ah = attn + (int64_t)h * Fh;
    const float* rh = orow + (int64_t)h * Fh;
    const float* lh = XL + (int64_t)col[k] * ldl + (int64_t)h * Fh;
    float acc = 0.f;
    for (int d = 0; d < Fh; ++d) acc += ah[d] * lrelu(lh[d] + rh[d], slope);
    s[(int64_t)k * lds + h] = acc;
  }
}

// Backward pass over a CSR (the in-CSR: dXR; its transpose with the node operands swapped:
// dXL), shaped as sum_heads_kernel: one wave per schedule item, 256 feature columns per wave
// (W = 4: one float4 per lane, its columns in one head; W = 1: four columns 64 apart), wider
// F in tiles along gridDim.y (tile index ft0 + blockIdx.y). Per entry the gathered row and
// the edge's ds value are loaded U at a time, t = gathered + own is recomputed, and
//   DX: acc += ds * lrelu'(t)      (attn factored out: one multiply per row, not per entry)
//   DA: da  += ds * lrelu(t)
// A split row's piece goes to its workspace slot for sum_merge_kernel, already scaled by
// attn. DA: the four waves of a workgroup add their da tiles through LDS in wave order and
// write one partial row per workgroup; colsum_rows_kernel reduces those in row order.
template <int W, bool DX, bool DA>
__global__ __launch_bounds__(kBlock) void gatv2_bwd_kernel(
    const int32_t* __restrict__ col, const int32_t* __restrict__ eslot, const int4* __restrict__ items,
    int n_items, const float* __restrict__ ds, int64_t ldds, const float* __restrict__ Xown, int64_t ldown,
    const float* __restrict__ Xgat, int64_t ldgat, const float* __restrict__ attn, int F, int Fh, int H,
    float slope, int ft0, float* __restrict__ dX, int64_t lddx, float* __restrict__ ws, int64_t ldw,
    float* __restrict__ da_part, int64_t ldp) {
  constexpr int NC = W == 4 ? 1 : 4;
  constexpr int U = 8;
  __shared__ float sda[DA ? kWavesPerBlock * kGTile : 1];
  const int wv = wave_id_uniform();
  const int it = blockIdx.x * kWavesPerBlock + wv;
  const bool active = it < n_items;
  if (!DA && !active) return;
  const int lane = lane_id();
  const int f0 = (ft0 + (int)blockIdx.y) * kGTile;
  const int Ft = min(kGTile, F - f0);
  float da[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < W; ++i) da[c][i] = 0.f;

  if (active) {
    const int4 item = items[it];
    const int row = item.x, k0 = item.y, k1 = item.z, slot = item.w;
    float own[NC][W], acc[NC][W];
    int hc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int fl = (c * kWave + lane) * W;
      hc[c] = min((f0 + fl) / Fh, H - 1);  // lanes past F: a valid head, result not stored
      load_tile<W>(Xown + (int64_t)row * ldown + f0, fl, Ft, own[c], 0.f);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[c][i] = 0.f;
    }
    Xgat += f0;

    for (int kw = k0; kw < k1; kw += kWave) {
      const int nw = min(kWave, k1 - kw);
      const int kl = kw + min(lane, nw - 1);
      const int idxv = col[kl];
      const int sv = eslot ? eslot[kl] : kl;
      for (int j = 0; j < nw; j += U) {
        const int nv = min(U, nw - j);
        float v[U][NC][W];
        float w[U][NC];
#pragma unroll
        for (int e = 0; e < U; ++e) {
          const int je = j + min(e, nv - 1);
          const float* xr = Xgat + (int64_t)bcast(idxv, je) * ldgat;
          const float* dr = ds + (int64_t)bcast(sv, je) * ldds;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            load_tile<W>(xr, (c * kWave + lane) * W, Ft, v[e][c], 0.f);
            w[e][c] = dr[hc[c]];
          }
        }
#pragma unroll
        for (int e = 0; e < U; ++e) {
          if (e < nv) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const float wsl = w[e][c] * slope;
#pragma unroll
              for (int i = 0; i < W; ++i) {
                const float t = v[e][c][i] + own[c][i];
                if constexpr (DX) acc[c][i] += t > 0.f ? w[e][c] : wsl;
                if constexpr (DA) da[c][i] += w[e][c] * lrelu(t, slope);
              }
            }
          }
        }
      }
    }
    if constexpr (DX) {
      float* orow = (slot < 0 ? dX + (int64_t)row * lddx : ws + (int64_t)slot * ldw) + f0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int fl = (c * kWave + lane) * W;
        float at[W];
        load_tile<W>(attn + f0, fl, Ft, at, 0.f);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[c][i] = at[i] * acc[c][i];
        store_tile<W>(orow, fl, Ft, acc[c]);
      }
    }
  }
  if constexpr (DA) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < W; ++i) sda[wv * kGTile + (c * kWave + lane) * W + i] = da[c][i];
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t < Ft) {
      float a = sda[t];
#pragma unroll
      for (int q = 1; q < kWavesPerBlock; ++q) a += sda[q * kGTile + t];
      da_part[(int64_t)blockIdx.x * ldp + f0 + t] = a;
    }
  }
}

// out[b, f] = sum of rows [b * R, min(n, (b + 1) * R)) of `in`, in row order: the fixed-order
// reduction of the dattn partial rows, applied until one row is left.
constexpr int kColsumR = 32;
__global__ __launch_bounds__(kBlock) void colsum_rows_kernel(
    const float* __restrict__ in, int64_t ldi, int n, int F, float* __restrict__ out, int64_t ldo) {
  const int r0 = (int)blockIdx.x * kColsumR, r1 = min(n, r0 + kColsumR);
  for (int f = threadIdx.x; f < F; f += kBlock) {
    float acc = 0.f;
    for (int r = r0; r < r1; r += 8) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = in[(int64_t)min(r + e, r1 - 1) * ldi + f];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (r + e < r1) acc += v[e];
    }
    out[(int64_t)blockIdx.x * ldo + f] = acc;
  }
}

inline int64_t colsum_rows_out(int64_t n) { return (n + kColsumR - 1) / kColsumR; }

}  // namespace

extern "C" {

int pg_gatv2_score(const pg_csr_t* g, const float* XL, int64_t ldl, const float* XR, int64_t ldr,
                   const float* attn, int32_t H, int64_t Fh, float slope, float* s, int64_t lds,
                   pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_gatv2_score", true));
  PG_TRY(pg::check_heads(g, "pg_gatv2_score", H, {lds}));
  PG_TRY(pg::check_head_features("pg_gatv2_score", H, Fh, {ldl, ldr}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!s || !XL || !XR || !attn) return pg::set_error(PG_ERR_INVALID, "pg_gatv2_score: NULL buffer");
  if (s == XL || s == XR || s == attn)
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_score: the output aliases an input");
  const int64_t F = (int64_t)H * Fh;
  const TilePlan tp = plan_tiles(F, {ldl, ldr}, {XL, XR, attn});
  const int blocks = grid_for(g->n_items);
  hipStream_t st = (hipStream_t)stream;
  if (tp.vec && Fh % 4 == 0)
    hipLaunchKernelGGL(gatv2_score_kernel, dim3(blocks), dim3(kBlock), 0, st, g->col, (const int4*)g->items,
                       (int)g->n_items, XL, ldl, XR, ldr, attn, (int)F, (int)Fh, slope, s, lds);
  else
    hipLaunchKernelGGL(gatv2_score_generic_kernel, dim3(blocks), dim3(kBlock), 0, st, g->col,
                       (const int4*)g->items, (int)g->n_items, XL, ldl, XR, ldr, attn, (int)H, (int)Fh, slope, s,
                       lds);
  return hip_status("pg_gatv2_score");
}

// workspace: [split-row slots: n_slots x ldw][dattn partial rows: one per workgroup x ldw]
// [their first reduction: a 32nd of them x ldw], each block 256-B padded
size_t pg_gatv2_bwd_workspace(const pg_csr_t* g, int32_t H, int64_t Fh, int with_dattn) {
  if (!g || H < 1 || Fh < 1) return 0;
  const int64_t ldw = ws_ld((int64_t)H * Fh);
  size_t n = g->n_slots > 0 ? (size_t)round_up(g->n_slots * ldw * 4, 256) : 0;
  if (with_dattn && g->n_items > 0) {
    const int64_t nb = grid_for(g->n_items);
    n += (size_t)round_up(nb * ldw * 4, 256) + (size_t)round_up(colsum_rows_out(nb) * ldw * 4, 256);
  }
  return n;
}

int pg_gatv2_bwd(const pg_csr_t* g, const float* ds, int64_t ldds, const float* Xown, int64_t ldown,
                 const float* Xgat, int64_t ldgat, const float* attn, int32_t H, int64_t Fh,
                 float slope, float* dXown, int64_t lddx, float* dattn, void* ws, size_t ws_bytes,
                 pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_gatv2_bwd", true));
  PG_TRY(pg::check_heads(g, "pg_gatv2_bwd", H, {ldds}));
  PG_TRY(pg::check_head_features("pg_gatv2_bwd", H, Fh, {ldown, ldgat, dXown ? lddx : (int64_t)H * Fh}));
  if (!dXown && !dattn) return pg::ok();
  const int64_t F = (int64_t)H * Fh;
  hipStream_t st = (hipStream_t)stream;
  if (g->n_rows == 0) {  // no rows: dXown is empty, dattn = 0
    if (dattn)
      hipLaunchKernelGGL(fill2d_kernel, dim3((unsigned)std::min<int64_t>(1024, (F + kBlock - 1) / kBlock)),
                         dim3(kBlock), 0, st, dattn, F, (int64_t)1, (int)F, 0.f);
    return hip_status("pg_gatv2_bwd");
  }
  if (!Xown || !Xgat || !attn || (g->nnz > 0 && !ds))
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_bwd: NULL buffer");
  if ((dXown && (dXown == Xown || dXown == Xgat || dXown == attn || dXown == ds)) ||
      (dattn && (dattn == Xown || dattn == Xgat || dattn == attn || dattn == ds || dattn == dXown)))
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_bwd: an output aliases an input");
  const size_t need = pg_gatv2_bwd_workspace(g, H, Fh, dattn != nullptr);
  PG_TRY(check_ws(ws_bytes, need, "pg_gatv2_bwd"));
  const int64_t ldw = ws_ld(F);
  const int64_t nb = grid_for(g->n_items);
  const size_t slot_bytes = g->n_slots > 0 ? (size_t)round_up(g->n_slots * ldw * 4, 256) : 0;
  float* w_slots = slot_bytes ? (float*)ws : nullptr;
  float* part_a = dattn ? (float*)((char*)ws + slot_bytes) : nullptr;
  float* part_b = dattn ? (float*)((char*)part_a + round_up(nb * ldw * 4, 256)) : nullptr;
  TilePlan tp = plan_tiles(F, {ldown, ldgat, dXown ? lddx : 4}, {Xown, Xgat, attn, dXown, w_slots});
  if (Fh % 4 != 0) tp.vec = false;  // a lane's four columns must share a head
  const int64_t n_ft = (F + kGTile - 1) / kGTile;
  constexpr int64_t kMaxY = 32768;
  for (int64_t y0 = 0; y0 < n_ft; y0 += kMaxY) {
    const dim3 grid((unsigned)nb, (unsigned)std::min<int64_t>(kMaxY, n_ft - y0));
    auto go = [&](auto w_c, auto dx_c, auto da_c) {
      hipLaunchKernelGGL((gatv2_bwd_kernel<decltype(w_c)::value, decltype(dx_c)::value, decltype(da_c)::value>),
                         grid, dim3(kBlock), 0, st, g->col, g->eslot, (const int4*)g->items, (int)g->n_items, ds,
                         ldds, Xown, ldown, Xgat, ldgat, attn, (int)F, (int)Fh, (int)H, slope, (int)y0, dXown,
                         lddx, w_slots, ldw, part_a, ldw);
    };
    auto by_out = [&](auto w_c) {
      if (dXown && dattn) go(w_c, std::true_type{}, std::true_type{});
      else if (dXown) go(w_c, std::true_type{}, std::false_type{});
      else go(w_c, std::false_type{}, std::true_type{});
    };
    if (tp.vec) by_out(std::integral_constant<int, 4>{});
    else by_out(std::integral_constant<int, 1>{});
  }
  if (dXown && g->n_merges > 0)
    hipLaunchKernelGGL(sum_merge_kernel<float>, dim3((unsigned)g->n_merges), dim3(kBlock), 0, st,
                       (const int4*)g->merges, (int)g->n_merges, (int)F, w_slots, ldw, g->ptr, 0, nullptr, 0,
                       dXown, lddx);
  if (dattn) {
    const float* src = part_a;
    float* other = part_b;
    int64_t n = nb;
    do {
      const int64_t n_out = colsum_rows_out(n);
      float* dst = n_out == 1 ? dattn : other;
      hipLaunchKernelGGL(colsum_rows_kernel, dim3((unsigned)n_out), dim3(kBlock), 0, st, src, ldw, (int)n, (int)F,
                         dst, ldw);
      other = const_cast<float*>(src);
      src = dst;
      n = n_out;
    } while (n > 1);
  }
  return hip_status("pg_gatv2_bwd");
}

}  // extern "C"
