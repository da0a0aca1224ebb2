// Host (CPU-device) implementations of the message-passing entry points.
//
// These serve tensors the caller keeps on the CPU device, the role DGL's CPU backend
// plays when the reference runs with `-d cpu` (code/main_normal.py:30, 66). They are a
// device choice made by the caller, never a fallback for a failed GPU call.
// Row-parallel over destinations with OpenMP, entries in CSR order, like DGL's
// SpMMCmpCsr CPU loop.
#include <algorithm>
#include <cmath>
#include <limits>
#include <new>
#include <utility>
#include <vector>
#include <type_traits>

#include "common.hpp"
#include "sample_key.hpp"

namespace {

template <typename A>
inline A none_val();
template <>
inline uint16_t none_val<uint16_t>() { return 0xFFFF; }
template <>
inline int32_t none_val<int32_t>() { return -1; }

template <typename A>
void max_fwd(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, float* out, int64_t ldo,
             A* arg, int64_t lda) {
  const float ninf = -std::numeric_limits<float>::infinity();
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    float* o = out + v * ldo;
    A* a = arg + v * lda;
    const int32_t b = g->ptr[v], e = g->ptr[v + 1];
    if (b == e) {
      for (int64_t f = 0; f < F; ++f) {
        o[f] = 0.f;
        a[f] = none_val<A>();
      }
      continue;
    }
    for (int64_t f = 0; f < F; ++f) {
      o[f] = ninf;
      a[f] = none_val<A>();
    }
    for (int32_t k = b; k < e; ++k) {
      const float* x = X + (int64_t)g->col[k] * ldx;
      const float w = g->ew ? g->ew[g->eslot ? g->eslot[k] : k] : 1.f;
      const A pos = (A)(k - b);
      for (int64_t f = 0; f < F; ++f) {
        const float m = g->ew ? x[f] * w : x[f];
        if (m > o[f]) {
          o[f] = m;
          a[f] = pos;
        }
      }
    }
    // DGL's _gspmm masks +-inf of a min/max reduce to 0 (replace_inf_with_zero)
    for (int64_t f = 0; f < F; ++f)
      if (std::isinf(o[f])) o[f] = 0.f;
  }
}

template <typename A>
void max_bwd(const pg_csr_t* g, const pg_csr_t* gt, const A* arg, int64_t lda, const float* dout,
             int64_t ldd, int64_t F, const float* mask, int64_t ldm, float* dx, int64_t ldx) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t u = 0; u < gt->n_rows; ++u) {
    float* d = dx + u * ldx;
    for (int64_t f = 0; f < F; ++f) d[f] = 0.f;
    for (int32_t t = gt->ptr[u]; t < gt->ptr[u + 1]; ++t) {
      const int32_t v = gt->col[t];
      const int32_t j = gt->eslot ? gt->eslot[t] : t;
      const A pos = (A)(j - g->ptr[v]);
      const float w = g->ew ? g->ew[j] : 1.f;
      const A* a = arg + (int64_t)v * lda;
      const float* go = dout + (int64_t)v * ldd;
      for (int64_t f = 0; f < F; ++f)
        if (a[f] == pos) d[f] += g->ew ? w * go[f] : go[f];
    }
    if (mask) {
      const float* m = mask + u * ldm;
      for (int64_t f = 0; f < F; ++f)
        if (!(m[f] > 0.f)) d[f] = 0.f;
    }
  }
}

// A = void: the plain form (no records read)
template <typename A>
void sddmm_dot(const pg_csr_t* g, const float* D, int64_t ldd, const float* X, int64_t ldx,
               int64_t F, bool mean, const A* arg, int64_t lda, float* de) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const int32_t b = g->ptr[v], e = g->ptr[v + 1];
    const float* d = D + v * ldd;
    const float deg = (float)(e - b);
    for (int32_t k = b; k < e; ++k) {
      const float* x = X + (int64_t)g->col[k] * ldx;
      float acc = 0.f;
      if constexpr (std::is_void<A>::value) {
        for (int64_t f = 0; f < F; ++f) acc += d[f] * x[f];
      } else {
        const A* a = arg + v * lda;
        const A pos = (A)(k - b);  // never the "none" value: k - b < max_deg
        for (int64_t f = 0; f < F; ++f)
          if (a[f] == pos) acc += d[f] * x[f];
      }
      de[k] = mean ? acc / deg : acc;
    }
  }
}

inline float gop(int op, float l, float r) {
  switch (op) {
    case PG_OP_ADD: return l + r;
    case PG_OP_SUB: return l - r;
    case PG_OP_MUL: return l * r;
    case PG_OP_DIV: return l / r;
    case PG_OP_COPY_LHS: return l;
    default: return r;
  }
}

// operand row of entry k of row v: the gathered row, the owning row or the edge row
inline const float* gop_row(const float* base, int64_t ld, int tgt, int32_t c, int64_t v, int32_t e) {
  if (!base) return nullptr;
  return base + (tgt == PG_TGT_U ? (int64_t)c : tgt == PG_TGT_V ? v : (int64_t)e) * ld;
}

inline void put_arg(void* arg, int arg_kind, int64_t i, int pos) {
  if (arg_kind == PG_ARG_U16) ((uint16_t*)arg)[i] = (uint16_t)pos;
  else ((int32_t*)arg)[i] = pos;
}
inline int get_arg(const void* arg, int arg_kind, int64_t i) {
  if (arg_kind == PG_ARG_U16) {
    const uint16_t a = ((const uint16_t*)arg)[i];
    return a == 0xFFFF ? -1 : (int)a;
  }
  return ((const int32_t*)arg)[i];
}

}  // namespace

extern "C" {

int pg_gspmm_cpu(const pg_csr_t* g, int op, int reduce, const float* L, int64_t ldl, int lt,
                 const float* R, int64_t ldr, int rt, const int32_t* eidx, int64_t F,
                 int norm_mode, float* out, int64_t ldo, void* argpos, int64_t lda, int arg_kind) {
  PG_TRY(pg::check_csr(g, "pg_gspmm_cpu", false));
  if (reduce < PG_RED_SUM || reduce > PG_RED_MIN)
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm_cpu: bad reduce %d", reduce);
  const bool sum = reduce == PG_RED_SUM;
  if (sum) argpos = nullptr;
  PG_TRY(pg::check_gop(g, "pg_gspmm_cpu", op, ldl, lt, ldr, rt, F, ldo, false, argpos, lda, arg_kind));
  if (norm_mode < 0 || norm_mode > 1 || (norm_mode == 1 && !sum))
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm_cpu: bad norm_mode %d", norm_mode);
  if (F == 0 || g->n_rows == 0) return pg::ok();
  const bool ul = pg::gop_reads_lhs(op), ur = pg::gop_reads_rhs(op);
  if (!out || (g->nnz > 0 && ((ul && !L) || (ur && !R))))
    return pg::set_error(PG_ERR_INVALID, "pg_gspmm_cpu: NULL buffer");
  if (!ul) L = nullptr;
  if (!ur) R = nullptr;
  const int32_t* emap = eidx ? eidx : g->eslot;
  const float inf = std::numeric_limits<float>::infinity();
  const float init = sum ? 0.f : (reduce == PG_RED_MIN ? inf : -inf);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    float* o = out + v * ldo;
    const int32_t b = g->ptr[v], e = g->ptr[v + 1];
    for (int64_t f = 0; f < F; ++f) o[f] = init;
    if (argpos)
      for (int64_t f = 0; f < F; ++f) put_arg(argpos, arg_kind, v * lda + f, -1);
    for (int32_t k = b; k < e; ++k) {
      const int32_t ek = emap ? emap[k] : k;
      const float* l = gop_row(L, ldl, lt, g->col[k], v, ek);
      const float* r = gop_row(R, ldr, rt, g->col[k], v, ek);
      for (int64_t f = 0; f < F; ++f) {
        const float m = gop(op, l ? l[f] : 0.f, r ? r[f] : 0.f);
        if (sum) {
          o[f] += m;
        } else if (reduce == PG_RED_MIN ? m < o[f] : m > o[f]) {
          o[f] = m;
          if (argpos) put_arg(argpos, arg_kind, v * lda + f, k - b);
        }
      }
    }
    if (sum) {
      if (norm_mode == 1 && e > b) {
        const float d = (float)(e - b);
        for (int64_t f = 0; f < F; ++f) o[f] = o[f] / d;
      }
    } else {
      for (int64_t f = 0; f < F; ++f)
        if (std::isinf(o[f])) o[f] = 0.f;
    }
  }
  return pg::ok();
}

int pg_gsddmm_cpu(const pg_csr_t* g, int op, const float* L, int64_t ldl, int lt, const float* R,
                  int64_t ldr, int rt, const int32_t* eidx, int64_t F, float* out, int64_t ldo,
                  const void* argpos, int64_t lda, int arg_kind) {
  PG_TRY(pg::check_csr(g, "pg_gsddmm_cpu", false));
  PG_TRY(pg::check_gop(g, "pg_gsddmm_cpu", op, ldl, lt, ldr, rt, F, ldo, true, argpos, lda, arg_kind));
  if (F == 0 || g->n_rows == 0 || g->nnz == 0) return pg::ok();
  const bool ul = pg::gop_reads_lhs(op), ur = pg::gop_reads_rhs(op);
  if (!out || (ul && !L) || (ur && !R)) return pg::set_error(PG_ERR_INVALID, "pg_gsddmm_cpu: NULL buffer");
  if ((ul && out == L) || (ur && out == R))
    return pg::set_error(PG_ERR_INVALID, "pg_gsddmm_cpu: the output aliases an input");
  if (!ul) L = nullptr;
  if (!ur) R = nullptr;
  const int32_t* emap = eidx ? eidx : g->eslot;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const int32_t b = g->ptr[v];
    for (int32_t k = b; k < g->ptr[v + 1]; ++k) {
      const int32_t ek = emap ? emap[k] : k;
      const float* l = gop_row(L, ldl, lt, g->col[k], v, ek);
      const float* r = gop_row(R, ldr, rt, g->col[k], v, ek);
      float* o = out + (int64_t)ek * ldo;
      for (int64_t f = 0; f < F; ++f) {
        const bool take = !argpos || get_arg(argpos, arg_kind, v * lda + f) == k - b;
        o[f] = take ? gop(op, l ? l[f] : 0.f, r ? r[f] : 0.f) : 0.f;
      }
    }
  }
  return pg::ok();
}

int pg_spmm_max_fwd_cpu(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, float* out,
                        int64_t ldo, void* argpos, int64_t lda, int arg_kind) {
  PG_TRY(pg::check_csr(g, "pg_spmm_max_fwd_cpu", false));
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd_cpu: bad arg_kind %d", arg_kind);
  if (F < 0 || ldx < F || ldo < F || lda < F)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd_cpu: bad F/leading dims");
  if (arg_kind == PG_ARG_U16 && g->max_deg >= 0xFFFF)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_fwd_cpu: degree too large for u16");
  if (arg_kind == PG_ARG_U16)
    max_fwd<uint16_t>(g, X, ldx, F, out, ldo, (uint16_t*)argpos, lda);
  else
    max_fwd<int32_t>(g, X, ldx, F, out, ldo, (int32_t*)argpos, lda);
  return pg::ok();
}

int pg_spmm_max_bwd_cpu(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                        int arg_kind, const float* dout, int64_t ldd, int64_t F,
                        const float* mask_src, int64_t ldm, float* dx, int64_t ldx) {
  PG_TRY(pg::check_csr(g, "pg_spmm_max_bwd_cpu", false));
  PG_TRY(pg::check_csr(gt, "pg_spmm_max_bwd_cpu", false));
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd_cpu: bad arg_kind %d", arg_kind);
  if (F < 0 || ldd < F || ldx < F || lda < F || (mask_src && ldm < F))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd_cpu: bad F/leading dims");
  if (arg_kind == PG_ARG_U16)
    max_bwd<uint16_t>(g, gt, (const uint16_t*)argpos, lda, dout, ldd, F, mask_src, ldm, dx, ldx);
  else
    max_bwd<int32_t>(g, gt, (const int32_t*)argpos, lda, dout, ldd, F, mask_src, ldm, dx, ldx);
  return pg::ok();
}

int pg_spmm_sum_cpu(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, int norm_mode,
                    const int32_t* norm_ptr, float* out, int64_t ldo) {
  PG_TRY(pg::check_csr(g, "pg_spmm_sum_cpu", false));
  if (F < 0 || ldx < F || ldo < F)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_cpu: bad F/leading dims");
  if (norm_mode < 0 || norm_mode > 2 || (norm_mode == 2 && !norm_ptr))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_cpu: bad norm_mode %d", norm_mode);
  if (F == 0 || g->n_rows == 0) return pg::ok();
  if (!X || !out) return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_cpu: NULL buffer");
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t r = 0; r < g->n_rows; ++r) {
    float* o = out + r * ldo;
    for (int64_t f = 0; f < F; ++f) o[f] = 0.f;
    const int32_t b = g->ptr[r], e = g->ptr[r + 1];
    for (int32_t k = b; k < e; ++k) {
      const int32_t c = g->col[k];
      const float* x = X + (int64_t)c * ldx;
      const float w = g->ew ? g->ew[g->eslot ? g->eslot[k] : k] : 1.f;
      const float dc = norm_mode == 2 ? (float)(norm_ptr[c + 1] - norm_ptr[c]) : 1.f;
      for (int64_t f = 0; f < F; ++f) {
        float t = g->ew ? x[f] * w : x[f];
        if (norm_mode == 2) t = t / dc;
        o[f] += t;
      }
    }
    if (norm_mode == 1 && e > b) {
      const float d = (float)(e - b);
      for (int64_t f = 0; f < F; ++f) o[f] = o[f] / d;
    }
  }
  return pg::ok();
}

int pg_argpos_to_src_cpu(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                         int64_t F, int64_t* argx, int64_t ldx) {
  PG_TRY(pg::check_csr(g, "pg_argpos_to_src_cpu", false));
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_argpos_to_src_cpu: bad arg_kind %d", arg_kind);
#pragma omp parallel for
  for (int64_t v = 0; v < g->n_rows; ++v) {
    for (int64_t f = 0; f < F; ++f) {
      int64_t p;
      if (arg_kind == PG_ARG_U16) {
        const uint16_t a = ((const uint16_t*)argpos)[v * lda + f];
        p = a == 0xFFFF ? -1 : (int64_t)a;
      } else {
        p = ((const int32_t*)argpos)[v * lda + f];
      }
      argx[v * ldx + f] = p < 0 ? -1 : (int64_t)g->col[g->ptr[v] + p];
    }
  }
  return pg::ok();
}

int pg_sddmm_dot_cpu(const pg_csr_t* g, const float* D, int64_t ldd, const float* X, int64_t ldx,
                     int64_t F, int norm_mode, const void* argpos, int64_t lda, int arg_kind,
                     float* de) {
  PG_TRY(pg::check_csr(g, "pg_sddmm_dot_cpu", false));
  PG_TRY(pg::check_sddmm(g, "pg_sddmm_dot_cpu", ldd, ldx, F, norm_mode, argpos, lda, arg_kind));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!de || (F > 0 && (!D || !X))) return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot_cpu: NULL buffer");
  const bool mean = norm_mode == 1;
  if (!argpos)
    sddmm_dot<void>(g, D, ldd, X, ldx, F, mean, nullptr, 0, de);
  else if ((arg_kind & ~PG_ARG_DEAD_NONE) == PG_ARG_U16)
    sddmm_dot<uint16_t>(g, D, ldd, X, ldx, F, mean, (const uint16_t*)argpos, lda, de);
  else
    sddmm_dot<int32_t>(g, D, ldd, X, ldx, F, mean, (const int32_t*)argpos, lda, de);
  return pg::ok();
}

// ---- multi-head attention: row reductions in ascending k, dots in ascending j ----------
int pg_edge_softmax_fwd_cpu(const pg_csr_t* g, const float* s, int64_t lds, int32_t H, float* a, int64_t lda) {
  PG_TRY(pg::check_csr(g, "pg_edge_softmax_fwd_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_edge_softmax_fwd_cpu", H, {lds, lda}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!s || !a) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_fwd_cpu: NULL buffer");
  if (s == a) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_fwd_cpu: the output aliases an input");
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const int32_t b = g->ptr[v], e = g->ptr[v + 1];
    for (int32_t h = 0; h < H; ++h) {
      float m = -std::numeric_limits<float>::infinity();
      for (int32_t k = b; k < e; ++k) m = std::fmax(m, s[k * lds + h]);
      float sum = 0.f;
      for (int32_t k = b; k < e; ++k) {
        const float t = std::exp(s[k * lds + h] - m);
        a[k * lda + h] = t;
        sum += t;
      }
      for (int32_t k = b; k < e; ++k) a[k * lda + h] = a[k * lda + h] / sum;
    }
  }
  return pg::ok();
}

int pg_edge_softmax_bwd_cpu(const pg_csr_t* g, const float* a, int64_t lda, const float* da, int64_t ldda,
                            int32_t H, float* ds, int64_t ldds) {
  PG_TRY(pg::check_csr(g, "pg_edge_softmax_bwd_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_edge_softmax_bwd_cpu", H, {lda, ldda, ldds}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!a || !da || !ds) return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_bwd_cpu: NULL buffer");
  if (ds == a || ds == da)
    return pg::set_error(PG_ERR_INVALID, "pg_edge_softmax_bwd_cpu: the output aliases an input");
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const int32_t b = g->ptr[v], e = g->ptr[v + 1];
    for (int32_t h = 0; h < H; ++h) {
      float sum = 0.f;
      for (int32_t k = b; k < e; ++k) sum += a[k * lda + h] * da[k * ldda + h];
      for (int32_t k = b; k < e; ++k) ds[k * ldds + h] = a[k * lda + h] * (da[k * ldda + h] - sum);
    }
  }
  return pg::ok();
}

int pg_spmm_sum_heads_cpu(const pg_csr_t* g, const float* A, int64_t lda, int32_t H, const float* X, int64_t ldx,
                          int64_t Fh, float* out, int64_t ldo) {
  PG_TRY(pg::check_csr(g, "pg_spmm_sum_heads_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_spmm_sum_heads_cpu", H, {lda}));
  PG_TRY(pg::check_head_features("pg_spmm_sum_heads_cpu", H, Fh, {ldx, ldo}));
  if (g->n_rows == 0) return pg::ok();
  if (!X || !out || (g->nnz > 0 && !A)) return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_heads_cpu: NULL buffer");
  if (out == X || out == A)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_sum_heads_cpu: the output aliases an input");
  const int64_t F = (int64_t)H * Fh;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t r = 0; r < g->n_rows; ++r) {
    float* o = out + r * ldo;
    for (int64_t f = 0; f < F; ++f) o[f] = 0.f;
    for (int32_t k = g->ptr[r]; k < g->ptr[r + 1]; ++k) {
      const float* x = X + (int64_t)g->col[k] * ldx;
      const float* w = A + (int64_t)(g->eslot ? g->eslot[k] : k) * lda;
      for (int32_t h = 0; h < H; ++h)
        for (int64_t j = 0; j < Fh; ++j) o[h * Fh + j] += x[h * Fh + j] * w[h];
    }
  }
  return pg::ok();
}

int pg_sddmm_dot_heads_cpu(const pg_csr_t* g, const float* Dm, int64_t ldd, const float* X, int64_t ldx,
                           int32_t H, int64_t Fh, float* de, int64_t lde) {
  PG_TRY(pg::check_csr(g, "pg_sddmm_dot_heads_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_sddmm_dot_heads_cpu", H, {lde}));
  PG_TRY(pg::check_head_features("pg_sddmm_dot_heads_cpu", H, Fh, {ldd, ldx}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!de || !Dm || !X) return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot_heads_cpu: NULL buffer");
  if (de == Dm || de == X)
    return pg::set_error(PG_ERR_INVALID, "pg_sddmm_dot_heads_cpu: the output aliases an input");
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const float* d = Dm + v * ldd;
    for (int32_t k = g->ptr[v]; k < g->ptr[v + 1]; ++k) {
      const float* x = X + (int64_t)g->col[k] * ldx;
      for (int32_t h = 0; h < H; ++h) {
        float acc = 0.f;
        for (int64_t j = 0; j < Fh; ++j) acc += d[h * Fh + j] * x[h * Fh + j];
        de[(int64_t)k * lde + h] = acc;
      }
    }
  }
  return pg::ok();
}

// ---- GATv2 attention scores: t_k recomputed from the two node rows, nothing edge-sized ------
int pg_gatv2_score_cpu(const pg_csr_t* g, const float* XL, int64_t ldl, const float* XR, int64_t ldr,
                       const float* attn, int32_t H, int64_t Fh, float slope, float* s, int64_t lds) {
  PG_TRY(pg::check_csr(g, "pg_gatv2_score_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_gatv2_score_cpu", H, {lds}));
  PG_TRY(pg::check_head_features("pg_gatv2_score_cpu", H, Fh, {ldl, ldr}));
  if (g->nnz == 0 || g->n_rows == 0) return pg::ok();
  if (!s || !XL || !XR || !attn) return pg::set_error(PG_ERR_INVALID, "pg_gatv2_score_cpu: NULL buffer");
  if (s == XL || s == XR || s == attn)
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_score_cpu: the output aliases an input");
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t v = 0; v < g->n_rows; ++v) {
    const float* r = XR + v * ldr;
    for (int32_t k = g->ptr[v]; k < g->ptr[v + 1]; ++k) {
      const float* l = XL + (int64_t)g->col[k] * ldl;
      for (int32_t h = 0; h < H; ++h) {
        float acc = 0.f;
        for (int64_t d = h * Fh; d < (h + 1) * Fh; ++d) {
          const float t = l[d] + r[d];
          acc += attn[d] * (t > 0.f ? t : slope * t);
        }
        s[(int64_t)k * lds + h] = acc;
      }
    }
  }
  return pg::ok();
}

int pg_gatv2_bwd_cpu(const pg_csr_t* g, const float* ds, int64_t ldds, const float* Xown, int64_t ldown,
                     const float* Xgat, int64_t ldgat, const float* attn, int32_t H, int64_t Fh, float slope,
                     float* dXown, int64_t lddx, float* dattn) {
  PG_TRY(pg::check_csr(g, "pg_gatv2_bwd_cpu", false));
  PG_TRY(pg::check_heads(g, "pg_gatv2_bwd_cpu", H, {ldds}));
  PG_TRY(pg::check_head_features("pg_gatv2_bwd_cpu", H, Fh, {ldown, ldgat, dXown ? lddx : (int64_t)H * Fh}));
  if (!dXown && !dattn) return pg::ok();
  const int64_t F = (int64_t)H * Fh;
  if (g->n_rows == 0) {
    if (dattn)
      for (int64_t f = 0; f < F; ++f) dattn[f] = 0.f;
    return pg::ok();
  }
  if (!Xown || !Xgat || !attn || (g->nnz > 0 && !ds))
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_bwd_cpu: NULL buffer");
  if ((dXown && (dXown == Xown || dXown == Xgat || dXown == attn || dXown == ds)) ||
      (dattn && (dattn == Xown || dattn == Xgat || dattn == attn || dattn == ds || dattn == dXown)))
    return pg::set_error(PG_ERR_INVALID, "pg_gatv2_bwd_cpu: an output aliases an input");
  if (dXown) {  // attn factored out of the row sum, as the device kernel
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t r = 0; r < g->n_rows; ++r) {
      const float* own = Xown + r * ldown;
      float* o = dXown + r * lddx;
      for (int64_t f = 0; f < F; ++f) o[f] = 0.f;
      for (int32_t k = g->ptr[r]; k < g->ptr[r + 1]; ++k) {
        const float* x = Xgat + (int64_t)g->col[k] * ldgat;
        const float* w = ds + (int64_t)(g->eslot ? g->eslot[k] : k) * ldds;
        for (int32_t h = 0; h < H; ++h) {
          const float wsl = w[h] * slope;
          for (int64_t f = h * Fh; f < (h + 1) * Fh; ++f) o[f] += (x[f] + own[f]) > 0.f ? w[h] : wsl;
        }
      }
      for (int64_t f = 0; f < F; ++f) o[f] = attn[f] * o[f];
    }
  }
  if (dattn) {  // a column's terms in ascending k, columns in parallel
#pragma omp parallel for schedule(static)
    for (int64_t f = 0; f < F; ++f) {
      const int64_t h = f / Fh;
      float acc = 0.f;
      for (int64_t r = 0; r < g->n_rows; ++r) {
        const float own = Xown[r * ldown + f];
        for (int32_t k = g->ptr[r]; k < g->ptr[r + 1]; ++k) {
          const float t = Xgat[(int64_t)g->col[k] * ldgat + f] + own;
          acc += ds[(int64_t)(g->eslot ? g->eslot[k] : k) * ldds + h] * (t > 0.f ? t : slope * t);
        }
      }
      dattn[f] = acc;
    }
  }
  return pg::ok();
}

// ---- neighbour sampling and block compaction: the statement of the device results
static inline int32_t sample_row_count(const pg_csr_t* g, int32_t s, int32_t fanout) {
  if (s < 0 || s >= g->n_rows) return 0;
  const int32_t d = std::max(0, g->ptr[s + 1] - g->ptr[s]);
  return (fanout >= 0 && d > fanout) ? fanout : d;
}

int pg_sample_count_cpu(const pg_csr_t* g, const int32_t* seeds, int64_t n_seeds, int32_t fanout,
                        int32_t* out_ptr) {
  const char* who = "pg_sample_count_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  int64_t run = 0;
  for (int64_t i = 0; i < n_seeds; ++i) {
    out_ptr[i] = (int32_t)run;
    run += sample_row_count(g, seeds[i], fanout);
    if (run > INT32_MAX) return pg::set_error(PG_ERR_UNSUPPORTED, "%s: more than 2^31 sampled entries", who);
  }
  out_ptr[n_seeds] = (int32_t)run;
  return pg::ok();
}

int pg_sample_fill_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                       int32_t fanout, uint64_t seed64, const int32_t* out_ptr, int32_t* out_col,
                       int32_t* out_eid) {
  const char* who = "pg_sample_fill_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  if (n_seeds == 0 || g->nnz == 0 || fanout == 0) return pg::ok();
  if (!out_col || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  bool failed = false;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n_seeds; ++i) {
    const int32_t s = seeds[i];
    if (s < 0 || s >= g->n_rows) continue;
    const int32_t b = g->ptr[s], deg = g->ptr[s + 1] - b;
    if (deg <= 0) continue;
    const int64_t o = out_ptr[i];
    if (fanout < 0 || deg <= fanout) {
      for (int32_t j = 0; j < deg; ++j) {
        out_col[o + j] = g->col[b + j];
        out_eid[o + j] = eid ? eid[b + j] : b + j;
      }
      continue;
    }
    // the fanout smallest (key, edge id) pairs; positions ascend with the edge ids of a row
    std::vector<std::pair<uint32_t, int32_t>> kp;
    try {
      kp.resize((size_t)deg);
    } catch (const std::bad_alloc&) {
      failed = true;
      continue;
    }
    for (int32_t j = 0; j < deg; ++j) kp[(size_t)j] = {pg::sample_key(seed64, eid ? eid[b + j] : b + j), j};
    std::nth_element(kp.begin(), kp.begin() + (fanout - 1), kp.end());
    std::vector<int32_t> keep((size_t)fanout);
    for (int32_t q = 0; q < fanout; ++q) keep[(size_t)q] = kp[(size_t)q].second;
    std::sort(keep.begin(), keep.end());
    for (int32_t q = 0; q < fanout; ++q) {
      const int32_t j = keep[(size_t)q];
      out_col[o + q] = g->col[b + j];
      out_eid[o + q] = eid ? eid[b + j] : b + j;
    }
  }
  if (failed) return pg::set_error(PG_ERR_HOST, "%s: out of host memory", who);
  return pg::ok();
}

int pg_block_compact_cpu(const int32_t* dst_ids, int64_t n_dst, const int32_t* col, int64_t nnz,
                         int64_t n_parent, int32_t* src_ids, int32_t* col_local, int32_t* n_src) {
  const char* who = "pg_block_compact_cpu";
  if (n_dst < 0 || nnz < 0 || n_parent < 0 || n_dst + nnz > INT32_MAX - 1 || n_parent > INT32_MAX)
    return pg::set_error(PG_ERR_INVALID, "%s: bad sizes", who);
  if (!n_src || (n_dst > 0 && !dst_ids) || (nnz > 0 && (!col || !col_local)) || (n_dst + nnz > 0 && !src_ids))
    return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  std::vector<int32_t> local;
  try {
    local.assign((size_t)n_parent, -1);
  } catch (const std::bad_alloc&) {
    return pg::set_error(PG_ERR_HOST, "%s: out of host memory", who);
  }
  for (int64_t i = 0; i < n_dst; ++i)
    if (dst_ids[i] < 0 || dst_ids[i] >= n_parent) return *n_src = -2, pg::ok();
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= n_parent) return *n_src = -2, pg::ok();
  int32_t n = 0;
  for (int64_t i = 0; i < n_dst; ++i) {
    if (local[(size_t)dst_ids[i]] >= 0) return *n_src = -1, pg::ok();
    local[(size_t)dst_ids[i]] = n;
    src_ids[n++] = dst_ids[i];
  }
  for (int64_t k = 0; k < nnz; ++k) {
    int32_t& l = local[(size_t)col[k]];
    if (l < 0) {
      l = n;
      src_ids[n++] = col[k];
    }
    col_local[k] = l;
  }
  *n_src = n;
  return pg::ok();
}

// ---- link-prediction mini-batches: the statement of the device results
static inline bool edge_excluded(const uint32_t* bits, int64_t n_ids, int32_t e) {
  return bits && e >= 0 && e < n_ids && ((bits[e >> 5] >> (e & 31)) & 1u);
}

int pg_edge_bits_update_cpu(uint32_t* bits, int64_t n_edge_ids, const int32_t* eids, int64_t n, int set,
                            int32_t* status) {
  const char* who = "pg_edge_bits_update_cpu";
  if (n_edge_ids < 0 || n_edge_ids > INT32_MAX || n < 0 || n > INT32_MAX)
    return pg::set_error(PG_ERR_INVALID, "%s: bad sizes", who);
  if (n == 0) return pg::ok();
  if (!eids || (n_edge_ids > 0 && !bits)) return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t e = eids[i];
    if (e < 0 || e >= n_edge_ids) {
      if (status) *status = -2;
      continue;
    }
    const uint32_t m = 1u << (e & 31);
    if (set)
      bits[e >> 5] |= m;
    else
      bits[e >> 5] &= ~m;
  }
  return pg::ok();
}

// the positions of row s (in range) whose edge id is not excluded
static inline int32_t remaining_in_row(const pg_csr_t* g, const int32_t* eid, int32_t s, const uint32_t* bits) {
  const int32_t b = g->ptr[s], deg = g->ptr[s + 1] - b;
  int32_t rem = 0;
  for (int32_t j = 0; j < deg; ++j) rem += !edge_excluded(bits, g->nnz, eid ? eid[b + j] : b + j);
  return rem;
}

int pg_sample_count_excl_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                             int32_t fanout, const uint32_t* excl_bits, int32_t* out_ptr) {
  const char* who = "pg_sample_count_excl_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  int64_t run = 0;
  for (int64_t i = 0; i < n_seeds; ++i) {
    out_ptr[i] = (int32_t)run;
    const int32_t s = seeds[i];
    if (s < 0 || s >= g->n_rows) continue;
    const int32_t rem = remaining_in_row(g, eid, s, excl_bits);
    run += (fanout >= 0 && rem > fanout) ? fanout : rem;
    if (run > INT32_MAX) return pg::set_error(PG_ERR_UNSUPPORTED, "%s: more than 2^31 sampled entries", who);
  }
  out_ptr[n_seeds] = (int32_t)run;
  return pg::ok();
}

int pg_sample_fill_excl_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                            int32_t fanout, uint64_t seed64, const uint32_t* excl_bits, const int32_t* out_ptr,
                            int32_t* out_col, int32_t* out_eid) {
  const char* who = "pg_sample_fill_excl_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_seeds < 0 || n_seeds > INT32_MAX || !out_ptr || (n_seeds > 0 && !seeds))
    return pg::set_error(PG_ERR_INVALID, "%s: bad seeds / out_ptr", who);
  if (n_seeds == 0 || g->nnz == 0 || fanout == 0) return pg::ok();
  if (!out_col || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  bool failed = false;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n_seeds; ++i) {
    const int32_t s = seeds[i];
    if (s < 0 || s >= g->n_rows) continue;
    const int32_t b = g->ptr[s], deg = g->ptr[s + 1] - b;
    if (deg <= 0) continue;
    const int64_t o = out_ptr[i];
    // the (key, position) pairs that remain; positions ascend with the edge ids of a row
    std::vector<std::pair<uint32_t, int32_t>> kp;
    try {
      kp.reserve((size_t)deg);
    } catch (const std::bad_alloc&) {
      failed = true;
      continue;
    }
    for (int32_t j = 0; j < deg; ++j) {
      const int32_t e = eid ? eid[b + j] : b + j;
      if (!edge_excluded(excl_bits, g->nnz, e)) kp.push_back({pg::sample_key(seed64, e), j});
    }
    const int32_t rem = (int32_t)kp.size();
    int32_t keep = rem;
    if (fanout >= 0 && rem > fanout) {
      std::nth_element(kp.begin(), kp.begin() + (fanout - 1), kp.end());
      keep = fanout;
    }
    std::sort(kp.begin(), kp.begin() + keep,
              [](const std::pair<uint32_t, int32_t>& x, const std::pair<uint32_t, int32_t>& y) {
                return x.second < y.second;
              });
    for (int32_t q = 0; q < keep; ++q) {
      const int32_t j = kp[(size_t)q].second;
      out_col[o + q] = g->col[b + j];
      out_eid[o + q] = eid ? eid[b + j] : b + j;
    }
  }
  if (failed) return pg::set_error(PG_ERR_HOST, "%s: out of host memory", who);
  return pg::ok();
}

// the slot of the first entry of row v (in range) whose column is u, -1: none
static inline int32_t row_find(const pg_csr_t* g, int32_t v, int32_t u) {
  for (int32_t k = g->ptr[v]; k < g->ptr[v + 1]; ++k)
    if (g->col[k] == u) return k;
  return -1;
}

int pg_edge_lookup_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* u, const int32_t* v, int64_t n,
                       int32_t* out_eid) {
  const char* who = "pg_edge_lookup_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n < 0 || n > INT32_MAX) return pg::set_error(PG_ERR_INVALID, "%s: bad n", who);
  if (n == 0) return pg::ok();
  if (!u || !v || !out_eid) return pg::set_error(PG_ERR_INVALID, "%s: NULL buffer", who);
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i = 0; i < n; ++i) {
    int32_t slot = -1;
    if (u[i] >= 0 && u[i] < g->n_cols && v[i] >= 0 && v[i] < g->n_rows) slot = row_find(g, v[i], u[i]);
    out_eid[i] = slot < 0 ? -1 : (eid ? eid[slot] : slot);
  }
  return pg::ok();
}

int pg_negative_sample_cpu(const pg_csr_t* g, const int32_t* pos_src, const int32_t* pos_id, int64_t n_pos,
                           int32_t k, int32_t tries, int flags, uint64_t seed64, int32_t* neg_src,
                           int32_t* neg_dst, int32_t* n_fail) {
  const char* who = "pg_negative_sample_cpu";
  PG_TRY(pg::check_csr(g, who, false));
  if (n_pos < 0 || k < 1 || tries < 1 || tries > 64 || n_pos * (int64_t)k > INT32_MAX ||
      (flags & ~(PG_NEG_REJECT_EDGE | PG_NEG_REJECT_SELF)))
    return pg::set_error(PG_ERR_INVALID, "%s: n_pos >= 0, k >= 1, 1 <= tries <= 64, n_pos k < 2^31, known flags", who);
  if (!n_fail || (n_pos > 0 && (!neg_src || !neg_dst))) return pg::set_error(PG_ERR_INVALID, "%s: NULL output", who);
  int64_t fails = 0;
  const int64_t n_slots = n_pos * k;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : fails)
  for (int64_t slot = 0; slot < n_slots; ++slot) {
    const int64_t i = slot / k;
    const int32_t j = (int32_t)(slot - i * k);
    const int32_t id = pos_id ? pos_id[i] : (int32_t)i;
    const int32_t fixed = pos_src ? pos_src[i] : 0;
    int32_t ru = -1, rv = -1;
    const bool can = g->n_rows > 0 && g->n_cols > 0 && fixed >= 0 && fixed < g->n_cols;
    for (int32_t t = 0; can && t < tries; ++t) {
      const int32_t uu = pos_src ? fixed : pg::key_to_range(pg::negative_key(seed64, id, j, t, 0), g->n_cols);
      const int32_t vv = pg::key_to_range(pg::negative_key(seed64, id, j, t, 1), g->n_rows);
      if ((flags & PG_NEG_REJECT_SELF) && uu == vv) continue;
      if ((flags & PG_NEG_REJECT_EDGE) && row_find(g, vv, uu) >= 0) continue;
      ru = uu;
      rv = vv;
      break;
    }
    neg_src[slot] = ru;
    neg_dst[slot] = rv;
    fails += ru < 0;
  }
  *n_fail = (int32_t)fails;
  return pg::ok();
}

}  // extern "C"
