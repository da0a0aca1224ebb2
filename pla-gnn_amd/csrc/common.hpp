// Shared helpers of the plagnn C-ABI: thread-local error text, argument checks,
// launch-error translation. Included by every translation unit of libplagnn.so.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../include/plagnn.h"

namespace pg {

// Thread-local error string returned by pg_last_error_string().
char* error_buffer();
int set_error(int code, const char* fmt, ...);

inline int ok() {
  error_buffer()[0] = '\0';
  return PG_OK;
}

// Arg-kind helpers
inline bool valid_arg_kind(int k) { return k == PG_ARG_U16 || k == PG_ARG_I32; }
inline size_t arg_bytes(int k) { return k == PG_ARG_U16 ? 2 : 4; }

inline int check_csr(const pg_csr_t* g, const char* who, bool need_sched) {
  if (!g) return set_error(PG_ERR_INVALID, "%s: csr descriptor is NULL", who);
  if (g->n_rows < 0 || g->n_cols < 0 || g->nnz < 0)
    return set_error(PG_ERR_INVALID, "%s: negative csr size", who);
  if (g->n_rows > INT32_MAX || g->n_cols > INT32_MAX || g->nnz > INT32_MAX)
    return set_error(PG_ERR_UNSUPPORTED, "%s: csr larger than int32 ids", who);
  if (!g->ptr) return set_error(PG_ERR_INVALID, "%s: csr ptr is NULL", who);
  if (g->nnz > 0 && !g->col) return set_error(PG_ERR_INVALID, "%s: csr col is NULL", who);
  if (need_sched) {
    if (g->n_rows > 0 && (!g->items || g->n_items <= 0))
      return set_error(PG_ERR_INVALID, "%s: csr has no work schedule", who);
    if (g->n_merges > 0 && !g->merges)
      return set_error(PG_ERR_INVALID, "%s: csr merges missing", who);
  }
  return PG_OK;
}

// pg_sddmm_dot[_cpu]: the checks both entry points share (argpos NULL: arg_kind is not read)
inline int check_sddmm(const pg_csr_t* g, const char* who, int64_t ldd, int64_t ldx, int64_t F,
                       int norm_mode, const void* argpos, int64_t lda, int arg_kind) {
  if (F < 0 || ldd < F || ldx < F || (argpos && lda < F))
    return set_error(PG_ERR_INVALID, "%s: bad F/leading dims", who);
  if (norm_mode < 0 || norm_mode > 1)
    return set_error(PG_ERR_INVALID, "%s: bad norm_mode %d", who, norm_mode);
  if (argpos && !valid_arg_kind(arg_kind & ~PG_ARG_DEAD_NONE))
    return set_error(PG_ERR_INVALID, "%s: bad arg_kind %d", who, arg_kind);
  if (argpos && (arg_kind & ~PG_ARG_DEAD_NONE) == PG_ARG_U16 && g->max_deg >= 0xFFFF)
    return set_error(PG_ERR_INVALID, "%s: degree too large for u16 records", who);
  return PG_OK;
}

// log2 of a power of two, -1 for anything else
inline int log2_exact(int32_t x) {
  if (x <= 0 || (x & (x - 1)) != 0) return -1;
  int l = 0;
  while ((1 << l) < x) ++l;
  return l;
}

// the multi-head entry points ([_cpu] too): 1 <= H <= 64 heads, edge features [nnz][ld >= H]
// whose nnz * H values are indexed in int32
inline int check_heads(const pg_csr_t* g, const char* who, int32_t H, std::initializer_list<int64_t> edge_lds) {
  if (H < 1 || H > 64) return set_error(PG_ERR_INVALID, "%s: H = %d heads, 1 .. 64 supported", who, (int)H);
  for (int64_t ld : edge_lds)
    if (ld < H) return set_error(PG_ERR_INVALID, "%s: bad edge leading dims", who);
  if (g->nnz * H > INT32_MAX) return set_error(PG_ERR_UNSUPPORTED, "%s: nnz * H larger than int32", who);
  return PG_OK;
}

// node features [n][ld >= H * Fh], H * Fh within pg_spmm_sum's range
inline int check_head_features(const char* who, int32_t H, int64_t Fh, std::initializer_list<int64_t> lds) {
  if (Fh < 1 || Fh > (1 << 30) / H) return set_error(PG_ERR_INVALID, "%s: bad Fh", who);
  for (int64_t ld : lds)
    if (ld < H * Fh) return set_error(PG_ERR_INVALID, "%s: bad F/leading dims", who);
  return PG_OK;
}

// pg_gspmm / pg_gsddmm [_cpu]: operator, targets (allow_v: pg_gsddmm), F and the leading
// dimensions of the operands the operator reads, the record kind when records are passed
inline bool gop_reads_lhs(int op) { return op != PG_OP_COPY_RHS; }
inline bool gop_reads_rhs(int op) { return op != PG_OP_COPY_LHS; }
inline int check_gop(const pg_csr_t* g, const char* who, int op, int64_t ldl, int lt, int64_t ldr,
                     int rt, int64_t F, int64_t ldo, bool allow_v, const void* argpos, int64_t lda,
                     int arg_kind) {
  if (op < PG_OP_ADD || op > PG_OP_COPY_RHS) return set_error(PG_ERR_INVALID, "%s: bad op %d", who, op);
  auto tgt_ok = [&](int t) { return t == PG_TGT_U || t == PG_TGT_E || (allow_v && t == PG_TGT_V); };
  if ((gop_reads_lhs(op) && !tgt_ok(lt)) || (gop_reads_rhs(op) && !tgt_ok(rt)))
    return set_error(PG_ERR_INVALID, "%s: bad operand target (%d, %d)", who, lt, rt);
  if (F < 0 || ldo < F || (gop_reads_lhs(op) && ldl < F) || (gop_reads_rhs(op) && ldr < F) ||
      (argpos && lda < F))
    return set_error(PG_ERR_INVALID, "%s: bad F/leading dims", who);
  if (F > (1 << 23)) return set_error(PG_ERR_UNSUPPORTED, "%s: F too large", who);
  if (argpos && !valid_arg_kind(arg_kind)) return set_error(PG_ERR_INVALID, "%s: bad arg_kind %d", who, arg_kind);
  if (argpos && arg_kind == PG_ARG_U16 && g->max_deg >= 0xFFFF)
    return set_error(PG_ERR_INVALID, "%s: degree too large for u16 records", who);
  return PG_OK;
}

}  // namespace pg

#define PG_TRY(expr)           \
  do {                          \
    int _rc = (expr);           \
    if (_rc != PG_OK) return _rc; \
  } while (0)
