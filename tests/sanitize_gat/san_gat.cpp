// ASan + UBSan driver for the multi-head attention host entry points of csrc/cpu_backend.cpp
// (pg_edge_softmax_fwd_cpu / _bwd_cpu, pg_spmm_sum_heads_cpu on the in-CSR and on its
// transpose, pg_sddmm_dot_heads_cpu) on graphs built through pg_csr_from_coo,
// pg_csr_transpose and the pg_schedule_* calls (csrc/graph.cpp): a hub row, empty rows,
// duplicate edges; H in {1, 3, 8}, padded leading dimensions, exactly-sized buffers. Every
// result is checked against a double-precision loop within the bars of tests/gat_common.py.
// Built by tests/sanitize_gat/Makefile with -fsanitize=address,undefined and run by
// tests/test_sanitize_gat.py as a child process; any sanitizer report ends it with a non-zero
// status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/plagnn.h"

static int failures = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

static void run_case(int64_t n, int64_t e, int64_t hub, int32_t H, int64_t Fh, int64_t pad, int chunk,
                     uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<int64_t> src, dst;
  std::uniform_int_distribution<int64_t> any(0, n - 1), some(0, n - 2);  // node n-1: an empty row
  for (int64_t i = 0; i < e; ++i) {
    src.push_back(any(rng));
    dst.push_back(some(rng));
  }
  for (int64_t i = 0; i < hub; ++i) {  // hub row 0, duplicates allowed
    src.push_back(any(rng));
    dst.push_back(0);
  }
  const int64_t E = (int64_t)src.size();
  std::vector<int32_t> ptr(n + 1), col(E > 0 ? E : 1), eid(E > 0 ? E : 1);
  CHECK(pg_csr_from_coo(src.data(), dst.data(), E, n, n, ptr.data(), col.data(), eid.data()) == 0, "csr");
  std::vector<int32_t> tptr(n + 1), tcol(E > 0 ? E : 1), tslot(E > 0 ? E : 1), tpos(E > 0 ? E : 1);
  CHECK(pg_csr_transpose(ptr.data(), col.data(), n, n, E, tptr.data(), tcol.data(), tslot.data(), tpos.data()) == 0,
        "transpose");
  int64_t ni = 0, nm = 0, ns = 0;
  int32_t md = 0;
  CHECK(pg_schedule_count(ptr.data(), n, chunk, &ni, &nm, &ns, &md) == 0, "schedule count");
  std::vector<int32_t> items(4 * (ni > 0 ? ni : 1)), merges(4 * (nm > 0 ? nm : 1));
  CHECK(pg_schedule_build(ptr.data(), n, chunk, items.data(), merges.data()) == 0, "schedule build");
  pg_csr_t g{n, n, E, ptr.data(), col.data(), nullptr, nullptr, nullptr, items.data(), ni,
             nm ? merges.data() : nullptr, nm, ns, md, chunk};
  pg_csr_t gt{n, n, E, tptr.data(), tcol.data(), tslot.data(), tpos.data(), nullptr, nullptr, 0, nullptr, 0, 0, 0,
              chunk};

  const double u = std::ldexp(1.0, -24), tiny = std::ldexp(1.0, -126);
  const int64_t le = H + pad;  // exactly-sized: the last row holds H values only
  const int64_t esz = E > 0 ? (E - 1) * le + H : 0;
  std::normal_distribution<float> nd;
  std::vector<float> s(esz), a(esz), da(esz), ds(esz);
  for (auto& v : s) v = 3.f * nd(rng);
  for (auto& v : da) v = nd(rng);

  // ---- edge softmax, forward and backward
  CHECK(pg_edge_softmax_fwd_cpu(&g, s.data(), le, H, a.data(), le) == 0, "softmax fwd: %s", pg_last_error_string());
  CHECK(pg_edge_softmax_bwd_cpu(&g, a.data(), le, da.data(), le, H, ds.data(), le) == 0, "softmax bwd: %s",
        pg_last_error_string());
  for (int64_t v = 0; v < n; ++v) {
    const double deg = (double)(ptr[v + 1] - ptr[v]);
    for (int32_t h = 0; h < H; ++h) {
      double m = -INFINITY, tot = 0, dot = 0, S = 0, R = 0;
      for (int32_t k = ptr[v]; k < ptr[v + 1]; ++k) m = std::fmax(m, (double)s[k * le + h]);
      for (int32_t k = ptr[v]; k < ptr[v + 1]; ++k) {
        tot += std::exp((double)s[k * le + h] - m);
        R = std::fmax(R, m - (double)s[k * le + h]);
        dot += (double)a[k * le + h] * (double)da[k * le + h];
        S += std::fabs((double)a[k * le + h] * (double)da[k * le + h]);
      }
      for (int32_t k = ptr[v]; k < ptr[v + 1]; ++k) {
        const double a64 = std::exp((double)s[k * le + h] - m) / tot;
        CHECK(std::fabs(a[k * le + h] - a64) <= (3 * R + deg + 8) * u * a64 + tiny, "softmax fwd slot %d head %d", k, h);
        const double av = a[k * le + h], dv = da[k * le + h];
        CHECK(std::fabs(ds[k * le + h] - av * (dv - dot)) <= u * av * ((deg + 5) * S + 3 * std::fabs(dv)) + tiny,
              "softmax bwd slot %d head %d", k, h);
      }
    }
  }

  // ---- per-head weighted sum on both directions, per-head dots
  const int64_t F = (int64_t)H * Fh, ld = F + pad;
  std::vector<float> X((n - 1) * ld + F), D((n - 1) * ld + F), out((n - 1) * ld + F), outT((n - 1) * ld + F), de(esz);
  for (auto& v : X) v = nd(rng);
  for (auto& v : D) v = nd(rng);
  CHECK(pg_spmm_sum_heads_cpu(&g, s.data(), le, H, X.data(), ld, Fh, out.data(), ld) == 0, "sum heads: %s",
        pg_last_error_string());
  CHECK(pg_spmm_sum_heads_cpu(&gt, s.data(), le, H, X.data(), ld, Fh, outT.data(), ld) == 0, "sum heads T: %s",
        pg_last_error_string());
  CHECK(pg_sddmm_dot_heads_cpu(&g, D.data(), ld, X.data(), ld, H, Fh, de.data(), le) == 0, "dot heads: %s",
        pg_last_error_string());
  for (int dir = 0; dir < 2; ++dir) {
    const pg_csr_t& c = dir ? gt : g;
    const float* o = dir ? outT.data() : out.data();
    for (int64_t r = 0; r < n; ++r) {
      const double deg = (double)(c.ptr[r + 1] - c.ptr[r]);
      for (int64_t f = 0; f < F; ++f) {
        double acc = 0, ab = 0;
        for (int32_t k = c.ptr[r]; k < c.ptr[r + 1]; ++k) {
          const int64_t sl = c.eslot ? c.eslot[k] : k;
          const double t = (double)s[sl * le + f / Fh] * (double)X[(int64_t)c.col[k] * ld + f];
          acc += t;
          ab += std::fabs(t);
        }
        CHECK(std::fabs(o[r * ld + f] - acc) <= (deg + 2) * u * ab + 1e-30, "sum heads dir %d row %d col %d", dir,
              (int)r, (int)f);
        if (deg == 0) CHECK(o[r * ld + f] == 0.f, "empty row is exactly 0");
      }
    }
  }
  for (int64_t v = 0; v < n; ++v)
    for (int32_t k = ptr[v]; k < ptr[v + 1]; ++k)
      for (int32_t h = 0; h < H; ++h) {
        double acc = 0, ab = 0;
        for (int64_t j = 0; j < Fh; ++j) {
          const double t = (double)D[v * ld + h * Fh + j] * (double)X[(int64_t)col[k] * ld + h * Fh + j];
          acc += t;
          ab += std::fabs(t);
        }
        CHECK(std::fabs(de[k * le + h] - acc) <= (Fh + 2) * u * ab + 1e-30, "dot heads slot %d head %d", k, h);
      }

  // argument errors
  CHECK(pg_edge_softmax_fwd_cpu(&g, s.data(), le, 65, a.data(), 65) == PG_ERR_INVALID, "H = 65");
  CHECK(pg_edge_softmax_fwd_cpu(&g, s.data(), H - 1, H, a.data(), le) == PG_ERR_INVALID, "lds");
  CHECK(pg_spmm_sum_heads_cpu(&g, s.data(), le, H, X.data(), F - 1, Fh, out.data(), ld) == PG_ERR_INVALID, "ldx");
  CHECK(pg_sddmm_dot_heads_cpu(&g, D.data(), ld, X.data(), ld, H, 0, de.data(), le) == PG_ERR_INVALID, "Fh = 0");
}

int main() {
  for (int32_t H : {1, 3, 8}) {
    run_case(300, 2000, 0, H, 7, 0, 256, 1 + H);
    run_case(200, 800, 700, H, 12, 3, 256, 2 + H);  // hub row, padded rows
    run_case(64, 200, 2000, H, 5, 1, 64, 3 + H);    // chunk 64: many pieces
    run_case(5, 0, 0, H, 4, 0, 256, 4 + H);         // no edges at all
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize gat ok\n");
  return 0;
}
