// ASan + UBSan driver for pg_sddmm_dot_cpu (csrc/cpu_backend.cpp) on graphs built through
// pg_csr_from_coo and the pg_schedule_* calls (csrc/graph.cpp): a hub row the schedule
// splits, empty rows, duplicate edges; the plain, mean and max forms, the max form with u16
// and with i32 records (from pg_spmm_max_fwd_cpu), odd widths and padded leading dimensions.
// Every result is checked against a double-precision loop within the summation-order bar
// (F + 2) * 2^-24 * sum_f |D X|. Built by tests/sanitize_sddmm/Makefile with
// -fsanitize=address,undefined and run by tests/test_sanitize_sddmm.py as a child process;
// any sanitizer report ends it with a non-zero status.
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

static void run_case(int64_t n, int64_t e, int64_t hub, int64_t F, int64_t pad, int chunk, uint32_t seed) {
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
  int64_t ni = 0, nm = 0, ns = 0;
  int32_t md = 0;
  CHECK(pg_schedule_count(ptr.data(), n, chunk, &ni, &nm, &ns, &md) == 0, "schedule count");
  std::vector<int32_t> items(4 * (ni > 0 ? ni : 1)), merges(4 * (nm > 0 ? nm : 1));
  CHECK(pg_schedule_build(ptr.data(), n, chunk, items.data(), merges.data()) == 0, "schedule build");
  pg_csr_t g{n, n, E, ptr.data(), col.data(), nullptr, nullptr, nullptr, items.data(), ni,
             nm ? merges.data() : nullptr, nm, ns, md, chunk};

  const int64_t ld = F + pad;  // exactly-sized buffers: a read past a row's F columns of the last row is out of bounds
  std::normal_distribution<float> nd;
  std::vector<float> D((n - 1) * ld + F), X((n - 1) * ld + F), out(n * F);
  for (auto& v : D) v = nd(rng);
  for (auto& v : X) v = nd(rng);
  std::vector<uint16_t> a16(n * F);
  std::vector<int32_t> a32(n * F);
  CHECK(pg_spmm_max_fwd_cpu(&g, X.data(), ld, F, out.data(), F, a16.data(), F, PG_ARG_U16) == 0, "max fwd u16: %s",
        pg_last_error_string());
  CHECK(pg_spmm_max_fwd_cpu(&g, X.data(), ld, F, out.data(), F, a32.data(), F, PG_ARG_I32) == 0, "max fwd i32: %s",
        pg_last_error_string());

  std::vector<float> de(E), de_mean(E), de16(E), de32(E);
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 0, nullptr, 0, 0, de.data()) == 0, "plain: %s",
        pg_last_error_string());
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 1, nullptr, 0, 0, de_mean.data()) == 0, "mean: %s",
        pg_last_error_string());
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 0, a16.data(), F, PG_ARG_U16, de16.data()) == 0,
        "max u16: %s", pg_last_error_string());
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 0, a32.data(), F, PG_ARG_I32 | PG_ARG_DEAD_NONE,
                         de32.data()) == 0,
        "max i32: %s", pg_last_error_string());
  const double u = std::ldexp(1.0, -24);
  for (int64_t v = 0; v < n; ++v) {
    const double deg = (double)(ptr[v + 1] - ptr[v]);
    for (int32_t k = ptr[v]; k < ptr[v + 1]; ++k) {
      double s = 0, sa = 0, m = 0, ma = 0;
      for (int64_t f = 0; f < F; ++f) {
        const double t = (double)D[v * ld + f] * (double)X[(int64_t)col[k] * ld + f];
        s += t;
        sa += std::fabs(t);
        if (a32[v * F + f] == k - ptr[v]) {
          m += t;
          ma += std::fabs(t);
        }
        CHECK((int32_t)a16[v * F + f] == a32[v * F + f], "records agree");
      }
      const double bar = (F + 2) * u * sa + 1e-30, bar_m = (F + 2) * u * ma + 1e-30;
      CHECK(std::fabs(de[k] - s) <= bar, "plain slot %d: %g vs %g", k, de[k], s);
      CHECK(std::fabs(de_mean[k] - s / deg) <= bar / deg, "mean slot %d", k);
      CHECK(std::fabs(de16[k] - m) <= bar_m, "max u16 slot %d: %g vs %g", k, de16[k], m);
      CHECK(std::fabs(de32[k] - m) <= bar_m, "max i32 slot %d", k);
    }
  }
  // argument errors leave the output alone
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 2, nullptr, 0, 0, de.data()) == PG_ERR_INVALID, "norm_mode");
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), F - 1, F, 0, nullptr, 0, 0, de.data()) == PG_ERR_INVALID, "ldx");
  CHECK(pg_sddmm_dot_cpu(&g, D.data(), ld, X.data(), ld, F, 0, a16.data(), F, 7, de.data()) == PG_ERR_INVALID, "arg_kind");
}

int main() {
  run_case(300, 2000, 0, 7, 0, 256, 1);
  run_case(200, 800, 700, 40, 3, 256, 2);  // hub row split into three items, padded rows
  run_case(200, 800, 700, 3, 1, 4, 3);     // chunk 4: many short items
  run_case(50, 100, 0, 1, 0, 256, 4);
  run_case(5, 0, 0, 4, 0, 256, 5);         // no edges at all
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize sddmm ok\n");
  return 0;
}
