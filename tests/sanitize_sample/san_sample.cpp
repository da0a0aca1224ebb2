// ASan + UBSan driver for the sampling host entry points of csrc/cpu_backend.cpp
// (pg_sample_count_cpu, pg_sample_fill_cpu, pg_block_compact_cpu) and the host calls
// CSRGraph.from_in_csr makes on a sampled block (pg_csr_transpose, pg_schedule_count,
// pg_schedule_build of csrc/graph.cpp), on a parent graph with in-degrees 0, 1, fanout - 1,
// fanout, fanout + 1, 63, 64, 65, the LDS key capacity, one more, and a hub row, for fanouts
// 0, 1, 5, 70, 600 and -1, with repeated seeds, an empty seed list and a graph without edges.
// Every buffer is exactly sized. The sampled rows are checked for count, membership,
// ascending edge ids; the compaction for src_ids[col_local] == col and the dst prefix.
// Built by tests/sanitize_sample/Makefile with -fsanitize=address,undefined and run by
// tests/test_sanitize_sample.py as a child process; any sanitizer report ends it with a
// non-zero status.
#include <algorithm>
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

struct Parent {
  int64_t n = 0, E = 0;
  std::vector<int32_t> ptr, col, eid;
  pg_csr_t csr() const {
    return pg_csr_t{n, n, E, ptr.data(), E ? col.data() : nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                    nullptr, 0, 0, 0, 256};
  }
};

static Parent build_parent(int64_t n, const std::vector<int32_t>& degs, uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<int64_t> src, dst;
  std::uniform_int_distribution<int64_t> any(0, n - 1);
  for (size_t v = 0; v < degs.size(); ++v)
    for (int32_t k = 0; k < degs[v]; ++k) {
      src.push_back(any(rng));
      dst.push_back((int64_t)v);
    }
  std::vector<size_t> perm(src.size());
  for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  std::vector<int64_t> s2(src.size()), d2(src.size());
  for (size_t i = 0; i < perm.size(); ++i) s2[i] = src[perm[i]], d2[i] = dst[perm[i]];
  Parent p;
  p.n = n;
  p.E = (int64_t)src.size();
  p.ptr.resize(n + 1);
  p.col.resize(p.E);
  p.eid.resize(p.E);
  CHECK(pg_csr_from_coo(s2.data(), d2.data(), p.E, n, n, p.ptr.data(), p.col.data(), p.eid.data()) == 0, "csr: %s",
        pg_last_error_string());
  return p;
}

static void run_sample(const Parent& p, const std::vector<int32_t>& seeds, int32_t fanout, uint64_t seed64) {
  const pg_csr_t g = p.csr();
  const int64_t ns = (int64_t)seeds.size();
  std::vector<int32_t> optr(ns + 1);
  CHECK(pg_sample_count_cpu(&g, seeds.data(), ns, fanout, optr.data()) == 0, "count: %s", pg_last_error_string());
  const int32_t total = optr[ns];
  std::vector<int32_t> ocol(total), oeid(total);
  CHECK(pg_sample_fill_cpu(&g, p.E ? p.eid.data() : nullptr, seeds.data(), ns, fanout, seed64, optr.data(),
                           ocol.data(), oeid.data()) == 0,
        "fill: %s", pg_last_error_string());
  for (int64_t i = 0; i < ns; ++i) {
    const int32_t s = seeds[i], b = p.ptr[s], deg = p.ptr[s + 1] - b;
    const int32_t want = fanout < 0 ? deg : std::min(deg, fanout);
    CHECK(optr[i + 1] - optr[i] == want, "row %lld: %d entries, want %d", (long long)i, optr[i + 1] - optr[i], want);
    for (int32_t q = optr[i]; q < optr[i + 1]; ++q) {
      CHECK(q == optr[i] || oeid[q] > oeid[q - 1], "row %lld: edge ids do not ascend", (long long)i);
      bool found = false;
      for (int32_t k = b; k < b + deg && !found; ++k) found = p.eid[k] == oeid[q] && p.col[k] == ocol[q];
      CHECK(found, "row %lld: entry %d is not in the parent row", (long long)i, q);
    }
  }
  // the same call again, and a rotated seed list: rows do not depend on their place
  std::vector<int32_t> ocol2(total), oeid2(total);
  CHECK(pg_sample_fill_cpu(&g, p.E ? p.eid.data() : nullptr, seeds.data(), ns, fanout, seed64, optr.data(),
                           ocol2.data(), oeid2.data()) == 0, "fill again");
  CHECK(ocol == ocol2 && oeid == oeid2, "two runs differ");
  if (ns > 1) {  // seeds rotated by one place: row i of this run is row i + 1 of the first
    std::vector<int32_t> rot(seeds.begin() + 1, seeds.end());
    rot.push_back(seeds[0]);
    std::vector<int32_t> rptr(ns + 1);
    CHECK(pg_sample_count_cpu(&g, rot.data(), ns, fanout, rptr.data()) == 0 && rptr[ns] == total, "count (rotated)");
    std::vector<int32_t> rcol(total), reid(total);
    CHECK(pg_sample_fill_cpu(&g, p.E ? p.eid.data() : nullptr, rot.data(), ns, fanout, seed64, rptr.data(),
                             rcol.data(), reid.data()) == 0, "fill (rotated)");
    for (int64_t i = 0; i < ns; ++i) {
      const int64_t was = (i + 1) % ns;
      const int32_t len = rptr[i + 1] - rptr[i];
      bool same = len == optr[was + 1] - optr[was];
      for (int32_t q = 0; same && q < len; ++q)
        same = rcol[rptr[i] + q] == ocol[optr[was] + q] && reid[rptr[i] + q] == oeid[optr[was] + q];
      CHECK(same, "row %lld depends on its place in seeds", (long long)was);
    }
  }

  // ---- the block of this sample: unique seeds as dst_ids, compaction, from_in_csr's host calls
  std::vector<int32_t> dst_ids;
  std::vector<int32_t> bptr(1, 0), bcol;
  std::vector<char> seen(p.n, 0);
  for (int64_t i = 0; i < ns; ++i) {
    if (seen[seeds[i]]) continue;
    seen[seeds[i]] = 1;
    dst_ids.push_back(seeds[i]);
    bcol.insert(bcol.end(), ocol.begin() + optr[i], ocol.begin() + optr[i + 1]);
    bptr.push_back((int32_t)bcol.size());
  }
  const int64_t nd = (int64_t)dst_ids.size(), nnz = (int64_t)bcol.size();
  std::vector<int32_t> src_ids(nd + nnz), local(nnz);
  int32_t n_src = -7;
  CHECK(pg_block_compact_cpu(dst_ids.data(), nd, bcol.data(), nnz, p.n, src_ids.data(), local.data(), &n_src) == 0,
        "compact: %s", pg_last_error_string());
  CHECK(n_src >= nd && n_src <= nd + nnz, "n_src %d", n_src);
  for (int64_t i = 0; i < nd; ++i) CHECK(src_ids[i] == dst_ids[i], "src_ids does not start with dst_ids");
  for (int64_t k = 0; k < nnz; ++k)
    CHECK(local[k] >= 0 && local[k] < n_src && src_ids[local[k]] == bcol[k], "src_ids[col_local] != col at %lld",
          (long long)k);
  if (nd > 1) {
    std::vector<int32_t> dup(dst_ids);
    dup.push_back(dst_ids[0]);
    std::vector<int32_t> s3(nd + 1 + nnz);
    int32_t n3 = 0;
    CHECK(pg_block_compact_cpu(dup.data(), nd + 1, bcol.data(), nnz, p.n, s3.data(), local.data(), &n3) == 0 && n3 == -1,
          "a duplicate dst id is not reported (%d)", n3);
  }
  if (n_src < 0) return;
  std::vector<int32_t> tptr(n_src + 1), tcol(nnz), tslot(nnz), tpos(nnz);
  CHECK(pg_csr_transpose(bptr.data(), local.data(), nd, n_src, nnz, tptr.data(), tcol.data(), tslot.data(),
                         tpos.data()) == 0, "transpose: %s", pg_last_error_string());
  for (int pass = 0; pass < 2; ++pass) {
    const int32_t* pp = pass ? tptr.data() : bptr.data();
    const int64_t rows = pass ? n_src : nd;
    const int32_t chunk = pass ? 64 : 256;
    int64_t ni = 0, nm = 0, nsl = 0;
    int32_t md = 0;
    CHECK(pg_schedule_count(pp, rows, chunk, &ni, &nm, &nsl, &md) == 0, "schedule count");
    std::vector<int32_t> items(4 * ni), merges(4 * nm);
    if (rows > 0)
      CHECK(pg_schedule_build(pp, rows, chunk, items.data(), nm ? merges.data() : nullptr) == 0, "schedule build: %s",
            pg_last_error_string());
    int64_t covered = 0;
    for (int64_t i = 0; i < ni; ++i) covered += items[4 * i + 2] - items[4 * i + 1];
    CHECK(covered == nnz, "schedule covers %lld of %lld entries", (long long)covered, (long long)nnz);
  }
}

int main() {
  const int32_t cap = PG_SAMPLE_LDS_KEYS;
  const std::vector<int32_t> degs = {0, 1, 4, 5, 6, 63, 64, 65, 0, 200, cap, cap + 1, 2 * cap + 37};
  const Parent p = build_parent(700, degs, 5);
  std::vector<int32_t> seeds;
  for (int32_t v = 0; v < (int32_t)degs.size(); ++v) seeds.push_back(v);
  seeds.insert(seeds.end(), {12, 3, 3, 650, 699});
  for (int32_t fanout : {0, 1, 5, 70, 600, -1}) run_sample(p, seeds, fanout, 1234 + (uint64_t)fanout);
  run_sample(p, {}, 5, 1);
  run_sample(p, {}, -1, 1);
  const Parent empty = build_parent(9, {}, 1);
  run_sample(empty, {0, 8, 3}, 4, 2);
  std::vector<int32_t> optr(2);
  const pg_csr_t g = p.csr();
  const int32_t bad = 5;
  CHECK(pg_sample_count_cpu(&g, &bad, -1, 2, optr.data()) != 0, "a negative seed count is accepted");
  CHECK(pg_sample_count_cpu(&g, &bad, 1, 2, nullptr) != 0, "a NULL out_ptr is accepted");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize sample ok\n");
  return 0;
}
