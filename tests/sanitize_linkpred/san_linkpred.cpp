// ASan + UBSan driver for the link-prediction host entry points of csrc/cpu_backend.cpp
// (pg_edge_bits_update_cpu, pg_sample_count_excl_cpu, pg_sample_fill_excl_cpu,
// pg_edge_lookup_cpu, pg_negative_sample_cpu) on the sampler's edge-case graph (in-degrees 0, 1,
// fanout - 1, fanout, fanout + 1, 63, 64, 65, the LDS key capacity, one more, and a hub row), for
// fanouts 0, 1, 5, 70, 600 and -1, with no exclusion, a random third of the edge ids, whole rows,
// and ids outside the graph. Every buffer is exactly sized (the bit set: ceil(E / 32) words).
// The sampled rows are checked against the rule (count, no excluded id, membership, ascending
// edge ids, and equality with pg_sample_*_cpu when nothing is excluded); the lookup against a
// scan; the negatives for range, the flags' meaning and the failure count.
// Built by tests/sanitize_linkpred/Makefile with -fsanitize=address,undefined and run by
// tests/test_sanitize_linkpred.py as a child process; any sanitizer report ends it with a
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

static bool bit(const std::vector<uint32_t>& bits, int32_t e) { return (bits[e >> 5] >> (e & 31)) & 1u; }

static void run_sample(const Parent& p, const std::vector<int32_t>& seeds, int32_t fanout, uint64_t seed64,
                       const std::vector<int32_t>& excl) {
  const pg_csr_t g = p.csr();
  const int64_t ns = (int64_t)seeds.size();
  const int32_t* eid = p.E ? p.eid.data() : nullptr;
  std::vector<uint32_t> bits((size_t)((p.E + 31) / 32), 0u);
  int32_t status = 0;
  CHECK(pg_edge_bits_update_cpu(bits.data(), p.E, excl.data(), (int64_t)excl.size(), 1, &status) == 0 && status == 0,
        "bits set: %s", pg_last_error_string());
  std::vector<int32_t> optr(ns + 1);
  CHECK(pg_sample_count_excl_cpu(&g, eid, seeds.data(), ns, fanout, bits.data(), optr.data()) == 0, "count: %s",
        pg_last_error_string());
  const int32_t total = optr[ns];
  std::vector<int32_t> ocol(total), oeid(total);
  CHECK(pg_sample_fill_excl_cpu(&g, eid, seeds.data(), ns, fanout, seed64, bits.data(), optr.data(), ocol.data(),
                                oeid.data()) == 0, "fill: %s", pg_last_error_string());
  for (int64_t i = 0; i < ns; ++i) {
    const int32_t s = seeds[i], b = p.ptr[s], deg = p.ptr[s + 1] - b;
    int32_t rem = 0;
    for (int32_t k = b; k < b + deg; ++k) rem += !bit(bits, p.eid[k]);
    const int32_t want = fanout < 0 ? rem : std::min(rem, fanout);
    CHECK(optr[i + 1] - optr[i] == want, "row %lld: %d entries, want %d", (long long)i, optr[i + 1] - optr[i], want);
    for (int32_t q = optr[i]; q < optr[i + 1]; ++q) {
      CHECK(q == optr[i] || oeid[q] > oeid[q - 1], "row %lld: edge ids do not ascend", (long long)i);
      CHECK(!bit(bits, oeid[q]), "row %lld: an excluded edge id was sampled", (long long)i);
      bool found = false;
      for (int32_t k = b; k < b + deg && !found; ++k) found = p.eid[k] == oeid[q] && p.col[k] == ocol[q];
      CHECK(found, "row %lld: entry %d is not in the parent row", (long long)i, q);
    }
  }
  if (excl.empty()) {  // nothing excluded, and a NULL bit set: pg_sample_*_cpu's result
    std::vector<int32_t> rptr(ns + 1), nptr(ns + 1);
    CHECK(pg_sample_count_cpu(&g, seeds.data(), ns, fanout, rptr.data()) == 0 && rptr == optr, "count != plain count");
    CHECK(pg_sample_count_excl_cpu(&g, eid, seeds.data(), ns, fanout, nullptr, nptr.data()) == 0 && nptr == optr,
          "count with NULL bits");
    std::vector<int32_t> rcol(total), reid(total), ncol(total), neid(total);
    CHECK(pg_sample_fill_cpu(&g, eid, seeds.data(), ns, fanout, seed64, rptr.data(), rcol.data(), reid.data()) == 0,
          "plain fill");
    CHECK(pg_sample_fill_excl_cpu(&g, eid, seeds.data(), ns, fanout, seed64, nullptr, optr.data(), ncol.data(),
                                  neid.data()) == 0, "fill with NULL bits");
    CHECK(rcol == ocol && reid == oeid && ncol == ocol && neid == oeid, "no exclusion differs from pg_sample_fill_cpu");
  }
  CHECK(pg_edge_bits_update_cpu(bits.data(), p.E, excl.data(), (int64_t)excl.size(), 0, &status) == 0 && status == 0,
        "bits clear");
  CHECK(std::all_of(bits.begin(), bits.end(), [](uint32_t w) { return w == 0; }), "set then clear leaves bits");
}

static void run_bits(int64_t n_ids) {
  std::vector<uint32_t> bits((size_t)((n_ids + 31) / 32), 0u);
  const std::vector<int32_t> bad = {0, (int32_t)n_ids, -1, (int32_t)n_ids - 1, 0};
  int32_t status = 0;
  CHECK(pg_edge_bits_update_cpu(bits.data(), n_ids, bad.data(), (int64_t)bad.size(), 1, &status) == 0, "bits");
  CHECK(status == -2, "an id outside [0, n) is not reported (%d)", status);
  CHECK(bit(bits, 0) && bit(bits, (int32_t)n_ids - 1), "the ids in range were not set");
  status = 0;
  CHECK(pg_edge_bits_update_cpu(bits.data(), n_ids, bad.data(), (int64_t)bad.size(), 0, &status) == 0 && status == -2,
        "bits clear");
  CHECK(std::all_of(bits.begin(), bits.end(), [](uint32_t w) { return w == 0; }), "bits left");
  CHECK(pg_edge_bits_update_cpu(nullptr, 0, nullptr, 0, 1, nullptr) == 0, "an empty update fails");
  CHECK(pg_edge_bits_update_cpu(bits.data(), n_ids, bad.data(), -1, 1, &status) != 0, "a negative count is accepted");
}

static int32_t scan_lookup(const Parent& p, int32_t u, int32_t v) {
  if (u < 0 || u >= p.n || v < 0 || v >= p.n) return -1;
  for (int32_t k = p.ptr[v]; k < p.ptr[v + 1]; ++k)
    if (p.col[k] == u) return p.eid[k];
  return -1;
}

static void run_lookup(const Parent& p) {
  const pg_csr_t g = p.csr();
  std::mt19937 rng(3);
  std::vector<int32_t> u, v;
  for (int32_t r = 0; r < 13; ++r)  // every entry of the first rows (degree 0 .. 65), and misses
    for (int32_t k = p.ptr[r]; k < p.ptr[r + 1] && k < p.ptr[r] + 70; ++k) u.push_back(p.col[k]), v.push_back(r);
  for (int q = 0; q < 500; ++q) u.push_back((int32_t)(rng() % p.n)), v.push_back((int32_t)(rng() % 13));
  for (int32_t x : {-1, (int32_t)p.n}) u.push_back(x), v.push_back(3), u.push_back(3), v.push_back(x);
  std::vector<int32_t> out(u.size());
  CHECK(pg_edge_lookup_cpu(&g, p.E ? p.eid.data() : nullptr, u.data(), v.data(), (int64_t)u.size(), out.data()) == 0,
        "lookup: %s", pg_last_error_string());
  for (size_t i = 0; i < u.size(); ++i)
    CHECK(out[i] == scan_lookup(p, u[i], v[i]), "lookup %d -> %d: %d", u[i], v[i], out[i]);
  CHECK(pg_edge_lookup_cpu(&g, nullptr, nullptr, nullptr, 0, nullptr) == 0, "an empty lookup fails");
}

static void run_negatives(const Parent& p) {
  const pg_csr_t g = p.csr();
  const int32_t k = 3;
  std::vector<int32_t> pos_src = {0, 5, (int32_t)p.n - 1, (int32_t)p.n, -1, 7}, pos_id = {9, 8, 7, 6, 5, 4};
  const int64_t n_pos = (int64_t)pos_src.size();
  for (int flags : {0, PG_NEG_REJECT_EDGE, PG_NEG_REJECT_SELF, PG_NEG_REJECT_EDGE | PG_NEG_REJECT_SELF})
    for (int given = 0; given < 2; ++given) {
      std::vector<int32_t> ns(n_pos * k), nd(n_pos * k);
      int32_t n_fail = -7;
      CHECK(pg_negative_sample_cpu(&g, given ? pos_src.data() : nullptr, given ? pos_id.data() : nullptr, n_pos, k, 16,
                                   flags, 11, ns.data(), nd.data(), &n_fail) == 0, "negatives: %s",
            pg_last_error_string());
      int32_t fails = 0;
      for (int64_t s = 0; s < n_pos * k; ++s) {
        if (ns[s] < 0) {
          CHECK(nd[s] == -1 && ns[s] == -1, "a failed slot is not (-1, -1)");
          ++fails;
          continue;
        }
        CHECK(ns[s] < p.n && nd[s] >= 0 && nd[s] < p.n, "slot %lld out of range", (long long)s);
        if (given) CHECK(ns[s] == pos_src[s / k], "slot %lld: the source is not pos_src", (long long)s);
        if (flags & PG_NEG_REJECT_SELF) CHECK(ns[s] != nd[s], "a self-pair came back");
        if (flags & PG_NEG_REJECT_EDGE) CHECK(scan_lookup(p, ns[s], nd[s]) < 0, "an edge came back");
      }
      CHECK(n_fail == fails && (!given || fails >= 2 * k), "n_fail %d, counted %d", n_fail, fails);
    }
  int32_t n_fail = 0;
  std::vector<int32_t> ns(k), nd(k);
  CHECK(pg_negative_sample_cpu(&g, nullptr, nullptr, 1, k, 0, 0, 1, ns.data(), nd.data(), &n_fail) != 0, "tries = 0");
  CHECK(pg_negative_sample_cpu(&g, nullptr, nullptr, 1, k, 65, 0, 1, ns.data(), nd.data(), &n_fail) != 0, "tries = 65");
  CHECK(pg_negative_sample_cpu(&g, nullptr, nullptr, 1, 0, 4, 0, 1, ns.data(), nd.data(), &n_fail) != 0, "k = 0");
  CHECK(pg_negative_sample_cpu(&g, nullptr, nullptr, 0, k, 4, 0, 1, nullptr, nullptr, &n_fail) == 0 && n_fail == 0,
        "an empty batch fails");
}

int main() {
  const int32_t cap = PG_SAMPLE_LDS_KEYS;
  const std::vector<int32_t> degs = {0, 1, 4, 5, 6, 63, 64, 65, 0, 200, cap, cap + 1, 2 * cap + 37};
  const Parent p = build_parent(700, degs, 5);
  std::vector<int32_t> seeds;
  for (int32_t v = 0; v < (int32_t)degs.size(); ++v) seeds.push_back(v);
  seeds.insert(seeds.end(), {12, 3, 3, 650, 699});
  std::mt19937 rng(2);
  std::vector<int32_t> third, rows;
  for (int32_t e = 0; e < p.E; ++e)
    if (rng() % 3 == 0) third.push_back(e);
  third.push_back(third[0]);  // a duplicate
  for (int32_t r : {4, 7, 11})
    for (int32_t k = p.ptr[r]; k < p.ptr[r + 1]; ++k) rows.push_back(p.eid[k]);
  for (int32_t k = p.ptr[12]; k < p.ptr[12] + cap + 36; ++k) rows.push_back(p.eid[k]);  // the hub row down to cap + 1
  const std::vector<int32_t> none;
  for (int32_t fanout : {0, 1, 5, 70, 600, -1})
    for (const std::vector<int32_t>* excl : {&none, (const std::vector<int32_t>*)&third, (const std::vector<int32_t>*)&rows})
      run_sample(p, seeds, fanout, 1234 + (uint64_t)fanout, *excl);
  run_sample(p, {}, 5, 1, third);
  const Parent empty = build_parent(9, {}, 1);
  run_sample(empty, {0, 8, 3}, 4, 2, {});
  run_bits(p.E);
  run_bits(33);
  run_lookup(p);
  run_negatives(p);
  run_negatives(empty);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize linkpred ok\n");
  return 0;
}
