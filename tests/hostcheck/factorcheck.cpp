// g++ build of neurec_amd/csrc/spmm_blocked_factor.h, the host side of the lane-group SpMM's 4-byte non-zeros: a
// stand-alone program (tests/test_spmm_factor_cpu.py builds and runs it, once more under the address and
// undefined-behaviour sanitizers).  It prints one line per case, "ok <name> <fnv1a of the layout's bytes>" or
// "refused <name>", and exits non-zero at the first broken property.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "spmm_blocked_factor.h"

using nr_plan::FactorLayout;

static void require(bool ok, const char* what, const char* name) {
  if (ok) return;
  fprintf(stderr, "factorcheck: %s: %s\n", name, what);
  exit(1);
}

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

// a deterministic matrix: n_rows x n_cols, `n_factors` distinct factor values spread over rows and columns
// (value k = 1 + k / 8192, exact in float32), a few non-zeros per row.  Returns 1 when refused.
static int run_case(const char* name, int64_t n_rows, int64_t n_cols, int n_factors, bool expect_refused) {
  std::vector<float> rf((size_t)n_rows), cf((size_t)n_cols);
  uint32_t lcg = 12345u + (uint32_t)n_cols;
  auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; };
  for (int64_t i = 0; i < n_rows + n_cols; ++i) {
    // every factor value is used at least once (the first n_factors slots), then at random
    const int k = i < n_factors ? (int)i : (int)(next() % (uint32_t)n_factors);
    const float f = 1.0f + (float)k / 8192.0f;
    if (i < n_rows) rf[(size_t)i] = f; else cf[(size_t)(i - n_rows)] = f;
  }
  FactorLayout a, b;
  nr_plan::Error err;
  const int rc = nr_plan::factor_layout(rf.data(), n_rows, cf.data(), n_cols, &a, &err);
  if (rc != nr_plan::kOk) {
    require(expect_refused && rc == nr_plan::kErrUnsupported && !err.msg.empty(), "refused unexpectedly", name);
    printf("refused %s\n", name);
    return 1;
  }
  require(!expect_refused, "accepted a layout that must be refused", name);
  // the layout
  require((int)a.table.size() == n_factors, "table size", name);
  for (size_t i = 1; i < a.table.size(); ++i)
    require(nr_plan::factor_bits(a.table[i - 1]) < nr_plan::factor_bits(a.table[i]), "table not strictly ascending", name);
  require(((int64_t)1 << a.col_bits) >= n_cols && (a.col_bits == 1 || ((int64_t)1 << (a.col_bits - 1)) < n_cols),
          "column bits are not ceil(log2(n_cols))", name);
  require(a.col_mask == (uint32_t)(((uint64_t)1 << a.col_bits) - 1), "column mask", name);
  for (int64_t r = 0; r < n_rows; ++r)
    require(nr_plan::factor_bits(a.table[a.row_code[(size_t)r]]) == nr_plan::factor_bits(rf[(size_t)r]), "row code", name);
  // every word of a few non-zeros per row, and of the corner columns, decodes to its column and its factor
  uint64_t h = 1469598103934665603ull;
  for (int64_t r = 0; r < n_rows; ++r)
    for (int j = 0; j < 6; ++j) {
      const int64_t c = j == 0 ? 0 : j == 1 ? n_cols - 1 : (int64_t)(next() % (uint32_t)n_cols);
      const uint32_t w = nr_plan::factor_word(a, c, a.col_code[(size_t)c]);
      require(w != nr_plan::kDroppedWord, "the reserved word was produced", name);
      require(nr_plan::factor_word_col(a, w) == c, "word does not decode to its column", name);
      const uint32_t code = nr_plan::factor_word_code(a, w);
      require(code < a.table.size() && nr_plan::factor_bits(a.table[code]) == nr_plan::factor_bits(cf[(size_t)c]),
              "word does not decode to its column's factor", name);
      h = fnv(h, &w, 4);
    }
  // the largest word the layout can produce is not the reserved one either
  require(nr_plan::factor_word(a, n_cols - 1, (uint16_t)(a.table.size() - 1)) != nr_plan::kDroppedWord,
          "the largest word is the reserved one", name);
  // built twice: the same bytes
  require(nr_plan::factor_layout(rf.data(), n_rows, cf.data(), n_cols, &b, &err) == nr_plan::kOk, "second build", name);
  require(a.col_bits == b.col_bits && a.table.size() == b.table.size() &&
              memcmp(a.table.data(), b.table.data(), a.table.size() * 4) == 0 && a.row_code == b.row_code &&
              a.col_code == b.col_code,
          "two builds differ", name);
  h = fnv(h, &a.col_bits, sizeof(int));
  h = fnv(h, a.table.data(), a.table.size() * 4);
  h = fnv(h, a.row_code.data(), a.row_code.size() * 2);
  h = fnv(h, a.col_code.data(), a.col_code.size() * 2);
  printf("ok %s %d %016llx\n", name, a.col_bits, (unsigned long long)h);
  return 0;
}

int main() {
  run_case("cols256", 300, 256, 37, false);          // 8 column bits
  run_case("cols257", 300, 257, 37, false);          // 9
  run_case("one_column", 5, 1, 3, false);
  run_case("factors1024", 900, 700, 1024, false);    // the table is full
  run_case("factors1025", 900, 700, 1025, true);     // one too many for the table
  // signed zeros and equal numbers with different bits are different factors; NaN bits are kept as they are
  {
    const float rf[3] = {0.0f, -0.0f, 1.0f}, cf[2] = {1.0f, 0.0f};
    FactorLayout l;
    nr_plan::Error err;
    require(nr_plan::factor_layout(rf, 3, cf, 2, &l, &err) == nr_plan::kOk && l.table.size() == 3, "signed zeros", "zeros");
    require(l.row_code[0] != l.row_code[1] && l.row_code[0] == l.col_code[1] && l.row_code[2] == l.col_code[0],
            "codes of signed zeros", "zeros");
    printf("ok zeros %d\n", l.col_bits);
  }
  // a column so wide that the codes no longer fit beside it: 2^22 columns leave 10 bits, 1,024 codes need the top
  // code free
  {
    const int64_t n_cols = (int64_t)1 << 22;
    std::vector<float> rf(1024), cf((size_t)n_cols, 1.0f);
    for (int i = 0; i < 1024; ++i) rf[(size_t)i] = 2.0f + (float)i / 8192.0f;       // 1,024 values + 1.0 = 1,025
    FactorLayout l;
    nr_plan::Error err;
    require(nr_plan::factor_layout(rf.data(), 1024, cf.data(), n_cols, &l, &err) == nr_plan::kErrUnsupported,
            "1,025 factors beside 22 column bits", "wide");
    rf[1023] = rf[1022];                                                           // 1,024 distinct: the top code is used
    require(nr_plan::factor_layout(rf.data(), 1024, cf.data(), n_cols, &l, &err) == nr_plan::kErrUnsupported,
            "1,024 codes beside 22 column bits leave no reserved word", "wide");
    rf[1023] = rf[1022] = rf[1021];                                                // 1,023: fits
    require(nr_plan::factor_layout(rf.data(), 1024, cf.data(), n_cols, &l, &err) == nr_plan::kOk && l.col_bits == 22,
            "1,023 codes beside 22 column bits", "wide");
    printf("ok wide %d\n", l.col_bits);
  }
  return 0;
}
