// spmm_blocked_factor.h — host side of the lane-group SpMM's 4-byte non-zeros (spmm_blocked.hip).
//
// The adjacencies of this project store value[r][c] = float32(row_factor[r] * col_factor[c]) with a few hundred
// distinct factors (graph.factor_values finds them), so a non-zero needs no fp32 value of its own: one word
//     column | code << col_bits        (code: index of the COLUMN's factor in a table of distinct factors)
// plus the row's factor, kept once per sub-list beside its descriptor, carries the same matrix.  This header
// builds the table, the codes and the word layout.  Like spmm_blocked_plan.h it is pure host code without a HIP
// header (tests/hostcheck/factorcheck.cpp checks it with g++); the device side verifies every product.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "spmm_blocked_plan.h"

namespace nr_plan {

constexpr int kMaxFactorCodes = kPlanFactorCodes;   // the table the kernels stage in LDS: 4 KB beside the accumulators
// never a packed word: free as a "pair masked out" mark for a kernel that compacts words in place (the staged masked
// hop did in a form that was measured and not kept: profiles/r20_packed_nonzeros.txt)
constexpr uint32_t kDroppedWord = 0xFFFFFFFFu;

struct FactorLayout {
  int col_bits = 0;                   // low bits of a word: the column
  uint32_t col_mask = 0;
  std::vector<float> table;           // distinct factors, ascending bit patterns (compared as bits, not as numbers)
  std::vector<uint16_t> row_code, col_code;
};

inline uint32_t factor_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline uint32_t factor_word(const FactorLayout& l, int64_t col, uint16_t code) {
  return (uint32_t)col | ((uint32_t)code << l.col_bits);
}
inline int64_t factor_word_col(const FactorLayout& l, uint32_t w) { return (int64_t)(w & l.col_mask); }
inline uint32_t factor_word_code(const FactorLayout& l, uint32_t w) { return w >> l.col_bits; }

// kOk: `out` holds the layout.  kErrUnsupported: the matrix keeps the two-array form (err says why): more
// distinct factors than the table holds, or more codes than the bits a column leaves in the word.
inline int factor_layout(const float* row_factor, int64_t n_rows, const float* col_factor, int64_t n_cols,
                         FactorLayout* out, Error* err) {
  NR_PLAN_REQUIRE(row_factor && col_factor && out && n_rows > 0 && n_cols > 0, kErrArg, "factor_layout: bad arguments");
  NR_PLAN_REQUIRE(n_cols <= ((int64_t)1 << 31), kErrUnsupported, "factor_layout: %lld columns", (long long)n_cols);
  std::vector<uint32_t> bits;
  bits.reserve((size_t)(n_rows + n_cols));
  for (int64_t r = 0; r < n_rows; ++r) bits.push_back(factor_bits(row_factor[r]));
  for (int64_t c = 0; c < n_cols; ++c) bits.push_back(factor_bits(col_factor[c]));
  std::vector<uint32_t> uniq(bits);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  NR_PLAN_REQUIRE((int64_t)uniq.size() <= kMaxFactorCodes, kErrUnsupported,
                  "factor_layout: %lld distinct factors > %d", (long long)uniq.size(), kMaxFactorCodes);
  int cb = 1;
  while (((int64_t)1 << cb) < n_cols) ++cb;
  // the top code of the word stays unused, so the all-ones word (kDroppedWord) is never produced
  NR_PLAN_REQUIRE((uint64_t)uniq.size() < ((uint64_t)1 << (32 - cb)), kErrUnsupported,
                  "factor_layout: %lld codes do not fit the %d bits beside a %d-bit column", (long long)uniq.size(),
                  32 - cb, cb);
  out->col_bits = cb;
  out->col_mask = (uint32_t)(((uint64_t)1 << cb) - 1);
  out->table.resize(uniq.size());
  memcpy(out->table.data(), uniq.data(), uniq.size() * 4);
  out->row_code.resize((size_t)n_rows);
  out->col_code.resize((size_t)n_cols);
  for (int64_t i = 0; i < n_rows + n_cols; ++i) {
    const uint16_t code = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), bits[(size_t)i]) - uniq.begin());
    if (i < n_rows) out->row_code[(size_t)i] = code;
    else out->col_code[(size_t)(i - n_rows)] = code;
  }
  return kOk;
}

}  // namespace nr_plan
