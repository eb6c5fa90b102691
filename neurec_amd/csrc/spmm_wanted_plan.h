// spmm_wanted_plan.h — the per-batch schedule of the row-masked forward hop (spmm_wanted_planned_kernel in
// spmm_blocked.hip): which wave gathers which sub-list of which batch row, worked out for every batch of an
// epoch in one launch (spmm_wanted_epoch_plan_kernel) from the sampler's sorted occurrence keys.
//
// Pure integer work, like spmm_blocked_plan.h: no HIP type, compiles with g++.  The device planner uses the
// same sort key, slot counts and item encoders (NR_WP_HD); plan_batch below is the host statement of what it
// must write, byte for byte, and tests/test_spmm_wanted_plan_cpu.py checks its invariants on the CPU.
//
// A batch's schedule is `stride` 16-byte records: a header {items, distinct rows, 0, 0}, then the items.
// Wave w of workgroup g runs item 16 g + w.  An item is ONE sub-list of <= 64 pairs:
//   x == 0 : the whole of a row of <= 64 non-zeros (w = row, y = length, z = first CSR position);
//            w == -1: nothing (padding)
//   x <  0 : segment sg of a row of 65..512 non-zeros, ns segments: x = -(1 + sg + 16 ns).  The ns items are
//            consecutive and never cross a workgroup: the wave of segment 0 adds the ns sums in segment order
//   x >  0 : a segment of a longer row (a hub): x = 1 + its global partial slot.  A hub's segments are
//            consecutive, in chunks of 8 that start on a multiple of 8; the first item of a chunk carries
//            1 + hub index in y >> 8, and its wave moves the hub's chunk counter once.
// A row takes 1, 2, 4 or 8 slots (its segments rounded up to a power of two; a hub 8 per chunk) and rows are
// ordered by slots descending, then non-zeros descending, then row id — so every run starts on a multiple of
// its own size, 16 consecutive items cost about the same, and the order is a pure function of the batch's
// rows and the graph.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "spmm_blocked_plan.h"

#ifdef __HIPCC__
#define NR_WP_HD __host__ __device__ __forceinline__
#else
#define NR_WP_HD inline
#endif

namespace nr_wplan {

constexpr int kSeg = 64;                       // pairs per item
constexpr int kChunk = nr_plan::kWaveChunk;    // segments per chunk of a hub
constexpr int kWaves = 16;                     // items per workgroup
constexpr int kMaxKeys = 16384;                // 3 * batch the one-workgroup planner sorts
constexpr int64_t kMaxRows = (int64_t)1 << 19; // row ids in the 31-bit sort key

NR_WP_HD int segments_of(int64_t len) { return len <= kSeg ? 1 : (int)((len + kSeg - 1) / kSeg); }
NR_WP_HD bool is_hub(int64_t len) { return len > (int64_t)kSeg * kChunk; }
// slots a row takes in the item list
NR_WP_HD int slots_of(int64_t len) {
  const int ns = segments_of(len);
  if (ns > kChunk) return (ns + kChunk - 1) / kChunk * kChunk;
  return ns <= 1 ? 1 : ns <= 2 ? 2 : ns <= 4 ? 4 : 8;
}
// ascending key = the item order: slot class (8, 4, 2, 1), then non-zeros descending (capped: hubs of >= 1023
// tie and fall back to the row id), then row id
NR_WP_HD uint32_t sort_key(int64_t len, int32_t row) {
  const int sl = slots_of(len);
  const uint32_t cls = sl >= 8 ? 0u : sl == 4 ? 1u : sl == 2 ? 2u : 3u;
  const uint32_t c = (uint32_t)(len < 1023 ? len : 1023);
  return (cls << 29) | ((1023u - c) << 19) | (uint32_t)row;
}
NR_WP_HD int32_t key_row(uint32_t key) { return (int32_t)(key & ((1u << 19) - 1u)); }
NR_WP_HD int seg_len(int64_t len, int sg) {
  const int64_t left = len - (int64_t)sg * kSeg;
  return (int)(left < 0 ? 0 : left < kSeg ? left : kSeg);
}

NR_WP_HD nr_plan::Int4 item_pad() { return nr_plan::Int4{0, 0, 0, -1}; }
NR_WP_HD nr_plan::Int4 item_short(int32_t row, int64_t first, int64_t len) {
  return nr_plan::Int4{0, (int32_t)len, (int32_t)(uint32_t)first, row};
}
NR_WP_HD nr_plan::Int4 item_lds(int32_t row, int64_t first, int64_t len, int sg) {
  return nr_plan::Int4{-(1 + sg + 16 * segments_of(len)), seg_len(len, sg),
                       (int32_t)(uint32_t)(first + (int64_t)sg * kSeg), row};
}
// hub_index / part0: the row's record in the lane-group plan (Plan::ww_hub: index, first global partial slot)
NR_WP_HD nr_plan::Int4 item_hub(int32_t row, int64_t first, int64_t len, int sg, int hub_index, int part0) {
  return nr_plan::Int4{1 + part0 + sg, seg_len(len, sg) | ((sg % kChunk == 0) ? (hub_index + 1) << 8 : 0),
                       (int32_t)(uint32_t)(first + (int64_t)sg * kSeg), row};
}
// slot s of a row's run (s < slots_of(len)); hub_index / part0 only read for hubs
NR_WP_HD nr_plan::Int4 item_of(int32_t row, int64_t first, int64_t len, int s, int hub_index, int part0) {
  const int ns = segments_of(len);
  if (s >= ns) return item_pad();
  if (ns == 1) return item_short(row, first, len);
  if (ns <= kChunk) return item_lds(row, first, len, s);
  return item_hub(row, first, len, s, hub_index, part0);
}

// ---- host side -----------------------------------------------------------------------------------------

// Upper bound of a batch's item count: the slots of the k = min(3 * batch, n_rows) most expensive rows.
// big_desc: slots of every row that takes more than one, descending.
struct SlotProfile { std::vector<int32_t> big_desc; int64_t n_rows = 0; };
inline SlotProfile slot_profile(const int64_t* indptr, int64_t n_rows) {
  SlotProfile p;
  p.n_rows = n_rows;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int s = slots_of(indptr[r + 1] - indptr[r]);
    if (s > 1) p.big_desc.push_back(s);
  }
  std::sort(p.big_desc.begin(), p.big_desc.end(), [](int32_t a, int32_t b) { return a > b; });
  return p;
}
inline int64_t items_bound(const SlotProfile& p, int batch) {
  const int64_t k = std::min<int64_t>(3 * (int64_t)batch, p.n_rows);
  const int64_t nb = std::min<int64_t>(k, (int64_t)p.big_desc.size());
  int64_t sum = k - nb;
  for (int64_t i = 0; i < nb; ++i) sum += p.big_desc[(size_t)i];
  return sum;
}
// records per batch: the header + the bound rounded up to whole workgroups
inline int64_t stride_of(const SlotProfile& p, int batch) {
  return 1 + (items_bound(p, batch) + kWaves - 1) / kWaves * kWaves;
}

// One batch's schedule, the way the device planner writes it.  keys: the batch's sorted occurrence keys
// (row << 32 | position); hubs: Plan::ww_hub (ascending rows).  out[0 .. stride): header, items, padding
// records up to the stride.  Returns the item count, or -1 when it exceeds stride - 1.
inline int64_t plan_batch(const int64_t* indptr, const std::vector<nr_plan::Int4>& hubs, const uint64_t* keys,
                          int n_keys, int64_t stride, nr_plan::Int4* out) {
  std::vector<uint32_t> sk;
  for (int i = 0; i < n_keys; ++i) {
    const int32_t row = (int32_t)(keys[i] >> 32);
    if (i > 0 && (int32_t)(keys[i - 1] >> 32) == row) continue;
    sk.push_back(sort_key(indptr[row + 1] - indptr[row], row));
  }
  std::sort(sk.begin(), sk.end());
  for (int64_t i = 0; i < stride; ++i) out[i] = nr_plan::Int4{0, 0, 0, 0};
  int64_t n = 0;
  for (uint32_t k : sk) {
    const int32_t row = key_row(k);
    const int64_t first = indptr[row], len = indptr[row + 1] - first;
    const int sl = slots_of(len);
    int hub = -1, part0 = 0;
    if (is_hub(len)) {
      auto it = std::lower_bound(hubs.begin(), hubs.end(), row, [](const nr_plan::Int4& h, int32_t r) { return h.x < r; });
      if (it == hubs.end() || it->x != row) return -1;
      hub = (int)(it - hubs.begin());
      part0 = it->y;
    }
    if (n + sl > stride - 1) return -1;
    for (int s = 0; s < sl; ++s) out[1 + n + s] = item_of(row, first, len, s, hub, part0);
    n += sl;
  }
  for (int64_t i = 1 + n; i < stride; ++i) out[i] = item_pad();
  out[0] = nr_plan::Int4{(int32_t)n, (int32_t)sk.size(), 0, 0};
  return n;
}

}  // namespace nr_wplan
