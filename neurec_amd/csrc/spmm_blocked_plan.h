// spmm_blocked_plan.h — the host side of the lane-group SpMM (spmm_blocked.hip): the schedule its kernels
// walk, built once per matrix from indptr / indices, and the layout of that schedule in the plan's device
// buffer.
//
// Pure integer work: no HIP header, no HIP type, no environment variable, no device query.  It compiles
// with g++ as well as with hipcc, and tests/test_spmm_plan_cpu.py (through tests/hostcheck/plancheck.cpp)
// checks the schedule's invariants on the CPU.  nrhip_spmm_blocked_plan_create resolves what depends on the
// process and the device (environment switches, CU count), calls build_plan and uploads the result.
//
// The stages, in the order build_plan runs them:
//   resolve_options -> choose_workgroup_count -> assign_workgroups_to_classes -> class_span_and_phases ->
//   deal_rows -> packed_order -> cut_rows_into_entries -> flatten_entries -> masked_hop_switches ->
//   wanted_rows_schedule -> wanted_wave_schedule;   then plan_sections / carve_sections place the arrays.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <queue>
#include <string>
#include <utility>
#include <vector>

namespace nr_plan {

constexpr int kSegDefault = 64;     // longest sub-list one lane group walks alone
constexpr int kRMaxDefault = 416;   // row accumulators per workgroup (104 KB)
constexpr int kPMaxDefault = 192;   // segment partial slots per workgroup and phase (48 KB)
constexpr int kMaxPhases = 32;
constexpr int kMaxLdsBytes = 160 * 1024;
constexpr int kPlanFactorCodes = 1024;   // entries of the factor table (spmm_blocked_factor.h: kMaxFactorCodes)
constexpr int kWaveChunk = 8;       // wave-cooperative wanted-rows hop: 64-segments per chunk of a hub row

// what the kernels read as int4 (uploaded as bytes)
struct Int4 { int32_t x, y, z, w; };
static_assert(sizeof(Int4) == 16, "descriptors are 16 bytes on the device");

// status codes: the values of NR_OK / NR_ERR_ARG / NR_ERR_UNSUPPORTED (nr_common.h; spmm_blocked.hip asserts it)
enum Status { kOk = 0, kErrArg = 1, kErrUnsupported = 2 };
struct Error { std::string msg; };

inline int fail(Error* err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err->msg = buf;
  return code;
}
#define NR_PLAN_REQUIRE(cond, code, ...) \
  do { if (!(cond)) return ::nr_plan::fail(err, (code), __VA_ARGS__); } while (0)
#define NR_PLAN_TRY(call) \
  do { const int rc_ = (call); if (rc_ != ::nr_plan::kOk) return rc_; } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Everything the planner depends on besides the matrix, as plain values.
struct Options {
  int d, waves, seg, r_max, p_max;
  int64_t block_bytes;              // > 0
  int64_t split_row;                // 0: one class of rows
  int n_wg;                         // workgroups (choose_workgroup_count)
  bool masked_fast = true;          // staged masked / wanted-rows kernels allowed (NEUREC_SPMM_MASKED_FAST != 0)
  bool wanted_wave = true;          // wave-cooperative wanted-rows kernel allowed (NEUREC_SPMM_WANTED_WAVE != 0)
  int wanted_nnz_cap = 0;           // > 0: upper limit on w_nnz_cap (tests force the chunked path)
};

// The schedule on the host: every array that goes to the device, and the scalars the launches need.
struct Plan {
  int64_t n_rows = 0, nnz = 0;
  int n_wg = 0, n_phases = 1;
  std::vector<int32_t> wg_row0, wg_nrows;      // [n_wg] the workgroup's rows: row_of[wg_row0[w] + slot]
  std::vector<int32_t> row_of;                 // [n_rows]
  std::vector<uint32_t> pk_src, pk_dst;        // [n_rows] first CSR position / [n_rows + 1] first packed position of row_of[k]
  std::vector<int32_t> ent_off, cmb_off;       // [n_wg][n_phases + 1]
  std::vector<Int4> ent;                       // {accumulator slot, length, first non-zero (packed), owning row (global id)}
  std::vector<Int4> cmb;                       // {row slot, first partial slot, segments, row (global id)}
  std::vector<uint32_t> wg_nnz;                // [n_wg][2] first packed non-zero of the workgroup's rows, count
  int64_t nnz_cap_exact = 0;                   // largest packed slice of a workgroup
  int nnz_cap = 0, ent_cap = 0;                // the same clamped to int / largest descriptor list, rounded up to 16
  int colmask_ok = 0;
  // staged wanted-rows schedule (spmm_wanted_rows_kernel); non-zero positions are CSR positions
  std::vector<Int4> w_ent;                     // {0 | r_max + partial slot, length, first non-zero, row}
  std::vector<Int4> w_cmb;                     // {row, first partial slot (+ r_max), segments, 0}
  std::vector<int32_t> w_ent_off, w_cmb_off;   // [n_wg][2] begin, end
  int wanted_ok = 0, w_ent_cap = 0, w_nnz_cap = 0, w_bitmap_words = 0;
  // wave-cooperative wanted-rows schedule (spmm_wanted_wave_kernel); CSR positions as well
  std::vector<int32_t> ww_off, ww_choff, ww_lcoff;   // [n_wg + 1] entries / chunks / one-chunk rows
  std::vector<Int4> ww_ent;                    // {0 | 1 + global partial slot | -(1 + LDS slot), length, first non-zero, row}
  std::vector<int32_t> ww_gch;                 // hub index of every chunk
  std::vector<Int4> ww_hub;                    // {row, first global partial slot, segments, chunks}
  std::vector<Int4> ww_lcmb;                   // {row, first LDS slot, segments, 0}
  int64_t ww_segments = 0;                     // global partial slots (segments of multi-chunk rows)
  int ww_ok = 0, ww_ent_cap = 0, ww_lds_slots = 0;
};

// rows [ra, rb) gather from columns [cmin, cmin + K * width), cut into K blocks of `width` columns
struct ClassDesc { int64_t ra, rb; std::vector<int> wgs; int32_t cmin; int64_t width, K; };

// cost of a row for balancing: its non-zeros plus a fixed cost per sub-list (descriptor, first
// index chunk and the short last gather round; fitted on the per-workgroup timeline,
// profiles/r01_exp_spmm_timeline.txt)
constexpr int kEntCost = 4;     // r05 (rows dealt): 0 .. 16 all within 1 us of each other, 2-4 best (profiles/r05_exp_entcost.txt)
inline int64_t row_cost(int64_t len, int seg) {
  return len + (int64_t)kEntCost * std::max<int64_t>(1, (len + seg - 1) / seg);
}

// Defaults for the arguments given as <= 0, and the shapes the kernels were built for.
inline int resolve_options(int d, int waves_per_wg, int seg_len, int r_max, int p_max, int64_t block_bytes,
                           int64_t split_row, int64_t n_rows, Options* opt, Error* err) {
  opt->d = d;
  opt->waves = waves_per_wg > 0 ? waves_per_wg : 16;
  opt->seg = seg_len > 0 ? seg_len : kSegDefault;
  opt->r_max = r_max > 0 ? r_max : kRMaxDefault * opt->waves / 16 * 64 / (d > 0 ? d : 64);
  opt->p_max = p_max > 0 ? p_max : kPMaxDefault * opt->waves / 16 * 64 / (d > 0 ? d : 64);
  NR_PLAN_REQUIRE(d == 16 || d == 32 || d == 64 || d == 128 || d == 256, kErrUnsupported,
                  "spmm_blocked: embedding dim %d not built (16, 32, 64, 128, 256)", d);
  NR_PLAN_REQUIRE(opt->waves == 16 || opt->waves == 8, kErrUnsupported,
                  "spmm_blocked: waves per workgroup %d (8, 16)", opt->waves);
  NR_PLAN_REQUIRE(opt->seg >= 16 && (size_t)(opt->r_max + opt->p_max) * d * 4 + (size_t)opt->r_max * 4 <= (size_t)kMaxLdsBytes,
                  kErrUnsupported, "spmm_blocked: seg %d / accumulators %d+%d do not fit", opt->seg, opt->r_max,
                  opt->p_max);
  opt->block_bytes = block_bytes > 0 ? block_bytes : (int64_t)1 << 40;     // measured: phases cost more than they save
  opt->split_row = (split_row <= 0 || split_row >= n_rows) ? 0 : split_row;
  opt->n_wg = 0;
  return kOk;
}

// n_wg: the caller's count, or (from_device) one workgroup per CU as the device reports it.
inline int choose_workgroup_count(int n_wg, bool from_device, int64_t n_rows, Options* opt, Error* err) {
  n_wg = n_wg / 8 * 8;
  if (from_device && n_wg >= 8) {
    // more rows than one workgroup per CU can hold accumulators for: launch a multiple of the CU
    // count (the extra workgroups queue behind the resident ones; without column blocking the
    // rounds are independent)
    const int64_t per_class = opt->split_row ? n_wg / 2 : n_wg;
    const int64_t biggest = opt->split_row ? std::max<int64_t>(opt->split_row, n_rows - opt->split_row) : n_rows;
    const int64_t cap = (int64_t)opt->r_max * 9 / 10;
    const int64_t mult = (biggest + per_class * cap - 1) / (per_class * cap);
    if (mult > 1) n_wg = (int)std::min<int64_t>((int64_t)n_wg * mult, 4096 + n_rows / 32) / 8 * 8;
  }
  NR_PLAN_REQUIRE(n_wg >= 8 && n_wg <= 4096 + n_rows / 32, kErrUnsupported, "spmm_blocked: %d workgroups", n_wg);
  opt->n_wg = n_wg;
  return kOk;
}

// With a bipartite split the user rows and the item rows are classes of their own (they gather from
// disjoint halves of the table), each with its own workgroups.
inline std::vector<ClassDesc> assign_workgroups_to_classes(const int64_t* indptr, int64_t n_rows, const Options& opt) {
  const int n_wg = opt.n_wg;
  const int64_t split_row = opt.split_row;
  std::vector<ClassDesc> classes;
  if (!split_row) {
    ClassDesc a{0, n_rows, {}, 0, 1, 1};
    for (int w = 0; w < n_wg; ++w) a.wgs.push_back(w);
    classes.push_back(a);
    return classes;
  }
  ClassDesc a{0, split_row, {}, 0, 1, 1}, b{split_row, n_rows, {}, 0, 1, 1};
  // workgroups per class in proportion to the class's cost; class A fills XCDs 0.. first
  // (workgroup w runs on XCD w % 8), so at most one XCD serves both halves of the table
  int64_t cost_a = 0, cost_b = 0;
  for (int64_t r = 0; r < n_rows; ++r) (r < split_row ? cost_a : cost_b) += row_cost(indptr[r + 1] - indptr[r], opt.seg);
  int n_a = (int)((double)n_wg * (double)cost_a / (double)std::max<int64_t>(cost_a + cost_b, 1) + 0.5);
  n_a = std::min(std::max(n_a, 1), n_wg - 1);
  {
    // every class must still fit its rows into its workgroups' accumulators
    const int64_t cap = (int64_t)opt.r_max * 9 / 10;
    const int need_a = (int)((split_row + cap - 1) / cap), need_b = (int)((n_rows - split_row + cap - 1) / cap);
    n_a = std::max(n_a, std::min(need_a, n_wg - 1));
    n_a = std::min(n_a, std::max(n_wg - need_b, 1));
  }
  std::vector<int> order;                    // workgroup ids, XCD-major
  for (int x = 0; x < 8; ++x)
    for (int w = x; w < n_wg; w += 8) order.push_back(w);
  for (int i = 0; i < n_wg; ++i) (i < n_a ? a : b).wgs.push_back(order[i]);
  std::sort(a.wgs.begin(), a.wgs.end());
  std::sort(b.wgs.begin(), b.wgs.end());
  classes.push_back(a);
  classes.push_back(b);
  return classes;
}

// The column range a class gathers from is cut into K blocks of <= block_bytes; phase k of the kernel
// walks the sub-lists of block k.
inline int class_span_and_phases(const int64_t* indptr, const int32_t* indices, const Options& opt, ClassDesc* cl,
                                 Error* err) {
  int32_t cmin = INT32_MAX, cmax = -1;
  for (int64_t t = indptr[cl->ra]; t < indptr[cl->rb]; ++t) {
    cmin = std::min(cmin, indices[t]);
    cmax = std::max(cmax, indices[t]);
  }
  if (cmax < cmin) { cmin = 0; cmax = 0; }
  const int64_t span = (int64_t)cmax + 1 - cmin;
  const int64_t K = std::max<int64_t>((span * opt.d * 4 + opt.block_bytes - 1) / opt.block_bytes, 1);
  NR_PLAN_REQUIRE(K <= kMaxPhases, kErrUnsupported,
                  "spmm_blocked: gathered table of %lld rows needs %lld column blocks (max %d) — "
                  "use the work-item kernel", (long long)span, (long long)K, kMaxPhases);
  cl->cmin = cmin;
  cl->width = (span + K - 1) / K;
  cl->K = K;
  return kOk;
}

// Which rows a workgroup owns.  r01-r04: contiguous runs balanced by cost — fine while a row's length is
// independent of its id (the first synthetic twin shuffled the popularity ranks), but in real interaction data
// (and in the r05 twin, whose item popularity follows the real test split) popular items cluster in id: the
// run of hub rows then holds few rows and the runs of tail rows hit the accumulator cap (kRMax rows of ~8
// non-zeros = 0.7 of the cost target), which pushes the excess onto the other runs — the slowest workgroup of
// the item class carried 1.9x the mean cost and the pass took 50 us instead of 34.  r05: rows are DEALT —
// sorted by cost, each to the least-loaded workgroup that still has an accumulator (LPT) — so every
// workgroup gets the same cost whatever the numbering; the plan lists a workgroup's rows (row_of) and owns
// the (column, value) pairs in that order.  (The r01-r04 contiguous runs left the product in r06:
// profiles/r05_exp_entcost.txt has the A/B.)
// wg_rows[w]: the rows of workgroup w, slot order.
inline int deal_rows(const int64_t* indptr, const ClassDesc& cl, const Options& opt,
                     std::vector<std::vector<int32_t>>* wg_rows, Error* err) {
  const int64_t n_cl = cl.rb - cl.ra;
  const int64_t nw = (int64_t)cl.wgs.size();
  NR_PLAN_REQUIRE(n_cl <= nw * (int64_t)opt.r_max, kErrUnsupported,
                  "spmm_blocked: %lld rows do not fit %zu workgroups x %d accumulators — use the work-item kernel",
                  (long long)n_cl, cl.wgs.size(), opt.r_max);
  std::vector<int32_t> by_cost((size_t)n_cl);
  for (int64_t q = 0; q < n_cl; ++q) by_cost[(size_t)q] = (int32_t)(cl.ra + q);
  std::stable_sort(by_cost.begin(), by_cost.end(), [&](int32_t x, int32_t y) {
    return indptr[x + 1] - indptr[x] > indptr[y + 1] - indptr[y];
  });
  // min-heap of (cost so far, workgroup); a workgroup whose accumulators are all taken leaves the heap
  typedef std::pair<int64_t, int> Load;
  std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
  for (int i = 0; i < (int)nw; ++i) heap.push(Load(0, i));
  // rows that cannot be placed freely any more (as many rows left as free accumulators) are not an issue:
  // every workgroup in the heap has a free accumulator and n_cl <= nw * kRMax
  for (int32_t row : by_cost) {
    Load top = heap.top();
    heap.pop();
    std::vector<int32_t>& list = (*wg_rows)[(size_t)cl.wgs[(size_t)top.second]];
    list.push_back(row);
    top.first += row_cost(indptr[row + 1] - indptr[row], opt.seg);
    if ((int64_t)list.size() < opt.r_max) heap.push(top);
  }
  return kOk;
}

// run order: workgroup by workgroup; the packed (column, value) arrays follow it
inline int packed_order(const int64_t* indptr, const std::vector<std::vector<int32_t>>& wg_rows, Plan* h, Error* err) {
  const size_t n_wg = wg_rows.size();
  h->wg_row0.assign(n_wg, 0);
  h->wg_nrows.assign(n_wg, 0);
  h->row_of.assign((size_t)h->n_rows, 0);
  h->pk_src.assign((size_t)h->n_rows, 0);
  h->pk_dst.assign((size_t)h->n_rows + 1, 0);
  int64_t k = 0;
  for (size_t w = 0; w < n_wg; ++w) {
    h->wg_row0[w] = (int32_t)k;
    h->wg_nrows[w] = (int32_t)wg_rows[w].size();
    for (int32_t row : wg_rows[w]) {
      h->row_of[(size_t)k] = row;
      h->pk_src[(size_t)k] = (uint32_t)indptr[row];
      h->pk_dst[(size_t)k + 1] = h->pk_dst[(size_t)k] + (uint32_t)(indptr[row + 1] - indptr[row]);
      ++k;
    }
  }
  NR_PLAN_REQUIRE(k == h->n_rows, kErrArg, "spmm_blocked: internal: %lld of %lld rows scheduled", (long long)k,
                  (long long)h->n_rows);
  return kOk;
}

// One workgroup's rows cut into sub-lists: a row's non-zeros (ascending columns) fall into <= K contiguous
// sub-lists, one per column block; a sub-list longer than `seg` (a hub) is cut into segments with partial
// accumulators of their own (slots r_max ..) and a combine record that adds them in segment order.
// pk_first[si]: packed position of the first pair of rows[si].  ent / cmb: [K] lists, longest entries first.
inline int cut_rows_into_entries(const int64_t* indptr, const int32_t* indices, const ClassDesc& cl,
                                 const std::vector<int32_t>& rows, const uint32_t* pk_first, const Options& opt,
                                 std::vector<std::vector<Int4>>* ent, std::vector<std::vector<Int4>>* cmb, Error* err) {
  ent->assign((size_t)cl.K, {});
  cmb->assign((size_t)cl.K, {});
  std::vector<int> pcount((size_t)cl.K, 0);
  for (size_t si = 0; si < rows.size(); ++si) {
    const int64_t row = rows[si];
    const int32_t slot = (int32_t)si;
    const int64_t shift = (int64_t)pk_first[si] - indptr[row];     // CSR position -> packed position
    int64_t t = indptr[row];
    const int64_t te = indptr[row + 1];
    if (t == te) (*ent)[0].push_back(Int4{slot, 0, (int32_t)(uint32_t)(t + shift), (int32_t)row});   // empty row
    while (t < te) {
      const int64_t k = ((int64_t)indices[t] - cl.cmin) / cl.width;
      int64_t t2 = t + 1;
      const int64_t col_end = cl.cmin + (k + 1) * cl.width;       // first column of the next block
      while (t2 < te && indices[t2] < col_end) ++t2;
      const int64_t len = t2 - t;
      if (len <= opt.seg) {
        (*ent)[(size_t)k].push_back(Int4{slot, (int32_t)len, (int32_t)(uint32_t)(t + shift), (int32_t)row});
      } else {
        const int ns = (int)((len + opt.seg - 1) / opt.seg);
        NR_PLAN_REQUIRE(pcount[(size_t)k] + ns <= opt.p_max, kErrUnsupported,
                        "spmm_blocked: more than %d hub segments in one workgroup phase — use the "
                        "work-item kernel", opt.p_max);
        const int first = opt.r_max + pcount[(size_t)k];
        for (int sg = 0; sg < ns; ++sg)
          (*ent)[(size_t)k].push_back(Int4{first + sg, (int32_t)std::min<int64_t>(opt.seg, len - (int64_t)sg * opt.seg),
                                           (int32_t)(uint32_t)(t + shift + (int64_t)sg * opt.seg), (int32_t)row});
        (*cmb)[(size_t)k].push_back(Int4{slot, first, ns, (int32_t)row});
        pcount[(size_t)k] += ns;
      }
      t = t2;
    }
  }
  for (auto& v : *ent)
    std::stable_sort(v.begin(), v.end(), [](const Int4& a, const Int4& b) { return a.y > b.y; });
  return kOk;
}

// wg_ent / wg_cmb [wg][phase][...] -> the flat arrays with their [n_wg][n_phases + 1] offsets, and each
// workgroup's slice of the packed pairs (the staged masked kernel reads it in bulk)
inline void flatten_entries(const std::vector<std::vector<std::vector<Int4>>>& wg_ent,
                            const std::vector<std::vector<std::vector<Int4>>>& wg_cmb, Plan* h) {
  const int n_wg = h->n_wg, n_phases = h->n_phases;
  h->ent_off.assign((size_t)n_wg * (n_phases + 1), 0);
  h->cmb_off.assign((size_t)n_wg * (n_phases + 1), 0);
  for (int w = 0; w < n_wg; ++w) {
    for (int k = 0; k <= n_phases; ++k) {
      h->ent_off[(size_t)w * (n_phases + 1) + k] = (int32_t)h->ent.size();
      h->cmb_off[(size_t)w * (n_phases + 1) + k] = (int32_t)h->cmb.size();
      if (k < n_phases && (size_t)k < wg_ent[w].size()) {       // (a class may have fewer blocks than the other)
        h->ent.insert(h->ent.end(), wg_ent[w][(size_t)k].begin(), wg_ent[w][(size_t)k].end());
        h->cmb.insert(h->cmb.end(), wg_cmb[w][(size_t)k].begin(), wg_cmb[w][(size_t)k].end());
      }
    }
  }
  h->wg_nnz.assign((size_t)n_wg * 2, 0);
  int64_t nnz_cap = 0, ent_cap = 0;
  for (int w = 0; w < n_wg; ++w) {
    const int64_t b = h->pk_dst[(size_t)h->wg_row0[w]], en = h->pk_dst[(size_t)h->wg_row0[w] + (size_t)h->wg_nrows[w]];
    h->wg_nnz[2 * (size_t)w] = (uint32_t)b;
    h->wg_nnz[2 * (size_t)w + 1] = (uint32_t)(en - b);
    nnz_cap = std::max(nnz_cap, en - b);
    ent_cap = std::max<int64_t>(ent_cap, h->ent_off[(size_t)w * (n_phases + 1) + n_phases] -
                                             h->ent_off[(size_t)w * (n_phases + 1)]);
  }
  h->nnz_cap_exact = nnz_cap;
  h->nnz_cap = (int)std::min<int64_t>(nnz_cap, INT32_MAX / 16);
  h->ent_cap = (int)std::min<int64_t>((ent_cap + 15) / 16 * 16, INT32_MAX / 32);
}

// masked hops of a training step (d = 64, one phase): may the dedicated kernels run on this plan?
inline void masked_hop_switches(const Options& opt, Plan* h) {
  const bool on = opt.d == 64 && opt.waves == 16 && h->n_phases == 1 && opt.masked_fast;
  const size_t base = (size_t)opt.p_max * 256 + (size_t)h->ent_cap * 16;
  h->colmask_ok = on && h->nnz_cap_exact < ((int64_t)1 << 24) && h->n_rows < ((int64_t)1 << 24) &&
                  base + (size_t)h->nnz_cap_exact * 8 <= (size_t)kMaxLdsBytes;
  h->wanted_ok = on && opt.seg <= 255 && h->n_rows < ((int64_t)1 << 24);
}

// Staged wanted-rows schedule (row-masked hop, spmm_wanted_rows_kernel): the same sub-lists dealt to the
// workgroups by descending row length, descriptors carry global rows.  Clears wanted_ok when it does not fit.
inline void wanted_rows_schedule(const int64_t* indptr, const Options& opt, Plan* h) {
  const int n_wg = h->n_wg;
  const int64_t n_rows = h->n_rows;
  h->w_ent_off.assign((size_t)n_wg * 2, 0);
  h->w_cmb_off.assign((size_t)n_wg * 2, 0);
  if (!h->wanted_ok) return;
  std::vector<int32_t> order((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; ++r) order[(size_t)r] = (int32_t)r;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b];
  });
  std::vector<std::vector<Int4>> we((size_t)n_wg), wc((size_t)n_wg);
  std::vector<int> wp((size_t)n_wg, 0);
  for (int64_t k = 0; k < n_rows && h->wanted_ok; ++k) {
    const int32_t row = order[(size_t)k];
    const size_t w = (size_t)(k % n_wg);
    const int64_t b = indptr[row], len = indptr[row + 1] - b;
    if (len <= opt.seg) {
      we[w].push_back(Int4{0, (int32_t)len, (int32_t)(uint32_t)b, row});
    } else {
      const int ns = (int)((len + opt.seg - 1) / opt.seg);
      if (wp[w] + ns > opt.p_max) { h->wanted_ok = 0; break; }
      for (int sg = 0; sg < ns; ++sg)
        we[w].push_back(Int4{opt.r_max + wp[w] + sg, (int32_t)std::min<int64_t>(opt.seg, len - (int64_t)sg * opt.seg),
                             (int32_t)(uint32_t)(b + (int64_t)sg * opt.seg), row});
      wc[w].push_back(Int4{row, opt.r_max + wp[w], ns, 0});
      wp[w] += ns;
    }
  }
  for (int w = 0; w < n_wg && h->wanted_ok; ++w) {
    h->w_ent_off[2 * (size_t)w] = (int32_t)h->w_ent.size();
    h->w_cmb_off[2 * (size_t)w] = (int32_t)h->w_cmb.size();
    h->w_ent.insert(h->w_ent.end(), we[(size_t)w].begin(), we[(size_t)w].end());
    h->w_cmb.insert(h->w_cmb.end(), wc[(size_t)w].begin(), wc[(size_t)w].end());
    h->w_ent_off[2 * (size_t)w + 1] = (int32_t)h->w_ent.size();
    h->w_cmb_off[2 * (size_t)w + 1] = (int32_t)h->w_cmb.size();
    h->w_ent_cap = std::max<int>(h->w_ent_cap, (int)we[(size_t)w].size());
  }
  h->w_ent_cap = (h->w_ent_cap + 15) / 16 * 16;
  // LDS: partial slots + two descriptor lists + whatever is left for staged (column, value) pairs
  // a bit per row for the batch form of the kernel, when the matrix is small enough to afford it
  h->w_bitmap_words = n_rows <= 131072 ? (int)((n_rows + 127) / 128 * 4) : 0;
  const int64_t left = (int64_t)kMaxLdsBytes - 256 - (int64_t)opt.p_max * 256 - 2 * (int64_t)h->w_ent_cap * 16 -
                       (int64_t)h->w_bitmap_words * 4;
  h->w_nnz_cap = (int)std::min<int64_t>(left / 8, (int64_t)1 << 22);
  if (opt.wanted_nnz_cap > 0) h->w_nnz_cap = std::min(h->w_nnz_cap, std::max(opt.wanted_nnz_cap, 4 * opt.seg));
  if (h->w_nnz_cap < 4 * opt.seg) h->wanted_ok = 0;
}

// Wave-cooperative row-masked hop (spmm_wanted_wave_kernel): its own schedule — whole rows of <= 64
// non-zeros and CHUNKS of <= kWaveChunk consecutive 64-segments of longer rows are the units, dealt to
// the workgroups by descending length (a hub's bytes spread over several CUs).  Segment sums of one-chunk
// rows stay in LDS, those of multi-chunk rows go to global memory (ww_part).
inline void wanted_wave_schedule(const int64_t* indptr, const Options& opt, Plan* h) {
  const int n_wg = h->n_wg;
  const int64_t n_rows = h->n_rows;
  h->ww_off.assign((size_t)n_wg + 1, 0);
  h->ww_choff.assign((size_t)n_wg + 1, 0);
  h->ww_lcoff.assign((size_t)n_wg + 1, 0);
  if (!(opt.d == 64 && opt.waves == 16 && opt.seg <= 64 && n_rows <= 131072 * 4 && opt.wanted_wave)) return;
  // hub >= 0: chunk of a multi-chunk row (global partials); hub == -2: a one-chunk row of > 64
  // non-zeros (segment sums in LDS); hub == -1: a whole row of <= 64
  struct Unit { int64_t len; int32_t row; int hub, seg0, nseg; };
  std::vector<Unit> units;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t len = indptr[r + 1] - indptr[r];
    if (len <= opt.seg) {
      units.push_back(Unit{len, (int32_t)r, -1, 0, 0});
      continue;
    }
    const int ns = (int)((len + opt.seg - 1) / opt.seg), nch = (ns + kWaveChunk - 1) / kWaveChunk;
    if (nch == 1) {
      units.push_back(Unit{len, (int32_t)r, -2, 0, ns});
      continue;
    }
    const int hub = (int)h->ww_hub.size();
    h->ww_hub.push_back(Int4{(int32_t)r, (int32_t)h->ww_segments, ns, nch});
    for (int ch = 0; ch < nch; ++ch) {
      const int s0 = ch * kWaveChunk, s1 = std::min(ns, s0 + kWaveChunk);
      units.push_back(Unit{std::min<int64_t>(len - (int64_t)s0 * opt.seg, (int64_t)(s1 - s0) * opt.seg), (int32_t)r,
                           hub, s0, s1 - s0});
    }
    h->ww_segments += ns;
  }
  std::stable_sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) { return a.len > b.len; });
  std::vector<std::vector<Int4>> per((size_t)n_wg), perl((size_t)n_wg);
  std::vector<std::vector<int32_t>> perch((size_t)n_wg);
  std::vector<int> lds_used((size_t)n_wg, 0);
  for (size_t k = 0; k < units.size(); ++k) {
    const Unit& u = units[k];
    const size_t w = k % (size_t)n_wg;
    const int64_t b = indptr[u.row], len = indptr[u.row + 1] - b;
    auto segment = [&](int32_t slot, int sg) {
      return Int4{slot, (int32_t)std::min<int64_t>(opt.seg, len - (int64_t)sg * opt.seg),
                  (int32_t)(uint32_t)(b + (int64_t)sg * opt.seg), u.row};
    };
    if (u.hub == -1) {
      per[w].push_back(Int4{0, (int32_t)len, (int32_t)(uint32_t)b, u.row});
    } else if (u.hub == -2) {
      perl[w].push_back(Int4{u.row, lds_used[w], u.nseg, 0});
      for (int sg = 0; sg < u.nseg; ++sg) per[w].push_back(segment(-(1 + lds_used[w] + sg), sg));
      lds_used[w] += u.nseg;
    } else {
      for (int sg = u.seg0; sg < u.seg0 + u.nseg; ++sg) per[w].push_back(segment(1 + h->ww_hub[(size_t)u.hub].y + sg, sg));
      perch[w].push_back(u.hub);
    }
  }
  for (int w = 0; w < n_wg; ++w) {
    h->ww_off[(size_t)w] = (int32_t)h->ww_ent.size();
    h->ww_choff[(size_t)w] = (int32_t)h->ww_gch.size();
    h->ww_lcoff[(size_t)w] = (int32_t)h->ww_lcmb.size();
    h->ww_ent.insert(h->ww_ent.end(), per[(size_t)w].begin(), per[(size_t)w].end());
    h->ww_gch.insert(h->ww_gch.end(), perch[(size_t)w].begin(), perch[(size_t)w].end());
    h->ww_lcmb.insert(h->ww_lcmb.end(), perl[(size_t)w].begin(), perl[(size_t)w].end());
    h->ww_ent_cap = std::max<int>(h->ww_ent_cap, (int)per[(size_t)w].size());
    h->ww_lds_slots = std::max(h->ww_lds_slots, lds_used[(size_t)w]);
  }
  h->ww_off[(size_t)n_wg] = (int32_t)h->ww_ent.size();
  h->ww_choff[(size_t)n_wg] = (int32_t)h->ww_gch.size();
  h->ww_lcoff[(size_t)n_wg] = (int32_t)h->ww_lcmb.size();
  h->ww_ent_cap = (h->ww_ent_cap + 15) / 16 * 16;
  h->ww_ok = h->ww_segments < ((int64_t)1 << 30) &&
             (size_t)h->ww_lds_slots * 256 + (size_t)h->ww_ent_cap * 16 + (size_t)((n_rows + 127) / 128 * 16) + 1024 <=
                 (size_t)kMaxLdsBytes;
}

// The whole schedule of one matrix.  opt: resolve_options + choose_workgroup_count.
inline int build_plan(const int64_t* indptr, const int32_t* indices, int64_t n_rows, const Options& opt, Plan* h,
                      Error* err) {
  *h = Plan();
  h->n_rows = n_rows;
  h->nnz = indptr[n_rows] - indptr[0];
  h->n_wg = opt.n_wg;
  std::vector<ClassDesc> classes = assign_workgroups_to_classes(indptr, n_rows, opt);
  std::vector<std::vector<int32_t>> wg_rows((size_t)opt.n_wg);         // [wg] its rows, slot order
  for (ClassDesc& cl : classes) {
    NR_PLAN_TRY(class_span_and_phases(indptr, indices, opt, &cl, err));
    h->n_phases = std::max<int>(h->n_phases, (int)cl.K);
    NR_PLAN_TRY(deal_rows(indptr, cl, opt, &wg_rows, err));
  }
  NR_PLAN_TRY(packed_order(indptr, wg_rows, h, err));
  std::vector<std::vector<std::vector<Int4>>> wg_ent((size_t)opt.n_wg), wg_cmb((size_t)opt.n_wg);   // [wg][phase][entries]
  for (const ClassDesc& cl : classes)
    for (int w : cl.wgs)
      NR_PLAN_TRY(cut_rows_into_entries(indptr, indices, cl, wg_rows[(size_t)w], h->pk_dst.data() + h->wg_row0[(size_t)w],
                                        opt, &wg_ent[(size_t)w], &wg_cmb[(size_t)w], err));
  flatten_entries(wg_ent, wg_cmb, h);
  masked_hop_switches(opt, h);
  wanted_rows_schedule(indptr, opt, h);
  wanted_wave_schedule(indptr, opt, h);
  return kOk;
}

// ---- the plan's device buffer ----------------------------------------------------------------------------
// Device addresses of the schedule's arrays (I4: int4 on the device side, Int4 in host tests); what each
// array holds is said at the member of the same name in Plan.
template <class I4>
struct PlanArrays {
  I4* ent; I4* cmb;
  int32_t* wg_row0; int32_t* wg_nrows;
  // r05: the rows of a workgroup are a LIST, not a run: row_of[wg_row0[w] + slot] (see deal_rows) — and the
  // plan owns the (column, value) pairs in that order, so a workgroup's pairs stay one contiguous slice (the
  // staged masked kernel reads it in bulk).  ent[].z / wg_nnz index the packed arrays.
  int32_t* row_of; uint32_t* pk_src; uint32_t* pk_dst;
  int32_t* pk_idx; float* pk_val;          // [nnz] filled on the device (nrhip_spmm_blocked_pack)
  // the same pairs as 4-byte words (spmm_blocked_factor.h), when the values factor (nrhip_spmm_blocked_pack_factored):
  uint32_t* pk_word;                       // [nnz] column | code of the column's factor
  float* ent_rf;                           // [entries] the factor of the descriptor's row
  float* pk_table;                         // [kMaxFactorCodes] distinct factors
  uint16_t* pk_code;                       // [2 * n_rows] scratch of the pack: row codes, then column codes
  uint32_t* pk_bad;                        // [1] set by the pack's check when a product misses its value
  int32_t* wg_ent_off; int32_t* wg_cmb_off;
  uint32_t* wg_nnz;
  I4* w_ent; I4* w_cmb; int32_t* w_ent_off; int32_t* w_cmb_off;
  // only with ww_ok (else null)
  int32_t* ww_off; int32_t* ww_choff; I4* ww_ent; int32_t* ww_gch; I4* ww_hub; int32_t* ww_lcoff; I4* ww_lcmb;
  float* ww_part;        // [segments of multi-chunk rows][64] partial sums
  unsigned* ww_cnt;      // [multi-chunk rows] chunks finished (zero between launches)
};

// One array of the buffer: which PlanArrays pointer gets its address, where its bytes come from (nullptr:
// nothing is uploaded), how many bytes, the tail padding carved after them (kernels prefetch past the end),
// and whether the array starts zeroed instead.
struct Section {
  void* field;
  void (*set)(void* field, void* addr);
  const void* src;
  size_t bytes, pad;
  bool zero;
  void* addr;       // set by carve_sections
};
template <class T>
Section section(T*& field, const void* src, size_t bytes, size_t pad = 0, bool zero = false) {
  return Section{&field, [](void* f, void* a) { *(T**)f = (T*)a; }, src, bytes, pad, zero, nullptr};
}
template <class T, class V>
Section section(T*& field, const std::vector<V>& v, size_t pad = 0) {
  return section(field, v.data(), v.size() * sizeof(V), pad);
}

// THE layout: sizes, order, carving and upload all come from this list.  Each section starts 256-byte aligned.
template <class I4>
std::vector<Section> plan_sections(PlanArrays<I4>& p, const Plan& h) {
  std::vector<Section> s = {
      section(p.ent, h.ent, 16),
      section(p.cmb, h.cmb, 16),
      section(p.wg_row0, h.wg_row0),
      section(p.wg_nrows, h.wg_nrows),
      section(p.row_of, h.row_of),
      section(p.pk_src, h.pk_src),
      section(p.pk_dst, h.pk_dst),
      section(p.pk_idx, nullptr, (size_t)h.nnz * 4, 4),
      section(p.pk_val, nullptr, (size_t)h.nnz * 4, 4),
      section(p.wg_ent_off, h.ent_off),
      section(p.wg_cmb_off, h.cmb_off),
      section(p.wg_nnz, h.wg_nnz),
      section(p.w_ent, h.w_ent, 16),
      section(p.w_cmb, h.w_cmb, 16),
      section(p.w_ent_off, h.w_ent_off),
      section(p.w_cmb_off, h.w_cmb_off),
  };
  if (h.ww_ok) {
    s.push_back(section(p.ww_off, h.ww_off));
    s.push_back(section(p.ww_choff, h.ww_choff));
    s.push_back(section(p.ww_ent, h.ww_ent, 16));
    s.push_back(section(p.ww_gch, h.ww_gch, 4));
    s.push_back(section(p.ww_hub, h.ww_hub, 16));
    s.push_back(section(p.ww_lcoff, h.ww_lcoff));
    s.push_back(section(p.ww_lcmb, h.ww_lcmb, 16));
    s.push_back(section(p.ww_part, nullptr, (size_t)h.ww_segments * 256, 256));
    s.push_back(section(p.ww_cnt, nullptr, h.ww_hub.size() * 4, 4, true));
  }
  return s;
}

// The sections of the 4-byte non-zeros (spmm_blocked_factor.h), carved behind plan_sections' by the plan's creator;
// nothing is uploaded (nrhip_spmm_blocked_pack_factored fills them on the device).
template <class I4>
std::vector<Section> factor_sections(PlanArrays<I4>& p, const Plan& h) {
  return {
      section(p.pk_word, nullptr, (size_t)h.nnz * 4, 4),
      section(p.ent_rf, nullptr, h.ent.size() * 4, 4),
      section(p.pk_table, nullptr, (size_t)kPlanFactorCodes * 4),
      section(p.pk_code, nullptr, (size_t)h.n_rows * 4),
      section(p.pk_bad, nullptr, 4, 0, true),
  };
}

// gives every section its address in the buffer at `base`; returns the bytes used
inline size_t carve_sections(std::vector<Section>* sections, void* base) {
  size_t off = 0;
  for (Section& s : *sections) {
    s.addr = (void*)((uintptr_t)base + off);
    s.set(s.field, s.addr);
    off += align_up(s.bytes + s.pad, 256);
  }
  return off;
}

// Closed-form upper bound of carve_sections for any plan of such a matrix (the buffer is allocated before
// the plan exists).  Term by term against plan_sections:
inline size_t blocked_plan_bytes(int64_t n_rows, int64_t nnz) {
  // ent: a sub-list per row and phase at most, plus the extra segments of hubs; cmb / w_cmb / ww_hub / ww_lcmb /
  // ww_cnt: a record per row of > seg >= 16 non-zeros and phase
  const size_t max_ent = (size_t)std::min<int64_t>(nnz, n_rows * (int64_t)kMaxPhases) + (size_t)(nnz / 16) + 64;
  const size_t max_cmb = (size_t)(nnz / 16) + 64;
  const size_t wg = 4096 + (size_t)(n_rows / 32);   // generous bound on workgroups (choose_workgroup_count)
  const size_t w_ent = (size_t)n_rows + (size_t)(nnz / 16) + 64;        // wanted-rows schedule (one phase)
  // wave-cooperative wanted-rows schedule: an entry per row or 64-segment, a partial row per segment
  const size_t ww_seg = (size_t)(nnz / 32) + 64, ww_ents = (size_t)n_rows + ww_seg;
  const size_t ww = 3 * align_up((wg + 1) * 4, 256) /* ww_off, ww_choff, ww_lcoff */ +
                    align_up(ww_ents * 16 + 16, 256) /* ww_ent */ + align_up(ww_seg * 4 + 4, 256) /* ww_gch */ +
                    2 * align_up(max_cmb * 16 + 16, 256) /* ww_hub, ww_lcmb */ +
                    align_up(ww_seg * 256 + 256, 256) /* ww_part */ + align_up(max_cmb * 4 + 4, 256) /* ww_cnt */;
  const size_t dealt = 3 * align_up(((size_t)n_rows + 1) * 4, 256) /* row_of, pk_src, pk_dst */ +
                       3 * align_up((size_t)nnz * 4 + 4, 256) /* pk_idx, pk_val, pk_word */ +
                       align_up(max_ent * 4 + 4, 256) /* ent_rf */ + align_up((size_t)kPlanFactorCodes * 4, 256) +
                       align_up((size_t)n_rows * 4, 256) /* pk_code */ + 256 /* pk_bad */;
  return ww + dealt + align_up(max_ent * 16, 256) /* ent */ + align_up(max_cmb * 16, 256) /* cmb */ +
         3 * align_up(wg * 8, 256) /* wg_row0, wg_nrows, wg_nnz */ +
         2 * align_up(wg * (kMaxPhases + 1) * 4, 256) /* wg_ent_off, wg_cmb_off */ +
         align_up(w_ent * 16, 256) /* w_ent */ + align_up(max_cmb * 16, 256) /* w_cmb */ +
         2 * align_up(wg * 8, 256) /* w_ent_off, w_cmb_off */;
}

}  // namespace nr_plan
