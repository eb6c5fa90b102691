// spmm_blocked.hip — persistent-workgroup, lane-group SpMM  Y = Â·X  for d = 16 / 32 / 64 / 128 / 256
// (optionally cache-blocked by column windows).
//
// Why: at the gowalla shape one pass gathers 1.62 M rows of 256 B (415 MB) out of an 18 MB
// table.  A pure random-gather micro-benchmark of that pattern (scripts/exp_gather.py) tops out
// at ≈9 TB/s — the L2-miss path into the Infinity Cache — and the work-item kernel of spmm.hip
// already sits on that ceiling.  The same gathers run at 16-17 TB/s when (a) every XCD only
// touches a ≤2.6 MB window of the table at a time, so its private 4 MB L2 holds it, and (b) a load
// instruction moves four rows (16 lanes × 16 B each) instead of one
// (scripts/exp_gather_blocked.py).  This kernel is built on those two facts.
//
// Schedule (host, once per matrix; built by spmm_blocked_plan.h, which holds the reasons stage by stage):
//   * one workgroup per CU (16 waves), workgroup b on XCD b % 8.  With a bipartite split the
//     user rows go to XCDs 0-3 and the item rows to XCDs 4-7 (they gather from disjoint halves
//     of the table); the rows of a class are dealt to its workgroups by cost, longest first, so a
//     workgroup owns a LIST of rows (row_of) and every workgroup carries the same cost;
//   * the column range a class gathers from is cut into K blocks of ≤ block_bytes; a row's
//     non-zeros (ascending columns) fall into ≤ K contiguous sub-lists, one per block;
//   * phase k of the kernel walks the sub-lists of block k.  All workgroups of an XCD move
//     through the phases at about the same pace (equal work, no barrier needed), so the XCD's
//     L2 holds one block at a time.
// Kernel: every row of the workgroup has a 256-byte accumulator in LDS that lives across the
// phases.  A 16-lane group owns one sub-list: it loads the accumulator, adds a_j·X[col_j] in
// ascending column order (products and sums rounded separately — the order of the reference's
// CPU kernel, so rows are bit-identical to oracle/), and stores it back.  Sub-lists longer
// than 64 are cut into segments with their own partial accumulators, added in segment order
// after the phase (deterministic; only such hub rows deviate from the sequential order).
// Epilogue as in spmm.hip: y += addend, sum_out = sum_in + y.
#include "nr_common.h"
#include "spmm_blocked_plan.h"
#include "spmm_blocked_factor.h"
#include "spmm_wanted_plan.h"
#include <algorithm>
#include <new>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace {

using nr_plan::kMaxLdsBytes;
using nr_plan::blocked_plan_bytes;
static_assert((int)nr_plan::kOk == NR_OK && (int)nr_plan::kErrArg == NR_ERR_ARG &&
              (int)nr_plan::kErrUnsupported == NR_ERR_UNSUPPORTED, "the planner returns the C ABI's status codes");

// The plan behind the C handle: the device addresses of the schedule's arrays (spmm_blocked_plan.h, where the
// layout of the buffer is listed) and the scalars the launches need.
struct BlockedPlan : nr_plan::PlanArrays<int4> {
  int64_t n_rows, nnz, n_ent, n_cmb;
  int pk_on, pk_codes, pk_col_bits;   // the 4-byte words stand for the packed pairs (verified); table entries; column bits
  int n_wg, n_phases;
  int seg, r_max, p_max, waves, d;
  const int32_t* pk_from_idx;   // the CSR arrays the packed copy was made from (nullptr: not yet)
  const float* pk_from_val;
  // masked hops of a training step (d = 64, one phase): dedicated kernels below
  int nnz_cap, ent_cap;  // largest slice / descriptor list of a workgroup
  int colmask_ok;
  int wanted_ok, w_ent_cap, w_nnz_cap, w_bitmap_words;      // staged wanted-rows schedule (row-masked hop)
  int ww_ok, ww_ent_cap;                                    // wave-cooperative row-masked hop
  int ww_lds_slots;      // LDS partial slots per workgroup
  int wp_ok, n_hubs;     // planned row-masked hop (spmm_wanted_plan.h): allowed; records in ww_hub
  nr_wplan::SlotProfile wp_profile;
};


// Store policy of a hop's row output Y (compile time).  A plain store leaves the line dirty in the XCD's L2 until
// the kernel boundary writes it back, and the next launch waits for that; the other two let it leave while the
// kernel still runs: nontemporal, or written through (sc1) with a raw buffer store (y_bytes: the size of Y, the
// descriptor's range; offsets are 32 bits).  Same bytes.  Measured: profiles/r18_latency_chain.txt.
enum { kStorePlain = 0, kStoreNt = 1, kStoreWt = 2 };
typedef float nr_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int nr_u32x4 __attribute__((ext_vector_type(4)));

template <int ST>
__device__ __forceinline__ void row_store(float4* __restrict__ Y, uint32_t y_bytes, int64_t o, float4 y) {
  if constexpr (ST == kStoreNt) {
    __builtin_nontemporal_store(nr_f32x4{y.x, y.y, y.z, y.w}, (nr_f32x4*)(Y + o));
  } else if constexpr (ST == kStoreWt) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)Y, 0, (int)y_bytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(nr_u32x4{__float_as_uint(y.x), __float_as_uint(y.y), __float_as_uint(y.z),
                                                    __float_as_uint(y.w)},
                                           rs, (int)(uint32_t)(o * 16), 0, 16);
  } else {
    Y[o] = y;
  }
}


// Optional fused optimiser epilogue (last backward hop of a LightGCN step): instead of storing
// y, treat g = y + grad_b[row] as the dense gradient of `var` and apply TF-1.12 ApplyAdam to the
// row (training_ops: m += (g-m)(1-b1); v += (g²-v)(1-b2); var -= m·alpha/(sqrt(v)+eps)).
struct AdamEpilogue {
  float4* var; float4* m; float4* v; const float4* grad_b;
  float alpha, omb1, omb2, eps;
  // optional: re-arm the step's sparse buffers on the way (what rows_clear would do afterwards):
  // zero the addend / grad_b entries that were non-zero and the row flags
  float4* addend_rw; float4* grad_b_rw; uint8_t* flag_rw;
};


// The packed pairs as 4-byte words (spmm_blocked_factor.h), handed to the kernels that walk the plan's schedule:
// word = column | code << col_bits, value = __fmul_rn(factor of the sub-list's row, table[code]) — verified equal to
// the stored value for every non-zero when the plan was packed.  word == nullptr: the two arrays are read.
static_assert(nr_plan::kMaxFactorCodes == 16 * NR_WAVE, "a 16-wave workgroup stages the factor table one entry per thread");
struct PackedNz {
  const uint32_t* word; const float* ent_rf; const float* table;
  int n_codes, col_bits;
};

// An entry of the workgroup's staged row list: the row, and in the sign bit "this row's flag is 0" (rows are < 2^31).
constexpr int kRowBits = 0x7FFFFFFF;
constexpr int kRowUnflagged = (int)0x80000000u;

// Epilogue shared by the full-pass kernels: the workgroup's finished row sums sit in LDS
// (s_acc[slot][LPR]); y += addend, then either the ApplyAdam epilogue or the stores of y and of the
// running layer sum — a row is LPR lanes x 16 B (whole cache lines at d >= 32), so a row LIST
// streams as well as a row run.
template <bool MASKED, bool ADAM, int LPR>
__device__ __forceinline__ void blocked_epilogue(const float4* s_acc, int r0, int nr, int tid, int nthreads,
                                                 float4* __restrict__ Y, const float4* __restrict__ addend,
                                                 const float4* sum_in, float4* sum_out,
                                                 const uint8_t* __restrict__ row_mask, const AdamEpilogue& ad,
                                                 const int32_t* s_rows = nullptr) {
  for (int i = tid; i < nr * LPR; i += nthreads) {
    // s_rows: the workgroup's row list (LDS; dealt rows), else its rows are the run [r0, r0 + nr)
    const int rw = s_rows ? s_rows[i / LPR] : r0 + i / LPR;
    const int row = rw & kRowBits;
    if constexpr (MASKED) {
      if (row_mask && row_mask[row] == 0) continue;
    }
    const int64_t o = (int64_t)row * LPR + (i & (LPR - 1));
    float4 y = s_acc[i];
    // with row flags (the addend of a backward hop, the step buffers the Adam pass re-arms) the addend / grad_b rows
    // of unflagged rows are all zero by contract and are not read: these streams touch batch rows only.  The flag
    // was staged with the row list (kRowUnflagged), so the loads below wait for LDS, not for a flag from memory.
    const bool flagged = rw >= 0;
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (addend) {
      if (flagged) hv = addend[o];
      y.x = __fadd_rn(y.x, hv.x); y.y = __fadd_rn(y.y, hv.y);
      y.z = __fadd_rn(y.z, hv.z); y.w = __fadd_rn(y.w, hv.w);
    }
    if constexpr (ADAM) {
      float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
      if (flagged) gb = ad.grad_b[o];
      if (ad.addend_rw) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hv.x != 0.f || hv.y != 0.f || hv.z != 0.f || hv.w != 0.f) ad.addend_rw[o] = zero;
        if (gb.x != 0.f || gb.y != 0.f || gb.z != 0.f || gb.w != 0.f) ad.grad_b_rw[o] = zero;
        if ((i & (LPR - 1)) == 0 && ad.flag_rw && flagged) ad.flag_rw[row] = 0;
      }
      float4 w = ad.var[o], mm = ad.m[o], vv = ad.v[o];
      nr::adam_dense_tf(__fadd_rn(y.x, gb.x), w.x, mm.x, vv.x, ad.alpha, ad.omb1, ad.omb2, ad.eps);
      nr::adam_dense_tf(__fadd_rn(y.y, gb.y), w.y, mm.y, vv.y, ad.alpha, ad.omb1, ad.omb2, ad.eps);
      nr::adam_dense_tf(__fadd_rn(y.z, gb.z), w.z, mm.z, vv.z, ad.alpha, ad.omb1, ad.omb2, ad.eps);
      nr::adam_dense_tf(__fadd_rn(y.w, gb.w), w.w, mm.w, vv.w, ad.alpha, ad.omb1, ad.omb2, ad.eps);
      ad.var[o] = w; ad.m[o] = mm; ad.v[o] = vv;
      continue;
    }
    if (Y) {
      // the d = 64 full passes write Y through: its 18 MB do not wait dirty in the L2s for the kernel boundary
      if constexpr (LPR == 16 && !MASKED) {
        if ((uint64_t)o * 16 + 16 <= 0xFFFFFFFFull) row_store<kStoreWt>(Y, 0xFFFFFFFFu, o, y);
        else Y[o] = y;
      } else {
        Y[o] = y;
      }
    }
    if (sum_out) {
      const float4 si = sum_in[o];
      sum_out[o] = make_float4(__fadd_rn(si.x, y.x), __fadd_rn(si.y, y.y), __fadd_rn(si.z, y.z),
                               __fadd_rn(si.w, y.w));
    }
  }
}

// per-workgroup phase stamps (experiments: build with NEUREC_HIPCC_EXTRA=-DNR_BLK_TIMELINE, scripts/exp_blk_timeline.py)
#ifdef NR_BLK_TIMELINE
__device__ unsigned long long g_blk_dbg[4096 * 24];
#define NR_BLK_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_blk_dbg[blockIdx.x * 24 + (i)] = wall_clock64(); } while (0)
#define NR_BLK_WSTAMP() do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096) g_blk_dbg[blockIdx.x * 24 + 8 + (threadIdx.x >> 6)] = wall_clock64(); } while (0)
extern "C" int nrhip_exp_blk_timeline(unsigned long long* h_out) {
  if (hipDeviceSynchronize() != hipSuccess) return NR_ERR_HIP;
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_blk_dbg), sizeof(unsigned long long) * 4096 * 24) == hipSuccess ? NR_OK : NR_ERR_HIP;
}
#else
#define NR_BLK_STAMP(i) do {} while (0)
#define NR_BLK_WSTAMP() do {} while (0)
#endif

template <bool MASKED, int kWaves, int kG, int D, bool ADAM = false>
__global__ __launch_bounds__(kWaves* NR_WAVE) void spmm_blocked_kernel(
    const int32_t* __restrict__ wg_row0, const int32_t* __restrict__ wg_nrows,
    const int32_t* __restrict__ wg_ent_off, const int32_t* __restrict__ wg_cmb_off,
    const int4* __restrict__ ent, const int4* __restrict__ cmb, int n_phases,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const float4* __restrict__ X, float4* __restrict__ Y, const float4* __restrict__ addend,
    const float4* sum_in, float4* sum_out, const uint8_t* __restrict__ col_mask,
    const uint8_t* __restrict__ row_mask, int kRMax, AdamEpilogue ad, const int32_t* __restrict__ row_of,
    int kPMax, const uint8_t* __restrict__ addend_flag, PackedNz pk) {
  constexpr int LPR = D / 4;                   // lanes per row: 16-byte pieces of a d-float row
  constexpr int GPW = NR_WAVE / LPR;           // lane groups (rows in flight) per wave: 4 / 2 / 1
  constexpr int kGroups = kWaves * GPW;
  // a 16-entry (column, value) chunk of a sub-list is carried by CL lanes of the group, IPL
  // entries each (narrow rows have fewer than 16 lanes per group)
  constexpr int CL = LPR < 16 ? LPR : 16;
  constexpr int IPL = 16 / CL;
  static_assert(kG % IPL == 0, "broadcast component must be a compile-time index");
  extern __shared__ float4 s_acc[];          // [(r_max + p_max)][LPR], then the row list [r_max]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & (LPR - 1), g = lane / LPR, gbase = lane & ~(LPR - 1);
  const int wg = blockIdx.x;
  NR_BLK_STAMP(0);
  const int r0 = wg_row0[wg], nr = wg_nrows[wg];
  int32_t* s_rows = (int32_t*)(s_acc + (size_t)(kRMax + kPMax) * LPR);
  // packed non-zeros (workgroup-uniform): `indices` holds the words, `vals` is not read, the factor table sits in
  // LDS behind the row list.  A lane decodes the entries it carries, once each, before the shuffles broadcast them.
  const bool packed = pk.word != nullptr;
  if (packed) indices = (const int32_t*)pk.word;
  float* s_tab = (float*)(s_rows + kRMax);
  const uint32_t cmask = (1u << pk.col_bits) - 1u;
  // the table's loads go out first and land in LDS behind the row list's: one round trip under the others, not one more
  constexpr int kTabPer = nr_plan::kMaxFactorCodes / (kWaves * NR_WAVE);
  float tab_v[kTabPer];
#pragma unroll
  for (int j = 0; j < kTabPer; ++j) {
    tab_v[j] = 0.f;
    if (packed && tid + j * kWaves * NR_WAVE < pk.n_codes) tab_v[j] = pk.table[tid + j * kWaves * NR_WAVE];
  }
  // the row list, read back in the epilogue, and with it the rows' flags (addend_flag: 0 = the addend row is zero
  // and is not read; the Adam pass takes the step's own flags): one byte gather per row here, none in the epilogue
  const uint8_t* fl = ADAM ? ad.flag_rw : addend_flag;                           // workgroup-uniform
  // (keeping a thread's entry in registers over the walk, so that the flag's round trip runs under the walk's first
  // loads, measured the same: profiles/r19_addend_by_flag.txt)
  for (int i = tid; i < nr; i += kWaves * NR_WAVE) {
    int row = row_of[r0 + i];
    if (fl && fl[row] == 0) row |= kRowUnflagged;
    s_rows[i] = row;
  }
  for (int i = tid; i < nr * LPR; i += kWaves * NR_WAVE) s_acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < kTabPer; ++j)
    if (packed && tid + j * kWaves * NR_WAVE < pk.n_codes) s_tab[tid + j * kWaves * NR_WAVE] = tab_v[j];
  __syncthreads();
  NR_BLK_STAMP(1);
  const int32_t* eoff = wg_ent_off + (int64_t)wg * (n_phases + 1);
  const int32_t* coff = wg_cmb_off + (int64_t)wg * (n_phases + 1);
  for (int k = 0; k < n_phases; ++k) {
    const int e0 = eoff[k], e1 = eoff[k + 1];
    // Software pipeline over this lane group's sub-lists (entries ei, ei+64, ...): the next
    // entry's descriptor is requested before, and its first 16 (column, value) pairs right
    // after, the current entry's gathers are issued — so in steady state a sub-list costs one
    // gather round trip, not three dependent ones.
    int ei = e0 + wave * GPW + g;
    int4 cur = make_int4(0, 0, 0, 0);
    float cur_rf = 0.f;                              // the factor of the entry's row: read beside the descriptor
    if (ei < e1) {
      cur = ent[ei];
      if (packed) cur_rf = pk.ent_rf[ei];
    }
    int cur_idx[IPL];
    float cur_val[IPL];
#pragma unroll
    for (int i = 0; i < IPL; ++i) {
      cur_idx[i] = 0;
      cur_val[i] = 0.f;
      if (c < CL && c * IPL + i < cur.y) {
        cur_idx[i] = indices[(uint32_t)cur.z + c * IPL + i];
        if (!packed) cur_val[i] = vals[(uint32_t)cur.z + c * IPL + i];
      }
    }
    int cur_want = 1;                                // row filter of the current entry (prefetched)
    if constexpr (MASKED) {
      if (row_mask && ei < e1) cur_want = row_mask[cur.w];
    }
    for (int base = e0 + wave * GPW; base < e1; base += kGroups) {
      const bool live = ei < e1;
      const int ein = ei + kGroups;
      int4 nxt = make_int4(0, 0, 0, 0);
      float nxt_rf = 0.f;
      if (ein < e1) {
        nxt = ent[ein];
        if (packed) nxt_rf = pk.ent_rf[ein];
      }
      const int slot = cur.x;
      int len = cur.y;
      const uint32_t begin = (uint32_t)cur.z;
      if constexpr (MASKED) {
        if (cur_want == 0) len = 0;                                    // output row not wanted
      }
      int nxt_want = 1;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && slot < kRMax) acc = s_acc[slot * LPR + c];           // segments start from zero
      int maxlen = len;
#pragma unroll
      for (int m = LPR; m < NR_WAVE; m <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, m, NR_WAVE));
      maxlen = __builtin_amdgcn_readfirstlane(maxlen);
      int nxt_idx[IPL];
      float nxt_val[IPL];
#pragma unroll
      for (int i = 0; i < IPL; ++i) { nxt_idx[i] = 0; nxt_val[i] = 0.f; }
      int ch_idx[IPL];                               // the NEXT 16-entry chunk of this sub-list, requested while
      float ch_val[IPL];                             // the current chunk's gathers are in flight
#pragma unroll
      for (int i = 0; i < IPL; ++i) { ch_idx[i] = 0; ch_val[i] = 0.f; }
      for (int k0 = 0; k0 < maxlen || k0 == 0; k0 += 16) {
        int my_idx[IPL];
        float my_val[IPL];
#pragma unroll
        for (int i = 0; i < IPL; ++i) {
          my_idx[i] = k0 == 0 ? cur_idx[i] : ch_idx[i];
          my_val[i] = k0 == 0 ? cur_val[i] : ch_val[i];
          if (packed) {                              // entries past the end hold word 0: never used (on[] / nn)
            const uint32_t w = (uint32_t)my_idx[i];
            my_idx[i] = (int)(w & cmask);
            my_val[i] = __fmul_rn(cur_rf, s_tab[w >> pk.col_bits]);
          }
          if constexpr (MASKED) {
            if (col_mask && c < CL && k0 + c * IPL + i < len && col_mask[my_idx[i]] == 0)
              my_idx[i] = -1;                        // X row all zero
          }
        }
        const int nn = min(16, maxlen - k0);
        for (int t0 = 0; t0 < nn || (k0 == 0 && t0 == 0); t0 += kG) {
          float a[kG];
          float4 x[kG];
          bool on[kG];
#pragma unroll
          for (int u = 0; u < kG; ++u) {
            // entry t0+u of the chunk sits in lane (t0+u)/IPL of the group, component u % IPL
            // (t0 is a multiple of kG, kG of IPL)
            const int src = gbase | (((t0 + u) & 15) / IPL);
            const int col = __shfl(my_idx[u % IPL], src, NR_WAVE);
            a[u] = __shfl(my_val[u % IPL], src, NR_WAVE);
            on[u] = k0 + t0 + u < len;
            if constexpr (MASKED) {
              on[u] = on[u] && col >= 0;
              x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
              if (on[u]) x[u] = X[(int64_t)col * LPR + c];
            } else {
              x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
              if (t0 + u < nn) x[u] = X[(int64_t)max(col, 0) * LPR + c];   // wave-uniform guard
            }
          }
          if (t0 == 0 && k0 + 16 < maxlen) {         // a long sub-list: its next chunk (wave-uniform guard) — a chunk
#pragma unroll                                       // used to cost index round trip + gather round trips in sequence
            for (int i = 0; i < IPL; ++i) {
              ch_idx[i] = 0;
              ch_val[i] = 0.f;
              if (c < CL && k0 + 16 + c * IPL + i < len) {
                ch_idx[i] = indices[begin + k0 + 16 + c * IPL + i];
                if (!packed) ch_val[i] = vals[begin + k0 + 16 + c * IPL + i];
              }
            }
          }
          if (k0 == 0 && t0 == 0) {                  // prefetch for the next sub-list: first chunk, row filter
#pragma unroll
            for (int i = 0; i < IPL; ++i)
              if (c < CL && c * IPL + i < nxt.y) {
                nxt_idx[i] = indices[(uint32_t)nxt.z + c * IPL + i];
                if (!packed) nxt_val[i] = vals[(uint32_t)nxt.z + c * IPL + i];
              }
            if constexpr (MASKED) {
              if (row_mask && ein < e1) nxt_want = row_mask[nxt.w];
            }
          }
#pragma unroll
          for (int u = 0; u < kG; ++u)
            if (on[u]) {
              acc.x = __fadd_rn(acc.x, __fmul_rn(a[u], x[u].x));
              acc.y = __fadd_rn(acc.y, __fmul_rn(a[u], x[u].y));
              acc.z = __fadd_rn(acc.z, __fmul_rn(a[u], x[u].z));
              acc.w = __fadd_rn(acc.w, __fmul_rn(a[u], x[u].w));
            }
        }
      }
      if (live) s_acc[slot * LPR + c] = acc;
      cur = nxt;
      cur_rf = nxt_rf;
#pragma unroll
      for (int i = 0; i < IPL; ++i) { cur_idx[i] = nxt_idx[i]; cur_val[i] = nxt_val[i]; }
      cur_want = nxt_want;
      ei = ein;
    }
    NR_BLK_WSTAMP();
    const int c0 = coff[k], c1 = coff[k + 1];
    if (c1 > c0) {                                  // workgroup-uniform
      __syncthreads();
      NR_BLK_STAMP(2);
      for (int ci = c0 + wave * GPW + g; ci < c1; ci += kGroups) {
        const int4 cm = cmb[ci];
        float4 acc = s_acc[cm.x * LPR + c];
        for (int s = 0; s < cm.z; ++s) {
          const float4 p = s_acc[(cm.y + s) * LPR + c];
          acc.x = __fadd_rn(acc.x, p.x); acc.y = __fadd_rn(acc.y, p.y);
          acc.z = __fadd_rn(acc.z, p.z); acc.w = __fadd_rn(acc.w, p.w);
        }
        s_acc[cm.x * LPR + c] = acc;
      }
    }
    __syncthreads();
  }
  NR_BLK_STAMP(3);
  blocked_epilogue<MASKED, ADAM, LPR>(s_acc, r0, nr, tid, kWaves * NR_WAVE, Y, addend, sum_in, sum_out,
                                      row_mask, ad, s_rows);
  NR_BLK_STAMP(4);
}


// ---------------------------------------------------------------------------------------------
// The masked hops of a LightGCN step (d = 64).  Column-masked (first backward hop): only columns of
// batch rows contribute.  In the general masked kernel above it costs 27-29 us: every lane group still walks
// all its sub-lists through the descriptor -> columns -> mask -> rows chain.  Here the workgroup's
// (column, value) slice is staged in LDS with one bulk read, the mask is applied there, every
// sub-list is compacted in place, and the walk only sees the survivors, several sub-lists in
// flight per lane group (no accumulators in LDS: a finished row goes straight to memory).
// Same sub-lists, same order of additions, same combine: bit-identical to spmm_blocked_kernel.
// (The mirror-image kernel for the row-masked forward hop — a wave per wanted sub-list — was built
// too and removed: a real batch is dominated by hub rows, whose gathers are ~45 % of a full pass,
// so that hop is bound by gather throughput, not by the walk: profiles/r01_exp_masked_hops.txt.)

struct LayerChain { const float4* a; const float4* b; };
__device__ __forceinline__ int4 zero_int4() { return make_int4(0, 0, 0, 0); }   // optional further terms of the running sum

__device__ __forceinline__ float4 chain_sum(float4 si, const LayerChain& ch, int64_t o) {
  if (ch.a) {
    const float4 t = ch.a[o];
    si = make_float4(__fadd_rn(si.x, t.x), __fadd_rn(si.y, t.y), __fadd_rn(si.z, t.z), __fadd_rn(si.w, t.w));
  }
  if (ch.b) {
    const float4 t = ch.b[o];
    si = make_float4(__fadd_rn(si.x, t.x), __fadd_rn(si.y, t.y), __fadd_rn(si.z, t.z), __fadd_rn(si.w, t.w));
  }
  return si;
}

template <int ST = kStorePlain>
__device__ __forceinline__ void masked_row_out(float4 y, int64_t o, const float4* __restrict__ addend,
                                               bool addend_row_nonzero, float4* __restrict__ Y,
                                               const float4* sum_in, float4* sum_out,
                                               const LayerChain* chain = nullptr, uint32_t y_bytes = 0) {
  if (addend) {
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f);       // a row promised zero is not read
    if (addend_row_nonzero) av = addend[o];
    y.x = __fadd_rn(y.x, av.x); y.y = __fadd_rn(y.y, av.y);
    y.z = __fadd_rn(y.z, av.z); y.w = __fadd_rn(y.w, av.w);
  }
  if (Y) row_store<ST>(Y, y_bytes, o, y);
  if (sum_out) {
    float4 si = sum_in[o];
    if (chain) si = chain_sum(si, *chain, o);
    sum_out[o] = make_float4(__fadd_rn(si.x, y.x), __fadd_rn(si.y, y.y), __fadd_rn(si.z, y.z),
                             __fadd_rn(si.w, y.w));
  }
}

// Walk of LDS-staged sub-lists by 16-lane groups (d = 64): rounds of kQ gathers per lane, three
// rounds in flight (the staged sub-lists are short, so depth comes from running several of them
// ahead); rounds retire in issue order.  s_ent[i] = {accumulator slot, length, offset into s_iv,
// row - r0 | bit 30: addend row may be non-zero | bit 29: row not wanted}.
// Every round issues exactly kQ + 1 loads, unconditionally (idle lanes and rounds read row 0 of X):
// only then can the compiler count the loads younger than the round it retires and wait with
// vmcnt(N > 0); with predicated loads it must assume none were issued and waits for all of them
// (vmcnt(0)), which silently turns the ring into one round in flight (measured: 14 us -> see
// profiles/r01_exp_masked_hops.txt).  The "+ 1" is the epilogue operand of the row a round
// completes (addend, else sum_in), requested with the round's gathers for the same reason.
// ST: store policy of Y (row_store; only the column-masked backward hop asks for another than plain).
template <int ST = kStorePlain>
__device__ __forceinline__ void staged_walk(const int4* s_ent, const int2* s_iv, int ne, int r0,
                                            const float4* __restrict__ X, float4* __restrict__ Y,
                                            const float4* __restrict__ addend, const float4* sum_in,
                                            float4* sum_out, float4* s_part, int kRMax, int wave,
                                            int g, int c, LayerChain chain = LayerChain{nullptr, nullptr},
                                            uint32_t y_bytes = 0) {
  constexpr int RS = 16, LPR = 16, GPW = 4, kGroups = 64;
  constexpr int kQ = 4;
  struct Round { float4 x[kQ]; float4 pre; int off, n, slot, owner; bool first, last, live, valid; };
  const float4* pre_src = addend ? addend : (sum_in ? sum_in : X);   // workgroup-uniform, never null
  int ibase = wave * GPW, it0 = 0, imax = 0;      // issue cursor: batch of sub-lists, position
  int4 ids = make_int4(0, 0, 0, 0);
  bool ihas = ibase < ne;                         // wave-uniform: rounds left to issue
  auto open = [&]() {
    ids = make_int4(0, 0, 0, 0);
    if (ibase + g < ne) ids = s_ent[ibase + g];
    int m = ids.y;
#pragma unroll
    for (int sh = LPR; sh < NR_WAVE; sh <<= 1) m = max(m, __shfl_xor(m, sh, NR_WAVE));
    imax = __builtin_amdgcn_readfirstlane(m);
  };
  auto issue = [&](Round& r) {
    r.valid = ihas;
    r.off = ids.z + it0;
    r.n = ihas ? ids.y - it0 : 0;
    r.slot = ids.x;
    r.owner = ids.w;
    r.first = it0 == 0;
    r.live = ihas && ibase + g < ne;
    r.last = ihas && it0 + kQ >= imax;
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
      int col = s_iv[u < r.n ? r.off + u : 0].x;
      if (u >= r.n) col = 0;
      r.x[u] = X[(int64_t)col * RS + c];
    }
    const bool want_pre = r.last && r.live && r.slot < kRMax && !((r.owner >> 29) & 1) &&
                          (!addend || ((r.owner >> 30) & 1));
    r.pre = pre_src[(want_pre ? ((int64_t)r0 + (r.owner & 0xFFFFFF)) * RS : 0) + c];
    if (r.last) {
      ibase += kGroups;
      it0 = 0;
      ihas = ibase < ne;
      if (ihas) open();
    } else if (ihas) {
      it0 += kQ;
    }
  };
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  auto retire = [&](const Round& r) {
    if (r.first) acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float a[kQ];
#pragma unroll
    for (int u = 0; u < kQ; ++u) a[u] = __int_as_float(s_iv[u < r.n ? r.off + u : 0].y);
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
      const float4 t = make_float4(__fadd_rn(acc.x, __fmul_rn(a[u], r.x[u].x)),
                                   __fadd_rn(acc.y, __fmul_rn(a[u], r.x[u].y)),
                                   __fadd_rn(acc.z, __fmul_rn(a[u], r.x[u].z)),
                                   __fadd_rn(acc.w, __fmul_rn(a[u], r.x[u].w)));
      if (u < r.n) acc = t;
    }
    if (r.last && r.live && !((r.owner >> 29) & 1)) {
      if (r.slot < kRMax) {
        const int64_t o = ((int64_t)r0 + (r.owner & 0xFFFFFF)) * RS + c;
        float4 y = acc;
        if (addend) {
          float4 av = make_float4(0.f, 0.f, 0.f, 0.f);     // a row promised zero was not read
          if ((r.owner >> 30) & 1) av = r.pre;
          y.x = __fadd_rn(y.x, av.x); y.y = __fadd_rn(y.y, av.y);
          y.z = __fadd_rn(y.z, av.z); y.w = __fadd_rn(y.w, av.w);
        }
        if (Y) row_store<ST>(Y, y_bytes, o, y);
        if (sum_out) {
          float4 si = r.pre;
          if (addend) si = sum_in[o];                      // both operands: this one is read late
          si = chain_sum(si, chain, o);
          sum_out[o] = make_float4(__fadd_rn(si.x, y.x), __fadd_rn(si.y, y.y), __fadd_rn(si.z, y.z),
                                   __fadd_rn(si.w, y.w));
        }
      } else {
        s_part[(size_t)(r.slot - kRMax) * RS + c] = acc;
      }
    }
  };
  Round q0, q1, q2;                               // three rounds in flight: what 128 VGPRs hold
  if (ihas) open();
  issue(q0);
  issue(q1);
  while (true) {
    issue(q2);
    if (!q0.valid) break;
    retire(q0);
    issue(q0);
    if (!q1.valid) break;
    retire(q1);
    issue(q1);
    if (!q2.valid) break;
    retire(q2);
  }
}

template <bool COLMASK, bool ROWMASK, int ST = kStorePlain>
__global__ __launch_bounds__(16 * NR_WAVE) void spmm_staged_masked_kernel(
    const int32_t* __restrict__ wg_row0, const int32_t* __restrict__ wg_ent_off,
    const int32_t* __restrict__ wg_cmb_off, const uint32_t* __restrict__ wg_nnz,
    const int4* __restrict__ ent, const int4* __restrict__ cmb,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const float4* __restrict__ X, float4* __restrict__ Y, const float4* __restrict__ addend,
    const float4* sum_in, float4* sum_out, const uint8_t* __restrict__ col_mask,
    const uint8_t* __restrict__ row_mask, int addend_masked, int kRMax, int p_max, int ent_cap, uint32_t y_bytes) {
  constexpr int RS = 16, LPR = 16, GPW = 4, kGroups = 64;
  extern __shared__ float4 s_mem[];
  float4* s_part = s_mem;                                          // [p_max][16]
  int4* s_ent = (int4*)(s_mem + (size_t)p_max * RS);               // [ent_cap]
  int2* s_iv = (int2*)(s_ent + ent_cap);                           // [non-zeros of the workgroup]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & (LPR - 1), g = lane / LPR;
  const int wg = blockIdx.x;
  const uint32_t nz0 = wg_nnz[2 * wg];
  const int nz = (int)wg_nnz[2 * wg + 1];
  const int e0 = wg_ent_off[2 * wg], ne = wg_ent_off[2 * wg + 1] - e0;
  const int c0 = wg_cmb_off[2 * wg], c1 = wg_cmb_off[2 * wg + 1];
  {
    constexpr int kStage = 8;                                      // loads in flight per lane while staging
    int4 e = make_int4(0, 0, 0, 0);
    if (tid < ne) e = ent[e0 + tid];                               // first 1024 descriptors ride along
    for (int i0 = 0; i0 < nz; i0 += kStage * 16 * NR_WAVE) {
      int col[kStage];
      float v[kStage];
      uint8_t keep[kStage];
#pragma unroll
      for (int k = 0; k < kStage; ++k) {
        const int i = i0 + k * 16 * NR_WAVE + tid;
        col[k] = 0;
        v[k] = 0.f;
        if (i < nz) {
          col[k] = indices[nz0 + i];
          v[k] = vals[nz0 + i];
        }
      }
#pragma unroll
      for (int k = 0; k < kStage; ++k) {
        keep[k] = 1;
        // (r02 A/B: replacing these per-pair mask bytes by a hash — no memory — takes the hop from 20.3 to
        // 18.6 us: an LDS bit set instead of the byte gathers could save at most ~1.5 us)
        if constexpr (COLMASK) keep[k] = col_mask[col[k]];
      }
#pragma unroll
      for (int k = 0; k < kStage; ++k) {
        const int i = i0 + k * 16 * NR_WAVE + tid;
        if (i < nz) s_iv[i] = make_int2(keep[k] ? col[k] : -1, __float_as_int(v[k]));
      }
    }
    for (int i = tid; i < ne; i += 16 * NR_WAVE) {
      if (i >= 16 * NR_WAVE) e = ent[e0 + i];
      e.z = (int)((uint32_t)e.z - nz0);                            // offset inside the staged slice
      // bit 30 of the owner: the addend row of this output row may be non-zero;
      // bit 29: the output row is not wanted (nothing is gathered, nothing is written)
      const int owner = e.w;                                       // the row itself (global id < 2^24)
      bool addend_on = true;
      if constexpr (COLMASK) addend_on = !addend_masked || col_mask[owner] != 0;
      if (addend_on) e.w |= 1 << 30;
      if constexpr (ROWMASK) {
        if (row_mask[owner] == 0) {
          e.y = 0;
          e.w |= 1 << 29;
        }
      }
      s_ent[i] = e;
    }
  }
  __syncthreads();
  // compact every sub-list to its surviving (column, value) pairs, in place and in order
  for (int base = wave * GPW; COLMASK && base < ne; base += kGroups) {
    const int ei = base + g;
    int4 ds = make_int4(0, 0, 0, 0);
    if (ei < ne) ds = s_ent[ei];
    int maxlen = ds.y;
#pragma unroll
    for (int sh = LPR; sh < NR_WAVE; sh <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, sh, NR_WAVE));
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    int w = 0;
    for (int k0 = 0; k0 < maxlen; k0 += LPR) {
      const bool in = k0 + c < ds.y;
      int2 iv = make_int2(-1, 0);
      if (in) iv = s_iv[ds.z + k0 + c];
      const bool keep = iv.x >= 0;
      const unsigned long long m = __ballot(keep);
      const uint32_t gm = (uint32_t)(m >> (g * LPR)) & 0xFFFFu;
      if (keep) s_iv[ds.z + w + __popc(gm & ((1u << c) - 1u))] = iv;
      w += __popc(gm);
    }
    if (ei < ne && c == 0) s_ent[ei].y = w;
  }
  staged_walk<ST>(s_ent, s_iv, ne, 0, X, Y, addend, sum_in, sum_out, s_part, kRMax, wave, g, c,
                  LayerChain{nullptr, nullptr}, y_bytes);
  if (c1 > c0) {                                           // workgroup-uniform
    __syncthreads();
    for (int ci = c0 + wave * GPW + g; ci < c1; ci += kGroups) {
      const int4 cm = cmb[ci];
      if constexpr (ROWMASK) {
        if (row_mask[cm.w] == 0) continue;
      }
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int sgm = 0; sgm < cm.z; ++sgm) {
        const float4 q = s_part[(size_t)(cm.y - kRMax + sgm) * RS + c];
        acc.x = __fadd_rn(acc.x, q.x); acc.y = __fadd_rn(acc.y, q.y);
        acc.z = __fadd_rn(acc.z, q.z); acc.w = __fadd_rn(acc.w, q.w);
      }
      bool addend_on = true;
      if constexpr (COLMASK) addend_on = !addend_masked || col_mask[cm.w] != 0;
      masked_row_out<ST>(acc, (int64_t)cm.w * RS + c, addend, addend_on, Y, sum_in, sum_out, nullptr, y_bytes);
    }
  }
}

struct BatchLists {        // a step's triplets; rows = users | n_users + pos | n_users + neg
  const int32_t* users; const int32_t* pos; const int32_t* neg;
  int batch, n_users;
  uint8_t* row_flag;       // out: 1 on the batch rows (must be zero elsewhere on entry)
  int32_t* rows_out;       // out (optional): the 3*batch rows, list order users, pos, neg
};

// Row-masked hop (last forward hop: only the batch rows are produced).  A real batch always holds
// the hub rows (positives are drawn in proportion to degree): ~45 % of all non-zeros belong to
// wanted rows, and in the row-run schedule they sit in a few workgroups that then do a full
// pass's work while the rest idle.  This kernel runs on a second schedule of the same sub-lists,
// dealt to the workgroups by descending row length (descriptors carry global rows): the
// workgroup collects its wanted sub-lists, stages their (column, value) pairs in LDS (a wave per
// sub-list, in chunks if they outgrow the buffer) and walks them with staged_walk.
__global__ __launch_bounds__(16 * NR_WAVE) void spmm_wanted_rows_kernel(
    const int32_t* __restrict__ w_ent_off, const int32_t* __restrict__ w_cmb_off,
    const int4* __restrict__ w_ent, const int4* __restrict__ w_cmb,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const float4* __restrict__ X, float4* __restrict__ Y, const float4* __restrict__ addend,
    const float4* sum_in, float4* sum_out, const uint8_t* __restrict__ row_mask, int kRMax,
    int p_max, int ent_cap, int nnz_cap, LayerChain chain, BatchLists bl, int bitmap_words) {
  constexpr int RS = 16;
  extern __shared__ float4 s_mem[];
  float4* s_part = s_mem;                                          // [p_max][16]
  int4* s_now = (int4*)(s_mem + (size_t)p_max * RS);               // sub-lists of this chunk
  int4* s_later = s_now + ent_cap;                                 // sub-lists that did not fit
  uint32_t* s_bits = (uint32_t*)(s_later + ent_cap);               // [bitmap_words] wanted rows (batch form)
  int2* s_iv = (int2*)(s_bits + bitmap_words);                     // [nnz_cap]
  __shared__ int s_n_now, s_n_later, s_cursor;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int wg = blockIdx.x;
  const int e0 = w_ent_off[2 * wg], ne = w_ent_off[2 * wg + 1] - e0;
  const int c0 = w_cmb_off[2 * wg], c1 = w_cmb_off[2 * wg + 1];
  if (tid == 0) { s_n_now = 0; s_n_later = 0; s_cursor = 0; }
  const bool by_batch = bl.users != nullptr;                       // workgroup-uniform
  if (by_batch) {
    // the batch itself says which rows are wanted: every workgroup builds the bit set in LDS
    // (no mark_batch launch before this kernel, no flag gather per descriptor); the workgroups
    // share the work of publishing the flags / row list the later kernels of the step read
    for (int i = tid; i < bitmap_words; i += 16 * NR_WAVE) s_bits[i] = 0u;
    __syncthreads();
    for (int i = tid; i < 3 * bl.batch; i += 16 * NR_WAVE) {
      const int which = i / bl.batch, b = i - which * bl.batch;
      const int row = which == 0 ? bl.users[b] : bl.n_users + (which == 1 ? bl.pos[b] : bl.neg[b]);
      atomicOr(&s_bits[row >> 5], 1u << (row & 31));
      if (i % (int)gridDim.x == wg) {
        bl.row_flag[row] = 1;
        if (bl.rows_out) bl.rows_out[i] = row;
      }
    }
  }
  __syncthreads();
  auto is_wanted = [&](int row) -> bool {
    return by_batch ? ((s_bits[row >> 5] >> (row & 31)) & 1u) != 0u : row_mask[row] != 0;
  };
  // wanted sub-lists of this workgroup, each with room reserved in the staging buffer (.x keeps
  // the slot, .z becomes the staging offset; the first non-zero moves to a register copy)
  for (int i = tid; i < ne; i += 16 * NR_WAVE) {
    const int4 e = w_ent[e0 + i];
    if (is_wanted(e.w)) {
      const int off = atomicAdd(&s_cursor, e.y);
      if (off + e.y <= nnz_cap) s_now[atomicAdd(&s_n_now, 1)] = make_int4(e.x, e.y | (off << 8), e.z, e.w);
      else s_later[atomicAdd(&s_n_later, 1)] = e;
    }
  }
  __syncthreads();
  while (true) {
    const int n_now = s_n_now, n_later = s_n_later;
    // stage: a wave per sub-list (<= 64 pairs, one coalesced read each); .y = length | offset << 8
    for (int k = wave; k < n_now; k += 16) {
      const int4 e = s_now[k];
      const int len = e.y & 0xFF, off = e.y >> 8;
      if (lane < len)
        s_iv[off + lane] = make_int2(indices[(uint32_t)e.z + lane], __float_as_int(vals[(uint32_t)e.z + lane]));
    }
    __syncthreads();
    for (int k = tid; k < n_now; k += 16 * NR_WAVE) {              // descriptors in staged_walk's format
      const int4 e = s_now[k];
      s_now[k] = make_int4(e.x, e.y & 0xFF, e.y >> 8, e.w | (1 << 30));
    }
    __syncthreads();
    staged_walk(s_now, s_iv, n_now, 0, X, Y, addend, sum_in, sum_out, s_part, kRMax, wave, g, c, chain);
    if (n_later == 0) break;                                       // workgroup-uniform
    __syncthreads();
    if (tid == 0) { s_n_now = 0; s_n_later = 0; s_cursor = 0; }
    __syncthreads();
    // next chunk: re-deal the deferred sub-lists (s_later -> s_now, overflow back into s_later's
    // already consumed prefix: entry k is read before any slot <= k is written)
    for (int k0 = 0; k0 < n_later; k0 += 16 * NR_WAVE) {
      const int k = k0 + tid;
      int4 e = make_int4(0, 0, 0, 0);
      if (k < n_later) e = s_later[k];
      __syncthreads();
      if (k < n_later) {
        const int off = atomicAdd(&s_cursor, e.y);
        if (off + e.y <= nnz_cap) s_now[atomicAdd(&s_n_now, 1)] = make_int4(e.x, e.y | (off << 8), e.z, e.w);
        else s_later[atomicAdd(&s_n_later, 1)] = e;
      }
      __syncthreads();
    }
  }
  if (c1 > c0) {                                                   // workgroup-uniform
    __syncthreads();
    for (int ci = c0 + wave * 4 + g; ci < c1; ci += 64) {
      const int4 cm = w_cmb[ci];
      if (!is_wanted(cm.x)) continue;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int sgm = 0; sgm < cm.z; ++sgm) {
        const float4 q = s_part[(size_t)(cm.y - kRMax + sgm) * RS + c];
        acc.x = __fadd_rn(acc.x, q.x); acc.y = __fadd_rn(acc.y, q.y);
        acc.z = __fadd_rn(acc.z, q.z); acc.w = __fadd_rn(acc.w, q.w);
      }
      masked_row_out(acc, (int64_t)cm.x * RS + c, addend, true, Y, sum_in, sum_out, &chain);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Row-masked hop, wave-cooperative form.  Two things bound the staged walk on a real batch (which
// always holds the hub rows: positives are drawn by degree):
//  (1) a sub-list given to ONE 16-lane group is up to sixteen dependent rounds of four gathers —
//      here a sub-list belongs to a whole wave: lane L holds pair L, lane group g gathers the rows
//      of pairs 16g..16g+15, so all 64 gathers of a segment are in flight at once, and the sums
//      still run in the strict order used everywhere else: group 0 adds its 16 products, hands
//      the running sum to group 1, ... (products and sums rounded separately: bit-identical);
//  (2) a hub's 3,077 x 256 B = 0.8 MB of gathers through ONE CU's vector-memory path (64 B/clk)
//      is >= 5 us whatever the waves do — here a row of > 64 non-zeros is cut into chunks of <= 8
//      consecutive 64-segments and every chunk is dealt on its own, so the biggest hub runs on 7 CUs.
//      Segment sums go to a global buffer (agent-scope stores); a chunk ends with ONE counter update
//      per row (not one per segment: 1,250 same-address atomics cost more than they saved,
//      profiles/r02_exp_wanted_hop.txt), and the chunk that finishes a row last adds ALL its segment
//      sums one by one in segment order — the same association as the full pass.
struct WantedEpi {
  float4* Y; const float4* addend; const float4* sum_in; float4* sum_out; LayerChain chain;
};
#ifdef NR_WW_TIMELINE      // experiment builds only (scripts/exp_wanted_timeline.sh): per-workgroup phase stamps
__device__ unsigned long long g_ww_dbg[256 * 8];
#define NR_WW_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 256) g_ww_dbg[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#define NR_WW_STAMP_END(i) do { __syncthreads(); NR_WW_STAMP(i); } while (0)
#else
#define NR_WW_STAMP(i)
#define NR_WW_STAMP_END(i)
#endif

// What the two wave-cooperative kernels (a schedule walked per workgroup / a per-batch item list) share.
// ww_sublist_sum: one sub-list of <= 64 pairs by one wave — lane L holds pair L (col, val; lanes past the end
// hold column 0); the ordered sum comes back in every lane for its column c.  between(): loads the caller
// wants in flight with the gathers.
template <class Between>
__device__ __forceinline__ float4 ww_sublist_sum(int col, float val, int len, const float4* __restrict__ X, int c,
                                                 int g, Between between) {
  constexpr int RS = 16;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 x[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int cj = __shfl(col, (g << 4) | j, NR_WAVE);           // lanes past the end hold column 0
    x[j] = X[(int64_t)cj * RS + c];
  }
  between();
  // products first (pair j of this lane group: value broadcast from lane 16g + j), in place
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float aj = __shfl(val, (g << 4) | j, NR_WAVE);
    x[j] = make_float4(__fmul_rn(aj, x[j].x), __fmul_rn(aj, x[j].y), __fmul_rn(aj, x[j].z), __fmul_rn(aj, x[j].w));
  }
  float4 acc = zero, carry = zero;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
    if (gg * 16 < len) {                                         // wave-uniform
      if (g == gg) {
        acc = carry;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 t = make_float4(__fadd_rn(acc.x, x[j].x), __fadd_rn(acc.y, x[j].y),
                                       __fadd_rn(acc.z, x[j].z), __fadd_rn(acc.w, x[j].w));
          if (gg * 16 + j < len) acc = t;
        }
      }
      const int src = (gg << 4) | c;
      carry = make_float4(__shfl(acc.x, src, NR_WAVE), __shfl(acc.y, src, NR_WAVE),
                          __shfl(acc.z, src, NR_WAVE), __shfl(acc.w, src, NR_WAVE));
    }
  }
  return carry;
}

// the row's epilogue operands ride with the gathers (requested after the sum they would be one more memory
// round trip per sub-list); rows that end in a partial slot read element 0
struct WwPre { float4 si, a, b; };
__device__ __forceinline__ WwPre ww_prefetch(const WantedEpi& ep, int64_t oe) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  WwPre p{zero, zero, zero};                                      // (an addend is read late: 128 VGPRs)
  if (ep.sum_out) {
    p.si = ep.sum_in[oe];
    if (ep.chain.a) p.a = ep.chain.a[oe];
    if (ep.chain.b) p.b = ep.chain.b[oe];
  }
  return p;
}

// lane group 0 puts a sub-list's sum where it belongs: slot == 0 the row itself (masked_row_out on the
// prefetched operands), slot < 0 an LDS partial (lds_dst: its 16 float4), slot > 0 global partial slot - 1
__device__ __forceinline__ void ww_sublist_out(float4 carry, int slot, int64_t o, int c, const WwPre& pre,
                                               const WantedEpi& ep, float4* lds_dst, float* ww_part) {
  if (slot == 0) {
    float4 y = carry;
    if (ep.addend) {
      const float4 pre_add = ep.addend[o];
      y = make_float4(__fadd_rn(y.x, pre_add.x), __fadd_rn(y.y, pre_add.y), __fadd_rn(y.z, pre_add.z),
                      __fadd_rn(y.w, pre_add.w));
    }
    if (ep.Y) ep.Y[o] = y;
    if (ep.sum_out) {
      float4 si = pre.si;
      if (ep.chain.a)
        si = make_float4(__fadd_rn(si.x, pre.a.x), __fadd_rn(si.y, pre.a.y), __fadd_rn(si.z, pre.a.z),
                         __fadd_rn(si.w, pre.a.w));
      if (ep.chain.b)
        si = make_float4(__fadd_rn(si.x, pre.b.x), __fadd_rn(si.y, pre.b.y), __fadd_rn(si.z, pre.b.z),
                         __fadd_rn(si.w, pre.b.w));
      ep.sum_out[o] = make_float4(__fadd_rn(si.x, y.x), __fadd_rn(si.y, y.y), __fadd_rn(si.z, y.z),
                                  __fadd_rn(si.w, y.w));
    }
  } else if (slot < 0) {                                       // a segment of a one-chunk row: LDS
    lds_dst[c] = carry;
  } else {                                                     // a segment of a multi-chunk row: global,
    float* mine = ww_part + (size_t)(slot - 1) * 64 + c * 4;   // agent scope (written through)
    __hip_atomic_store(mine + 0, carry.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, carry.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 2, carry.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 3, carry.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// a wave reports one finished chunk of hub `hub` (hd: {row, first partial slot, segments, chunks}); the wave
// that finishes the row last adds all its segment sums, 16 at a time in flight, in segment order
__device__ __forceinline__ void ww_chunk_done(int hub, const int4 hd, unsigned* ww_cnt, const float* ww_part,
                                              const WantedEpi& ep, int lane, int c, int g) {
  constexpr int RS = 16;
  unsigned old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(&ww_cnt[hub], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = __builtin_amdgcn_readfirstlane(old);
  if (old != (unsigned)hd.w - 1u) return;                      // another chunk of the row is still out
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s0 = 0; s0 < hd.z; s0 += 16) {
    float4 q[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float* qp = ww_part + ((size_t)hd.y + min(s0 + j, hd.z - 1)) * 64 + c * 4;
      q[j].x = __hip_atomic_load(qp + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      q[j].y = __hip_atomic_load(qp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      q[j].z = __hip_atomic_load(qp + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      q[j].w = __hip_atomic_load(qp + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (s0 + j < hd.z)
        sum = make_float4(__fadd_rn(sum.x, q[j].x), __fadd_rn(sum.y, q[j].y), __fadd_rn(sum.z, q[j].z),
                          __fadd_rn(sum.w, q[j].w));
  }
  if (g == 0)
    masked_row_out(sum, (int64_t)hd.x * RS + c, ep.addend, true, ep.Y, ep.sum_in, ep.sum_out, &ep.chain);
  if (lane == 0) __hip_atomic_store(&ww_cnt[hub], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed
}

// the batch's rows published for the later kernels of the step: a contiguous piece of the 3 * batch list
// positions per workgroup
__device__ __forceinline__ void ww_publish_batch(const BatchLists& bl, int wg, int n_wg, int tid) {
  const int total = 3 * bl.batch, per = (total + n_wg - 1) / n_wg;
  for (int i = wg * per + tid; i < min(total, (wg + 1) * per); i += 16 * NR_WAVE) {
    const int which = i / bl.batch, b = i - which * bl.batch;
    const int row = which == 0 ? bl.users[b] : bl.n_users + (which == 1 ? bl.pos[b] : bl.neg[b]);
    bl.row_flag[row] = 1;
    if (bl.rows_out) bl.rows_out[i] = row;
  }
}

__global__ __launch_bounds__(16 * NR_WAVE) void spmm_wanted_wave_kernel(
    const int32_t* __restrict__ ww_off, const int32_t* __restrict__ ww_choff,
    const int4* __restrict__ ww_ent, const int32_t* __restrict__ ww_gch, const int4* __restrict__ ww_hub,
    const int32_t* __restrict__ ww_lcoff, const int4* __restrict__ ww_lcmb,
    float* ww_part, unsigned* ww_cnt, const int32_t* __restrict__ indices,
    const float* __restrict__ vals, const float4* __restrict__ X, WantedEpi ep,
    const uint8_t* __restrict__ row_mask, BatchLists bl, int bitmap_words, int ent_cap, int lds_slots) {
  constexpr int RS = 16;
  extern __shared__ float4 s_mem[];
  float4* s_part = s_mem;                                          // [lds_slots][16] segment sums of one-chunk rows
  int4* s_want = (int4*)(s_mem + (size_t)lds_slots * RS);          // [ent_cap] wanted sub-lists
  uint32_t* s_bits = (uint32_t*)(s_want + ent_cap);                // [bitmap_words] wanted rows (batch form)
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int wg = blockIdx.x;
  const int e0 = ww_off[wg], ne = ww_off[wg + 1] - e0;
  const int h0 = ww_choff[wg], h1 = ww_choff[wg + 1];
  const int l0 = ww_lcoff[wg], l1 = ww_lcoff[wg + 1];
  NR_WW_STAMP(0);
  if (tid == 0) s_n = 0;
  const bool by_batch = bl.users != nullptr;                       // workgroup-uniform
  if (by_batch) {
    for (int i = tid; i < bitmap_words; i += 16 * NR_WAVE) s_bits[i] = 0u;
    __syncthreads();
    // every workgroup reads the whole batch (an 8,192-triplet global batch: 24 ids per thread).  A triplet's three ids
    // are requested together, unconditionally inside the loop (r06: three lists one after the other, each id behind its
    // own `i < batch` test, were waited for one by one — 3 round trips at B = 1,024, 24 at 8,192)
    for (int i = tid; i < bl.batch; i += 16 * NR_WAVE) {
      const int u = bl.users[i], p = bl.pos[i], q = bl.neg[i];
      const int ru = u, rp = bl.n_users + p, rq = bl.n_users + q;
      if (u >= 0) atomicOr(&s_bits[ru >> 5], 1u << (ru & 31));
      if (p >= 0) atomicOr(&s_bits[rp >> 5], 1u << (rp & 31));
      if (q >= 0) atomicOr(&s_bits[rq >> 5], 1u << (rq & 31));
    }
    ww_publish_batch(bl, wg, (int)gridDim.x, tid);
  }
  __syncthreads();
  auto is_wanted = [&](int row) -> bool {
    return by_batch ? ((s_bits[row >> 5] >> (row & 31)) & 1u) != 0u : row_mask[row] != 0;
  };
  NR_WW_STAMP(1);
  for (int i = tid; i < ne; i += 16 * NR_WAVE) {
    const int4 e = ww_ent[e0 + i];
    if (is_wanted(e.w)) s_want[atomicAdd(&s_n, 1)] = e;
  }
  __syncthreads();
  NR_WW_STAMP(2);
  const int n = s_n;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  // this wave's sub-lists: k = wave, wave + 16, ...; the next one's pairs are requested while the
  // current one's gathers are in flight
  int k = wave;
  int4 e = zero_int4();
  int col = 0;
  float val = 0.f;
  if (k < n) {
    e = s_want[k];
    if (lane < e.y) {
      col = indices[(uint32_t)e.z + lane];
      val = vals[(uint32_t)e.z + lane];
    }
  }
  while (k < n) {
    const int len = e.y, slot = e.x, row = e.w;
    const int64_t o = (int64_t)row * RS + c;
    WwPre pre;
    const int kn = k + 16;
    int4 en = zero_int4();
    int coln = 0;
    float valn = 0.f;
    // the next sub-list's pairs are requested while this one's gathers are in flight
    const float4 carry = ww_sublist_sum(col, val, len, X, c, g, [&]() {
      pre = ww_prefetch(ep, slot == 0 ? o : (int64_t)c);
      if (kn < n) {
        en = s_want[kn];
        if (lane < en.y) {
          coln = indices[(uint32_t)en.z + lane];
          valn = vals[(uint32_t)en.z + lane];
        }
      }
    });
    if (g == 0)
      ww_sublist_out(carry, slot, o, c, pre, ep, s_part + (size_t)(slot < 0 ? -slot - 1 : 0) * RS, ww_part);
    k = kn;
    e = en;
    col = coln;
    val = valn;
  }
  if (l1 > l0) {                                                   // workgroup-uniform: rows whose segments all ran here
    __syncthreads();
    for (int li = l0 + wave * 4 + g; li < l1; li += 64) {
      const int4 cm = ww_lcmb[li];                                 // {row, first LDS slot, segments}
      if (!is_wanted(cm.x)) continue;
      float4 acc = zero;
      for (int sgm = 0; sgm < cm.z; ++sgm) {
        const float4 q = s_part[(size_t)(cm.y + sgm) * RS + c];
        acc.x = __fadd_rn(acc.x, q.x); acc.y = __fadd_rn(acc.y, q.y);
        acc.z = __fadd_rn(acc.z, q.z); acc.w = __fadd_rn(acc.w, q.w);
      }
      masked_row_out(acc, (int64_t)cm.x * RS + c, ep.addend, true, ep.Y, ep.sum_in, ep.sum_out, &ep.chain);
    }
  }
  NR_WW_STAMP_END(3);
  if (tid == 0 && blockIdx.x < 256) {
#ifdef NR_WW_TIMELINE
    g_ww_dbg[blockIdx.x * 8 + 6] = (unsigned long long)n;
    g_ww_dbg[blockIdx.x * 8 + 7] = (unsigned long long)(h1 - h0);
#endif
  }
  if (h1 > h0) {                                                   // workgroup-uniform: this workgroup holds chunks
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);                                 // segment sums have left before a count moves
    __syncthreads();
    for (int hi = h0 + wave; hi < h1; hi += 16) {
      const int hub = ww_gch[hi];
      const int4 hd = ww_hub[hub];                                 // {row, first partial slot, segments, chunks}
      if (!is_wanted(hd.x)) continue;
      ww_chunk_done(hub, hd, ww_cnt, ww_part, ep, lane, c, g);
    }
  }
  NR_WW_STAMP_END(4);
}

// ---------------------------------------------------------------------------------------------
// Row-masked hop, planned form.  The by-batch kernel above finds its work inside the step's latency chain:
// every workgroup builds the batch's bit set, scans its ~306 static descriptors for the wanted ones, and runs
// whatever the static deal left it (21 wanted sub-lists on average, 39-44 at most: 2-3 rounds of its 16 waves).
// But a batch is known an epoch ahead (the sampler writes the whole stream and sorts every batch's occurrence
// keys): spmm_wanted_epoch_plan_kernel turns the keys of ALL batches into item lists in one launch (a workgroup
// per batch; layout and order: spmm_wanted_plan.h), and spmm_wanted_planned_kernel runs one batch's list — wave
// w of workgroup g takes item 16 g + w, nothing is searched, and no workgroup holds more than one round.
constexpr int kWpThreads = 1024;

__global__ __launch_bounds__(kWpThreads) void spmm_wanted_epoch_plan_kernel(
    const uint64_t* __restrict__ plans, int batch, int n_batches, int last_len, const int64_t* __restrict__ indptr,
    const int4* __restrict__ ww_hub, int n_hubs, int n2, int stride, int4* __restrict__ sched) {
  extern __shared__ uint32_t s_wp[];
  uint32_t* s_key = s_wp;                     // [n2] sort keys of the distinct rows (~0: none)
  int* s_off = (int*)(s_wp + n2);             // [n2] first item of sorted row j
  __shared__ int s_scan[kWpThreads];
  __shared__ int s_nhub, s_nrows;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = 3 * (b == n_batches - 1 ? last_len : batch);
  const uint64_t* keys = plans + 3 * (size_t)b * batch;
  int4* items = sched + (size_t)b * stride;
  if (tid == 0) { s_nhub = 0; s_nrows = 0; }
  // the sorted keys hold every row once per occurrence: the first of a run stands for the row
  for (int i = tid; i < n2; i += kWpThreads) {
    uint32_t k = ~0u;
    if (i < n) {
      const int32_t row = (int32_t)(keys[i] >> 32);
      const int32_t prev = i > 0 ? (int32_t)(keys[i - 1] >> 32) : -1;
      if (row != prev) k = nr_wplan::sort_key(indptr[row + 1] - indptr[row], row);
    }
    s_key[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += kWpThreads) {
        const int p = i ^ j;
        if (p > i) {
          const uint32_t x = s_key[i], y = s_key[p];
          if ((x > y) == ((i & k) == 0)) { s_key[i] = y; s_key[p] = x; }
        }
      }
      __syncthreads();
    }
  // slots of every sorted row, prefix-summed: thread t owns sorted positions [t * per, (t + 1) * per)
  const int per = n2 / kWpThreads;
  int sum = 0, hubs = 0, rows = 0;
  for (int j = tid * per; j < (tid + 1) * per; ++j) {
    const uint32_t k = s_key[j];
    s_off[j] = sum;
    if (k != ~0u) {
      const int32_t row = nr_wplan::key_row(k);
      const int64_t len = indptr[row + 1] - indptr[row];
      sum += nr_wplan::slots_of(len);
      hubs += nr_wplan::is_hub(len) ? 1 : 0;
      ++rows;
    }
  }
  s_scan[tid] = sum;
  if (hubs) atomicAdd(&s_nhub, hubs);
  if (rows) atomicAdd(&s_nrows, rows);
  __syncthreads();
  for (int off = 1; off < kWpThreads; off <<= 1) {
    const int v = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  const int before = s_scan[tid] - sum, total = s_scan[kWpThreads - 1];
  for (int j = tid * per; j < (tid + 1) * per; ++j) s_off[j] += before;
  __syncthreads();
  const int cap = stride - 1;                 // (the stride is an upper bound of `total`: never cut in practice)
  const int n_hub_rows = s_nhub;
  // hubs are the head of the order: the whole workgroup writes each one's items
  for (int j = 0; j < n_hub_rows; ++j) {
    const int32_t row = nr_wplan::key_row(s_key[j]);
    const int64_t first = indptr[row], len = indptr[row + 1] - first;
    int lo = 0, hi = n_hubs - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ww_hub[mid].x < row) lo = mid + 1; else hi = mid;
    }
    const int part0 = ww_hub[lo].y, sl = nr_wplan::slots_of(len), o = s_off[j];
    for (int s = tid; s < sl; s += kWpThreads)
      if (o + s < cap) {
        const nr_plan::Int4 it = nr_wplan::item_of(row, first, len, s, lo, part0);
        items[1 + o + s] = make_int4(it.x, it.y, it.z, it.w);
      }
  }
  for (int j = n_hub_rows + tid; j < n2; j += kWpThreads) {
    const uint32_t k = s_key[j];
    if (k == ~0u) continue;
    const int32_t row = nr_wplan::key_row(k);
    const int64_t first = indptr[row], len = indptr[row + 1] - first;
    const int sl = nr_wplan::slots_of(len), o = s_off[j];
    for (int s = 0; s < sl; ++s)
      if (o + s < cap) {
        const nr_plan::Int4 it = nr_wplan::item_of(row, first, len, s, 0, 0);
        items[1 + o + s] = make_int4(it.x, it.y, it.z, it.w);
      }
  }
  for (int i = 1 + min(total, cap) + tid; i < stride; i += kWpThreads) items[i] = make_int4(0, 0, 0, -1);
  if (tid == 0) items[0] = make_int4(min(total, cap), s_nrows, 0, 0);
}

__global__ __launch_bounds__(16 * NR_WAVE) void spmm_wanted_planned_kernel(
    const int4* __restrict__ items, const int4* __restrict__ ww_hub, float* ww_part, unsigned* ww_cnt,
    const int32_t* __restrict__ indices, const float* __restrict__ vals, const float4* __restrict__ X, WantedEpi ep,
    BatchLists bl) {
  constexpr int RS = 16;
  __shared__ float4 s_part[16 * RS];                               // a wave's segment sum (rows of 65..512 non-zeros)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int wg = blockIdx.x;
  const int n_items = items[0].x;
  ww_publish_batch(bl, wg, (int)gridDim.x, tid);
  if (wg * 16 >= n_items) return;                                  // the grid is the stride bound: surplus workgroups
  const int idx = wg * 16 + wave;
  const int4 it = idx < n_items ? items[1 + idx] : make_int4(0, 0, 0, -1);
  const int slot = it.x, len = it.y & 255, hub = (it.y >> 8) - 1, row = it.w;
  const int64_t o = (int64_t)row * RS + c;
  // segment 0 of a 65..512 row adds the row's segment sums after the barrier: it asks for the row's operands too
  const bool head = slot < 0 && ((-slot - 1) & 15) == 0;
  int4 hd = zero_int4();
  WwPre pre;
  if (row >= 0) {
    int col = 0;
    float val = 0.f;
    if (lane < len) {
      col = indices[(uint32_t)it.z + lane];
      val = vals[(uint32_t)it.z + lane];
    }
    if (hub >= 0) hd = ww_hub[hub];                                // {row, first partial slot, segments, chunks}
    const float4 carry = ww_sublist_sum(col, val, len, X, c, g,
                                        [&]() { pre = ww_prefetch(ep, (slot == 0 || head) ? o : (int64_t)c); });
    if (g == 0) ww_sublist_out(carry, slot, o, c, pre, ep, s_part + wave * RS, ww_part);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);                                   // segment sums have left before a count moves
  __syncthreads();
  if (row < 0) return;
  if (head && g == 0) {
    const int ns = (-slot - 1) >> 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sgm = 0; sgm < ns; ++sgm) {
      const float4 q = s_part[(wave + sgm) * RS + c];
      acc.x = __fadd_rn(acc.x, q.x); acc.y = __fadd_rn(acc.y, q.y);
      acc.z = __fadd_rn(acc.z, q.z); acc.w = __fadd_rn(acc.w, q.w);
    }
    ww_sublist_out(acc, 0, o, c, pre, ep, nullptr, nullptr);       // masked_row_out on the prefetched operands
  }
  if (hub >= 0) ww_chunk_done(hub, hd, ww_cnt, ww_part, ep, lane, c, g);
}

size_t wanted_lds_bytes(const BlockedPlan* p) {
  return (size_t)p->p_max * 256 + 2 * (size_t)p->w_ent_cap * 16 + (size_t)p->w_bitmap_words * 4 +
         (size_t)p->w_nnz_cap * 8;
}
int ww_bitmap_words(const BlockedPlan* p) { return (int)((p->n_rows + 127) / 128 * 4); }
size_t ww_lds_bytes(const BlockedPlan* p) {
  return (size_t)p->ww_lds_slots * 256 + (size_t)p->ww_ent_cap * 16 + (size_t)ww_bitmap_words(p) * 4 + 16;
}
size_t colmask_lds_bytes(const BlockedPlan* p) {
  return (size_t)p->p_max * 256 + (size_t)p->ent_cap * 16 + (size_t)p->nnz_cap * 8;
}

// launch of the wave-cooperative wanted-rows kernel (all three entrances of the row-masked hop)
int launch_wanted_wave(const BlockedPlan* p, const int32_t* d_indices, const float* d_vals, const float* d_X,
                       float* d_Y, const float* d_addend, const float* d_sum_in, float* d_sum_out,
                       const uint8_t* d_y_row_wanted, LayerChain chain, BatchLists bl, hipStream_t st) {
  hipLaunchKernelGGL(spmm_wanted_wave_kernel, dim3((unsigned)p->n_wg), dim3(16 * NR_WAVE), ww_lds_bytes(p), st,
                     p->ww_off, p->ww_choff, p->ww_ent, p->ww_gch, p->ww_hub, p->ww_lcoff, p->ww_lcmb, p->ww_part,
                     p->ww_cnt, d_indices, d_vals, (const float4*)d_X,
                     WantedEpi{(float4*)d_Y, (const float4*)d_addend, (const float4*)d_sum_in,
                               (float4*)d_sum_out, chain},
                     d_y_row_wanted, bl, ww_bitmap_words(p), p->ww_ent_cap, p->ww_lds_slots);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int s_gathers_in_flight = 8;     // tuning knob (nrhip_spmm_blocked_tune)
constexpr int kMaskedStoreDefault = kStoreWt;
int s_addend_by_flag = 1;        // tuning knob (nrhip_spmm_blocked_tune_addend_flag): 0 reads a flagged addend densely
int s_masked_store = kMaskedStoreDefault;   // tuning knob (nrhip_spmm_blocked_tune_store): how the column-masked hop stores Y
int s_packed = 1;                // tuning knob (nrhip_spmm_blocked_tune_packed): 0 reads the two arrays of a packed plan

// The words of a packed plan for spmm_blocked_kernel, or the "read the two arrays" form.  extra_lds: the factor
// table behind what the kernel has in LDS already.
PackedNz packed_for(const BlockedPlan* p, size_t lds, size_t* extra_lds) {
  *extra_lds = 0;
  const size_t tab = (size_t)p->pk_codes * 4;
  if (!p->pk_on || !s_packed || lds + tab > (size_t)kMaxLdsBytes) return PackedNz{nullptr, nullptr, nullptr, 0, 0};
  *extra_lds = tab;
  return PackedNz{p->pk_word, p->ent_rf, p->pk_table, p->pk_codes, p->pk_col_bits};
}

// (column, value) pairs copied into the plan's row order: row k of the order is CSR positions
// [src[k], src[k] + dst[k+1] - dst[k]) -> packed positions [dst[k], dst[k+1]).  Once per matrix.
__global__ __launch_bounds__(256) void row_order_pack_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                                                             int64_t n_rows, const int32_t* __restrict__ indices,
                                                             const float* __restrict__ vals, int32_t* __restrict__ pk_idx,
                                                             float* __restrict__ pk_val) {
  const int c = threadIdx.x & 15;
  for (int64_t k = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); k < n_rows; k += (int64_t)gridDim.x * 16) {
    const uint32_t s0 = src[k], d0 = dst[k], len = dst[k + 1] - d0;
    for (uint32_t j = c; j < len; j += 16) {
      pk_idx[d0 + j] = indices[s0 + j];
      pk_val[d0 + j] = vals[s0 + j];
    }
  }
}

// The same pairs as words (spmm_blocked_factor.h), every one checked: the product the kernels will form must have
// the stored value's bits, and the column must be one the codes cover.  A miss sets *bad; the plan then stays on
// the two arrays.  code[0 .. n_rows) row codes, code[n_rows ..) column codes.
__global__ __launch_bounds__(256) void row_order_pack_words_kernel(
    const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst, const int32_t* __restrict__ row_of,
    int64_t n_rows, int64_t n_cols, const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const uint16_t* __restrict__ code, const float* __restrict__ table, int col_bits, uint32_t* __restrict__ pk_word,
    uint32_t* __restrict__ bad) {
  const int c = threadIdx.x & 15;
  bool miss = false;
  for (int64_t k = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); k < n_rows; k += (int64_t)gridDim.x * 16) {
    const uint32_t s0 = src[k], d0 = dst[k], len = dst[k + 1] - d0;
    const float rf = table[code[row_of[k]]];
    for (uint32_t j = c; j < len; j += 16) {
      const int32_t col = indices[s0 + j];
      uint32_t w = 0;
      if (col < 0 || col >= n_cols) {
        miss = true;
      } else {
        const uint32_t cc = code[n_rows + col];
        if (__float_as_uint(__fmul_rn(rf, table[cc])) != __float_as_uint(vals[s0 + j])) miss = true;
        w = (uint32_t)col | (cc << col_bits);
      }
      pk_word[d0 + j] = w;
    }
  }
  if (miss) *bad = 1u;
}

// the factor of every descriptor's row, beside the descriptor
__global__ __launch_bounds__(256) void entry_row_factor_kernel(const int4* __restrict__ ent, int64_t n_ent,
                                                               const uint16_t* __restrict__ code,
                                                               const float* __restrict__ table,
                                                               float* __restrict__ ent_rf) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_ent; e += (int64_t)gridDim.x * 256)
    ent_rf[e] = table[code[ent[e].w]];
}

// The kernels of this plan's width may use the LDS their schedule needs (more than the 64 KB a kernel gets unasked).
static hipError_t allow_plan_lds(const BlockedPlan* p) {
  hipError_t e = hipSuccess;
  auto allow = [&](const void* fn, size_t lds) {
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  };
  // accumulators + the workgroup's row list + the factor table of a packed plan, where it fits
  const size_t tab = (size_t)nr_plan::kMaxFactorCodes * 4;
  size_t lds = (size_t)(p->r_max + p->p_max) * p->d * 4 + (size_t)p->r_max * 4;
  if (lds + tab <= (size_t)kMaxLdsBytes) lds += tab;
#define NR_ALLOW(DD)                                                                                                         \
  allow((const void*)spmm_blocked_kernel<false, 16, 8, DD>, lds); allow((const void*)spmm_blocked_kernel<true, 16, 8, DD>, lds); \
  allow((const void*)spmm_blocked_kernel<false, 16, 4, DD>, lds); allow((const void*)spmm_blocked_kernel<true, 16, 4, DD>, lds); \
  allow((const void*)spmm_blocked_kernel<false, 8, 8, DD>, lds); allow((const void*)spmm_blocked_kernel<true, 8, 8, DD>, lds);   \
  allow((const void*)spmm_blocked_kernel<false, 8, 4, DD>, lds); allow((const void*)spmm_blocked_kernel<true, 8, 4, DD>, lds)
  if (p->d == 16) { NR_ALLOW(16); } else if (p->d == 32) { NR_ALLOW(32); }
  else if (p->d == 64) {
    NR_ALLOW(64);
    allow((const void*)spmm_blocked_kernel<false, 16, 8, 64, true>, lds);
  }
  else if (p->d == 128) { NR_ALLOW(128); } else { NR_ALLOW(256); }
#undef NR_ALLOW
  if (p->wanted_ok) allow((const void*)spmm_wanted_rows_kernel, wanted_lds_bytes(p));
  if (p->ww_ok) allow((const void*)spmm_wanted_wave_kernel, ww_lds_bytes(p));
  if (p->colmask_ok)
    for (const void* fn : {(const void*)spmm_staged_masked_kernel<true, false>,
                           (const void*)spmm_staged_masked_kernel<true, false, kStoreNt>,
                           (const void*)spmm_staged_masked_kernel<true, false, kStoreWt>,
                           (const void*)spmm_staged_masked_kernel<false, true>,
                           (const void*)spmm_staged_masked_kernel<true, true>})
      allow(fn, colmask_lds_bytes(p));
  return e;
}

}  // namespace

extern "C" {

int nrhip_spmm_blocked_plan_bytes(int64_t n_rows, int64_t nnz, int d, size_t* bytes) {
  NR_REQUIRE(bytes && n_rows >= 0 && nnz >= 0, NR_ERR_ARG, "spmm_blocked_plan_bytes: bad arguments");
  (void)d;
  *bytes = blocked_plan_bytes(n_rows, nnz);
  return NR_OK;
}

int nrhip_spmm_blocked_plan_create(const int64_t* h_indptr, const int32_t* h_indices,
                                   int64_t n_rows, int64_t split_row, int d, int64_t block_bytes,
                                   int n_workgroups, int waves_per_wg, int seg_len, int r_max,
                                   int p_max, void* d_plan_buf, size_t plan_bytes, void* stream,
                                   void** plan_out) {
  nr_plan::Options opt;
  nr_plan::Error err;
  int rc = nr_plan::resolve_options(d, waves_per_wg, seg_len, r_max, p_max, block_bytes, split_row, n_rows, &opt, &err);
  NR_REQUIRE(rc == NR_OK, rc, "%s", err.msg.c_str());
  NR_REQUIRE(h_indptr && h_indices && d_plan_buf && plan_out && n_rows > 0, NR_ERR_ARG,
             "spmm_blocked_plan_create: bad arguments");
  const int64_t nnz = h_indptr[n_rows] - h_indptr[0];
  NR_REQUIRE(h_indptr[0] == 0 && nnz < ((int64_t)1 << 32), NR_ERR_UNSUPPORTED,
             "spmm_blocked: indptr must start at 0 and hold < 2^32 non-zeros");
  const size_t need_bytes = blocked_plan_bytes(n_rows, nnz);
  NR_REQUIRE(plan_bytes >= need_bytes, NR_ERR_WORKSPACE,
             "spmm_blocked_plan_create: plan buffer %zu < %zu bytes", plan_bytes, need_bytes);
  int n_wg = n_workgroups;
  if (n_wg <= 0) {                                           // one workgroup per CU
    int dev = 0;
    hipDeviceProp_t prop;
    NR_CHECK_HIP(hipGetDevice(&dev));
    NR_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    n_wg = prop.multiProcessorCount * (16 / opt.waves);
  }
  rc = nr_plan::choose_workgroup_count(n_wg, n_workgroups <= 0, n_rows, &opt, &err);
  NR_REQUIRE(rc == NR_OK, rc, "%s", err.msg.c_str());
  // "0" switches a kernel family off for A/B runs against the general kernel / the staged lane-group walker
  const char* env = getenv("NEUREC_SPMM_MASKED_FAST");
  opt.masked_fast = !(env && env[0] == '0');
  env = getenv("NEUREC_SPMM_WANTED_WAVE");
  opt.wanted_wave = !(env && env[0] == '0');
  env = getenv("NEUREC_SPMM_PACKED");                        // A/B runs of whole programs: nrhip_spmm_blocked_tune_packed
  if (env) s_packed = env[0] != '0';
  env = getenv("NEUREC_SPMM_WANTED_NNZ_CAP");                // tests: force the chunked path
  opt.wanted_nnz_cap = env ? std::max(atoi(env), 1) : 0;

  nr_plan::Plan h;
  rc = nr_plan::build_plan(h_indptr, h_indices, n_rows, opt, &h, &err);
  NR_REQUIRE(rc == NR_OK, rc, "%s", err.msg.c_str());

  BlockedPlan* p = new (std::nothrow) BlockedPlan();
  NR_REQUIRE(p, NR_ERR_ARG, "spmm_blocked_plan_create: out of host memory");
  p->n_rows = n_rows; p->nnz = nnz; p->n_wg = h.n_wg; p->n_phases = h.n_phases;
  p->seg = opt.seg; p->r_max = opt.r_max; p->p_max = opt.p_max; p->waves = opt.waves; p->d = d;
  p->n_ent = (int64_t)h.ent.size(); p->n_cmb = (int64_t)h.cmb.size();
  p->nnz_cap = h.nnz_cap; p->ent_cap = h.ent_cap; p->colmask_ok = h.colmask_ok;
  p->wanted_ok = h.wanted_ok; p->w_ent_cap = h.w_ent_cap; p->w_nnz_cap = h.w_nnz_cap; p->w_bitmap_words = h.w_bitmap_words;
  p->ww_ok = h.ww_ok; p->ww_ent_cap = h.ww_ent_cap; p->ww_lds_slots = h.ww_lds_slots;
  env = getenv("NEUREC_SPMM_WANTED_PLANNED");
  p->n_hubs = (int)h.ww_hub.size();
  p->wp_ok = h.ww_ok && opt.seg == nr_wplan::kSeg && n_rows <= nr_wplan::kMaxRows && !(env && env[0] == '0');
  if (p->wp_ok) p->wp_profile = nr_wplan::slot_profile(h_indptr, n_rows);
  std::vector<nr_plan::Section> sections = nr_plan::plan_sections(*p, h);
  for (const nr_plan::Section& fs : nr_plan::factor_sections(*p, h)) sections.push_back(fs);
  const size_t used = nr_plan::carve_sections(&sections, d_plan_buf);
  if (used > plan_bytes) {
    delete p;
    nrhip_set_error("spmm_blocked_plan_create: plan needs %zu bytes, buffer has %zu", used, plan_bytes);
    return NR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  for (const nr_plan::Section& s : sections) {
    if (e != hipSuccess) break;
    if (s.src && s.bytes) e = hipMemcpyAsync(s.addr, s.src, s.bytes, hipMemcpyHostToDevice, st);
    else if (s.zero) e = hipMemsetAsync(s.addr, 0, s.bytes + s.pad, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = allow_plan_lds(p);
  if (e != hipSuccess) {
    delete p;
    nrhip_set_error("spmm_blocked_plan_create: %s", hipGetErrorString(e));
    return NR_ERR_HIP;
  }
  *plan_out = p;
  return NR_OK;
}

/* Copy the matrix's (column, value) pairs into the plan's row order (once per matrix; again if the values change:
 * engine.SpmmCSR.values_changed).  The lane-group kernels read this private copy. */
int nrhip_spmm_blocked_pack(void* plan, const int32_t* d_indices, const float* d_vals, void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals, NR_ERR_ARG, "spmm_blocked_pack: null pointer argument");
  BlockedPlan* p = (BlockedPlan*)plan;
  if (p->nnz > 0) {
    // the (column, value) pairs in the plan's row order: a 16-lane group per row
    const unsigned blocks = (unsigned)std::min<int64_t>((p->n_rows + 15) / 16, 8192);
    hipLaunchKernelGGL(row_order_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p->pk_src, p->pk_dst,
                       p->n_rows, d_indices, d_vals, p->pk_idx, p->pk_val);
    NR_LAUNCH_CHECK();
  }
  p->pk_from_idx = d_indices;
  p->pk_from_val = d_vals;
  p->pk_on = 0;                         // the words (if any) stood for the values before this call
  return NR_OK;
}

/* nrhip_spmm_blocked_pack, and where the values factor also the 4-byte form of the same pairs: h_row_factor
 * [n_rows] and h_col_factor [n_cols] (host; both NULL: the plain pack) promise
 * float32(h_row_factor[r] * h_col_factor[c]) == value[r][c], which is checked on the device for every non-zero.
 * *packed (optional) says whether the kernels will read the words.  They do not, and the plan stays exactly as the
 * plain pack leaves it, when one product misses its value, when there are more distinct factors than the table in
 * LDS holds (1,024) or than the word has bits for beside the column, or when the matrix has more columns than rows
 * (the pack's code scratch is sized by the rows).  Synchronises the stream (init-time). */
int nrhip_spmm_blocked_pack_factored(void* plan, const int32_t* d_indices, const float* d_vals,
                                     const float* h_row_factor, const float* h_col_factor, int64_t n_cols,
                                     void* stream, int* packed) {
  if (packed) *packed = 0;
  NR_TRY(nrhip_spmm_blocked_pack(plan, d_indices, d_vals, stream));
  BlockedPlan* p = (BlockedPlan*)plan;
  if (!h_row_factor || !h_col_factor || p->nnz == 0 || n_cols <= 0 || n_cols > p->n_rows) return NR_OK;
  nr_plan::FactorLayout lay;
  nr_plan::Error err;
  if (nr_plan::factor_layout(h_row_factor, p->n_rows, h_col_factor, n_cols, &lay, &err) != nr_plan::kOk) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t zero = 0;
  NR_CHECK_HIP(hipMemcpyAsync(p->pk_table, lay.table.data(), lay.table.size() * 4, hipMemcpyHostToDevice, st));
  NR_CHECK_HIP(hipMemcpyAsync(p->pk_code, lay.row_code.data(), (size_t)p->n_rows * 2, hipMemcpyHostToDevice, st));
  NR_CHECK_HIP(hipMemcpyAsync(p->pk_code + p->n_rows, lay.col_code.data(), (size_t)n_cols * 2, hipMemcpyHostToDevice, st));
  NR_CHECK_HIP(hipMemcpyAsync(p->pk_bad, &zero, 4, hipMemcpyHostToDevice, st));
  const unsigned blocks = (unsigned)std::min<int64_t>((p->n_rows + 15) / 16, 8192);
  hipLaunchKernelGGL(row_order_pack_words_kernel, dim3(blocks), dim3(256), 0, st, p->pk_src, p->pk_dst, p->row_of,
                     p->n_rows, n_cols, d_indices, d_vals, p->pk_code, p->pk_table, lay.col_bits, p->pk_word, p->pk_bad);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(entry_row_factor_kernel, dim3((unsigned)std::min<int64_t>((p->n_ent + 255) / 256, 8192)),
                     dim3(256), 0, st, p->ent, p->n_ent, p->pk_code, p->pk_table, p->ent_rf);
  NR_LAUNCH_CHECK();
  uint32_t bad = 1;
  NR_CHECK_HIP(hipMemcpyAsync(&bad, p->pk_bad, 4, hipMemcpyDeviceToHost, st));
  NR_CHECK_HIP(hipStreamSynchronize(st));
  if (bad) return NR_OK;
  p->pk_codes = (int)lay.table.size();
  p->pk_col_bits = lay.col_bits;
  p->pk_on = 1;
  if (packed) *packed = 1;
  return NR_OK;
}

int nrhip_spmm_blocked_is_packed(const void* plan) {
  return plan && ((const BlockedPlan*)plan)->pk_on ? 1 : 0;
}

int nrhip_spmm_blocked_tune_packed(int on) {
  s_packed = on ? 1 : 0;
  return NR_OK;
}

// The kernels that walk the plan's own schedule read the plan's packed pairs; a call that hands in other CSR
// arrays than the ones packed (or none packed yet) packs first, on the caller's stream.
static int ensure_packed(const BlockedPlan* p, const int32_t* d_indices, const float* d_vals, void* stream) {
  if (p->pk_from_idx == d_indices && p->pk_from_val == d_vals) return NR_OK;
  return nrhip_spmm_blocked_pack((void*)p, d_indices, d_vals, stream);
}

#ifdef NR_WW_TIMELINE
int nrhip_ww_timeline(unsigned long long* h_out) {
  NR_CHECK_HIP(hipDeviceSynchronize());
  NR_CHECK_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_ww_dbg), sizeof(unsigned long long) * 256 * 8));
  return NR_OK;
}
#endif

int nrhip_spmm_blocked_tune(int gathers_in_flight) {
  NR_REQUIRE(gathers_in_flight == 4 || gathers_in_flight == 8, NR_ERR_UNSUPPORTED,
             "spmm_blocked_tune: gathers in flight %d (4, 8)", gathers_in_flight);
  s_gathers_in_flight = gathers_in_flight;
  return NR_OK;
}

int nrhip_spmm_blocked_tune_store(int masked_store) {
  NR_REQUIRE(masked_store >= -1 && masked_store <= kStoreWt, NR_ERR_ARG,
             "spmm_blocked_tune_store: store policy %d (-1 the default, 0 plain, 1 nontemporal, 2 written through)",
             masked_store);
  s_masked_store = masked_store < 0 ? kMaskedStoreDefault : masked_store;
  return NR_OK;
}

int nrhip_spmm_blocked_tune_addend_flag(int on) {
  s_addend_by_flag = on ? 1 : 0;
  return NR_OK;
}

int nrhip_spmm_blocked_plan_destroy(void* plan) {
  delete (BlockedPlan*)plan;
  return NR_OK;
}

int nrhip_spmm_blocked_plan_info(const void* plan, int* n_workgroups, int* n_phases,
                                 int64_t* n_entries, int64_t* n_split) {
  NR_REQUIRE(plan, NR_ERR_ARG, "spmm_blocked_plan_info: null plan");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  if (n_workgroups) *n_workgroups = p->n_wg;
  if (n_phases) *n_phases = p->n_phases;
  if (n_entries) *n_entries = p->n_ent;
  if (n_split) *n_split = p->n_cmb;
  return NR_OK;
}

int nrhip_spmm_blocked_flagged(const void* plan, const int32_t* d_indices, const float* d_vals,
                               const float* d_X, float* d_Y, const float* d_addend,
                               const uint8_t* d_addend_row_flag, const float* d_sum_in, float* d_sum_out,
                               const uint8_t* d_x_row_nonzero, const uint8_t* d_y_row_wanted, void* stream);

int nrhip_spmm_blocked(const void* plan, const int32_t* d_indices, const float* d_vals,
                       const float* d_X, float* d_Y, const float* d_addend, const float* d_sum_in,
                       float* d_sum_out, const uint8_t* d_x_row_nonzero,
                       const uint8_t* d_y_row_wanted, void* stream) {
  return nrhip_spmm_blocked_flagged(plan, d_indices, d_vals, d_X, d_Y, d_addend, nullptr, d_sum_in, d_sum_out,
                                    d_x_row_nonzero, d_y_row_wanted, stream);
}

/* nrhip_spmm_blocked with a promise about the addend: d_addend_row_flag[r] == 0 says row r of d_addend is all zero,
 * and the unmasked pass then does not read it (NULL: no promise).  The masked forms have their own promise
 * (an addend that is the operand) and take no flags. */
int nrhip_spmm_blocked_flagged(const void* plan, const int32_t* d_indices, const float* d_vals,
                               const float* d_X, float* d_Y, const float* d_addend,
                               const uint8_t* d_addend_row_flag, const float* d_sum_in, float* d_sum_out,
                               const uint8_t* d_x_row_nonzero, const uint8_t* d_y_row_wanted, void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals && d_X && (d_Y || d_sum_out), NR_ERR_ARG,
             "spmm_blocked: null pointer argument");
  NR_REQUIRE((d_sum_out == nullptr) || (d_sum_in != nullptr), NR_ERR_ARG,
             "spmm_blocked: sum_out needs sum_in");
  NR_REQUIRE(!d_addend_row_flag || (d_addend && !d_x_row_nonzero && !d_y_row_wanted), NR_ERR_ARG,
             "spmm_blocked: addend row flags need an addend and no masks");
  const uint8_t* addend_flag = s_addend_by_flag ? d_addend_row_flag : nullptr;
  const BlockedPlan* p = (const BlockedPlan*)plan;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)p->n_wg), block(p->waves * NR_WAVE);
  const size_t lds = (size_t)(p->r_max + p->p_max) * p->d * 4 + (size_t)p->r_max * 4;
  const bool masked = d_x_row_nonzero || d_y_row_wanted;
  const int gif = s_gathers_in_flight;
  if (p->ww_ok && d_y_row_wanted && !d_x_row_nonzero)
    return launch_wanted_wave(p, d_indices, d_vals, d_X, d_Y, d_addend, d_sum_in, d_sum_out, d_y_row_wanted,
                              LayerChain{nullptr, nullptr}, BatchLists{}, st);
  if (p->wanted_ok && d_y_row_wanted && !d_x_row_nonzero) {
    hipLaunchKernelGGL(spmm_wanted_rows_kernel, grid, block, wanted_lds_bytes(p), st, p->w_ent_off,
                       p->w_cmb_off, p->w_ent, p->w_cmb, d_indices, d_vals, (const float4*)d_X,
                       (float4*)d_Y, (const float4*)d_addend, (const float4*)d_sum_in,
                       (float4*)d_sum_out, d_y_row_wanted, p->r_max, p->p_max, p->w_ent_cap,
                       p->w_nnz_cap, LayerChain{nullptr, nullptr}, BatchLists{}, p->w_bitmap_words);
    NR_LAUNCH_CHECK();
    return NR_OK;
  }
  NR_TRY(ensure_packed(p, d_indices, d_vals, stream));
  if (p->colmask_ok && masked) {
    // an addend that is the operand itself shares its promise (zero rows where the mask is 0)
    const int addend_masked = d_x_row_nonzero && d_addend == d_X ? 1 : 0;
    // Y's bytes for the written-through form's buffer descriptor (32-bit offsets: a larger Y is stored plainly)
    const uint64_t y_all = (uint64_t)p->n_rows * p->d * 4;
    const int store = d_Y && y_all <= 0xFFFFFFFFull ? s_masked_store : kStorePlain;
#define NR_STAGED(CM, RM, ST)                                                                      \
  hipLaunchKernelGGL((spmm_staged_masked_kernel<CM, RM, ST>), grid, block, colmask_lds_bytes(p), st, \
                     p->wg_row0, p->wg_ent_off, p->wg_cmb_off, p->wg_nnz, p->ent, p->cmb, p->pk_idx, \
                     p->pk_val, (const float4*)d_X, (float4*)d_Y, (const float4*)d_addend,          \
                     (const float4*)d_sum_in, (float4*)d_sum_out, d_x_row_nonzero, d_y_row_wanted,  \
                     addend_masked, p->r_max, p->p_max, p->ent_cap, (uint32_t)y_all)
    if (d_x_row_nonzero && d_y_row_wanted) NR_STAGED(true, true, kStorePlain);
    else if (d_x_row_nonzero && store == kStoreNt) NR_STAGED(true, false, kStoreNt);
    else if (d_x_row_nonzero && store == kStoreWt) NR_STAGED(true, false, kStoreWt);
    else if (d_x_row_nonzero) NR_STAGED(true, false, kStorePlain);
    else NR_STAGED(false, true, kStorePlain);
#undef NR_STAGED
    NR_LAUNCH_CHECK();
    return NR_OK;
  }
  size_t tab_lds = 0;
  const PackedNz pk = packed_for(p, lds, &tab_lds);
#define NR_BLK(M, W, GG, DD)                                                                       \
  hipLaunchKernelGGL((spmm_blocked_kernel<M, W, GG, DD>), grid, block, lds + tab_lds, st, p->wg_row0, \
                     p->wg_nrows, p->wg_ent_off, p->wg_cmb_off, p->ent, p->cmb, p->n_phases,        \
                     p->pk_idx, p->pk_val, (const float4*)d_X, (float4*)d_Y, (const float4*)d_addend, \
                     (const float4*)d_sum_in, (float4*)d_sum_out, d_x_row_nonzero, d_y_row_wanted,  \
                     p->r_max, AdamEpilogue{}, p->row_of, p->p_max, addend_flag, pk)
#define NR_BLK_D(DD)                                                                               \
  if (p->waves == 16) {                                                                            \
    if (masked) { if (gif == 4) NR_BLK(true, 16, 4, DD); else NR_BLK(true, 16, 8, DD); }           \
    else { if (gif == 4) NR_BLK(false, 16, 4, DD); else NR_BLK(false, 16, 8, DD); }                \
  } else {                                                                                         \
    if (masked) { if (gif == 4) NR_BLK(true, 8, 4, DD); else NR_BLK(true, 8, 8, DD); }             \
    else { if (gif == 4) NR_BLK(false, 8, 4, DD); else NR_BLK(false, 8, 8, DD); }                  \
  }
  if (p->d == 16) { NR_BLK_D(16) } else if (p->d == 32) { NR_BLK_D(32) } else if (p->d == 64) { NR_BLK_D(64) }
  else if (p->d == 128) { NR_BLK_D(128) } else { NR_BLK_D(256) }
#undef NR_BLK_D
#undef NR_BLK
  NR_LAUNCH_CHECK();
  return NR_OK;
}

/* Row-masked hop with the running layer sum completed on the way (LightGCN.py:143-146 on the batch
 * rows): d_sum_out[r] = ((d_sum_in[r] + d_layer_a[r]) + d_layer_b[r]) + (A·X)[r] for the rows with
 * d_y_row_wanted[r] != 0 (d_layer_a / d_layer_b optional) — the full hops before it then need no
 * running-sum streams at all.  Needs the wanted-rows schedule (d = 64). */
int nrhip_spmm_blocked_wanted_layers(const void* plan, const int32_t* d_indices, const float* d_vals,
                                     const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                     const float* d_layer_b, float* d_sum_out,
                                     const uint8_t* d_y_row_wanted, void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals && d_X && d_sum_in && d_sum_out && d_y_row_wanted, NR_ERR_ARG,
             "spmm_blocked_wanted_layers: null pointer argument");
  NR_REQUIRE(d_layer_a || !d_layer_b, NR_ERR_ARG, "spmm_blocked_wanted_layers: layer_b without layer_a");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  if (p->ww_ok)
    return launch_wanted_wave(p, d_indices, d_vals, d_X, nullptr, nullptr, d_sum_in, d_sum_out, d_y_row_wanted,
                              LayerChain{(const float4*)d_layer_a, (const float4*)d_layer_b}, BatchLists{},
                              (hipStream_t)stream);
  NR_REQUIRE(p->wanted_ok, NR_ERR_UNSUPPORTED, "spmm_blocked_wanted_layers: no wanted-rows schedule");
  hipLaunchKernelGGL(spmm_wanted_rows_kernel, dim3((unsigned)p->n_wg), dim3(p->waves * NR_WAVE),
                     wanted_lds_bytes(p), (hipStream_t)stream, p->w_ent_off, p->w_cmb_off, p->w_ent,
                     p->w_cmb, d_indices, d_vals, (const float4*)d_X, (float4*)nullptr,
                     (const float4*)nullptr, (const float4*)d_sum_in, (float4*)d_sum_out,
                     d_y_row_wanted, p->r_max, p->p_max, p->w_ent_cap, p->w_nnz_cap,
                     LayerChain{(const float4*)d_layer_a, (const float4*)d_layer_b}, BatchLists{},
                     p->w_bitmap_words);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

/* The same hop told the batch instead of flags: wanted rows = d_users | n_users + d_pos |
 * n_users + d_neg.  It also does nrhip_lightgcn_mark_batch's job on the way: d_row_flag (zero on
 * entry) gets 1 on those rows, d_rows_out (optional) the 3*batch rows.  Needs
 * nrhip_spmm_blocked_has_wanted(plan) == 2 (wanted-rows schedule and a matrix of <= 131072 rows). */
int nrhip_spmm_blocked_wanted_batch(const void* plan, const int32_t* d_indices, const float* d_vals,
                                    const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                    const float* d_layer_b, float* d_sum_out, const int32_t* d_users,
                                    const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                                    uint8_t* d_row_flag, int32_t* d_rows_out, void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals && d_X && d_sum_in && d_sum_out && d_users && d_pos && d_neg &&
                 d_row_flag && batch >= 0 && n_users >= 0,
             NR_ERR_ARG, "spmm_blocked_wanted_batch: bad arguments");
  NR_REQUIRE(d_layer_a || !d_layer_b, NR_ERR_ARG, "spmm_blocked_wanted_batch: layer_b without layer_a");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  if (batch == 0) return NR_OK;
  if (p->ww_ok)
    return launch_wanted_wave(p, d_indices, d_vals, d_X, nullptr, nullptr, d_sum_in, d_sum_out, nullptr,
                              LayerChain{(const float4*)d_layer_a, (const float4*)d_layer_b},
                              BatchLists{d_users, d_pos, d_neg, batch, n_users, d_row_flag, d_rows_out},
                              (hipStream_t)stream);
  NR_REQUIRE(p->wanted_ok && p->w_bitmap_words > 0, NR_ERR_UNSUPPORTED,
             "spmm_blocked_wanted_batch: no wanted-rows schedule with a row bit set");
  hipLaunchKernelGGL(spmm_wanted_rows_kernel, dim3((unsigned)p->n_wg), dim3(p->waves * NR_WAVE),
                     wanted_lds_bytes(p), (hipStream_t)stream, p->w_ent_off, p->w_cmb_off, p->w_ent,
                     p->w_cmb, d_indices, d_vals, (const float4*)d_X, (float4*)nullptr,
                     (const float4*)nullptr, (const float4*)d_sum_in, (float4*)d_sum_out,
                     (const uint8_t*)nullptr, p->r_max, p->p_max, p->w_ent_cap, p->w_nnz_cap,
                     LayerChain{(const float4*)d_layer_a, (const float4*)d_layer_b},
                     BatchLists{d_users, d_pos, d_neg, batch, n_users, d_row_flag, d_rows_out},
                     p->w_bitmap_words);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

/* The same hop from a per-batch item list made an epoch ahead (spmm_wanted_plan.h).
 * _has_wanted_planned: 1 when this plan can (wave-cooperative schedule, 64-pair segments, <= 2^19 rows,
 * NEUREC_SPMM_WANTED_PLANNED != 0).
 * _epoch_plan_bytes: records per batch (*stride, 16 bytes each) and the bytes of n_batches of them, for batches
 * of up to `batch` triplets (3 * batch <= 16384, else NR_ERR_UNSUPPORTED).
 * _epoch_plan: d_plans = nrhip_bpr_plan's output for the epoch stream (3 * batch keys per batch, the last batch
 * last_len triplets); writes every batch's list at d_sched + k * stride * 16.  One launch, no host read.
 * _wanted_planned: nrhip_spmm_blocked_wanted_batch on d_batch_sched = the batch's own records. */
int nrhip_spmm_blocked_has_wanted_planned(const void* plan) {
  return plan && ((const BlockedPlan*)plan)->wp_ok ? 1 : 0;
}

int nrhip_spmm_blocked_wanted_epoch_plan_bytes(const void* plan, int batch, int64_t n_batches, size_t* bytes,
                                               int* stride) {
  NR_REQUIRE(plan && bytes && stride && batch >= 1 && n_batches >= 0, NR_ERR_ARG,
             "spmm_blocked_wanted_epoch_plan_bytes: bad arguments");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  NR_REQUIRE(p->wp_ok, NR_ERR_UNSUPPORTED, "spmm_blocked_wanted_epoch_plan_bytes: no planned form for this plan");
  NR_REQUIRE(3 * (int64_t)batch <= nr_wplan::kMaxKeys, NR_ERR_UNSUPPORTED,
             "spmm_blocked_wanted_epoch_plan_bytes: batch %d > %d", batch, nr_wplan::kMaxKeys / 3);
  const int64_t st = nr_wplan::stride_of(p->wp_profile, batch);
  NR_REQUIRE(st < ((int64_t)1 << 24), NR_ERR_UNSUPPORTED, "spmm_blocked_wanted_epoch_plan_bytes: %lld items per batch",
             (long long)st);
  *stride = (int)st;
  *bytes = (size_t)st * 16 * (size_t)n_batches;
  return NR_OK;
}

int nrhip_spmm_blocked_wanted_epoch_plan(const void* plan, const int64_t* d_indptr, const uint64_t* d_plans, int batch,
                                         int64_t n_batches, int last_len, void* d_sched, size_t sched_bytes,
                                         void* stream) {
  NR_REQUIRE(plan && d_indptr && d_plans && d_sched && batch >= 1 && n_batches >= 1 && last_len >= 1 &&
                 last_len <= batch && n_batches < ((int64_t)1 << 30),
             NR_ERR_ARG, "spmm_blocked_wanted_epoch_plan: bad arguments");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  size_t need = 0;
  int stride = 0;
  NR_TRY(nrhip_spmm_blocked_wanted_epoch_plan_bytes(plan, batch, n_batches, &need, &stride));
  NR_REQUIRE(sched_bytes >= need, NR_ERR_WORKSPACE, "spmm_blocked_wanted_epoch_plan: buffer %zu < %zu bytes",
             sched_bytes, need);
  int n2 = kWpThreads;
  while (n2 < 3 * batch) n2 <<= 1;
  hipLaunchKernelGGL(spmm_wanted_epoch_plan_kernel, dim3((unsigned)n_batches), dim3(kWpThreads), (size_t)n2 * 8,
                     (hipStream_t)stream, d_plans, batch, (int)n_batches, last_len, d_indptr, p->ww_hub, p->n_hubs, n2,
                     stride, (int4*)d_sched);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_spmm_blocked_wanted_planned(const void* plan, const int32_t* d_indices, const float* d_vals,
                                      const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                      const float* d_layer_b, float* d_sum_out, const int32_t* d_users,
                                      const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                                      uint8_t* d_row_flag, int32_t* d_rows_out, const void* d_batch_sched, int stride,
                                      void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals && d_X && d_sum_in && d_sum_out && d_users && d_pos && d_neg &&
                 d_row_flag && d_batch_sched && batch >= 1 && n_users >= 0 && stride > 1 && (stride - 1) % 16 == 0,
             NR_ERR_ARG, "spmm_blocked_wanted_planned: bad arguments");
  NR_REQUIRE(d_layer_a || !d_layer_b, NR_ERR_ARG, "spmm_blocked_wanted_planned: layer_b without layer_a");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  NR_REQUIRE(p->wp_ok, NR_ERR_UNSUPPORTED, "spmm_blocked_wanted_planned: no planned form for this plan");
  hipLaunchKernelGGL(spmm_wanted_planned_kernel, dim3((unsigned)((stride - 1) / 16)), dim3(16 * NR_WAVE), 0,
                     (hipStream_t)stream, (const int4*)d_batch_sched, p->ww_hub, p->ww_part, p->ww_cnt, d_indices,
                     d_vals, (const float4*)d_X,
                     WantedEpi{nullptr, nullptr, (const float4*)d_sum_in, (float4*)d_sum_out,
                               LayerChain{(const float4*)d_layer_a, (const float4*)d_layer_b}},
                     BatchLists{d_users, d_pos, d_neg, batch, n_users, d_row_flag, d_rows_out});
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_spmm_blocked_has_wanted(const void* plan) {      // 0 no, 1 flag form, 2 flag and batch forms
  if (plan && ((const BlockedPlan*)plan)->ww_ok) return 2;
  if (!plan || !((const BlockedPlan*)plan)->wanted_ok) return 0;
  return ((const BlockedPlan*)plan)->w_bitmap_words > 0 ? 2 : 1;
}

/* Y is not stored: the rows' results (plus d_addend) are consumed as the dense gradient
 * g = y + d_grad_b and TF-Adam is applied to d_var / d_m / d_v in the same pass (d = 64 only).
 * clear_consumed: also zero the non-zero entries of d_addend / d_grad_b and the set bytes of
 * d_row_flag (may be NULL) once read — the re-arming nrhip_rows_clear would do afterwards. */
int nrhip_spmm_blocked_adam(const void* plan, const int32_t* d_indices, const float* d_vals,
                            const float* d_X, float* d_addend, float* d_grad_b, float* d_var,
                            float* d_m, float* d_v, float alpha, float beta1, float beta2,
                            float eps, int clear_consumed, uint8_t* d_row_flag, void* stream) {
  NR_REQUIRE(plan && d_indices && d_vals && d_X && d_grad_b && d_var && d_m && d_v, NR_ERR_ARG,
             "spmm_blocked_adam: null pointer argument");
  const BlockedPlan* p = (const BlockedPlan*)plan;
  NR_REQUIRE(p->d == 64 && p->waves == 16, NR_ERR_UNSUPPORTED,
             "spmm_blocked_adam: built for d = 64 schedules with 16 waves");
  NR_REQUIRE(d_X != d_var, NR_ERR_ARG, "spmm_blocked_adam: the operand must not be the updated table");
  const size_t lds = (size_t)(p->r_max + p->p_max) * p->d * 4 + (size_t)p->r_max * 4;   // allowed at plan creation
  NR_TRY(ensure_packed(p, d_indices, d_vals, stream));
  NR_REQUIRE(!clear_consumed || d_addend, NR_ERR_ARG, "spmm_blocked_adam: clear_consumed needs an addend");
  AdamEpilogue ad{(float4*)d_var, (float4*)d_m, (float4*)d_v, (const float4*)d_grad_b,
                  alpha, 1.0f - beta1, 1.0f - beta2, eps,
                  clear_consumed ? (float4*)d_addend : nullptr,
                  clear_consumed ? (float4*)d_grad_b : nullptr, clear_consumed ? d_row_flag : nullptr};
  size_t tab_lds = 0;
  const PackedNz pk = packed_for(p, lds, &tab_lds);
  hipLaunchKernelGGL((spmm_blocked_kernel<false, 16, 8, 64, true>), dim3((unsigned)p->n_wg),
                     dim3(16 * NR_WAVE), lds + tab_lds, (hipStream_t)stream, p->wg_row0, p->wg_nrows,
                     p->wg_ent_off, p->wg_cmb_off, p->ent, p->cmb, p->n_phases, p->pk_idx, p->pk_val,
                     (const float4*)d_X, (float4*)nullptr, (const float4*)d_addend,
                     (const float4*)nullptr, (float4*)nullptr, (const uint8_t*)nullptr,
                     (const uint8_t*)nullptr, p->r_max, ad, p->row_of, p->p_max, (const uint8_t*)nullptr, pk);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
