// ItemKNN as the reference builds it (model/general_recommender/ItemKNN.py): the item-item similarity of the train
// matrix R (U x I), each column cut to its top-K neighbours (W, I x I sparse), and the scores R W of a batch of users.
//
//   itemknn_column_kernel   one workgroup per column i of a block of columns.  It
//                             1. sums the co-occurrences c_ij = sum_{u in users(i)} r_ui r_uj into an accumulator column
//                                of I floats: users in CSC order, one at a time, the lanes over that user's CSR row
//                                (distinct j: no two lanes meet), a barrier between users — a fixed order, no atomics on
//                                floats.  The column lives in LDS when I <= NRHIP_ITEMKNN_LDS_ITEMS, else in a row of the
//                                global slab [block][I];
//                             2. applies the similarity's elementwise formula in place (diagonal = 0);
//                             3. finds the K-th largest entry by a radix select over the order-preserving bit pattern
//                                of the floats (4 passes of 8 bits, a 256-bin LDS histogram; exact zeros are counted
//                                once and added to their bin, most columns are mostly zero), and, when equal values
//                                straddle the K-th place, the index of the last one to keep by the same select over
//                                the indices: larger value first, lower index first among equals;
//                             4. gathers the winners that are not zero, sorts them (bitonic network over
//                                (value, ~index) keys in LDS) and writes the column's neighbour list.
//   itemknn_keys_kernel /   W^T in CSR form: a key (j, i, slot) per stored entry, sorted by nrhip_sort_u64, then split
//   itemknn_unpack_kernel   into the row pointer, the column ids (ascending inside a row) and the values.
//   itemknn_score_kernel    one workgroup per user of the batch: the row of S is zeroed, then for every history item j in
//                           CSR order the lanes walk row j of W^T (distinct i) and add r_uj W[j][i]; a barrier between
//                           history items.  Work = sum_j len(W^T row j), long rows are strided over the workgroup.
// Every float sum is taken in a fixed order: two builds / two score calls are bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "neurec_hip.h"
#include "nr_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsItems = NRHIP_ITEMKNN_LDS_ITEMS;
constexpr int kMaxK = NRHIP_ITEMKNN_MAX_NEIGHBOR;
constexpr int kSlotBits = 10;  // 2^10 = kMaxK slots of a column in a transpose key
static_assert((1 << kSlotBits) == kMaxK, "slot bits");
// nrhip_sort_u64 pads its count to a power of two and steps a stride to twice that, both in an int
constexpr int64_t kMaxKeys = (int64_t)1 << 29;

enum { kCosine = 0, kTanimoto = 1, kDice = 2, kTversky = 3, kEuclidean = 4 };

struct SimParams {
  int kind;
  float shrink, ta, tb;
};

// bit pattern whose unsigned order is the order of the floats (-inf < ... < -0 < +0 < ... < +inf)
__device__ __forceinline__ uint32_t orderable(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_orderable(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
constexpr uint32_t kZeroKey = 0x80000000u;  // orderable(+0.f)

__device__ __forceinline__ int64_t shfl_i64(int64_t x, int src) {
  const int lo = __shfl((int)(uint32_t)x, src, NR_WAVE), hi = __shfl((int)(x >> 32), src, NR_WAVE);
  return ((int64_t)hi << 32) | (uint32_t)lo;
}

// out[cols[q]] += r * vals[q] over the rows named by list[lb, le) (ids into the row pointer `indptr`), one row at a
// time in list order, the workgroup's threads over a row's entries.  Every wave fetches the next 64 (row, r, begin,
// end) with one coalesced load each and broadcasts them: a row costs one dependent gather, not three.
__device__ __forceinline__ void walk_rows(const int32_t* __restrict__ list, const float* __restrict__ list_vals,
                                          int64_t lb, int64_t le, const int64_t* __restrict__ indptr, int n_rows,
                                          const int32_t* __restrict__ cols, const float* __restrict__ vals, int n_cols,
                                          float* out) {
  const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1);
  for (int64_t p0 = lb; p0 < le; p0 += NR_WAVE) {
    const int nb = (int)(le - p0 < NR_WAVE ? le - p0 : NR_WAVE);
    const int64_t p = p0 + (lane < nb ? lane : nb - 1);
    const int row = list[p];
    const float r = list_vals[p];
    const bool ok = (uint32_t)row < (uint32_t)n_rows;
    const int64_t lo = ok ? indptr[row] : 0, hi = ok ? indptr[row + 1] : 0;
    for (int k = 0; k < nb; ++k) {
      const float rk = __shfl(r, k, NR_WAVE);
      const int64_t lok = shfl_i64(lo, k), hik = shfl_i64(hi, k);
      for (int64_t q = lok + tid; q < hik; q += kThreads) {
        const int c = cols[q];
        if ((uint32_t)c < (uint32_t)n_cols) out[c] = fmaf(rk, vals[q], out[c]);
      }
      __syncthreads();  // the next row may name the same columns
    }
  }
}

__device__ __forceinline__ float similarity_of(const SimParams& sp, float c, float nai, float nbi, float naj,
                                               float nbj) {
  switch (sp.kind) {
    case kCosine:  // cosine / adjusted / pearson (na = nb = norms), asymmetric (na = s^2a, nb = s^2(1-a))
      return c / (nai * nbj + sp.shrink + 1e-6f);
    case kTanimoto:
      return c / (nai + naj - c + sp.shrink + 1e-6f);
    case kDice:
      return c / (nai + naj + sp.shrink + 1e-6f);
    case kTversky:
      return c / (c + (nai - c) * sp.ta + (naj - c) * sp.tb + sp.shrink + 1e-6f);
    default: {     // euclidean, normalised: na = sums of squares, nb = norms
      const float den = nbi * nbj;
      if (!(den > 0.f)) return 0.f;  // an empty item: distance inf -> 0; two empty items (0/0 in the reference) -> 0
      const float d2 = fmaxf(nai + naj - 2.f * c, 0.f);
      return 1.f / (sqrtf(d2 / den) + sp.shrink + 1e-9f);
    }
  }
}

// One step of a radix select by thread 0: pick the bin that holds the `want`-th element counted from the top
// (descending) or from the bottom.  Returns the bin; `want` becomes the rank inside it, `in_bin` its population.
__device__ __forceinline__ int pick_bin(const uint32_t* hist, bool descending, uint32_t& want, uint32_t& in_bin) {
  uint32_t cum = 0;
  for (int s = 0; s < 256; ++s) {
    const int b = descending ? 255 - s : s;
    const uint32_t h = hist[b];
    if (cum + h >= want) {
      want -= cum;
      in_bin = h;
      return b;
    }
    cum += h;
  }
  in_bin = 0;  // not reached while want <= the number of elements
  return descending ? 0 : 255;
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void itemknn_column_kernel(
    const int64_t* __restrict__ csc_indptr, const int32_t* __restrict__ csc_users, const float* __restrict__ csc_vals,
    const int64_t* __restrict__ csr_indptr, const int32_t* __restrict__ csr_items, const float* __restrict__ csr_vals,
    const float* __restrict__ na, const float* __restrict__ nb, int n_users, int n_items, int col0, SimParams sp,
    int top_k, int ldk, float* __restrict__ slab, int32_t* __restrict__ w_idx, float* __restrict__ w_val,
    int32_t* __restrict__ w_cnt) {
  __shared__ float acc_lds[kLds ? kLdsItems : 1];
  __shared__ uint64_t keys[kMaxK];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_nzero, s_prefix, s_want, s_in_bin, s_count;
  const int tid = threadIdx.x;
  const int i = col0 + blockIdx.x;
  float* acc = kLds ? acc_lds : slab + (size_t)blockIdx.x * n_items;

  for (int j = tid; j < n_items; j += kThreads) acc[j] = 0.f;
  if (tid == 0) s_nzero = 0, s_prefix = 0, s_want = (uint32_t)top_k, s_in_bin = 0, s_count = 0;
  __syncthreads();
  walk_rows(csc_users, csc_vals, csc_indptr[i], csc_indptr[i + 1], csr_indptr, n_users, csr_items, csr_vals, n_items,
            acc);

  // the similarity, in place; exact zeros counted
  const float nai = na[i], nbi = nb[i];
  uint32_t nz = 0;
  for (int j = tid; j < n_items; j += kThreads) {
    float x = j == i ? 0.f : similarity_of(sp, acc[j], nai, nbi, na[j], nb[j]);
    if (!(x == x) || x == 0.f) x = 0.f;  // no NaN, no -0
    acc[j] = x;
    nz += x == 0.f;
  }
  if (nz) atomicAdd(&s_nzero, nz);
  __syncthreads();
  const uint32_t nzero = s_nzero;

  // K-th largest value: 4 passes over the bytes of the orderable pattern, most significant first
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    for (int j = tid; j < n_items; j += kThreads) {
      const float x = acc[j];
      if (x == 0.f) continue;
      const uint32_t k = orderable(x);
      if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      if ((kZeroKey & himask) == prefix) hist[(kZeroKey >> shift) & 255u] += nzero;
      uint32_t want = s_want, in_bin;
      const int b = pick_bin(hist, true, want, in_bin);
      s_prefix = prefix | ((uint32_t)b << shift);
      s_want = want;
      s_in_bin = in_bin;
    }
    __syncthreads();
  }
  const uint32_t tkey = s_prefix;       // the K-th largest value
  const uint32_t need_eq = s_want;      // how many entries equal to it are inside the top K ...
  const bool all_eq = need_eq == s_in_bin || tkey == kZeroKey;   // ... all of them (or they are zeros: dropped anyway)
  uint32_t jt = 0xffffffffu;            // equal entries are kept up to this index
  if (!all_eq) {
    // the need_eq-th smallest index among the entries equal to the threshold: the same select over the index bytes
    const int nbytes = n_items <= (1 << 8) ? 1 : n_items <= (1 << 16) ? 2 : n_items <= (1 << 24) ? 3 : 4;
    __syncthreads();
    if (tid == 0) s_prefix = 0;
    for (int pass = 4 - nbytes; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
      hist[tid] = 0;
      __syncthreads();
      const uint32_t prefix = s_prefix;
      for (int j = tid; j < n_items; j += kThreads) {
        const float x = acc[j];
        if (x != 0.f && orderable(x) == tkey && ((uint32_t)j & himask) == prefix)
          atomicAdd(&hist[((uint32_t)j >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t want = s_want, in_bin;
        const int b = pick_bin(hist, false, want, in_bin);
        s_prefix = prefix | ((uint32_t)b << shift);
        s_want = want;
      }
      __syncthreads();
    }
    jt = s_prefix;
  }

  // the winners that are not zero, in any order: the sort below fixes it
  for (int j = tid; j < n_items; j += kThreads) {
    const float x = acc[j];
    if (x == 0.f) continue;
    const uint32_t k = orderable(x);
    if (k > tkey || (k == tkey && (uint32_t)j <= jt)) {
      const uint32_t slot = atomicAdd(&s_count, 1u);
      if (slot < (uint32_t)kMaxK) keys[slot] = ((uint64_t)k << 32) | (0xffffffffu - (uint32_t)j);
    }
  }
  __syncthreads();
  const int n = (int)(s_count < (uint32_t)top_k ? s_count : (uint32_t)top_k);
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int t = n + tid; t < np2; t += kThreads) keys[t] = 0;
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < np2; t += kThreads) {
        const int l = t ^ jj;
        if (l > t) {
          const uint64_t a = keys[t], b = keys[l];
          if ((t & k) == 0 ? a < b : a > b) keys[t] = b, keys[l] = a;
        }
      }
      __syncthreads();
    }
  int32_t* oi = w_idx + (size_t)i * ldk;
  float* ov = w_val + (size_t)i * ldk;
  for (int s = tid; s < ldk; s += kThreads) {
    const uint64_t key = s < n ? keys[s] : 0;
    oi[s] = s < n ? (int32_t)(0xffffffffu - (uint32_t)key) : -1;
    ov[s] = s < n ? from_orderable((uint32_t)(key >> 32)) : 0.f;
  }
  if (tid == 0) w_cnt[i] = n;
}

// key of slot s of column i: (neighbour j, i, s); empty slots get j = n_items and sort behind every row
__global__ __launch_bounds__(kThreads) void itemknn_keys_kernel(const int32_t* __restrict__ w_idx,
                                                                const int32_t* __restrict__ w_cnt, int n_items,
                                                                int ldk, int shift, uint64_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (int64_t)n_items * ldk) return;
  const int i = (int)(e / ldk), s = (int)(e % ldk);
  int j = s < w_cnt[i] ? w_idx[e] : n_items;
  if ((uint32_t)j > (uint32_t)n_items) j = n_items;
  keys[e] = ((uint64_t)j << shift) | ((uint64_t)i << kSlotBits) | (uint64_t)s;
}

// position p of the sorted keys: entry p of W^T, and the start of every row that begins at p
__global__ __launch_bounds__(kThreads) void itemknn_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                                  int n_items, int ldk, int shift,
                                                                  const float* __restrict__ w_val,
                                                                  int64_t* __restrict__ t_indptr,
                                                                  int32_t* __restrict__ t_cols,
                                                                  float* __restrict__ t_vals) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p > n) return;
  const uint64_t key = p < n ? keys[p] : 0;
  const int64_t jp = p < n ? (int64_t)(key >> shift) : n_items;
  const int64_t jprev = p > 0 ? (int64_t)(keys[p - 1] >> shift) : -1;
  for (int64_t r = jprev + 1; r <= jp && r <= n_items; ++r) t_indptr[r] = p;
  if (p < n && jp < n_items) {
    const int i = (int)((key >> kSlotBits) & ((1ull << (shift - kSlotBits)) - 1)), s = (int)(key & (kMaxK - 1));
    t_cols[p] = i;
    t_vals[p] = (i < n_items && s < ldk) ? w_val[(size_t)i * ldk + s] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void itemknn_score_kernel(
    const int32_t* __restrict__ users, const int64_t* __restrict__ csr_indptr, const int32_t* __restrict__ csr_items,
    const float* __restrict__ csr_vals, int n_users, int n_items, const int64_t* __restrict__ t_indptr,
    const int32_t* __restrict__ t_cols, const float* __restrict__ t_vals, float* __restrict__ S, int64_t ld_s) {
  const int u = users[blockIdx.x];
  float* row = S + (size_t)blockIdx.x * ld_s;
  for (int c = threadIdx.x; c < n_items; c += kThreads) row[c] = 0.f;
  __syncthreads();
  if ((uint32_t)u >= (uint32_t)n_users) return;
  walk_rows(csr_items, csr_vals, csr_indptr[u], csr_indptr[u + 1], t_indptr, n_items, t_cols, t_vals, n_items, row);
}

int bits_of(uint64_t x) {  // bits needed to write x
  int b = 0;
  while (x) ++b, x >>= 1;
  return b;
}

int check_sizes(int n_users, int n_items, int neighbor, int block_cols, int* shift) {
  NR_REQUIRE(n_users >= 0 && n_items >= 1, NR_ERR_ARG, "itemknn: bad matrix shape %d x %d", n_users, n_items);
  NR_REQUIRE(neighbor >= 1, NR_ERR_ARG, "itemknn: neighbor must be >= 1, got %d", neighbor);
  NR_REQUIRE(neighbor <= kMaxK, NR_ERR_UNSUPPORTED, "itemknn: neighbor %d is not supported (at most %d)", neighbor,
             kMaxK);
  NR_REQUIRE(block_cols >= 1, NR_ERR_ARG, "itemknn: block_cols must be >= 1, got %d", block_cols);
  const int sh = kSlotBits + bits_of((uint64_t)n_items - 1);
  NR_REQUIRE(sh + bits_of((uint64_t)n_items) <= 63 && (int64_t)n_items * neighbor <= kMaxKeys, NR_ERR_UNSUPPORTED,
             "itemknn: %d items x %d neighbours is past the transpose's key sort (items * neighbor <= 2^29)", n_items,
             neighbor);
  if (shift) *shift = sh;
  return NR_OK;
}

size_t slab_bytes(int n_items, int block_cols) {
  if (n_items <= kLdsItems) return 0;
  const int bc = block_cols < n_items ? block_cols : n_items;
  return nr_align_up((size_t)bc * n_items * sizeof(float), 256);
}

}  // namespace

extern "C" {

int nrhip_itemknn_workspace_bytes(int n_items, int neighbor, int block_cols, size_t* bytes) {
  NR_REQUIRE(bytes, NR_ERR_ARG, "itemknn_workspace_bytes: bad arguments");
  NR_TRY(check_sizes(0, n_items, neighbor, block_cols, nullptr));
  *bytes = slab_bytes(n_items, block_cols) + (size_t)n_items * neighbor * sizeof(uint64_t);
  return NR_OK;
}

int nrhip_itemknn_build(const int64_t* d_csc_indptr, const int32_t* d_csc_users, const float* d_csc_vals,
                        const int64_t* d_csr_indptr, const int32_t* d_csr_items, const float* d_csr_vals,
                        const float* d_na, const float* d_nb, int n_users, int n_items, int kind, float shrink,
                        float tversky_alpha, float tversky_beta, int neighbor, int block_cols, int32_t* d_w_idx,
                        float* d_w_val, int32_t* d_w_cnt, int64_t* d_t_indptr, int32_t* d_t_cols, float* d_t_vals,
                        void* d_ws, size_t ws_bytes, void* stream) {
  NR_REQUIRE(d_csc_indptr && d_csc_users && d_csc_vals && d_csr_indptr && d_csr_items && d_csr_vals && d_na && d_nb &&
                 d_w_idx && d_w_val && d_w_cnt && d_t_indptr && d_t_cols && d_t_vals,
             NR_ERR_ARG, "itemknn_build: bad arguments");
  NR_REQUIRE(kind >= kCosine && kind <= kEuclidean, NR_ERR_ARG, "itemknn_build: unknown similarity kind %d", kind);
  NR_REQUIRE(std::isfinite(shrink) && shrink >= 0.f, NR_ERR_ARG, "itemknn_build: shrink must be >= 0, got %g",
             (double)shrink);
  int shift = 0;
  NR_TRY(check_sizes(n_users, n_items, neighbor, block_cols, &shift));
  const size_t slab = slab_bytes(n_items, block_cols);
  const int64_t n_keys = (int64_t)n_items * neighbor;
  const size_t need = slab + (size_t)n_keys * sizeof(uint64_t);
  NR_REQUIRE(d_ws && ws_bytes >= need, NR_ERR_WORKSPACE, "itemknn_build: workspace of %zu bytes, %zu needed", ws_bytes,
             need);
  hipStream_t st = (hipStream_t)stream;
  const SimParams sp{kind, shrink, tversky_alpha, tversky_beta};
  const int top_k = neighbor < n_items ? neighbor : n_items;
  float* d_slab = (float*)d_ws;
  uint64_t* d_keys = (uint64_t*)((char*)d_ws + slab);
  for (int col0 = 0; col0 < n_items; col0 += block_cols) {
    const int nc = n_items - col0 < block_cols ? n_items - col0 : block_cols;
    if (n_items <= kLdsItems)
      hipLaunchKernelGGL(itemknn_column_kernel<true>, dim3(nc), dim3(kThreads), 0, st, d_csc_indptr, d_csc_users,
                         d_csc_vals, d_csr_indptr, d_csr_items, d_csr_vals, d_na, d_nb, n_users, n_items, col0, sp,
                         top_k, neighbor, d_slab, d_w_idx, d_w_val, d_w_cnt);
    else
      hipLaunchKernelGGL(itemknn_column_kernel<false>, dim3(nc), dim3(kThreads), 0, st, d_csc_indptr, d_csc_users,
                         d_csc_vals, d_csr_indptr, d_csr_items, d_csr_vals, d_na, d_nb, n_users, n_items, col0, sp,
                         top_k, neighbor, d_slab, d_w_idx, d_w_val, d_w_cnt);
    NR_LAUNCH_CHECK();
  }
  const unsigned key_blocks = (unsigned)((n_keys + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(itemknn_keys_kernel, dim3(key_blocks), dim3(kThreads), 0, st, d_w_idx, d_w_cnt, n_items, neighbor,
                     shift, d_keys);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(d_keys, (int)n_keys, stream));
  hipLaunchKernelGGL(itemknn_unpack_kernel, dim3((unsigned)((n_keys + 1 + kThreads - 1) / kThreads)), dim3(kThreads),
                     0, st, d_keys, n_keys, n_items, neighbor, shift, d_w_val, d_t_indptr, d_t_cols, d_t_vals);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_itemknn_score(const int32_t* d_users, int batch, const int64_t* d_csr_indptr, const int32_t* d_csr_items,
                        const float* d_csr_vals, int n_users, int n_items, const int64_t* d_t_indptr,
                        const int32_t* d_t_cols, const float* d_t_vals, float* d_S, int64_t ld_s, void* stream) {
  NR_REQUIRE(batch >= 0 && n_users >= 0 && n_items >= 1 && ld_s >= n_items && d_csr_indptr && d_csr_items &&
                 d_csr_vals && d_t_indptr && d_t_cols && d_t_vals && (batch == 0 || (d_users && d_S)),
             NR_ERR_ARG, "itemknn_score: bad arguments");
  if (batch == 0) return NR_OK;
  hipLaunchKernelGGL(itemknn_score_kernel, dim3(batch), dim3(kThreads), 0, (hipStream_t)stream, d_users, d_csr_indptr,
                     d_csr_items, d_csr_vals, n_users, n_items, d_t_indptr, d_t_cols, d_t_vals, d_S, ld_s);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
