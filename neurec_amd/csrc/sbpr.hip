// sbpr.hip — SBPR (Zhao et al., CIKM 2014; model/social_recommender/SBPR.py) on gfx950: the social item sets, one
// epoch's instance stream and the step.
//
// Sets (SBPR.py:40-49, once per model).  C_u = the distinct items of the users u trusts that u has not, each with the
// number of trusted users who hold it (suk - 1, SBPR.py:143-145): the product S R with counts, minus R's own pattern.
// A block of whole users [u0, u1) whose expansion fits the workspace:
//   sbpr_sizes_kernel     E_u = sum over f in S_u of |R_f| (0 for a user without train items; a trusted user without
//                         train items adds nothing)
//   sbpr_expand_kernel    a workgroup per user: (u, f in S_u, k in R_f) -> key u << 32 | k at the user's offset
//   nrhip_sort_u64        the keys, ascending: a user's keys lie together already, so every user's segment is sorted
//                         on its own — nrhip_sort_u64_segments for the segments one workgroup's LDS holds, one
//                         nrhip_sort_u64 per larger one (or one sort of the whole block when no lengths are given)
//   sbpr_mark_kernel      the head of a run counts its length; a run whose k is in R_u (binary search) counts 0.  The
//                         survivors of each chunk of 1,024 keys are counted
//   sbpr_scan_kernel      one workgroup: the chunks' exclusive offsets and the total
//   sbpr_compact_kernel   every key's output position (the exclusive count of survivors before it); the survivors'
//                         items and counts written there, in key order
//   sbpr_indptr_kernel    per user the position of its first key
// Nothing is ordered by an atomic: the result is the same on every run.
//
// Stream (SBPR.py:122-148 and DataIterator(shuffle=True)).  One slot per (eligible user, train item) in user order;
// output position p carries slot perm(p) as sampler.hip's sample_instances_kernel does.  The draws of slot s come from
// nr::XorShift64s seeded (seed, epoch, s): word 0 picks k = C_u[mulhi64(h, |C_u|)], the following words are the
// attempts at j, uniform over [0, I) and rejected while in R_u or C_u (two binary searches).  After nr::kMaxRejects
// rejections j is the r-th free item, r = mulhi64(h, free), found by bisecting the count of free items below an id.
//
// Step (SBPR.py:68-92), slot t = (u, i, k, j, suk):
//     x_a = P_u . Q_a + b_a;   y1 = (x_i - x_k) / suk,  y2 = x_k - x_j
//     loss = f(y1) + f(y2) + reg l2(P_u, Q_k, Q_i, Q_j, b_i, b_k, b_j)
//     g1 = f'(y1) / suk,  g2 = f'(y2):   d/dx_i = g1,  d/dx_k = g2 - g1,  d/dx_j = -g2
//   sbpr_forward_kernel   one lane group per slot: the three dots, g1 and g2, the slot's loss and l2, the row flags and
//                         the slot's four keys over one key space of U + I rows, key = row << 32 | t << 2 | role:
//                             keys [0, B) P row u (role 0), [B, 2B) Q row U + i (1), [2B, 3B) U + k (2), [3B, 4B) U + j (3)
//   loss_kernel           (loss term, regulariser term) in double
//   sbpr_rows_kernel      one lane group per sorted key: the head of a run sums the row's occurrences in key order — by
//                         slot, and in one slot i before k before j — and STORES the row's gradient.  i, k and j may
//                         coincide in a slot and across slots: one row is one run whatever its roles
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

enum { ROLE_USER = 0, ROLE_POS = 1, ROLE_SOCIAL = 2, ROLE_NEG = 3 };
enum { S_G1 = S_G, S_G2 = S_OK };                          // the slot's two derivatives in d_scal

constexpr int kChunk = 1024;                               // keys of one workgroup of the mark and compact kernels

// ------------------------------------------------------------------------------------------------------ sets
__global__ __launch_bounds__(256) void sbpr_sizes_kernel(const int64_t* __restrict__ tr_indptr,
                                                         const int64_t* __restrict__ s_indptr,
                                                         const int32_t* __restrict__ s_indices, int n_users,
                                                         int64_t* __restrict__ out) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_users) return;
  int64_t e = 0;
  if (tr_indptr[u + 1] > tr_indptr[u]) {
    for (int64_t q = s_indptr[u]; q < s_indptr[u + 1]; ++q) {
      const int f = s_indices[q];
      if (f >= 0 && f < n_users) e += tr_indptr[f + 1] - tr_indptr[f];
    }
  }
  out[u] = e;
}

__global__ __launch_bounds__(256) void sbpr_expand_kernel(nrhip_sbpr_sets_args a) {
  const int u = a.u0 + blockIdx.x;
  if (a.d_tr_indptr[u + 1] == a.d_tr_indptr[u]) return;      // not in train_dict: no set
  int64_t off = a.d_pair_off[blockIdx.x];
  const int64_t end = a.d_pair_off[blockIdx.x + 1];
  for (int64_t q = a.d_s_indptr[u]; q < a.d_s_indptr[u + 1]; ++q) {
    const int f = a.d_s_indices[q];
    if (f < 0 || f >= a.n_users) continue;
    const int64_t rb = a.d_tr_indptr[f], len = a.d_tr_indptr[f + 1] - rb;
    for (int64_t x = threadIdx.x; x < len; x += 256)
      if (off + x < end) a.d_keys[off + x] = row_key(u, (uint32_t)a.d_tr_indices[rb + x]);
    off += len;
  }
}

__global__ __launch_bounds__(256) void sbpr_mark_kernel(nrhip_sbpr_sets_args a) {
  __shared__ int s_sum[256];
  const int64_t n = a.n_pairs, p0 = (int64_t)blockIdx.x * kChunk + threadIdx.x * 4;
  int mine = 0;
  for (int e = 0; e < 4; ++e) {
    const int64_t p = p0 + e;
    if (p >= n) break;
    const uint64_t key = a.d_keys[p];
    int cnt = 0;
    if (p == 0 || a.d_keys[p - 1] != key) {
      const int u = (int)(key >> 32);
      const int64_t rb = u >= a.u0 && u < a.u1 ? a.d_tr_indptr[u] : 0;
      if (u >= a.u0 && u < a.u1 &&
          !nr::sorted_contains(a.d_tr_indices + rb, (int)(a.d_tr_indptr[u + 1] - rb), (int32_t)(uint32_t)key)) {
        int64_t q = p + 1;
        while (q < n && a.d_keys[q] == key) ++q;
        cnt = (int)(q - p);
        ++mine;
      }
    }
    a.d_cnt[p] = cnt;
  }
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.d_chunk[blockIdx.x] = s_sum[0];
}

// d_chunk [n_chunks] sums -> exclusive offsets, d_chunk[n_chunks] and *d_total the total
__global__ __launch_bounds__(256) void sbpr_scan_kernel(int64_t* __restrict__ chunk, int64_t n_chunks,
                                                        int64_t* __restrict__ total) {
  __shared__ int64_t s_part[256];
  const int64_t per = (n_chunks + 255) / 256;
  const int64_t lo = min((int64_t)threadIdx.x * per, n_chunks), hi = min(lo + per, n_chunks);
  int64_t sum = 0;
  for (int64_t x = lo; x < hi; ++x) sum += chunk[x];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    for (int t = 0; t < 256; ++t) {
      const int64_t v = s_part[t];
      s_part[t] = acc;
      acc += v;
    }
    chunk[n_chunks] = acc;
    *total = acc;
  }
  __syncthreads();
  int64_t acc = s_part[threadIdx.x];
  for (int64_t x = lo; x < hi; ++x) {
    const int64_t v = chunk[x];
    chunk[x] = acc;
    acc += v;
  }
}

__global__ __launch_bounds__(256) void sbpr_compact_kernel(nrhip_sbpr_sets_args a) {
  __shared__ int s_scan[256];
  const int64_t n = a.n_pairs, p0 = (int64_t)blockIdx.x * kChunk + threadIdx.x * 4;
  int cnt[4], mine = 0;
  for (int e = 0; e < 4; ++e) {
    cnt[e] = p0 + e < n ? a.d_cnt[p0 + e] : 0;
    mine += cnt[e] > 0;
  }
  s_scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = (int)threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t pos = a.d_chunk[blockIdx.x] + (s_scan[threadIdx.x] - mine);
  for (int e = 0; e < 4; ++e) {
    const int64_t p = p0 + e;
    if (p >= n) break;
    a.d_pos[p] = (int32_t)pos;
    if (cnt[e] > 0) {
      a.d_items_out[pos] = (int32_t)(uint32_t)a.d_keys[p];
      a.d_counts_out[pos] = cnt[e];
      ++pos;
    }
  }
}

__global__ __launch_bounds__(256) void sbpr_indptr_kernel(nrhip_sbpr_sets_args a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x > a.u1 - a.u0) return;
  const uint64_t want = (uint64_t)(uint32_t)(a.u0 + x) << 32;
  int64_t lo = 0, hi = a.n_pairs;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.d_keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  a.d_indptr_out[x] = lo < a.n_pairs ? (int64_t)a.d_pos[lo] : *a.d_total;
}

// ------------------------------------------------------------------------------------------------------ stream
// the number of ids <= x in an ascending list
__device__ __forceinline__ int count_le(const int32_t* a, int n, int32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sbpr_stream_kernel(const nrhip_sbpr_stream_args a) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.out_count) return;
  const int64_t p = a.out_begin + q;
  const uint64_t perm_key = nr::splitmix64(a.seed ^ nr::splitmix64(a.epoch + 0x51ed27ull));
  const int64_t s = a.shuffle ? (int64_t)nr::permute_index((uint64_t)p, (uint64_t)a.n_slots, perm_key) : p;
  const int32_t r = a.d_slot_row[s];
  const int u = a.d_elig[r];
  const int64_t rb = a.d_tr_indptr[u], cb = a.d_c_indptr[u];
  const int nr_ = (int)(a.d_tr_indptr[u + 1] - rb), nc = (int)(a.d_c_indptr[u + 1] - cb);
  const int32_t* R = a.d_tr_indices + rb;
  const int32_t* Cs = a.d_c_items + cb;
  a.d_users_out[q] = u;
  a.d_items_out[q] = R[s - a.d_slot_ptr[r]];
  nr::XorShift64s g;
  g.seed(a.seed, a.epoch, (uint64_t)s);
  int k = -1, j = -1;
  float suk = 1.0f;
  if (nc > 0) {                                            // an eligible user has a social item
    const int at = (int)__umul64hi(g.next(), (uint64_t)nc);
    k = Cs[at];
    suk = (float)(a.d_c_counts[cb + at] + 1);
  }
  const int free_n = a.n_items - nr_ - nc;
  if (free_n > 0) {
    for (int tries = 0; tries < nr::kMaxRejects && j < 0; ++tries) {
      const int32_t cand = (int32_t)__umul64hi(g.next(), (uint64_t)a.n_items);
      if (!nr::sorted_contains(R, nr_, cand) && !nr::sorted_contains(Cs, nc, cand)) j = cand;
    }
    if (j < 0) {
      // the rank-th free item: the smallest x with rank + 1 free ids in [0, x]
      const int rank = (int)__umul64hi(g.next(), (uint64_t)free_n);
      int lo = 0, hi = a.n_items - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mid + 1 - count_le(R, nr_, mid) - count_le(Cs, nc, mid) >= rank + 1) hi = mid; else lo = mid + 1;
      }
      j = lo;
    }
  }
  a.d_social_out[q] = k;
  a.d_neg_out[q] = j;
  a.d_suk_out[q] = suk;
}

// ------------------------------------------------------------------------------------------------------ step
__device__ __forceinline__ uint64_t slot_key(int row, int t, int role) {
  return row_key(row, ((uint32_t)t << 2) | (uint32_t)role);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void sbpr_forward_kernel(nrhip_sbpr_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items;
  const bool in = t < B;
  int u = -1, i = -1, k = -1, j = -1;
  float suk = 1.f;
  if (in) {
    u = a.d_users[t];
    i = a.d_items[t];
    k = a.d_social[t];
    j = a.d_neg[t];
    suk = a.d_suk[t];
  }
  // a slot takes part as a whole or not at all: every lookup must be a table row
  const bool ok = in && u >= 0 && u < U && i >= 0 && i < I && k >= 0 && k < I && j >= 0 && j < I;
  float di = 0.f, dk = 0.f, dj = 0.f, sq = 0.f;
  if (ok) {
#pragma unroll
    for (int m = 0; m < CPL; ++m) {
      const int col = c + m * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col];
        const float qi = a.d_Q[(int64_t)i * d + col], qk = a.d_Q[(int64_t)k * d + col];
        const float qj = a.d_Q[(int64_t)j * d + col];
        di += p * qi;
        dk += p * qk;
        dj += p * qj;
        sq += p * p + qk * qk + qi * qi + qj * qj;
      }
    }
  }
  group_sum<DP>(di, dk, dj, sq);
  if (!in || c != 0) return;
  float g1 = 0.f, g2 = 0.f, loss = 0.f;
  if (ok) {
    const float bi = a.d_b[i], bk = a.d_b[k], bj = a.d_b[j];
    const float xi = di + bi, xk = dk + bk, xj = dj + bj;
    const float y1 = (xi - xk) / suk, y2 = xk - xj;
    loss = nr::pairwise_loss(a.loss_kind, y1) + nr::pairwise_loss(a.loss_kind, y2);
    g1 = nr::pairwise_dloss(a.loss_kind, y1) / suk;
    g2 = nr::pairwise_dloss(a.loss_kind, y2);
    sq += bi * bi + bk * bk + bj * bj;
    if (a.d_flag_P) a.d_flag_P[u] = 1;
    if (a.d_flag_Q) {
      a.d_flag_Q[i] = 1;
      a.d_flag_Q[k] = 1;
      a.d_flag_Q[j] = 1;
    }
    if (a.d_flag_b) {
      a.d_flag_b[i] = 1;
      a.d_flag_b[k] = 1;
      a.d_flag_b[j] = 1;
    }
  }
  float* sc = a.d_scal + (int64_t)t * kScal;
  store_slot(sc, g1, loss, sq, ok);
  sc[S_G2] = g2;
  a.d_keys[t] = ok ? slot_key(u, t, ROLE_USER) : kSentinel;
  a.d_keys[(int64_t)B + t] = ok ? slot_key(U + i, t, ROLE_POS) : kSentinel;
  a.d_keys[2 * (int64_t)B + t] = ok ? slot_key(U + k, t, ROLE_SOCIAL) : kSentinel;
  a.d_keys[3 * (int64_t)B + t] = ok ? slot_key(U + j, t, ROLE_NEG) : kSentinel;
}

// the sum of one run of the sorted keys: the row's occurrences in key order
template <int DP, int CPL>
__global__ __launch_bounds__(256) void sbpr_rows_kernel(nrhip_sbpr_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int d = a.d, U = a.n_users;
  const int64_t n_keys = 4 * (int64_t)a.batch;
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  const float reg = a.reg;
  const bool is_user = row < U;
  const int r = is_user ? row : row - U;
  float own[CPL], acc[CPL] = {};
  load_row<DP, CPL>(is_user ? a.d_P : a.d_Q, r, d, c, own);
  const float own_b = is_user ? 0.f : a.d_b[r];
  float gb = 0.f;
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t low) {
    const int role = (int)(low & 3u), t = (int)(low >> 2);
    const float g1 = a.d_scal[(int64_t)t * kScal + S_G1], g2 = a.d_scal[(int64_t)t * kScal + S_G2];
    if (role == ROLE_USER) {
      const int i = a.d_items[t], k = a.d_social[t], j = a.d_neg[t];
      const float gk = g2 - g1;
#pragma unroll
      for (int m = 0; m < CPL; ++m) {
        const int col = c + m * DP;
        if (col < d)
          acc[m] += ((g1 * a.d_Q[(int64_t)i * d + col] + gk * a.d_Q[(int64_t)k * d + col]) -
                     g2 * a.d_Q[(int64_t)j * d + col]) + reg * own[m];
      }
    } else {
      const float s = role == ROLE_POS ? g1 : role == ROLE_SOCIAL ? g2 - g1 : -g2;
      const int u = a.d_users[t];
      gb += s + reg * own_b;
#pragma unroll
      for (int m = 0; m < CPL; ++m) {
        const int col = c + m * DP;
        if (col < d) acc[m] += s * a.d_P[(int64_t)u * d + col] + reg * own[m];
      }
    }
  });
  store_row<DP, CPL>(is_user ? a.d_G_P : a.d_G_Q, r, d, c, acc);
  if (!is_user && c == 0) a.d_G_b[r] = gb;
}

}  // namespace

extern "C" {

int nrhip_sbpr_expansion_sizes(const int64_t* d_tr_indptr, const int64_t* d_s_indptr, const int32_t* d_s_indices,
                               int n_users, int64_t* d_sizes, void* stream) {
  NR_REQUIRE(n_users >= 0, NR_ERR_ARG, "sbpr_expansion_sizes: bad sizes");
  if (n_users == 0) return NR_OK;
  NR_REQUIRE(d_tr_indptr && d_s_indptr && d_sizes, NR_ERR_ARG, "sbpr_expansion_sizes: null pointer argument");
  hipLaunchKernelGGL(sbpr_sizes_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     d_tr_indptr, d_s_indptr, d_s_indices, n_users, d_sizes);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_sbpr_sets_block(const nrhip_sbpr_sets_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "sbpr_sets_block: null argument block");
  const nrhip_sbpr_sets_args a = *args;
  NR_REQUIRE(a.n_users >= 0 && a.n_items >= 0 && a.u0 >= 0 && a.u0 <= a.u1 && a.u1 <= a.n_users && a.n_pairs >= 0 &&
                 a.n_pairs <= NRHIP_SBPR_MAX_PAIRS, NR_ERR_ARG,
             "sbpr_sets_block: bad sizes (users [%d, %d) of %d, %lld pairs, at most %lld)", a.u0, a.u1, a.n_users,
             (long long)a.n_pairs, (long long)NRHIP_SBPR_MAX_PAIRS);
  NR_REQUIRE(a.d_indptr_out && a.d_total, NR_ERR_ARG, "sbpr_sets_block: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int n_block = a.u1 - a.u0;
  if (a.n_pairs == 0 || n_block == 0) {
    NR_CHECK_HIP(hipMemsetAsync(a.d_indptr_out, 0, sizeof(int64_t) * (size_t)(n_block + 1), st));
    NR_CHECK_HIP(hipMemsetAsync(a.d_total, 0, sizeof(int64_t), st));
    return NR_OK;
  }
  NR_REQUIRE(a.d_tr_indptr && a.d_tr_indices && a.d_s_indptr && a.d_s_indices && a.d_pair_off && a.d_keys && a.d_cnt &&
                 a.d_pos && a.d_chunk && a.d_items_out && a.d_counts_out, NR_ERR_ARG,
             "sbpr_sets_block: null pointer argument");
  const int64_t n_chunks = (a.n_pairs + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(sbpr_expand_kernel, dim3((unsigned)n_block), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  if (a.d_seg_len) {
    // the keys of a user lie together already: each user's segment sorted on its own gives the order of the whole
    NR_REQUIRE(a.max_seg_len >= 0 && a.n_big >= 0 && (a.n_big == 0 || (a.h_big_off && a.h_big_len)), NR_ERR_ARG,
               "sbpr_sets_block: bad segment arguments");
    NR_TRY(nrhip_sort_u64_segments(a.d_keys, a.d_pair_off, a.d_seg_len, n_block, a.max_seg_len, stream));
    for (int x = 0; x < a.n_big; ++x) {
      const int64_t off = a.h_big_off[x], len = a.h_big_len[x];
      NR_REQUIRE(off >= 0 && len >= 0 && off + len <= a.n_pairs, NR_ERR_ARG,
                 "sbpr_sets_block: segment [%lld,+%lld) outside the %lld pairs", (long long)off, (long long)len,
                 (long long)a.n_pairs);
      NR_TRY(nrhip_sort_u64(a.d_keys + off, (int)len, stream));
    }
  } else {
    NR_TRY(nrhip_sort_u64(a.d_keys, (int)a.n_pairs, stream));
  }
  hipLaunchKernelGGL(sbpr_mark_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sbpr_scan_kernel, dim3(1), dim3(256), 0, st, a.d_chunk, n_chunks, a.d_total);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sbpr_compact_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sbpr_indptr_kernel, dim3((unsigned)((n_block + 1 + 255) / 256)), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_sbpr_stream(const nrhip_sbpr_stream_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "sbpr_stream: null argument block");
  const nrhip_sbpr_stream_args a = *args;
  NR_REQUIRE(a.n_items >= 1 && a.n_users >= 0 && a.n_elig >= 0 && a.n_slots >= 0 && a.out_begin >= 0 &&
                 a.out_count >= 0 && a.out_begin + a.out_count <= a.n_slots, NR_ERR_ARG,
             "sbpr_stream: bad range [%lld,+%lld) of %lld", (long long)a.out_begin, (long long)a.out_count,
             (long long)a.n_slots);
  if (a.out_count == 0) return NR_OK;
  NR_REQUIRE(a.d_tr_indptr && a.d_tr_indices && a.d_c_indptr && a.d_c_items && a.d_c_counts && a.d_slot_ptr &&
                 a.d_slot_row && a.d_elig && a.d_users_out && a.d_items_out && a.d_social_out && a.d_neg_out &&
                 a.d_suk_out, NR_ERR_ARG, "sbpr_stream: null pointer argument");
  hipLaunchKernelGGL(sbpr_stream_kernel, dim3((unsigned)((a.out_count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_sbpr_step(const nrhip_sbpr_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "sbpr_step: null argument block");
  const nrhip_sbpr_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_SBPR_MAX_D, NR_ERR_UNSUPPORTED, "sbpr_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_SBPR_MAX_D);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_SBPR_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG, "sbpr_step: bad sizes");
  NR_TRY(check_loss_kind("sbpr_step", 1, a.loss_kind));
  const int B = a.batch;
  if (B == 0) return NR_OK;                                // no work: nothing is launched, nothing is written
  NR_REQUIRE(a.d_P && a.d_Q && a.d_b && a.d_G_P && a.d_G_Q && a.d_G_b && a.d_users && a.d_items && a.d_social &&
                 a.d_neg && a.d_suk && a.d_keys && a.d_scal && a.d_loss2, NR_ERR_ARG,
             "sbpr_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int n_keys = 4 * B;
  NR_BY_WIDTH(sbpr_forward_kernel, a.d, B, st, a);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(a.d_keys, n_keys, stream));
  hipLaunchKernelGGL(loss_kernel<nrhip_sbpr_step_args>, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  NR_BY_WIDTH(sbpr_rows_kernel, a.d, n_keys, st, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
