// hrm.hip — HRM (Wang et al., SIGIR 2015): the step of model/sequential_recommender/HRM.py on gfx950.
//
// An instance is (user u, recents r_0..r_{L-1}, item i, label y) over two row tables P [U][d] and V [I][d]:
//     s = session_agg over l of V[r_l]   (L >= 2: column-wise max or mean; L == 1: V[r_0])           HRM.py:68-77
//     h = pre_agg over {P[u], s}         (column-wise max or the mean of the two)                    HRM.py:78-81
//     x = <h, V[i]>                                                                                  HRM.py:82-83
// Both tables are read through embedding_lookup only: the gradients are sparse and a row's gradient is the sum over its
// occurrences in the batch.  V is looked up in two roles; the sum of a V row is taken in the order of its sort keys
// (row | position): its TARGET occurrences first, by batch slot t (positions 0..B), then its RECENT occurrences by
// (slot t, column l) (positions B + t L + l).  A user's occurrences come by batch slot.
//
// The max's derivative goes to the inputs equal to the maximum, in equal shares (TF's _MinOrMaxGrad: indicators /
// num_selected * grad).  The shares are decided ONCE, in the forward kernel, and carried to the rows kernel in two
// [B][d] buffers: d_s, the pooled session row, and d_ds, the derivative of the loss with respect to s already divided
// by the number of tied recents (max) or by L (mean).  A recent occurrence of row r then takes d_ds[c] where
// V[r][c] == d_s[c] (max) or d_ds[c] outright (mean, L == 1); an item that stands twice among one instance's recents
// ties with itself and receives its share twice.  The user's and the target's rows recompute h and the user's share
// from P[u] and d_s with the function the forward used (pool_pre).
//
//   hrm_forward_kernel    one lane group (DP lanes, DP = 16 / 32 / 64 by d) per batch slot: gathers P[u], V[i] and the L
//                         recents (pool_session: one pass, the running max and its tie count), h, x, the loss and its
//                         derivative g, the l2 sum, d_s / d_ds and the slot's 2 + L sort keys:
//                             keys [0, B)          P row u           at position t
//                             keys [B, 2B)         V row n_users + i at position t
//                             keys [2B, 2B + B L)  V row n_users + r at position B + t L + l
//                         a slot that takes no part writes the sentinel key and g = 0
//   loss_kernel           rowkey_common.h: one workgroup, the loss and regulariser sums in a fixed order
//   nrhip_sort_u64        the keys, ascending
//   hrm_rows_kernel       one lane group per sorted key: the head of a run walks it and STORES the row's gradient
//   hrm_factors_kernel    h_u per user from a [U][L] table of last items: pool_session and pool_pre again
//
// Nothing is kept per (slot, recent): no [B][L][d] block exists.  Every float sum is taken in a fixed order and
// nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

// The session row of `L` item ids (entries outside [0, n_items) are skipped), columns c + k DP of one lane: the
// column-wise max with cnt = the number of rows that hold it, or the mean (cnt = the number of rows pooled).  One row
// alone is that row under either rule.  sq adds the rows' squares.  Returns the number of rows pooled; with none
// pooled s is not a row (callers pool the user alone then).
template <int DP, int CPL>
__device__ __forceinline__ int pool_session(const float* __restrict__ V, int d, int n_items,
                                            const int32_t* __restrict__ ids, int L, bool use_max, int c,
                                            float (&s)[CPL], float (&cnt)[CPL], float& sq) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    s[k] = use_max ? -INFINITY : 0.f;
    cnt[k] = 0.f;
  }
  for (int l = 0; l < L; ++l) {
    const int r = ids[l];
    if (r >= 0 && r < n_items) {
      // selects, no branch on the comparison: the running max and the number of rows that hold it
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        const float v = col < d ? V[(int64_t)r * d + col] : 0.f;
        sq += v * v;
        const bool gt = v > s[k], eq = v == s[k];
        const float top = gt ? v : s[k], held = gt ? 1.f : eq ? cnt[k] + 1.f : cnt[k];
        s[k] = use_max ? top : s[k] + v;
        cnt[k] = held;
      }
      ++m;
    }
  }
  if (!use_max && m > 0) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      cnt[k] = (float)m;
      s[k] = s[k] / (float)m;
    }
  }
  return m;
}

// h = pre_agg over {p, s} in one column and the two inputs' shares of its derivative (a tie: one half each)
__device__ __forceinline__ float pool_pre(float p, float s, bool use_max, float& share_p, float& share_s) {
  if (!use_max) {
    share_p = share_s = 0.5f;
    return (p + s) / 2.0f;
  }
  share_p = p > s ? 1.f : p == s ? 0.5f : 0.f;
  share_s = 1.f - share_p;
  return p > s ? p : s;
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void hrm_forward_kernel(nrhip_hrm_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items, L = a.L;
  const bool in = t < B;
  const bool session_max = a.session_max && L > 1, pre_max = a.pre_max != 0;
  int u = -1, i = -1, r_mine = 0;
  if (in) {
    u = a.d_users[t];
    i = a.d_items[t];
    if (c < L) r_mine = a.d_recents[(int64_t)t * L + c];            // L <= 16 <= DP: lane c holds recent c
  }
  // an instance takes part as a whole or not at all: every lookup must be a table row
  const int bad = !in || u < 0 || u >= U || i < 0 || i >= I || (c < L && (r_mine < 0 || r_mine >= I));
  const bool ok = !group_any<DP>(bad);
  float x = 0.f, sq = 0.f;
  float s[CPL], cnt[CPL], vi[CPL], share_s[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) s[k] = cnt[k] = vi[k] = share_s[k] = 0.f;
  if (ok) {
    pool_session<DP, CPL>(a.d_V, d, I, a.d_recents + (int64_t)t * L, L, session_max, c, s, cnt, sq);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col];
        vi[k] = a.d_V[(int64_t)i * d + col];
        float share_p;
        const float h = pool_pre(p, s[k], pre_max, share_p, share_s[k]);
        x += h * vi[k];
        sq += p * p + vi[k] * vi[k];
      }
    }
  }
  group_sum<DP>(x, sq);
  if (!in) return;
  float g = 0.f, loss = 0.f;
  if (ok) {
    pointwise_loss_g(a.loss_kind, B, a.d_labels[t], x, loss, g);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        a.d_s[(int64_t)t * d + col] = s[k];
        a.d_ds[(int64_t)t * d + col] = ((g * vi[k]) * share_s[k]) / cnt[k];
      }
    }
  }
  if (c < L) {
    a.d_keys[2 * (int64_t)B + (int64_t)t * L + c] = ok ? row_key(U + r_mine, (uint32_t)B + (uint32_t)t * L + c) : kSentinel;
    if (ok && a.d_flag_V) a.d_flag_V[r_mine] = 1;
  }
  if (c != 0) return;
  if (ok) {
    if (a.d_flag_P) a.d_flag_P[u] = 1;
    if (a.d_flag_V) a.d_flag_V[i] = 1;
  }
  store_slot(a.d_scal + (int64_t)t * kScal, g, loss, sq, ok);
  a.d_keys[t] = ok ? row_key(u, (uint32_t)t) : kSentinel;
  a.d_keys[(int64_t)B + t] = ok ? row_key(U + i, (uint32_t)t) : kSentinel;
}

// the sum of one run of the sorted keys
template <int DP, int CPL>
__global__ __launch_bounds__(256) void hrm_rows_kernel(nrhip_hrm_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int B = a.batch, d = a.d, U = a.n_users, L = a.L;
  const int64_t n_keys = (int64_t)B * (2 + L);
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  const float reg = a.reg;
  const bool session_max = a.session_max && L > 1, pre_max = a.pre_max != 0;
  const bool is_user = row < U;
  const int r = is_user ? row : row - U;
  const float* table = is_user ? a.d_P : a.d_V;
  float* dst = is_user ? a.d_G_P : a.d_G_V;
  float own[CPL], acc[CPL] = {};
  load_row<DP, CPL>(table, r, d, c, own);
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t pos) {
    if (is_user || pos < (uint32_t)B) {
      // the user's row: its share of g V[i]; the target's row: g h — both from P[u] and the slot's s
      const int t = (int)pos;
      const float g = a.d_scal[(int64_t)t * kScal + S_G];
      const int other = is_user ? a.d_items[t] : a.d_users[t];
      const float* partner = is_user ? a.d_V : a.d_P;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) {
          const float o = partner[(int64_t)other * d + col], s = a.d_s[(int64_t)t * d + col];
          float share_p, share_s;
          const float h = pool_pre(is_user ? own[k] : o, s, pre_max, share_p, share_s);
          acc[k] += (is_user ? (g * o) * share_p : g * h) + reg * own[k];
        }
      }
    } else {
      // a recent: the slot's divided derivative where this row holds the maximum (max), or outright
      const int t = (int)((pos - (uint32_t)B) / (uint32_t)L);
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) {
          const float ds = a.d_ds[(int64_t)t * d + col];
          const bool takes = !session_max || own[k] == a.d_s[(int64_t)t * d + col];
          acc[k] += (takes ? ds : 0.f) + reg * own[k];
        }
      }
    }
  });
  store_row<DP, CPL>(dst, r, d, c, acc);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void hrm_factors_kernel(const float* __restrict__ P, const float* __restrict__ V,
                                                          int n_users, int n_items, int d, int L, int pre_max,
                                                          int session_max, const int32_t* __restrict__ last,
                                                          const int32_t* __restrict__ users, int batch,
                                                          float* __restrict__ out, int64_t ld) {
  const int c = group_lane<DP>(), b = group_index<DP>();
  if (b >= batch) return;
  const int u = users ? users[b] : b;
  float s[CPL], cnt[CPL], sq = 0.f;
  int m = 0;
  const bool known = u >= 0 && u < n_users;
  if (known) m = pool_session<DP, CPL>(V, d, n_items, last + (int64_t)u * L, L, session_max != 0, c, s, cnt, sq);
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) {
      float h = 0.f;
      if (known) {
        const float p = P[(int64_t)u * d + col];
        float share_p, share_s;
        h = m > 0 ? pool_pre(p, s[k], pre_max != 0, share_p, share_s) : p;   // no item: the user alone
      }
      out[(int64_t)b * ld + col] = h;
    }
  }
}

}  // namespace

extern "C" {

int nrhip_hrm_step(const nrhip_hrm_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "hrm_step: null argument block");
  const nrhip_hrm_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_HRM_MAX_D, NR_ERR_UNSUPPORTED, "hrm_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_HRM_MAX_D);
  NR_REQUIRE(a.L >= 1 && a.L <= NRHIP_HRM_MAX_ORDER, NR_ERR_UNSUPPORTED, "hrm_step: high_order %d outside 1..%d", a.L,
             NRHIP_HRM_MAX_ORDER);
  NR_REQUIRE(a.d_P && a.d_V && a.d_G_P && a.d_G_V && a.d_users && a.d_recents && a.d_items && a.d_labels && a.d_keys &&
                 a.d_scal && a.d_s && a.d_ds && a.d_loss2, NR_ERR_ARG, "hrm_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_HRM_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG, "hrm_step: bad sizes");
  NR_TRY(check_loss_kind("hrm_step", 0, a.loss_kind));
  hipStream_t st = (hipStream_t)stream;
  const int B = a.batch;
  const int64_t n_keys = (int64_t)B * (2 + a.L);
  if (B > 0) {
    NR_BY_WIDTH(hrm_forward_kernel, a.d, B, st, a);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
  }
  hipLaunchKernelGGL(loss_kernel<nrhip_hrm_step_args>, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  if (B > 0) {
    NR_BY_WIDTH(hrm_rows_kernel, a.d, n_keys, st, a);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_hrm_user_factors(const float* d_P, const float* d_V, int n_users, int n_items, int d, int L, int pre_max,
                           int session_max, const int32_t* d_last, const int32_t* d_users, int batch, float* d_out,
                           int64_t ld, void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_HRM_MAX_D, NR_ERR_UNSUPPORTED, "hrm_user_factors: embedding_size %d outside 1..%d", d,
             NRHIP_HRM_MAX_D);
  NR_REQUIRE(L >= 1 && L <= NRHIP_HRM_MAX_ORDER, NR_ERR_UNSUPPORTED, "hrm_user_factors: high_order %d outside 1..%d", L,
             NRHIP_HRM_MAX_ORDER);
  NR_REQUIRE(d_P && d_V && d_last && d_out && n_users >= 0 && n_items >= 0 && batch >= 0 && ld >= d &&
                 (d_users || batch <= n_users), NR_ERR_ARG, "hrm_user_factors: bad arguments");
  if (batch == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_BY_WIDTH(hrm_factors_kernel, d, batch, st, d_P, d_V, n_users, n_items, d, L, pre_max, session_max,
                  d_last, d_users, batch, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
