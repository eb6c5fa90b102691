// npe.hip — NPE (Nguyen et al., IJCAI 2018): the step of model/sequential_recommender/NPE.py on gfx950.
//
// An instance is (user u, recents r_0..r_{L-1} oldest first, item i, label y) over three row tables P [U][d],
// V [I][d] (the reference's embeddings_IU) and W [I][d] (embeddings_IL, read only through the recents):
//     s = sum over l of W[r_l]          (summed in l order)                                          NPE.py:59-61
//     q = relu(P[u]) + relu(s)
//     x = sum over c of relu(V[i])_c q_c                                                             NPE.py:62-64
//     loss = pointwise_loss(kind, y, x) + reg l2_loss(P[u], V[i], W[r_.])                            NPE.py:70-71
// All three tables are read through embedding_lookup only: the gradients are sparse and a row's gradient is the sum
// over its occurrences in the batch, taken in the order of its sort keys (row | position).  The rows of the three
// tables share one key space of U + 2 I rows: P row u, V row U + i, W row U + I + r.
//
// The ReLU gates are strict (TF's ReluGrad: features > 0): an input that is exactly 0, or -0, passes nothing.  With
// g = dloss/dx the gradients per column c are
//     P[u]:                     g relu(v_c) [p_c > 0] + reg p_c
//     V[i]:                     g q_c       [v_c > 0] + reg v_c
//     each occurrence of W[r]:  g relu(v_c) [s_c > 0] + reg w_c
// The gate on s is decided ONCE, in the forward kernel, and carried to the rows kernel in two [B][d] buffers: d_s, the
// context sum, and d_ds, the already-gated derivative with respect to s.  A recent occurrence takes its d_ds entry
// outright; the user's and the target's row heads recompute their gate from their own row and the partner's (the
// target's q from P[u] and d_s with the function the forward used, gate_q).
//
//   npe_forward_kernel    one lane group (DP lanes, DP = 16 / 32 / 64 by d) per batch slot: gathers P[u], V[i] and the L
//                         rows of W (context_sum), q, x, the loss and its derivative g, the l2 sum, d_s / d_ds and the
//                         slot's 2 + L sort keys:
//                             keys [0, B)          P row u             at position t
//                             keys [B, 2B)         V row U + i         at position t
//                             keys [2B, 2B + B L)  W row U + I + r_l   at position t L + l
//                         a slot that takes no part writes the sentinel key and g = 0
//   loss_kernel           rowkey_common.h: one workgroup, the loss and regulariser sums in a fixed order, in double
//   nrhip_sort_u64        the keys, ascending
//   npe_rows_kernel       one lane group per sorted key: the head of a run walks it and STORES the row's gradient
//   npe_factors_kernel    h_u = relu(P[u]) + relu(sum of W[last[u][l]]) per user: context_sum and gate_q again
//   npe_relu_kernel       the evaluator's item side, relu(V)
//
// Nothing is kept per (slot, recent): no [B][L][d] block exists.  Every float sum is taken in a fixed order and
// nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

// TF's Relu and the indicator of its ReluGrad: strictly positive inputs pass, 0 and -0 do not
__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }

// The context sum of `L` item ids (entries outside [0, n_items) are skipped), columns c + k DP of one lane, added in
// l order.  sq adds the rows' squares.  Returns the number of rows summed.
template <int DP, int CPL>
__device__ __forceinline__ int context_sum(const float* __restrict__ W, int d, int n_items,
                                           const int32_t* __restrict__ ids, int L, int c, float (&s)[CPL], float& sq) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < CPL; ++k) s[k] = 0.f;
  for (int l = 0; l < L; ++l) {
    const int r = ids[l];
    if (r >= 0 && r < n_items) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        const float w = col < d ? W[(int64_t)r * d + col] : 0.f;
        sq += w * w;
        s[k] += w;
      }
      ++m;
    }
  }
  return m;
}

// q = relu(p) + relu(s) in one column: the user's side of the score
__device__ __forceinline__ float gate_q(float p, float s) { return relu(p) + relu(s); }

template <int DP, int CPL>
__global__ __launch_bounds__(256) void npe_forward_kernel(nrhip_npe_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items, L = a.L;
  const bool in = t < B;
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
  float s[CPL], rv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) s[k] = rv[k] = 0.f;
  if (ok) {
    context_sum<DP, CPL>(a.d_W, d, I, a.d_recents + (int64_t)t * L, L, c, s, sq);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col], v = a.d_V[(int64_t)i * d + col];
        rv[k] = relu(v);
        x += rv[k] * gate_q(p, s[k]);
        sq += p * p + v * v;
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
        a.d_ds[(int64_t)t * d + col] = s[k] > 0.f ? g * rv[k] : 0.f;
      }
    }
  }
  if (c < L) {
    a.d_keys[2 * (int64_t)B + (int64_t)t * L + c] = ok ? row_key(U + I + r_mine, (uint32_t)t * L + c) : kSentinel;
    if (ok && a.d_flag_W) a.d_flag_W[r_mine] = 1;
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
__global__ __launch_bounds__(256) void npe_rows_kernel(nrhip_npe_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items, L = a.L;
  const int64_t n_keys = (int64_t)B * (2 + L);
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  const float reg = a.reg;
  const bool is_user = row < U, is_target = !is_user && row < U + I;
  const int r = is_user ? row : is_target ? row - U : row - U - I;
  const float* table = is_user ? a.d_P : is_target ? a.d_V : a.d_W;
  float* dst = is_user ? a.d_G_P : is_target ? a.d_G_V : a.d_G_W;
  float own[CPL], acc[CPL] = {};
  load_row<DP, CPL>(table, r, d, c, own);
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t pos) {
    if (is_user) {
      // the user's row: g relu(V[i]) where its own entry is positive
      const int t = (int)pos;
      const float g = a.d_scal[(int64_t)t * kScal + S_G];
      const int i = a.d_items[t];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) {
          const float v = a.d_V[(int64_t)i * d + col];
          acc[k] += (own[k] > 0.f ? g * relu(v) : 0.f) + reg * own[k];
        }
      }
    } else if (is_target) {
      // the target's row: g q where its own entry is positive, q from P[u] and the slot's s
      const int t = (int)pos;
      const float g = a.d_scal[(int64_t)t * kScal + S_G];
      const int u = a.d_users[t];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) {
          const float p = a.d_P[(int64_t)u * d + col], s = a.d_s[(int64_t)t * d + col];
          acc[k] += (own[k] > 0.f ? g * gate_q(p, s) : 0.f) + reg * own[k];
        }
      }
    } else {
      // a recent: the slot's gated derivative outright, and the regulariser once per occurrence
      const int t = (int)(pos / (uint32_t)L);
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) acc[k] += a.d_ds[(int64_t)t * d + col] + reg * own[k];
      }
    }
  });
  store_row<DP, CPL>(dst, r, d, c, acc);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void npe_factors_kernel(const float* __restrict__ P, const float* __restrict__ W,
                                                          int n_users, int n_items, int d, int L,
                                                          const int32_t* __restrict__ last,
                                                          const int32_t* __restrict__ users, int batch,
                                                          float* __restrict__ out, int64_t ld) {
  const int c = group_lane<DP>(), b = group_index<DP>();
  if (b >= batch) return;
  const int u = users ? users[b] : b;
  float s[CPL], sq = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) s[k] = 0.f;
  const bool known = u >= 0 && u < n_users;
  if (known) context_sum<DP, CPL>(W, d, n_items, last + (int64_t)u * L, L, c, s, sq);   // no entry: s = 0
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) out[(int64_t)b * ld + col] = known ? gate_q(P[(int64_t)u * d + col], s[k]) : 0.f;
  }
}

__global__ __launch_bounds__(256) void npe_relu_kernel(const float* __restrict__ V, int64_t n, float* __restrict__ out) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) out[k] = relu(V[k]);
}

}  // namespace

extern "C" {

int nrhip_npe_step(const nrhip_npe_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "npe_step: null argument block");
  const nrhip_npe_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_NPE_MAX_D, NR_ERR_UNSUPPORTED, "npe_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_NPE_MAX_D);
  NR_REQUIRE(a.L >= 1 && a.L <= NRHIP_NPE_MAX_ORDER, NR_ERR_UNSUPPORTED, "npe_step: high_order %d outside 1..%d", a.L,
             NRHIP_NPE_MAX_ORDER);
  NR_REQUIRE(a.d_P && a.d_V && a.d_W && a.d_G_P && a.d_G_V && a.d_G_W && a.d_users && a.d_recents && a.d_items &&
                 a.d_labels && a.d_keys && a.d_scal && a.d_s && a.d_ds && a.d_loss2, NR_ERR_ARG,
             "npe_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_NPE_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + 2 * (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG,
             "npe_step: bad sizes (batch 0..%d, n_users + 2 n_items < 2^31 - 1)", NRHIP_NPE_MAX_BATCH);
  NR_TRY(check_loss_kind("npe_step", 0, a.loss_kind));
  hipStream_t st = (hipStream_t)stream;
  const int B = a.batch;
  const int64_t n_keys = (int64_t)B * (2 + a.L);
  if (B > 0) {
    NR_BY_WIDTH(npe_forward_kernel, a.d, B, st, a);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
  }
  hipLaunchKernelGGL(loss_kernel<nrhip_npe_step_args>, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  if (B > 0) {
    NR_BY_WIDTH(npe_rows_kernel, a.d, n_keys, st, a);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_npe_user_factors(const float* d_P, const float* d_W, int n_users, int n_items, int d, int L,
                           const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                           void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_NPE_MAX_D, NR_ERR_UNSUPPORTED, "npe_user_factors: embedding_size %d outside 1..%d", d,
             NRHIP_NPE_MAX_D);
  NR_REQUIRE(L >= 1 && L <= NRHIP_NPE_MAX_ORDER, NR_ERR_UNSUPPORTED, "npe_user_factors: high_order %d outside 1..%d", L,
             NRHIP_NPE_MAX_ORDER);
  NR_REQUIRE(d_P && d_W && d_last && d_out && n_users >= 0 && n_items >= 0 && batch >= 0 && ld >= d &&
                 (d_users || batch <= n_users), NR_ERR_ARG, "npe_user_factors: bad arguments");
  if (batch == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_BY_WIDTH(npe_factors_kernel, d, batch, st, d_P, d_W, n_users, n_items, d, L, d_last, d_users, batch,
                  d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_npe_item_factors(const float* d_V, int n_items, int d, float* d_out, void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_NPE_MAX_D, NR_ERR_UNSUPPORTED, "npe_item_factors: embedding_size %d outside 1..%d", d,
             NRHIP_NPE_MAX_D);
  NR_REQUIRE(d_V && d_out && n_items >= 0, NR_ERR_ARG, "npe_item_factors: bad arguments");
  const int64_t n = (int64_t)n_items * d;
  if (n == 0) return NR_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(npe_relu_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, d_V, n, d_out);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
