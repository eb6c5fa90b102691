// fism.hip — FISM (Kabbur et al., KDD 2013): history pooling, its loss and its gradients on gfx950.
//
// Replaces the graph of model/general_recommender/FISM.py:66-88 run on padded [B, Lmax] feeds.  An instance is
// (user u, item i, excluded item e or none, count n): its history H is the user's train row without e,
//     p = sum_{h in H} c1[h]        out = n^-alpha (p . Q[i]) + bias[i]
// and neither the padded id matrix nor the [B, Lmax, d] gather exist: a wave walks the CSR row.
//
//   prepare_kernel        history_common.h: the batch -> instances and the 2N sort keys
//   fism_forward_kernel   (a) one wave per instance: 64 / DP history rows at a time (DP = lanes per row), fp64
//                         partial sums per lane, combined across the row groups by a fixed xor tree (pool_row,
//                         history_common.h)
//   loss_kernel           (b) history_common.h: dout per instance, the loss and regulariser sums in a fixed order
//   fism_rows_kernel      (c) per run of the sorted keys (item_run_head, history_common.h): a user's run head publishes
//                         its slot; an item's run head sums G_Q[i] and G_bias[i] in batch order; one more wave per
//                         instance forms g = dout n^-alpha Q[i] + reg_p p
//   fism_walk_kernel      (c) one wave per item h (walk_column, history_common.h): the column of the TRANSPOSED train
//                         matrix (users ascending) against the slot map; G_c1[h] = sum over the batch's users of that
//                         column, ascending, over their instances in batch order, of g — except the instances that
//                         excluded h.  Every row of G_c1 is written (TF's gradient of c1 is dense: it is read through
//                         tf.concat).
//   fism_factors_kernel   (d) [n^-alpha p_u | 1] per user: the evaluation's user factors against [Q | bias]
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "history_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::hist;

template <int DP, int CPL>
__global__ __launch_bounds__(256) void fism_forward_kernel(nrhip_fism_step_args a, int N) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= N) return;
  float* sc = a.d_scal + (int64_t)b * kScal;
  const int flags = a.d_inst[4 * b + 3];
  if (!(flags & F_VALID)) {
    if (lane < kScal) sc[lane] = 0.f;
    return;
  }
  const int u = a.d_inst[4 * b], item = a.d_inst[4 * b + 1], excl = a.d_inst[4 * b + 2];
  const int d = a.d, grp = lane / DP, c = lane % DP;
  double acc[CPL];
  pool_row<DP, CPL>(a.d_indptr, a.d_indices, a.d_c1, d, u, excl, lane, acc, a.d_flag_c1);
  float dot = 0.f, psq = 0.f, qsq = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = c + j * DP;
    if (col < d) {
      const float pf = (float)acc[j], q = a.d_Q[(int64_t)item * d + col];
      if (grp == 0) a.d_p[(int64_t)b * d + col] = pf;
      dot += pf * q;
      psq += pf * pf;
      qsq += q * q;
    }
  }
#pragma unroll
  for (int m = DP / 2; m >= 1; m >>= 1) {
    dot += __shfl_xor(dot, m, NR_WAVE);
    psq += __shfl_xor(psq, m, NR_WAVE);
    qsq += __shfl_xor(qsq, m, NR_WAVE);
  }
  if (lane == 0) {
    const float coeff = count_coeff(a.d_n[b], a.alpha);
    sc[S_OUT] = coeff * dot + a.d_bias[item];
    sc[S_COEFF] = coeff;
    sc[S_RSQ] = psq;
    sc[S_QSQ] = qsq;
  }
}

// waves [0, 2N): the sorted keys; waves [2N, 3N): g of instance w - 2N
template <int CPL>
__global__ __launch_bounds__(256) void fism_rows_kernel(nrhip_fism_step_args a, int N) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int d = a.d;
  if (w >= 3 * N) return;
  if (w >= 2 * N) {
    const int b = w - 2 * N;
    const int flags = a.d_inst[4 * b + 3];
    if (!(flags & F_VALID)) return;
    const float* sc = a.d_scal + (int64_t)b * kScal;
    const float f = sc[S_DOUT] * sc[S_COEFF];
    const int item = a.d_inst[4 * b + 1];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) {
        float g = f * a.d_Q[(int64_t)item * d + col];
        if (flags & F_REGP) g += a.reg_p * a.d_p[(int64_t)b * d + col];
        a.d_g[(int64_t)b * d + col] = g;
      }
    }
    return;
  }
  const int head = item_run_head(a, w, lane);
  if (head < 0) return;
  const uint32_t row = (uint32_t)head;
  const int item = head - a.n_users;
  float acc[CPL], q[CPL], gb = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    acc[j] = 0.f;
    q[j] = col < d ? a.d_Q[(int64_t)item * d + col] : 0.f;
  }
  for (int k = w; k < 2 * N; ++k) {
    const uint64_t kk = a.d_keys[k];
    if ((uint32_t)(kk >> 32) != row) break;
    const int b = (int)(uint32_t)kk;
    const float* sc = a.d_scal + (int64_t)b * kScal;
    const float dout = sc[S_DOUT], f = dout * sc[S_COEFF];
    gb += dout;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) acc[j] += f * a.d_p[(int64_t)b * d + col] + a.reg_q * q[j];
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < d) a.d_G_Q[(int64_t)item * d + col] = acc[j];
  }
  if (lane == 0) a.d_G_bias[item] = gb;
}

template <int CPL>
__global__ __launch_bounds__(256) void fism_walk_kernel(nrhip_fism_step_args a, int N) {
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= a.n_items) return;
  walk_column<CPL>(a, N, h, lane, [](int) { return (int64_t)0; },
                   [&](int b, int64_t) { return a.d_g + (int64_t)b * a.d; });
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void fism_factors_kernel(const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int n_users,
                                                           const float* __restrict__ c1, int d, float alpha,
                                                           const int32_t* __restrict__ users, int batch,
                                                           float* __restrict__ out, int64_t ld) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= batch) return;
  const int u = users ? users[b] : b;
  const int grp = lane / DP, c = lane % DP;
  float* row = out + (int64_t)b * ld;
  if (u < 0 || u >= n_users) {                           // no such train row: the score is the bias alone
    for (int col = lane; col < d; col += NR_WAVE) row[col] = 0.f;
    if (lane == 0) row[d] = 1.f;
    return;
  }
  double acc[CPL];
  pool_row<DP, CPL>(indptr, indices, c1, d, u, -1, lane, acc);
  const float coeff = count_coeff((float)(indptr[u + 1] - indptr[u]), alpha);
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = c + j * DP;
    if (grp == 0 && col < d) row[col] = coeff * (float)acc[j];
  }
  if (lane == 0) row[d] = 1.f;
}

}  // namespace

extern "C" {

int nrhip_fism_step(const nrhip_fism_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "fism_step: null argument block");
  const nrhip_fism_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_FISM_MAX_D, NR_ERR_UNSUPPORTED, "fism_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_FISM_MAX_D);
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_t_indptr && a.d_t_users && a.d_c1 && a.d_Q && a.d_bias && a.d_G_c1 &&
                 a.d_G_Q && a.d_G_bias && a.d_users && a.d_items && a.d_third && a.d_keys && a.d_inst && a.d_n &&
                 a.d_p && a.d_g && a.d_scal && a.d_slot, NR_ERR_ARG, "fism_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_FISM_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 && a.step >= 1 &&
                 (int64_t)a.n_users + a.n_items < ((int64_t)1 << 31), NR_ERR_ARG, "fism_step: bad sizes");
  if (a.pairwise)
    NR_REQUIRE(a.loss_kind >= nr::NR_PAIR_BPR && a.loss_kind <= nr::NR_PAIR_SQUARE, NR_ERR_ARG,
               "fism_step: unknown pairwise loss %d (0 bpr, 1 hinge, 2 square)", a.loss_kind);
  else
    NR_REQUIRE(a.loss_kind == nr::NR_POINT_CROSS_ENTROPY || a.loss_kind == nr::NR_POINT_SQUARE, NR_ERR_ARG,
               "fism_step: unknown pointwise loss %d (0 cross_entropy, 1 square)", a.loss_kind);
  hipStream_t st = (hipStream_t)stream;
  const int N = a.batch * (a.pairwise ? 2 : 1), d = a.d;
  if (N > 0) {
    hipLaunchKernelGGL(prepare_kernel<nrhip_fism_step_args>, dim3((N + 255) / 256), dim3(256), 0, st, a, N);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, 2 * N, stream));
    NR_BY_WIDTH(fism_forward_kernel, d, dim3((N + 3) / 4), st, a, N);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(loss_kernel<nrhip_fism_step_args>, dim3(1), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  if (N > 0) {
    const dim3 grid((3 * N + 3) / 4);
    NR_HIST_BY_CPL(fism_rows_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  if (a.n_items > 0) {
    const dim3 grid((a.n_items + 3) / 4);
    NR_HIST_BY_CPL(fism_walk_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_fism_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, const float* d_c1, int d,
                            float alpha, const int32_t* d_users, int batch, float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_FISM_MAX_D, NR_ERR_UNSUPPORTED, "fism_user_factors: embedding_size %d outside 1..%d",
             d, NRHIP_FISM_MAX_D);
  NR_REQUIRE(d_indptr && d_indices && d_c1 && d_out && n_users >= 0 && batch >= 0 && ld >= d + 1 &&
                 (d_users || batch <= n_users), NR_ERR_ARG, "fism_user_factors: bad arguments");
  if (batch == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_BY_WIDTH(fism_factors_kernel, d, dim3((batch + 3) / 4), st, d_indptr, d_indices, n_users, d_c1, d, alpha,
                   d_users, batch, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
