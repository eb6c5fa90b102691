// fossil.hip — Fossil (He & McAuley, ICDM 2016): FISM's long-term term plus a personalised Markov term of order L
// over the same c1 table, its loss and its gradients on gfx950.
//
// Replaces the graph of model/sequential_recommender/Fossil.py:59-102 run on padded [B, Lmax] feeds.  An instance is
// (user u, item i, excluded item e or none, count n, recents r_0..r_{L-1}, most recent first):
//     p = sum_{h in R_u \ {e}} c1[h]     w_l = eta_bias[l] + eta[u, l]     s = sum_l w_l c1[r_l]
//     out = n^-alpha (p . Q[i]) + (s . Q[i]) + bias[i]
//
//   prepare_kernel        history_common.h under FossilRule: n = |R_u| - 1 without the item, |R_u| on the whole
//                         history; a slot takes part only if |R_u| > L and every recent is a train item of its user
//   fossil_forward_kernel (a) one wave per instance: p as FISM pools it (pool_row), then a loop over the L recent rows:
//                         s in fp32 in the order l = 0..L-1, the L dots <c1[r_l], Q[i]>, the rows' square sum
//   loss_kernel           (b) history_common.h under FossilRule: the pair's / instance's eta[u] term on top
//   fossil_rows_kernel    (c) per run of the sorted keys (run_head, history_common.h): a user's run head publishes its
//                         slot and sums G_eta[u, :] in batch order; an item's run head sums G_Q[i] and G_bias[i] in
//                         batch order; one more wave per instance forms g = dout n^-alpha Q[i] + reg_p p
//   fossil_eta_bias_kernel(c) one workgroup: G_eta_bias[l] over the batch in a fixed order, and eta_bias's share of
//                         the regulariser, once per step
//   fossil_walk_kernel    (c) one wave per item h (walk_column_acc, history_common.h): per user of the batch in column
//                         h, per instance in batch order: g unless the instance excluded h, and for every l with
//                         r_l == h the short-term row dout w_l Q[i] (+ reg_q c1[h] once per pointwise instance / pair).
//                         Every recent is a train item of its user, so this walk meets it: no second key set.
//   fossil_factors_kernel (d) [ |R_u|^-alpha p_u + sum_l w_{u,l} c1[last_l(u)] | 1 ] per user
//
// Kept per instance in HBM: p and x = n^-alpha p + s ([N][d] each: the rows kernel re-reads both), g [N][d] (the walk
// re-reads it), the L dots ([N][L]) and 8 scalars.  The recents are read from the batch; neither a padded id matrix nor
// a [B, L, d] block of recent rows exists.  Nothing held in registers grows with L: the kernels loop over it.
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "history_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::hist;

enum { S_SSQ = 5, S_ESQ = 6 };                            // d_scal: the recents' rows' square sum, |eta[u]|^2

__device__ __forceinline__ const int32_t* recents_of(const nrhip_fossil_step_args& a, int b) {
  return a.d_recents + (int64_t)(b >= a.batch ? b - a.batch : b) * a.L;
}

struct FossilRule {
  static constexpr int kCount = -1;
  static constexpr bool kExtraReg = true;
  // |R_u| > L, and every recent of the slot in the user's (ascending) train row
  __device__ static bool takes_part(const nrhip_fossil_step_args& a, int t, int u, int s) {
    if (s <= a.L) return false;
    const int64_t b0 = a.d_indptr[u], e0 = a.d_indptr[u + 1];
    for (int l = 0; l < a.L; ++l) {
      const int r = a.d_recents[(int64_t)t * a.L + l];
      int64_t lo = b0, hi = e0;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.d_indices[mid] < r) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= e0 || a.d_indices[lo] != r) return false;
    }
    return true;
  }
  __device__ static double extra_reg(const nrhip_fossil_step_args& a, const float* sp) {
    return (double)(a.reg_q * (0.5f * sp[S_SSQ])) + (double)(a.reg_eta * (0.5f * sp[S_ESQ]));
  }
};

template <int DP, int CPL>
__global__ __launch_bounds__(256) void fossil_forward_kernel(nrhip_fossil_step_args a, int N) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= N) return;
  float* sc = a.d_scal + (int64_t)b * kScal;
  const int flags = a.d_inst[4 * b + 3];
  if (!(flags & F_VALID)) {
    if (lane < kScal) sc[lane] = 0.f;
    return;
  }
  const int u = a.d_inst[4 * b], item = a.d_inst[4 * b + 1], excl = a.d_inst[4 * b + 2];
  const int d = a.d, L = a.L, grp = lane / DP, c = lane % DP;
  double acc[CPL];
  pool_row<DP, CPL>(a.d_indptr, a.d_indices, a.d_c1, d, u, excl, lane, acc, a.d_flag_c1);
  float q[CPL], s[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = c + j * DP;
    q[j] = col < d ? a.d_Q[(int64_t)item * d + col] : 0.f;
    s[j] = 0.f;
  }
  const int32_t* rec = recents_of(a, b);
  float ssq = 0.f, esq = 0.f;
  for (int l = 0; l < L; ++l) {
    const int r = rec[l];
    const float e = a.d_eta[(int64_t)u * L + l], w = a.d_eta_bias[l] + e;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = c + j * DP;
      const float v = col < d ? a.d_c1[(int64_t)r * d + col] : 0.f;
      s[j] += w * v;
      dot += v * q[j];
      ssq += v * v;
    }
#pragma unroll
    for (int m = DP / 2; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, NR_WAVE);
    esq += e * e;
    if (lane == 0) {
      a.d_dots[(int64_t)b * L + l] = dot;
      if (a.d_flag_c1) a.d_flag_c1[r] = 1;
    }
  }
  const float coeff = count_coeff(a.d_n[b], a.alpha);
  float dp = 0.f, ds = 0.f, psq = 0.f, qsq = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = c + j * DP;
    if (col < d) {
      const float pf = (float)acc[j];
      if (grp == 0) {
        a.d_p[(int64_t)b * d + col] = pf;
        a.d_x[(int64_t)b * d + col] = coeff * pf + s[j];
      }
      dp += pf * q[j];
      ds += s[j] * q[j];
      psq += pf * pf;
      qsq += q[j] * q[j];
    }
  }
#pragma unroll
  for (int m = DP / 2; m >= 1; m >>= 1) {
    dp += __shfl_xor(dp, m, NR_WAVE);
    ds += __shfl_xor(ds, m, NR_WAVE);
    psq += __shfl_xor(psq, m, NR_WAVE);
    qsq += __shfl_xor(qsq, m, NR_WAVE);
    ssq += __shfl_xor(ssq, m, NR_WAVE);
  }
  if (lane == 0) {
    sc[S_OUT] = coeff * dp + ds + a.d_bias[item];
    sc[S_COEFF] = coeff;
    sc[S_RSQ] = psq;
    sc[S_QSQ] = qsq;
    sc[S_SSQ] = ssq;
    sc[S_ESQ] = esq;
  }
}

// waves [0, 2N): the sorted keys; waves [2N, 3N): g of instance w - 2N
template <int CPL>
__global__ __launch_bounds__(256) void fossil_rows_kernel(nrhip_fossil_step_args a, int N) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int d = a.d, L = a.L;
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
  const int head = run_head(a, w, lane);
  if (head < 0) return;
  const uint32_t row = (uint32_t)head;
  if (head < a.n_users) {
    // G_eta[u, l] = sum dout <c1[r_l], Q[i]> over the user's instances in batch order, + reg_eta eta[u, l] once per
    // pointwise instance / pair; lane l takes column l
    const float e = lane < L ? a.d_eta[(int64_t)head * L + lane] : 0.f;
    float ge = 0.f;
    for (int k = w; k < 2 * N; ++k) {
      const uint64_t kk = a.d_keys[k];
      if ((uint32_t)(kk >> 32) != row) break;
      const int b = (int)(uint32_t)kk;
      const float dout = a.d_scal[(int64_t)b * kScal + S_DOUT];
      if (lane < L) {
        ge += dout * a.d_dots[(int64_t)b * L + lane];
        if (a.d_inst[4 * b + 3] & F_REGP) ge += a.reg_eta * e;
      }
    }
    if (lane < L) a.d_G_eta[(int64_t)head * L + lane] = ge;
    if (lane == 0 && a.d_flag_eta) a.d_flag_eta[head] = 1;
    return;
  }
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
    const float dout = a.d_scal[(int64_t)b * kScal + S_DOUT];
    gb += dout;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) acc[j] += dout * a.d_x[(int64_t)b * d + col] + a.reg_q * q[j];
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < d) a.d_G_Q[(int64_t)item * d + col] = acc[j];
  }
  if (lane == 0) a.d_G_bias[item] = gb;
}

// thread (l = tid & 15, part = tid >> 4): instances part, part + 16, ... of column l in fp64, then a fixed tree over
// the 16 parts.  Runs after loss_kernel: thread 0 adds eta_bias's share to the regulariser term.
__global__ __launch_bounds__(256) void fossil_eta_bias_kernel(nrhip_fossil_step_args a, int N) {
  __shared__ double s_g[256];
  const int l = threadIdx.x & 15, part = threadIdx.x >> 4, L = a.L;
  double g = 0.0;
  if (l < L)
    for (int b = part; b < N; b += 16)
      if (a.d_inst[4 * b + 3] & F_VALID)
        g += (double)(a.d_scal[(int64_t)b * kScal + S_DOUT] * a.d_dots[(int64_t)b * L + l]);
  s_g[threadIdx.x] = g;
  __syncthreads();
  for (int s = 128; s >= 16; s >>= 1) {
    if ((int)threadIdx.x < s) s_g[threadIdx.x] += s_g[threadIdx.x + s];
    __syncthreads();
  }
  if ((int)threadIdx.x < L) a.d_G_eta_bias[threadIdx.x] = (float)s_g[threadIdx.x] + a.reg_eta * a.d_eta_bias[threadIdx.x];
  if (threadIdx.x == 0 && a.d_loss2) {
    float sq = 0.f;
    for (int k = 0; k < L; ++k) sq += a.d_eta_bias[k] * a.d_eta_bias[k];
    a.d_loss2[1] += a.reg_eta * (0.5f * sq);
  }
}

template <int CPL>
__global__ __launch_bounds__(256) void fossil_walk_kernel(nrhip_fossil_step_args a, int N) {
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= a.n_items) return;
  const int d = a.d, L = a.L;
  float ch[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    ch[j] = col < d ? a.d_c1[(int64_t)h * d + col] : 0.f;
  }
  walk_column_acc<CPL>(a, N, h, lane, [](int uu) { return (int64_t)uu; },
                       [&](int b, int64_t uu, bool pooled, float (&acc)[CPL]) {
    if (pooled) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int col = lane + j * NR_WAVE;
        if (col < d) acc[j] += a.d_g[(int64_t)b * d + col];
      }
    }
    const int r = lane < L ? recents_of(a, b)[lane] : -1;
    uint64_t hit = __ballot(r == h);
    if (!hit) return;
    const float dout = a.d_scal[(int64_t)b * kScal + S_DOUT];
    const int item = a.d_inst[4 * b + 1];
    const bool reg = a.d_inst[4 * b + 3] & F_REGP;
    while (hit) {                                         // the eta columns at which this instance holds h, ascending
      const int l = __builtin_ctzll(hit);
      hit &= hit - 1;
      const float f = dout * (a.d_eta_bias[l] + a.d_eta[uu * L + l]);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int col = lane + j * NR_WAVE;
        if (col < d) {
          acc[j] += f * a.d_Q[(int64_t)item * d + col];
          if (reg) acc[j] += a.reg_q * ch[j];
        }
      }
    }
  });
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void fossil_factors_kernel(const int64_t* __restrict__ indptr,
                                                             const int32_t* __restrict__ indices, int n_users,
                                                             int n_items, const float* __restrict__ c1,
                                                             const float* __restrict__ eta,
                                                             const float* __restrict__ eta_bias,
                                                             const int32_t* __restrict__ last, int d, int L,
                                                             float alpha, const int32_t* __restrict__ users, int batch,
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
  float s[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) s[j] = 0.f;
  for (int l = 0; l < L; ++l) {
    const int r = last[(int64_t)u * L + l];
    if (r < 0 || r >= n_items) continue;                  // the zero row
    const float w = eta_bias[l] + eta[(int64_t)u * L + l];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = c + j * DP;
      if (col < d) s[j] += w * c1[(int64_t)r * d + col];
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = c + j * DP;
    if (grp == 0 && col < d) row[col] = coeff * (float)acc[j] + s[j];
  }
  if (lane == 0) row[d] = 1.f;
}

}  // namespace

extern "C" {

int nrhip_fossil_step(const nrhip_fossil_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "fossil_step: null argument block");
  const nrhip_fossil_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_FOSSIL_MAX_D, NR_ERR_UNSUPPORTED, "fossil_step: embedding_size %d outside 1..%d",
             a.d, NRHIP_FOSSIL_MAX_D);
  NR_REQUIRE(a.L >= 1 && a.L <= NRHIP_FOSSIL_MAX_ORDER, NR_ERR_UNSUPPORTED, "fossil_step: high_order %d outside 1..%d",
             a.L, NRHIP_FOSSIL_MAX_ORDER);
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_t_indptr && a.d_t_users && a.d_c1 && a.d_Q && a.d_bias && a.d_eta &&
                 a.d_eta_bias && a.d_G_c1 && a.d_G_Q && a.d_G_bias && a.d_G_eta && a.d_G_eta_bias && a.d_users &&
                 a.d_recents && a.d_items && a.d_third && a.d_keys && a.d_inst && a.d_n && a.d_p && a.d_x && a.d_g &&
                 a.d_dots && a.d_scal && a.d_slot, NR_ERR_ARG, "fossil_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_FOSSIL_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 && a.step >= 1 &&
                 (int64_t)a.n_users + a.n_items < ((int64_t)1 << 31), NR_ERR_ARG, "fossil_step: bad sizes");
  if (a.pairwise)
    NR_REQUIRE(a.loss_kind >= nr::NR_PAIR_BPR && a.loss_kind <= nr::NR_PAIR_SQUARE, NR_ERR_ARG,
               "fossil_step: unknown pairwise loss %d (0 bpr, 1 hinge, 2 square)", a.loss_kind);
  else
    NR_REQUIRE(a.loss_kind == nr::NR_POINT_CROSS_ENTROPY || a.loss_kind == nr::NR_POINT_SQUARE, NR_ERR_ARG,
               "fossil_step: unknown pointwise loss %d (0 cross_entropy, 1 square)", a.loss_kind);
  hipStream_t st = (hipStream_t)stream;
  const int N = a.batch * (a.pairwise ? 2 : 1), d = a.d;
  if (N > 0) {
    hipLaunchKernelGGL((prepare_kernel<nrhip_fossil_step_args, FossilRule>), dim3((N + 255) / 256), dim3(256), 0, st, a,
                       N);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, 2 * N, stream));
    NR_BY_WIDTH(fossil_forward_kernel, d, dim3((N + 3) / 4), st, a, N);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((loss_kernel<nrhip_fossil_step_args, FossilRule>), dim3(1), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fossil_eta_bias_kernel, dim3(1), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  if (N > 0) {
    const dim3 grid((3 * N + 3) / 4);
    NR_HIST_BY_CPL(fossil_rows_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  if (a.n_items > 0) {
    const dim3 grid((a.n_items + 3) / 4);
    NR_HIST_BY_CPL(fossil_walk_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_fossil_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, int n_items,
                              const float* d_c1, const float* d_eta, const float* d_eta_bias, const int32_t* d_last,
                              int d, int L, float alpha, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                              void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_FOSSIL_MAX_D, NR_ERR_UNSUPPORTED,
             "fossil_user_factors: embedding_size %d outside 1..%d", d, NRHIP_FOSSIL_MAX_D);
  NR_REQUIRE(L >= 1 && L <= NRHIP_FOSSIL_MAX_ORDER, NR_ERR_UNSUPPORTED,
             "fossil_user_factors: high_order %d outside 1..%d", L, NRHIP_FOSSIL_MAX_ORDER);
  NR_REQUIRE(d_indptr && d_indices && d_c1 && d_eta && d_eta_bias && d_last && d_out && n_users >= 0 && n_items >= 0 &&
                 batch >= 0 && ld >= d + 1 && (d_users || batch <= n_users), NR_ERR_ARG,
             "fossil_user_factors: bad arguments");
  if (batch == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_BY_WIDTH(fossil_factors_kernel, d, dim3((batch + 3) / 4), st, d_indptr, d_indices, n_users, n_items, d_c1,
                     d_eta, d_eta_bias, d_last, d, L, alpha, d_users, batch, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
