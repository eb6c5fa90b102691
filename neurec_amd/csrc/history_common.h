// history_common.h — what the steps of the history models share (fism.hip, nais.hip, fossil.hip): an instance is
// (user u, item i, excluded item e or none, count n) and the user is pooled from the train row without e.
//
//   prepare_kernel   the batch -> instances (pointwise: 1 per slot; pairwise: positive side then negative side) and
//                    the 2N sort keys (user | position) and (n_users + item | position); an instance that takes no
//                    part gets the sentinel key and no F_VALID
//   pool_row         p of one CSR row without the excluded item, fp64 partials combined by a fixed xor tree
//   loss_kernel      one workgroup: dout per instance, the loss and regulariser sums in a fixed order
//   run_head / item_run_head   the rows kernels' opening: a user's run head publishes slot[user] = (step, position),
//                    an item's run head gets its row n_users + item
//   walk_column_acc / walk_column   one wave against a column of the TRANSPOSED train matrix (users ascending) and the
//                    slot map: the batch's users of the column, ascending, their instances in batch order
//
// The kernels are templates over the argument struct: nrhip_fism_step_args, nrhip_nais_step_args and
// nrhip_fossil_step_args name every field read here alike.  A model whose instances differ from FISM's names a Rule
// (PlainRule: FISM's and NAIS's).  Every float sum is taken in a fixed order.  The sentinel, the head test under
// run_head, loss_kernel's tree and the width ladder (NR_BY_WIDTH) are rowkey_common.h's.
#pragma once
#include "rowkey_common.h"

namespace nr {
namespace hist {

using rowkey::kSentinel;                                  // an instance that takes no part sorts behind every key
constexpr int kScal = 8;                                  // floats per instance in d_scal; slots 5..7 are the model's
// S_RSQ: the square sum reg_p multiplies (FISM: |p|^2; NAIS: the history rows' |c1[h]|^2)
enum { S_OUT = 0, S_COEFF = 1, S_RSQ = 2, S_QSQ = 3, S_DOUT = 4 };
enum { F_VALID = 1, F_REGP = 2 };                         // d_inst[4 b + 3]; further bits are the model's

__device__ __forceinline__ double shfl_xor_f64(double x, int m) {
  return __longlong_as_double((long long)nr_shfl_xor_u64((uint64_t)__double_as_longlong(x), m));
}

// What a model may change of the instance rule and of the regulariser (the default: FISM, NAIS).
//   kCount         n = |R_u| + kCount with the item excluded, |R_u| + 1 + kCount on the whole history
//   takes_part     a further test of slot t (user u, a table row, with s train items)
//   kExtraReg / extra_reg   a further regulariser term per pointwise instance / per pair, from its d_scal slots
struct PlainRule {
  static constexpr int kCount = 0;
  static constexpr bool kExtraReg = false;
  template <class Args>
  __device__ static bool takes_part(const Args& a, int, int, int s) { return !a.pairwise || s > 1; }
  template <class Args>
  __device__ static double extra_reg(const Args&, const float*) { return 0.0; }
};

template <class Args, class Rule = PlainRule>
__global__ __launch_bounds__(256) void prepare_kernel(Args a, int N) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= N) return;
  const int side = b / a.batch, t = b - side * a.batch;
  const int u = a.d_users[t];
  int item, excl, flags;
  float n = 0.f;
  bool ok = u >= 0 && u < a.n_users;
  const int s = ok ? (int)(a.d_indptr[u + 1] - a.d_indptr[u]) : 0;
  ok = ok && Rule::takes_part(a, t, u, s);
  if (!a.pairwise) {
    item = a.d_items[t];
    const bool pos = ((const float*)a.d_third)[t] > 0.5f;
    excl = pos ? item : -1;
    n = (float)((pos ? s : s + 1) + Rule::kCount);
    flags = F_REGP;
  } else {
    // a pair takes part as a whole or not at all: both items must be table rows
    const int pos_item = a.d_items[t], neg_item = ((const int32_t*)a.d_third)[t];
    ok = ok && pos_item >= 0 && pos_item < a.n_items && neg_item >= 0 && neg_item < a.n_items;
    item = side == 0 ? pos_item : neg_item;
    excl = side == 0 ? pos_item : -1;
    n = (float)((side == 0 ? s : s + 1) + Rule::kCount);
    flags = side == 0 ? F_REGP : 0;
  }
  ok = ok && item >= 0 && item < a.n_items;
  if (ok) flags |= F_VALID;
  a.d_inst[4 * b + 0] = u;
  a.d_inst[4 * b + 1] = item;
  a.d_inst[4 * b + 2] = excl;
  a.d_inst[4 * b + 3] = flags;
  a.d_n[b] = n;
  a.d_keys[b] = ok ? (((uint64_t)(uint32_t)u << 32) | (uint32_t)b) : kSentinel;
  a.d_keys[N + b] = ok ? (((uint64_t)(uint32_t)(a.n_users + item) << 32) | (uint32_t)b) : kSentinel;
  if (ok && a.d_flag_Q) a.d_flag_Q[item] = 1;
  if (ok && a.d_flag_bias) a.d_flag_bias[item] = 1;
}

__device__ __forceinline__ float count_coeff(float n, float alpha) { return n > 0.f ? powf(n, -alpha) : 0.f; }

// p of one CSR row without `excl`, columns c + j * DP of this lane, in every lane group
template <int DP, int CPL>
__device__ __forceinline__ void pool_row(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                         const float* __restrict__ c1, int d, int u, int excl, int lane,
                                         double (&acc)[CPL], uint8_t* __restrict__ flag = nullptr) {
  constexpr int G = NR_WAVE / DP;
  const int grp = lane / DP, c = lane % DP;
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0.0;
  const int64_t b0 = indptr[u], e0 = indptr[u + 1];
  for (int64_t k = b0 + grp; k < e0; k += G) {
    const int h = indices[k];
    if (h == excl) continue;
    if (flag && c == 0) flag[h] = 1;                      // row application of c1: the rows this batch pooled
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = c + j * DP;
      if (col < d) acc[j] += (double)c1[(int64_t)h * d + col];
    }
  }
#pragma unroll
  for (int m = DP; m < NR_WAVE; m <<= 1) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] += shfl_xor_f64(acc[j], m);
  }
}

template <class Args, class Rule = PlainRule>
__global__ __launch_bounds__(256) void loss_kernel(Args a, int N) {
  const int B = a.batch;
  // tf.losses.sigmoid_cross_entropy is a MEAN over the batch, every other loss of util/learner.py a sum
  const float scale = (!a.pairwise && a.loss_kind == nr::NR_POINT_CROSS_ENTROPY) ? 1.0f / (float)B : 1.0f;
  double v[2] = {0.0, 0.0};
  double &la = v[0], &lb = v[1];
  for (int t = threadIdx.x; t < B; t += 256) {
    float* sp = a.d_scal + (int64_t)t * kScal;
    if (!(a.d_inst[4 * t + 3] & F_VALID)) continue;
    if (!a.pairwise) {
      const float z = ((const float*)a.d_third)[t], x = sp[S_OUT];
      la += (double)(scale * nr::pointwise_loss(a.loss_kind, z, x));
      sp[S_DOUT] = scale * nr::pointwise_dloss(a.loss_kind, z, x);
      lb += (double)(a.reg_p * (0.5f * sp[S_RSQ])) + (double)(a.reg_q * (0.5f * sp[S_QSQ]));
      if constexpr (Rule::kExtraReg) lb += Rule::extra_reg(a, sp);
    } else {
      float* sn = a.d_scal + (int64_t)(B + t) * kScal;
      const float y = sp[S_OUT] - sn[S_OUT];
      la += (double)nr::pairwise_loss(a.loss_kind, y);
      const float dl = nr::pairwise_dloss(a.loss_kind, y);
      sp[S_DOUT] = dl;
      sn[S_DOUT] = -dl;
      lb += (double)(a.reg_p * (0.5f * sp[S_RSQ])) + (double)(a.reg_q * (0.5f * sn[S_QSQ] + 0.5f * sp[S_QSQ]));
      if constexpr (Rule::kExtraReg) lb += Rule::extra_reg(a, sp);
    }
  }
  rowkey::block_sum(v);
  if (threadIdx.x == 0 && a.d_loss2) {
    a.d_loss2[0] = (float)la;
    a.d_loss2[1] = (float)lb;
  }
}

// wave w of the sorted keys: -1 unless it stands on the head of a run, then the run's row (the upper half of its
// keys: a user, or n_users + item).  The head of a user's run publishes the user's slot on the way.
template <class Args>
__device__ __forceinline__ int run_head(const Args& a, int w, int lane) {
  const int row = rowkey::head_row(a.d_keys, w);
  if (row >= 0 && row < a.n_users && lane == 0) a.d_slot[row] = ((int64_t)a.step << 32) | (uint32_t)w;
  return row;
}

// run_head for the heads of the items' runs alone
template <class Args>
__device__ __forceinline__ int item_run_head(const Args& a, int w, int lane) {
  const int row = run_head(a, w, lane);
  return row < a.n_users ? -1 : row;
}

// G_c1[h] = the sum over column h: per user of the batch in it, ascending, `at_user(user)` gives a token (negative:
// the user adds nothing), and per instance b of that user, in batch order, `add(b, token, pooled, acc)` adds what the
// instance gives to acc[j] (column lane + 64 j); pooled: b's history holds h (it did not exclude it)
template <int CPL, class Args, class AtUser, class Add>
__device__ __forceinline__ void walk_column_acc(const Args& a, int N, int h, int lane, AtUser at_user, Add add) {
  const int d = a.d;
  float acc[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
  const int64_t tb = a.d_t_indptr[h], te = a.d_t_indptr[h + 1];
  for (int64_t base = tb; base < te; base += NR_WAVE) {
    const int64_t k = base + lane;
    const int u = k < te ? a.d_t_users[k] : -1;
    const int64_t sl = (u >= 0 && u < a.n_users) ? a.d_slot[u] : 0;
    const bool hit = (int)(sl >> 32) == a.step;
    uint64_t mask = __ballot(hit);
    while (mask) {                                        // the batch's users of this column, ascending
      const int j0 = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int k0 = __shfl((int)(uint32_t)sl, j0, NR_WAVE);
      const int uu = __shfl(u, j0, NR_WAVE);
      const int64_t token = at_user(uu);
      if (token < 0) continue;
      for (int kk = k0; kk < 2 * N; ++kk) {               // that user's instances, in batch order
        const uint64_t key = a.d_keys[kk];
        if ((uint32_t)(key >> 32) != (uint32_t)uu) break;
        const int b = (int)(uint32_t)key;
        add(b, token, a.d_inst[4 * b + 2] != h, acc);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < d) a.d_G_c1[(int64_t)h * d + col] = acc[j];
  }
}

// walk_column_acc where an instance adds one row, and only when it pooled h: `row_of(b, token)` (nullptr: none)
template <int CPL, class Args, class AtUser, class RowOf>
__device__ __forceinline__ void walk_column(const Args& a, int N, int h, int lane, AtUser at_user, RowOf row_of) {
  const int d = a.d;
  walk_column_acc<CPL>(a, N, h, lane, at_user, [&](int b, int64_t token, bool pooled, float (&acc)[CPL]) {
    if (!pooled) return;                                  // this instance pooled without h
    const float* row = row_of(b, token);
    if (!row) return;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) acc[j] += row[col];
    }
  });
}

}  // namespace hist
}  // namespace nr

// KERNEL<1> up to 64 columns (one per lane), KERNEL<2> beyond
#define NR_HIST_BY_CPL(KERNEL, d, grid, st, ...)                                          \
  do {                                                                                    \
    if ((d) <= 64) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, st, __VA_ARGS__);    \
    else hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, st, __VA_ARGS__);              \
  } while (0)
