// fpmc.hip — FPMC (Rendle et al., WWW 2010): the step of model/sequential_recommender/FPMC.py on gfx950.
//
// An instance is (user u, recent item l, item i[, negative j]) and its score
//     x(u, l, i) = <UI[u], IU[i]> + <IL[i], LI[l]>
// Four row tables, every one read through embedding_lookup: the gradients are sparse, a row's gradient is the sum over
// its occurrences in the batch, and TF adds them in the order of the concatenated lookups.  That order is the
// contract of nrhip_bpr_plan: row, then position in the batch, the first inference's lookups (positions 0..B) before
// the second's (B..2B).
//
//   fpmc_forward_kernel   one lane group (DP lanes, DP = 16 / 32 / 64 by d) per batch slot: gathers the rows, the
//                         score(s), the loss and its derivative g, the l2 sum, and the 3 N sort keys
//                         (row | position) of the slot's lookups — N = B (pointwise) or 2 B (pairwise):
//                             keys [0, N)     UI row u                      at positions t and B + t
//                             keys [N, 2N)    IU / IL row n_users + i | j   (one run serves both tables: same index)
//                             keys [2N, 3N)   LI row n_users + n_items + l  at positions t and B + t
//                         a slot that takes no part writes the sentinel key and g = 0
//   loss_kernel           rowkey_common.h: one workgroup, the loss and regulariser sums in a fixed order
//   nrhip_sort_u64        the keys, ascending
//   fpmc_rows_kernel      one lane group per sorted key: the head of a run walks it and STORES the row's gradient,
//                         every occurrence recomputed from the gathered rows: g * partner row + reg * own row
//                         (UI and LI through the negative's score: -g * partner row alone)
//   fpmc_factors_kernel   [UI[u] | LI[last(u)]] per user: the evaluation's user factors against [IU | IL]
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

template <int DP, int CPL>
__global__ __launch_bounds__(256) void fpmc_forward_kernel(nrhip_fpmc_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items;
  const int N = a.pairwise ? 2 * B : B;
  const bool in = t < B;
  int u = -1, l = -1, i = -1, j = -1;
  if (in) {
    u = a.d_users[t];
    l = a.d_recent[t];
    i = a.d_items[t];
    if (a.pairwise) j = ((const int32_t*)a.d_third)[t];
  }
  // an instance takes part as a whole or not at all: every lookup must be a table row
  const bool ok = in && u >= 0 && u < U && l >= 0 && l < I && i >= 0 && i < I && (!a.pairwise || (j >= 0 && j < I));
  float xi = 0.f, xj = 0.f, sq = 0.f;
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float ui = a.d_UI[(int64_t)u * d + col], li = a.d_LI[(int64_t)l * d + col];
        const float iu = a.d_IU[(int64_t)i * d + col], il = a.d_IL[(int64_t)i * d + col];
        xi += ui * iu + il * li;
        sq += ui * ui + iu * iu + il * il + li * li;
        if (a.pairwise) {
          const float ju = a.d_IU[(int64_t)j * d + col], jl = a.d_IL[(int64_t)j * d + col];
          xj += ui * ju + jl * li;
          sq += ju * ju + jl * jl;
        }
      }
    }
  }
  // group_sum's tree in the kernel's own text: through the helper the compiler issues the loads of d_third and of the
  // flag pointers behind the tree instead of ahead of it, and the step measured 0.2 us slower
#pragma unroll
  for (int m = DP / 2; m >= 1; m >>= 1) {
    xi += __shfl_xor(xi, m, NR_WAVE);
    xj += __shfl_xor(xj, m, NR_WAVE);
    sq += __shfl_xor(sq, m, NR_WAVE);
  }
  if (!in || c != 0) return;
  float g = 0.f, loss = 0.f;
  if (ok) {
    instance_loss_g(a.pairwise, a.loss_kind, B, a.d_third, t, xi, xj, loss, g);
    if (a.d_flag_UI) a.d_flag_UI[u] = 1;
    if (a.d_flag_LI) a.d_flag_LI[l] = 1;
    if (a.d_flag_IU) a.d_flag_IU[i] = 1;
    if (a.d_flag_IL) a.d_flag_IL[i] = 1;
    if (a.pairwise) {
      if (a.d_flag_IU) a.d_flag_IU[j] = 1;
      if (a.d_flag_IL) a.d_flag_IL[j] = 1;
    }
  }
  store_slot(a.d_scal + (int64_t)t * kScal, g, loss, sq, ok);
  a.d_keys[t] = ok ? row_key(u, t) : kSentinel;
  a.d_keys[N + t] = ok ? row_key(U + i, t) : kSentinel;
  a.d_keys[2 * (int64_t)N + t] = ok ? row_key(U + I + l, t) : kSentinel;
  if (a.pairwise) {
    a.d_keys[B + t] = ok ? row_key(u, B + t) : kSentinel;
    a.d_keys[N + B + t] = ok ? row_key(U + j, B + t) : kSentinel;
    a.d_keys[2 * (int64_t)N + B + t] = ok ? row_key(U + I + l, B + t) : kSentinel;
  }
}

// the sum of one run of the sorted keys: own row `own` of the table, per occurrence g * partner row (+ reg * own row)
template <int DP, int CPL>
__global__ __launch_bounds__(256) void fpmc_rows_kernel(nrhip_fpmc_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items;
  const int64_t n_keys = 3 * (int64_t)(a.pairwise ? 2 * B : B);
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  const float reg = a.reg;
  const int32_t* negs = (const int32_t*)a.d_third;
  if (row >= U && row < U + I) {
    // an item as the target of an inference: its IU row against UI[u], its IL row against LI[l]
    const int item = row - U;
    float own_u[CPL], own_l[CPL], acc_u[CPL] = {}, acc_l[CPL] = {};
#pragma unroll
    for (int k = 0; k < CPL; ++k) {                        // both rows in one pass: two load_row calls wait in turn
      const int col = c + k * DP;
      own_u[k] = col < d ? a.d_IU[(int64_t)item * d + col] : 0.f;
      own_l[k] = col < d ? a.d_IL[(int64_t)item * d + col] : 0.f;
    }
    for_run(a.d_keys, n_keys, w, row, [&](uint32_t low) {
      const int pos = (int)low;
      const int t = pos >= B ? pos - B : pos;
      const float g0 = a.d_scal[(int64_t)t * kScal + S_G], g = pos >= B ? -g0 : g0;
      const int u = a.d_users[t], l = a.d_recent[t];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) {
          acc_u[k] += g * a.d_UI[(int64_t)u * d + col] + reg * own_u[k];
          acc_l[k] += g * a.d_LI[(int64_t)l * d + col] + reg * own_l[k];
        }
      }
    });
    store_row<DP, CPL>(a.d_G_IU, item, d, c, acc_u);
    store_row<DP, CPL>(a.d_G_IL, item, d, c, acc_l);
    return;
  }
  // a user's UI row against IU[item], or a recent item's LI row against IL[item]; the lookup of the second
  // inference carries the gradient through the negative's score and no regulariser term
  const bool is_user = row < U;
  const int r = is_user ? row : row - U - I;
  const float* table = is_user ? a.d_UI : a.d_LI;
  const float* partner = is_user ? a.d_IU : a.d_IL;
  float* dst = is_user ? a.d_G_UI : a.d_G_LI;
  float own[CPL], acc[CPL] = {};
  load_row<DP, CPL>(table, r, d, c, own);
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t low) {
    const int pos = (int)low;
    const bool second = pos >= B;
    const int t = second ? pos - B : pos;
    const float g0 = a.d_scal[(int64_t)t * kScal + S_G];
    const int item = second ? negs[t] : a.d_items[t];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = partner[(int64_t)item * d + col];
        acc[k] += second ? -g0 * p : g0 * p + reg * own[k];
      }
    }
  });
  store_row<DP, CPL>(dst, r, d, c, acc);
}

__global__ __launch_bounds__(256) void fpmc_factors_kernel(const float* __restrict__ UI, const float* __restrict__ LI,
                                                           int n_users, int n_items, int d,
                                                           const int32_t* __restrict__ last,
                                                           const int32_t* __restrict__ users, int batch,
                                                           float* __restrict__ out, int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * 2 * d) return;
  const int b = (int)(idx / (2 * d)), col = (int)(idx - (int64_t)b * 2 * d);
  const int u = users ? users[b] : b;
  float v = 0.f;
  if (u >= 0 && u < n_users) {
    if (col < d) {
      v = UI[(int64_t)u * d + col];
    } else {
      const int l = last[u];
      if (l >= 0 && l < n_items) v = LI[(int64_t)l * d + col - d];
    }
  }
  out[(int64_t)b * ld + col] = v;
}

}  // namespace

extern "C" {

int nrhip_fpmc_step(const nrhip_fpmc_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "fpmc_step: null argument block");
  const nrhip_fpmc_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_FPMC_MAX_D, NR_ERR_UNSUPPORTED, "fpmc_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_FPMC_MAX_D);
  NR_REQUIRE(a.d_UI && a.d_IU && a.d_IL && a.d_LI && a.d_G_UI && a.d_G_IU && a.d_G_IL && a.d_G_LI && a.d_users &&
                 a.d_recent && a.d_items && a.d_third && a.d_keys && a.d_scal && a.d_loss2, NR_ERR_ARG,
             "fpmc_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_FPMC_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + 2 * (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG, "fpmc_step: bad sizes");
  NR_TRY(check_loss_kind("fpmc_step", a.pairwise, a.loss_kind));
  hipStream_t st = (hipStream_t)stream;
  const int B = a.batch, n_keys = 3 * B * (a.pairwise ? 2 : 1);
  if (B > 0) {
    NR_BY_WIDTH(fpmc_forward_kernel, a.d, B, st, a);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, n_keys, stream));
  }
  hipLaunchKernelGGL(loss_kernel<nrhip_fpmc_step_args>, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  if (B > 0) {
    NR_BY_WIDTH(fpmc_rows_kernel, a.d, n_keys, st, a);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_fpmc_user_factors(const float* d_UI, const float* d_LI, int n_users, int n_items, int d,
                            const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                            void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_FPMC_MAX_D, NR_ERR_UNSUPPORTED, "fpmc_user_factors: embedding_size %d outside 1..%d",
             d, NRHIP_FPMC_MAX_D);
  NR_REQUIRE(d_UI && d_LI && d_last && d_out && n_users >= 0 && n_items >= 0 && batch >= 0 && ld >= 2 * d &&
                 (d_users || batch <= n_users), NR_ERR_ARG, "fpmc_user_factors: bad arguments");
  if (batch == 0) return NR_OK;
  const int64_t n = (int64_t)batch * 2 * d;
  hipLaunchKernelGGL(fpmc_factors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_UI,
                     d_LI, n_users, n_items, d, d_last, d_users, batch, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
