// nais.hip — NAIS (He et al., TKDE 2018): attention over item histories, its loss, its gradients and predict() on gfx950.
//
// Replaces the graph of model/general_recommender/NAIS.py:96-176 run on padded [B, Lmax] feeds, and the per-user
// sess.run over num_items copies of the history in predict() (NAIS.py:232-258).  An instance is FISM's
// (user u, item i, excluded item e or none, count n = |H| + 1); H is the train row without e, q = Q[i]:
//     x_j = c1[h_j] (.) q  (algorithm 0)  |  [c1[h_j], q]  (algorithm 1)       z_j = x_j W + b      a_j = act(z_j)
//     s_j = a_j . h     e_j = exp(s_j)     S = sum e_j (+ e_pad)     A_j = e_j / S^beta     p = sum A_j c1[h_j]
//     out = n^alpha (p . q) + bias[i]
// e_pad is the reference's padding term (one zero row inside sequence_mask(num_idx) whenever the history is shorter
// than the longest of its side of the batch): exp(h . act(b)) for algorithm 0, exp(h . act(q W[d:2d] + b)) for 1.
// Neither the padded id matrix nor a [B, Lmax, d] block exist: a wave walks the CSR row.
//
//   prepare_kernel         history_common.h (shared with fism.hip): the batch -> instances and the 2N sort keys
//   nais_scan_kernel       one workgroup: the exclusive prefix of the instances' row lengths (the ragged buffer's
//                          offsets) and the longest history of each side
//   nais_forward_kernel    one wave per instance, 64 / WP history rows at a time (WP lanes = the columns of W): ONE pass
//                          gives e_j, S and sum e_j c1[h_j] in fp64 partials, combined by a fixed xor tree
//   loss_kernel            history_common.h: one workgroup, dout per instance, loss and regulariser sums in a fixed order
//   nais_backward_kernel   one wave per instance: the position's terms again, ds_j by the closed form of the softmax's
//                          cross term, the c1 row gradient of every position into the ragged [positions, d] buffer, and
//                          the instance's partials of dW (top d rows), db, dh, dQ[i]
//   nais_rows_kernel       per run of the sorted keys (item_run_head, history_common.h): a user's run head publishes its
//                          slot; an item's run head sums G_Q[i] and G_bias[i] in batch order
//   nais_walk_kernel       one wave per item h (walk_column, history_common.h): the column of the transposed train matrix
//                          against the slot map; G_c1[h] = the ragged buffer's rows of h, users ascending, their
//                          instances in batch order
//   nais_reduce_kernel     dW, db, dh: the instances' partials in batch order (algorithm 1: rows d..2d of dW are
//                          sum_b Q[i_b] (x) db_b)
//   nais_mark / compact / pairs / gather   predict(): the block's distinct history items H*, then per tile of target
//                          items e(i, h) and e(i, h)(c1[h] . Q[i]) for h in H* ONCE (they do not depend on the user),
//                          and per user the sums of both over the user's row — I |H*| d w multiply-adds per block
//                          of users instead of nnz I d w
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "nais_kernels.h"

extern "C" {

int nrhip_nais_step(const nrhip_nais_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "nais_step: null argument block");
  const nrhip_nais_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_NAIS_MAX_D, NR_ERR_UNSUPPORTED, "nais_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_NAIS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_NAIS_MAX_W, NR_ERR_UNSUPPORTED, "nais_step: weight_size %d outside 1..%d", a.w,
             NRHIP_NAIS_MAX_W);
  NR_REQUIRE(a.beta >= 0.f, NR_ERR_ARG, "nais_step: beta %g is negative", (double)a.beta);
  NR_REQUIRE(a.algorithm == 0 || a.algorithm == 1, NR_ERR_ARG, "nais_step: algorithm %d (0 product, 1 concat)",
             a.algorithm);
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_t_indptr && a.d_t_users && a.d_c1 && a.d_Q && a.d_bias && a.d_W &&
                 a.d_b && a.d_h && a.d_G_c1 && a.d_G_Q && a.d_G_bias && a.d_G_W && a.d_G_b && a.d_G_h && a.d_users &&
                 a.d_items && a.d_third && a.d_keys && a.d_inst && a.d_n && a.d_p && a.d_scal && a.d_slot &&
                 a.d_off && a.d_need && a.d_rows && a.d_dWp && a.d_dbp && a.d_dhp && a.d_dqp, NR_ERR_ARG,
             "nais_step: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_NAIS_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 && a.step >= 1 &&
                 a.row_cap >= 0 && a.row_cap < ((int64_t)1 << 31) && (!a.c1_sort || a.d_pkeys) &&
                 (int64_t)a.n_users + a.n_items < ((int64_t)1 << 31), NR_ERR_ARG,
             "nais_step: bad sizes");
  if (a.pairwise)
    NR_REQUIRE(a.loss_kind >= nr::NR_PAIR_BPR && a.loss_kind <= nr::NR_PAIR_SQUARE, NR_ERR_ARG,
               "nais_step: unknown pairwise loss %d (0 bpr, 1 hinge, 2 square)", a.loss_kind);
  else
    NR_REQUIRE(a.loss_kind == nr::NR_POINT_CROSS_ENTROPY || a.loss_kind == nr::NR_POINT_SQUARE, NR_ERR_ARG,
               "nais_step: unknown pointwise loss %d (0 cross_entropy, 1 square)", a.loss_kind);
  hipStream_t st = (hipStream_t)stream;
  const int N = a.batch * (a.pairwise ? 2 : 1), d = a.d;
  if (N > 0) {
    hipLaunchKernelGGL(prepare_kernel<nrhip_nais_step_args>, dim3((N + 255) / 256), dim3(256), 0, st, a, N);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nais_scan_kernel, dim3(1), dim3(256), 0, st, a, N);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, 2 * N, stream));
    NR_NAIS_BY_SHAPE(nais_forward_kernel, dim3((N + 3) / 4), st, a, N);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(loss_kernel<nrhip_nais_step_args>, dim3(1), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  if (a.c1_sort && a.row_cap > 0) {
    hipLaunchKernelGGL(nais_fill_keys_kernel, dim3((unsigned)((a.row_cap + 255) / 256)), dim3(256), 0, st, a);
    NR_LAUNCH_CHECK();
  }
  if (N > 0) {
    NR_NAIS_BY_SHAPE(nais_backward_kernel, dim3((N + 3) / 4), st, a, N);
    NR_LAUNCH_CHECK();
    const dim3 grid((2 * N + 3) / 4);
    NR_HIST_BY_CPL(nais_rows_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  if (a.c1_sort) {
    NR_CHECK_HIP(hipMemsetAsync(a.d_G_c1, 0, sizeof(float) * (size_t)a.n_items * d, st));
    if (a.row_cap > 0) {
      NR_TRY(nrhip_sort_u64(a.d_pkeys, (int)a.row_cap, stream));
      const dim3 grid((unsigned)((a.row_cap + 3) / 4));
      NR_HIST_BY_CPL(nais_segsum_kernel, d, grid, st, a);
      NR_LAUNCH_CHECK();
    }
  } else if (a.n_items > 0) {
    const dim3 grid((a.n_items + 3) / 4);
    NR_HIST_BY_CPL(nais_walk_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  const int entries = (a.algorithm == 1 ? 2 * d : d) * a.w + 2 * a.w;
  hipLaunchKernelGGL(nais_reduce_kernel, dim3((entries + 255) / 256), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_nais_scores(const nrhip_nais_scores_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "nais_scores: null argument block");
  const nrhip_nais_scores_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_NAIS_MAX_D, NR_ERR_UNSUPPORTED, "nais_scores: embedding_size %d outside 1..%d",
             a.d, NRHIP_NAIS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_NAIS_MAX_W, NR_ERR_UNSUPPORTED, "nais_scores: weight_size %d outside 1..%d", a.w,
             NRHIP_NAIS_MAX_W);
  NR_REQUIRE(a.beta >= 0.f && (a.algorithm == 0 || a.algorithm == 1), NR_ERR_ARG, "nais_scores: bad beta / algorithm");
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_c1 && a.d_Q && a.d_bias && a.d_W && a.d_b && a.d_h && a.d_users &&
                 a.d_out && a.d_map && a.d_hs && a.d_cnt && a.d_E && a.d_F && (a.algorithm == 0 || (a.d_cW && a.d_qW)),
             NR_ERR_ARG, "nais_scores: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= 65535 && a.n_users >= 0 && a.n_items >= 0 && a.ld >= a.n_items &&
                 a.h_cap >= 1 && a.tile >= 256 && a.tile % 256 == 0, NR_ERR_ARG, "nais_scores: bad sizes");
  NR_REQUIRE(!a.mfma || (a.algorithm == 0 && a.d <= 16 && a.w <= 16), NR_ERR_UNSUPPORTED,
             "nais_scores: the matrix-core pair kernel takes algorithm 0 with d <= 16 and w <= 16");
  if (a.batch == 0 || a.n_items == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (a.algorithm == 1 && a.project) {
    const int64_t n = (int64_t)a.n_items * a.w;
    hipLaunchKernelGGL(nais_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    NR_LAUNCH_CHECK();
  }
  NR_CHECK_HIP(hipMemsetAsync(a.d_map, 0xff, sizeof(int32_t) * (size_t)a.n_items, st));
  hipLaunchKernelGGL(nais_mark_kernel, dim3((a.batch + 3) / 4), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(nais_compact_kernel, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  const int hmax = a.h_cap < a.n_items ? a.h_cap : a.n_items;
  NR_REQUIRE((hmax + kHC - 1) / kHC <= 65535, NR_ERR_UNSUPPORTED, "nais_scores: %d history items in one block", hmax);
  for (int i0 = 0; i0 < a.n_items; i0 += a.tile) {
    const int ti = a.tile;
    const dim3 grid(ti / 256, (hmax + kHC - 1) / kHC);
    if (a.mfma) hipLaunchKernelGGL(nais_pairs_mfma_kernel, grid, dim3(256), 0, st, a, i0, ti);
    else if (a.d <= 16) launch_pairs_w<16>(a, i0, ti, grid, st);
    else if (a.d <= 32) launch_pairs_w<32>(a, i0, ti, grid, st);
    else if (a.d <= 64) launch_pairs_w<64>(a, i0, ti, grid, st);
    else launch_pairs_w<128>(a, i0, ti, grid, st);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nais_gather_kernel, dim3(ti / 256, a.batch), dim3(256), 0, st, a, i0, ti);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

}  // extern "C"
