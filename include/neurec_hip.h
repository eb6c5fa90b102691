/* neurec_hip.h — C ABI of libneurec_hip.so, the MI355X (gfx950) engine for the
 * NeuRec embedding hot path.
 *
 * Conventions
 *   - Every pointer named d_* is a DEVICE pointer owned by the caller (e.g. a
 *     PyTorch-ROCm tensor's data_ptr()).  The library never allocates or frees
 *     caller-visible memory; scratch space is passed in as an explicit
 *     workspace whose size comes from the matching *_workspace_bytes query.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *     and the call returns without synchronising.
 *   - Return value: 0 on success, otherwise one of NRHIP_ERR_*; a message is
 *     available from nrhip_last_error() (thread-local).
 *   - int = 32 bit, float = IEEE fp32, exactly as the reference asserts at
 *     import (util/cython/tools.pyx:7-27).
 *   - Item/user id arrays are int32, CSR index pointers are int64 where the
 *     number of interactions may exceed 2^31 (training CSR, adjacency) and
 *     int32 otherwise.
 *
 * Each entry point names the reference interface it stands in for
 * (paths relative to the NeuRec tree, wubinzzu/NeuRec @ v1).
 */
#ifndef NEUREC_HIP_H
#define NEUREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRHIP_OK 0
#define NRHIP_ERR_ARG 1
#define NRHIP_ERR_UNSUPPORTED 2
#define NRHIP_ERR_HIP 3
#define NRHIP_ERR_WORKSPACE 4

#define NRHIP_ABI_VERSION 4
#define NRHIP_MAX_TOPK 128 /* largest top_k the selection kernels accept */

/* ---- library ------------------------------------------------------------ */
int nrhip_abi_version(void);
const char* nrhip_last_error(void);
/* device facts used by bench/roofline reporting */
int nrhip_device_info(int* cu_count, int* clock_khz, size_t* hbm_bytes, char* name, int name_len);

/* ---- evaluator ----------------------------------------------------------
 * Replaces: cpp_evaluate_matrix / eval_one_user
 *           (evaluator/backend/cpp/include/evaluate.h:23-72),
 *           metric functions (evaluator/backend/cpp/include/metric.h:17-117),
 *           the -inf train mask loop (evaluator/backend/cpp/uni_evaluator.py:140-143),
 *           arg_top_k_2d (util/cython/include/arg_topk.h:15-45).
 */

/* Scratch needed by nrhip_eval_scores / nrhip_arg_topk for `rows` rows. */
int nrhip_eval_workspace_bytes(int rows, int top_k, size_t* bytes);

/* scores[r][train items of users[r]] = -inf, in place
 * (uni_evaluator.py:140-143).  tr_indptr has one entry per user id + 1. */
int nrhip_mask_train(float* d_scores, int64_t ld, const int32_t* d_users, int rows, int cols,
                     const int64_t* d_tr_indptr, const int32_t* d_tr_indices, void* stream);

/* Per row: rank the `cols` scores exactly like eval_one_user (partial sort of
 * min(2*top_k, cols) indices by descending score, cut to top_k, libstdc++ tie
 * behaviour included), then write n_metric*top_k cumulative metric values,
 * metric-major (evaluate.h:43-47).  Truth of row r is the ascending id list
 * d_truth_indices[d_truth_indptr[t] .. d_truth_indptr[t+1]) with
 * t = d_users ? d_users[r] : r.  metric ids: 1 Precision 2 Recall 3 MAP
 * 4 NDCG 5 MRR (metric.h:111-117).  d_topk_out (optional, may be NULL)
 * receives the top_k ranked item ids per row.  d_n_exact (optional) receives
 * the number of rows that needed the exact tie path. */
int nrhip_eval_scores(const float* d_scores, int64_t ld, int rows, int cols,
                      const int32_t* d_users, const int64_t* d_truth_indptr,
                      const int32_t* d_truth_indices, const int32_t* metric_ids_host,
                      int n_metric, int top_k, float* d_out, int32_t* d_topk_out,
                      int32_t* d_n_exact, void* d_ws, size_t ws_bytes, void* stream);

/* nrhip_eval_scores without the top_k <= 128 limit (cpp_evaluate_matrix / eval_one_user take any K:
 * evaluator/backend/cpp/include/evaluate.h:23-50): one thread per row replays std::partial_sort_copy and the metric
 * loops sequentially.  Same arguments, same output layout; its own workspace query. */
int nrhip_eval_any_k_workspace_bytes(int rows, int cols, int top_k, size_t* bytes);
int nrhip_eval_scores_any_k(const float* d_scores, int64_t ld, int rows, int cols, const int32_t* d_users,
                            const int64_t* d_truth_indptr, const int32_t* d_truth_indices,
                            const int32_t* metric_ids_host, int n_metric, int top_k, float* d_out,
                            int32_t* d_topk_out, void* d_ws, size_t ws_bytes, void* stream);

/* Per row arg-top-K with std::partial_sort_copy(K) semantics
 * (arg_topk.h:15-25): d_out[rows][top_k] int32. */
int nrhip_arg_topk(const float* d_scores, int64_t ld, int rows, int cols, int top_k,
                   int32_t* d_out, int32_t* d_n_exact, void* d_ws, size_t ws_bytes,
                   void* stream);

/* Column sums of a [rows][cols] fp32 matrix in fp64 (the np.mean of
 * uni_evaluator.py:150-151 is sum/rows; the division is the caller's). */
int nrhip_colsum_workspace_bytes(int rows, int cols, size_t* bytes);
int nrhip_colsum_f64(const float* d_mat, int64_t ld, int rows, int cols, double* d_out,
                     void* d_ws, size_t ws_bytes, void* stream);

/* Scoring GEMM: S[r][i] = sum_k P[users[r]][k] * Q[i][k], fp32 MFMA, k
 * ascending fused-multiply-add chain.  Replaces np.matmul(user_embed,
 * item_embeddings.T) (model/general_recommender/MF.py:120-122) and the TF
 * matmul of LightGCN.py:118-119.  d_users may be NULL (rows 0..rows-1).
 * S has leading dimension lds >= cols; columns [cols, lds_pad) may be
 * written with zeros where lds_pad = min(lds, roundup(cols,64)). */
int nrhip_score_gemm_workspace_bytes(int rows, int cols, int d, size_t* bytes);
/* Prepare the item side once per evaluation (k-major copy of Q inside ws). */
int nrhip_score_gemm_prepare_items(const float* d_Q, int64_t ldq, int cols, int d, void* d_ws,
                                   size_t ws_bytes, void* stream);
int nrhip_score_gemm(const float* d_P, int64_t ldp, const int32_t* d_users, int rows, int cols,
                     int d, float* d_S, int64_t lds, void* d_ws, size_t ws_bytes, void* stream);

/* ---- pruned full-rank evaluation (no score matrix) --------------------------------
 * Same results as nrhip_score_gemm + nrhip_mask_train + nrhip_eval_scores
 * (uni_evaluator.py:132-151 -> evaluate.h:23-72) without materialising the [rows][cols] scores:
 *   level 1  nrhip_score_tilemax: the scoring loop keeps, per user, only the maximum admissible
 *            score of every 32-item tile (train items and pad columns struck out in registers):
 *            d_M[rows][mld], mld even and >= 2*ceil(cols/64) (32-item tiles).  Item side prepared as
 *            for nrhip_score_gemm.
 *   level 2  nrhip_eval_tiles: the top_k+1 best items of a user lie in the top_k+1 tiles with the
 *            largest maxima; those tiles are rescored (same k-ascending fmaf chain, bit-identical),
 *            ranked and measured.  d_flag_out[r] = 1 marks rows whose ranking may depend on ties
 *            (inside the kept set, or between the two boundary tile maxima): their rows of d_out
 *            are provisional — recompute them through the full score path.
 * Needs 2*ceil(cols/64) >= top_k + 2 and top_k <= 62. */
int nrhip_score_tilemax(const float* d_P, int64_t ldp, const int32_t* d_users, int rows, int cols,
                        int d, const int64_t* d_tr_indptr, const int32_t* d_tr_indices,
                        float* d_M, int64_t mld, void* d_ws, size_t ws_bytes, void* stream);
/* Level 1 in two launches (the faster form): nrhip_score_tilemax with d_tr_indptr = d_tr_indices = NULL leaves the
 * train items IN the maxima (the scoring loop carries no cursors and no strike code), and nrhip_score_tilemax_fix
 * recomputes — same MFMA chain, same operand roles, bit-identical values — only the (user, tile) pairs that hold a
 * train item, from a plan built once per train matrix: pairs sorted by 32-item tile (d_tile_ptr[n_tiles32 + 1],
 * d_plan_user[e], d_plan_mask[e]: bit r = item 32*tile + r is a train item of that user), cut into chunks of <= 32
 * pairs of one tile (d_chunk_tile[c], d_chunk_begin[c]).  d_row_of[user] = the user's row in the evaluation order
 * (-1: not evaluated; NULL: row = user); M holds rows [row_lo, row_lo + rows).  Afterwards M equals the one-launch
 * form's, bit for bit (uni_evaluator.py:132-140: ranking_score[train items] = -inf, as a property of the maxima). */
int nrhip_score_tilemax_fix(const float* d_P, int64_t ldp, int d, int cols, const int32_t* d_chunk_tile,
                            const int64_t* d_chunk_begin, int n_chunks, const int64_t* d_tile_ptr,
                            const int32_t* d_plan_user, const uint32_t* d_plan_mask, const int32_t* d_row_of,
                            int row_lo, int rows, float* d_M, int64_t mld, const void* d_ws, size_t ws_bytes,
                            void* stream);

/* The strike plan itself, built on the device (r05: was construction-time torch code): pairs (user, 32-item tile) that
 * hold a train item of the user — uni_evaluator.py:132-140 strikes those items of every batch on the host — grouped by
 * tile, chunks of <= 32 pairs.  Capacities: d_plan_user / d_plan_mask nnz entries; d_tile_ptr n_tiles + 1 with
 * n_tiles = 2 * ceil(cols / 64); d_chunk_tile / d_chunk_begin nnz / 32 + n_tiles + 1; d_counts[2] = {pairs, chunks};
 * d_ws 8 * n_tiles bytes.  The order of the pairs inside a tile is unspecified (each pair is independent). */
int nrhip_tile_strike_plan(const int64_t* d_indptr, const int32_t* d_indices, int n_users, int cols,
                           int32_t* d_plan_user, uint32_t* d_plan_mask, int64_t* d_tile_ptr, int32_t* d_chunk_tile,
                           int64_t* d_chunk_begin, int32_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);
/* Level 1 as a bounded filter on the bf16 matrix cores (csrc/score_bf16.hip; d <= 128).  The fp32 chain stays the
 * definition of every score that is ranked: this only SEARCHES for the tiles worth rescoring, 4-5x faster than the
 * fp32 MFMA loop.  x = hi + lo + r with hi, lo bf16 (round to nearest even), u.i ~= sum_k uh*ih + uh*il + ul*ih in
 * fp32 accumulators, and |approx - chain| <= kappa(d) * ||u|| * max_i ||i|| = d_eps[row] (kappa: nrhip_score_filter_kappa;
 * the derivation stands at the top of score_bf16.hip).  nrhip_score_filter_prepare_items splits the item table once
 * per evaluation (it replaces np.matmul's operand, MF.py:120-122); nrhip_score_filter_tilemax fills d_M like
 * nrhip_score_tilemax without train lists (nrhip_score_tilemax_fix must follow: it writes exact fp32 maxima, error 0)
 * and d_eps[rows].  nrhip_eval_tiles_bounded then certifies each row against its bound or flags it. */
int nrhip_score_filter_workspace_bytes(int rows, int cols, int d, size_t* bytes);
int nrhip_score_filter_kappa(int d, float* kappa);
int nrhip_score_filter_prepare_items(const float* d_Q, int64_t ldq, int cols, int d, void* d_ws, size_t ws_bytes,
                                     int max_rows, void* stream);
int nrhip_score_filter_tilemax(const float* d_P, int64_t ldp, const int32_t* d_users, int rows, int cols, int d,
                               float* d_M, int64_t mld, float* d_eps, void* d_ws, size_t ws_bytes, int max_rows,
                               void* stream);
/* The same bounded filter on the int8 matrix cores (csrc/score_i8.hip; d <= 128): 15-bit fixed point — one scale per
 * user row, one for the whole item table, two int8 planes per entry, three v_mfma_i32_32x32x32_i8 products in exact
 * integer accumulators, the tile maximum taken on the integers.  Same outputs as nrhip_score_filter_tilemax, with a
 * ONE-SIDED contract (what nrhip_eval_tiles_bounded's certificate needs): d_M[r][t] is an upper-bound maximum — the
 * approximate maximum plus the tile's own share of the quantisation error, 0.525*su*sI*max_{i in t} sum|qi| — and
 * fp32 chain maximum of tile t <= d_M[r][t] + d_eps[r],   d_M[r][t] - that maximum <= d_eps[r] + 2 x the tile's share,
 * with d_eps[r] = su*sI*[0.525*sum|qu| + 0.27*d + 64*sum|lu|] + the chain's own rounding, DERIVED from the
 * quantisation (top of score_i8.hip) — no model of the matrix pipe is assumed.  d_eps[r] = NaN for rows (or item
 * tables) whose largest magnitude lies outside [2^-40, 2^40] or is not finite: every certificate fails for them and
 * the caller's fp32 path takes the row.  It replaces the same reference lines (np.matmul's operand, MF.py:120-122;
 * LightGCN.py:187-189). */
int nrhip_score_filter_i8_workspace_bytes(int rows, int cols, int d, size_t* bytes);
int nrhip_score_filter_i8_prepare_items(const float* d_Q, int64_t ldq, int cols, int d, void* d_ws, size_t ws_bytes,
                                        int max_rows, void* stream);
int nrhip_score_filter_i8_tilemax(const float* d_P, int64_t ldp, const int32_t* d_users, int rows, int cols, int d,
                                  float* d_M, int64_t mld, float* d_eps, void* d_ws, size_t ws_bytes, int max_rows,
                                  void* stream);
int nrhip_eval_tiles_workspace_bytes(int rows, int top_k, size_t* bytes);
/* d_gemm_ws: the workspace nrhip_score_gemm_prepare_items filled (the rescoring reads its k-major
 * item copy, one coalesced 256-byte load per k and tile). */
int nrhip_score_gemm_items_kmajor(const void* d_ws, int cols, int d, const float** qt, int* ipad);
int nrhip_eval_tiles(const float* d_M, int64_t mld, const float* d_P, int64_t ldp,
                     const void* d_gemm_ws, int d, const int32_t* d_users, int rows, int cols,
                     const int64_t* d_tr_indptr, const int32_t* d_tr_indices,
                     const int64_t* d_truth_indptr, const int32_t* d_truth_indices,
                     const int32_t* metric_ids_host, int n_metric, int top_k, float* d_out,
                     int32_t* d_flag_out, void* d_ws, size_t ws_bytes, void* stream);
/* Level 2 for BOUNDED maxima (nrhip_score_filter_tilemax, then nrhip_score_tilemax_fix): the n_keep best tiles
 * (top_k + 1 <= n_keep <= 63) are rescored with the fp32 chain and ranked as in nrhip_eval_tiles; a row stands when its
 * top_k-th rescored score exceeds the largest maximum among the tiles NOT rescored by more than d_eps[row] — no item
 * outside the rescored tiles can then reach or tie the kept set in the fp32 chain — otherwise d_flag_out[row] = 1 and
 * the caller recomputes the row from a full fp32 score row (as for ties).  evaluate.h:23-50 stays the definition.
 * d_eps = NULL: the maxima are exact (nrhip_score_tilemax), n_keep = top_k + 1, nrhip_eval_tiles' rule.  The rescoring
 * runs grouped by tile (32 users of one tile per wave on the fp32 matrix cores: the item tile is read once per 32
 * users, not once per user) where the shape allows; same scores bit for bit. */
int nrhip_eval_tiles_bounded_workspace_bytes(int rows, int cols, int top_k, int n_keep, size_t* bytes);
int nrhip_eval_tiles_bounded(const float* d_M, int64_t mld, const float* d_eps, int n_keep, const float* d_P,
                             int64_t ldp, const void* d_gemm_ws, int d, const int32_t* d_users, int rows, int cols,
                             const int64_t* d_tr_indptr, const int32_t* d_tr_indices,
                             const int64_t* d_truth_indptr, const int32_t* d_truth_indices,
                             const int32_t* metric_ids_host, int n_metric, int top_k, float* d_out,
                             int32_t* d_flag_out, void* d_ws, size_t ws_bytes, void* stream);

/* The pruned evaluation of a whole user list as one call: the batch loop of UniEvaluator.evaluate
 * (evaluator/backend/cpp/uni_evaluator.py:101-157) over nrhip_score_filter_tilemax / nrhip_score_filter_i8_tilemax
 * (use_filter = 1 / 2) or nrhip_score_tilemax,
 * nrhip_score_tilemax_fix and nrhip_eval_tiles_bounded, then (d_sums != NULL) the fp64 column sums of d_out and the
 * number of flagged rows in d_sums[n_metric*top_k] (and, behind it, how many of them failed their certificate: flag
 * bit 1; bit 0 = ties / bucket overflow) — one device->host copy brings the means and says whether any row
 * must be redone.  Pointers are device pointers except metric_ids (host). */
typedef struct nrhip_eval_pruned_args {
  const float* d_P; int64_t ldp;                 /* user factors [n_table_users][ldp] */
  const float* d_Q; int64_t ldq;                 /* item factors [cols][ldq] */
  int d, cols;
  const int32_t* d_users; int n_users, batch_rows;
  const int64_t* d_tr_indptr; const int32_t* d_tr_indices;          /* train CSR (struck items) */
  const int64_t* d_truth_indptr; const int32_t* d_truth_indices;    /* test CSR */
  const int32_t* d_chunk_tile; const int64_t* d_chunk_begin; int n_chunks;   /* strike plan (nrhip_score_tilemax_fix) */
  const int64_t* d_tile_ptr; const int32_t* d_plan_user; const uint32_t* d_plan_mask;
  const int32_t* d_row_of;                       /* user -> evaluation row (-1: not evaluated) */
  const int32_t* metric_ids; int n_metric, top_k, n_keep;
  int use_filter, prepare_items;                 /* bounded search: 0 none, 1 bf16, 2 int8 (d_filter_ws of that form) / (re)build the item-side copies first:
                                                  * 1 all of them; 2 (with a filter) all but the fp32 scoring loop's operand copy, which this call does not read —
                                                  * nrhip_score_gemm_prepare_items must run before nrhip_score_gemm / nrhip_score_tilemax use that workspace */
  void* d_gemm_ws; size_t gemm_ws_bytes;         /* nrhip_score_gemm_workspace_bytes(batch_rows, cols, d) */
  void* d_filter_ws; size_t filter_ws_bytes;     /* nrhip_score_filter_workspace_bytes(batch_rows, cols, d) */
  void* d_tiles_ws; size_t tiles_ws_bytes;       /* nrhip_eval_tiles_bounded_workspace_bytes(batch_rows, cols, top_k, n_keep) */
  float* d_M; int64_t mld;                       /* [batch_rows][mld] tile maxima */
  float* d_eps;                                  /* [batch_rows] */
  float* d_out;                                  /* [n_users][n_metric*top_k] */
  int32_t* d_flags;                              /* [n_users] */
  double* d_sums;                                /* [n_metric*top_k + 2] or NULL */
  void* d_colsum_ws; size_t colsum_ws_bytes;     /* nrhip_colsum_workspace_bytes(n_users, n_metric*top_k) */
} NrhipEvalPruned;
int nrhip_eval_pruned(const NrhipEvalPruned* args, void* stream);

/* The rows nrhip_eval_pruned flagged (ties that could change a metric, a certificate that did not hold, a full bucket),
 * ranked again from full fp32 score rows — nrhip_score_gemm + nrhip_mask_train + nrhip_eval_scores, the materialised
 * path, exact whatever the cause (uni_evaluator.py:132-151 -> evaluate.h:23-72) — and written over their rows of
 * ev->d_out, then (ev->d_sums != NULL) the column sums again: one call, no host round trip inside.  n_flagged is the
 * count nrhip_eval_pruned left in d_sums[n_metric*top_k] (the caller has read it); ev is that call's argument block,
 * unchanged.  The rows are collected in whatever order the device finds them (every row is independent). */
typedef struct nrhip_eval_redo_args {
  const NrhipEvalPruned* ev;
  int n_flagged;
  int reload_items;                              /* the fp32 scoring loop's item side first: 1 nrhip_score_gemm_prepare_items; 2 its operand
                                                  * copy only (ev ran with prepare_items = 2 on this table: the k-major copy stands) */
  float* d_scores; int64_t lds; int slab_rows;   /* score slab [slab_rows][lds], lds >= roundup(cols, 64), slab_rows <= ev->batch_rows */
  int32_t* d_rows;                               /* [n_flagged] out: the flagged rows */
  int32_t* d_row_users;                          /* [n_flagged] out: their users */
  int32_t* d_count;                              /* one word */
  float* d_fixed;                                /* [slab_rows][n_metric*top_k] */
  void* d_ws; size_t ws_bytes;                   /* nrhip_eval_workspace_bytes(slab_rows, top_k) */
} NrhipEvalRedo;
int nrhip_eval_redo(const NrhipEvalRedo* args, void* stream);

/* ---- sampler ------------------------------------------------------------
 * Replaces: PairwiseSampler.__iter__ = _sampling_negative_items +
 *           DataIterator(shuffle) (data/sampler.py:71-90,198-206;
 *           util/data_iterator.py:58-60,145-152) and the rejection loop of
 *           randint_choice (util/cython/random_choice.pyx:20-62).
 *
 * Train CSR: indptr[n_users+1] (int64), indices ascending per row; d_row_of[E]
 * is the user of each CSR position (users_list of sampler.py:24-39).
 * Output position p of the epoch stream holds triplet perm(p); with
 * shuffle == 0 perm is the identity (user-major order, as the reference with
 * shuffle=False).  d_neg_out has E*neg_num entries, row-major [E][neg_num]. */
int nrhip_sample_bpr_epoch(const int64_t* d_tr_indptr, const int32_t* d_tr_indices,
                           const int32_t* d_row_of, int64_t n_inter, int n_items, int neg_num,
                           uint64_t seed, uint64_t epoch, int shuffle, int64_t out_begin,
                           int64_t out_count, int32_t* d_users_out, int32_t* d_pos_out,
                           int32_t* d_neg_out, void* stream);

/* Epoch stream of training INSTANCES on the device — replaces the __iter__ of
 * PointwiseSampler (data/sampler.py:137-149), TimeOrderPointwiseSampler
 * (:269-282) and TimeOrderPairwiseSampler (:339-347): _sampling_negative_items
 * (:71-90) + the Python-list layout (:131-135, :141-143, :259-266) +
 * DataIterator(shuffle) (util/data_iterator.py:58-60,145-152), in one launch.
 *
 * Rows r = 0..R-1 in the iteration order of user_pos_dict; d_row_user[r] = user
 * id; d_seq[d_seq_ptr[r]..) the row's items as the dict holds them (time order
 * for the TimeOrder samplers); d_excl[d_excl_ptr[r]..) the same set ascending
 * (exclusion test).  Instance t = d_inst_ptr[r] + k (k < len_r - high_order,
 * _generative_time_order_positive_items, data/sampler.py:42-68; high_order 0:
 * _generate_positive_items, :24-39), d_inst_row[t] = r.  pointwise == 0: slot =
 * instance, d_items_out = positive, d_neg_out [count][neg_num].  pointwise != 0:
 * n_inst*(neg_num+1) slots, slot s = (c = s / n_inst, t = s % n_inst), c = 0 the
 * positive (label 1), else negative c-1 of instance t (label 0).  d_recent_out
 * [count][high_order] (may be NULL when high_order == 0).  Output position p of
 * the epoch carries slot perm(p); shuffle == 0: identity (the reference's list
 * order). */
int nrhip_sample_instances_epoch(const int64_t* d_seq_ptr, const int32_t* d_seq,
                                 const int64_t* d_excl_ptr, const int32_t* d_excl,
                                 const int64_t* d_inst_ptr, const int32_t* d_inst_row,
                                 const int32_t* d_row_user, int64_t n_inst, int high_order,
                                 int n_items, int neg_num, int pointwise, uint64_t seed,
                                 uint64_t epoch, int shuffle, int64_t out_begin, int64_t out_count,
                                 int32_t* d_users_out, int32_t* d_recent_out, int32_t* d_items_out,
                                 int32_t* d_neg_out, float* d_labels_out, void* stream);

/* batch_randint_choice(high, size, replace, p=None, exclusion)
 * (random_choice.pyx:64-89): request q draws size[q] =
 * d_out_offsets[q+1]-d_out_offsets[q] values into d_out[d_out_offsets[q] ..)
 * (d_out_offsets has n_req+1 entries, total = d_out_offsets[n_req]),
 * excluding the ascending, duplicate-free list
 * d_excl[d_excl_indptr[q] .. d_excl_indptr[q+1]).  replace == 0 additionally
 * forbids repeats inside one request. */
int nrhip_randint_choice_batch(int high, int n_req, int64_t total, const int64_t* d_out_offsets,
                               const int64_t* d_excl_indptr, const int32_t* d_excl, int replace,
                               uint64_t seed, uint64_t call_counter, int32_t* d_out, void* stream);

/* ---- BPR-MF training step -------------------------------------------------
 * Replaces one sess.run((loss, optimizer)) of MF.train_model
 * (model/general_recommender/MF.py:54-76,101; util/learner.py:9-10,19-22;
 * util/tool.py:216-217).
 *   plan:  the occurrences (row, position) of every batch of an epoch stream sorted
 *          by row then position — what makes the row-gradient sums deterministic:
 *          TF adds the IndexedSlices that hit one row in batch order
 *          (unsorted_segment_sum; the positive lookups' slices before the negative
 *          lookups'), and so do the kernels given this order.  d_third = NULL for
 *          pointwise (user, item) instances.  Batch k covers stream elements
 *          [k*batch, min((k+1)*batch, n_total)); its n_cls*len keys are written at
 *          d_plan_out + n_cls*k*batch (n_cls = 3 with d_third, else 2).  Item ids are
 *          offset by n_users in the keys.  Batches of up to (n_cls-1)*batch = 16384 item
 *          occurrences are sorted by one workgroup each in one launch; larger ones by a
 *          segmented multi-workgroup network (a few launches per call).
 *   grad:  gathers p_u,q_i,q_j; x=<p,q_i>-<p,q_j>; loss_b=softplus(-x);
 *          row gradients (duplicates summed in batch order) STORED into the rows of
 *          dense d_GP/d_GQ the batch touches (all other rows are left alone: keep them
 *          zero); d_work is scratch for 8*batch floats (per-triplet loss and l2 terms,
 *          reduced in a fixed order; then room for a plan); d_plan = this batch's slice
 *          of an nrhip_bpr_plan output, or NULL: the plan is then sorted on the spot
 *          (one more launch); d_loss2[0] = sum_b loss_b, d_loss2[1] = reg * sum_b l2_b,
 *          the two addends of MF.py:68-69 (the fetched loss is their sum).
 *   adam:  TF-1.12 sparse Adam = all rows swept (see nr_core.h), and the
 *          gradient buffer is cleared for the next step.               */
int nrhip_bpr_plan(const int32_t* d_users, const int32_t* d_items, const int32_t* d_third,
                   int64_t n_total, int batch, int n_users, uint64_t* d_plan_out, void* stream);
int nrhip_bpr_mf_grad(const float* d_P, const float* d_Q, int d, int n_users,
                      const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int batch,
                      float reg, float* d_GP, float* d_GQ, float* d_work, float* d_loss2,
                      const uint64_t* d_plan, void* stream);
int nrhip_adam_sparse_tf(float* d_var, float* d_m, float* d_v, float* d_grad, int64_t n,
                         float alpha, float beta1, float beta2, float eps, void* stream);
/* The same optimiser, exactly, without the sweep (SURVEY.md H2 "lazy replay"): d_last[row] = last
 * step applied to the row (int32, zero at step 0); when step t touches a row its missed
 * zero-gradient steps are replayed in registers with the step sizes d_alpha_tab[s] (fp32, 1-based,
 * >= t + 1 entries, each made exactly like the `alpha` of nrhip_adam_sparse_tf), then step t is
 * applied with the row's gradient (cleared afterwards).  d_plan / n_occ: the batch's nrhip_bpr_plan
 * slice — rows must be rows of this [n_rows][d] table (user rows first, item rows offset by the plan's
 * n_users).  Every call also brings rows r = t (mod period) up to step t, so no row is ever more
 * than `period` steps behind.  d_next_plan / n_next_occ (optional): the NEXT step's batch plan — its
 * rows are brought to step t too, so that the next gradient kernel replays nothing.
 * d_plan = NULL, n_occ = 0, period = 1: flush every row to step t — required before the table (or m,
 * v) is read; afterwards the buffers are bit-identical to t sweeps. */
int nrhip_adam_sparse_tf_lazy(float* d_var, float* d_m, float* d_v, float* d_grad, int32_t* d_last,
                              const int32_t* d_stamp, int64_t n_rows, int d, const uint64_t* d_plan,
                              int n_occ, const uint64_t* d_next_plan, int n_next_occ,
                              const float* d_alpha_tab, int t, int period, float beta1, float beta2,
                              float eps, void* stream);
/* The gradient half of a lazy step: nrhip_bpr_mf_grad on the one-allocation table [n_users +
 * n_items][d] (d_G likewise), every gathered row first brought to step t - 1 in registers (nothing
 * written back), the batch's rows stamped d_stamp[row] = t (int32 per row; the optimiser call of the
 * same step takes it to tell batch rows from scheduled rows).  d_plan is required. */
int nrhip_bpr_mf_grad_lazy(const float* d_table, const float* d_m, const float* d_v,
                           const int32_t* d_last, const float* d_alpha_tab, int32_t* d_stamp, int t,
                           float beta1, float beta2, float eps, int d, int n_users,
                           const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int batch,
                           float reg, float* d_G, float* d_work, float* d_loss2, const uint64_t* d_plan,
                           void* stream);
/* TF-1.12 dense ApplyAdam; d_grad cleared afterwards when clear_grad != 0. */
int nrhip_adam_dense_tf(float* d_var, float* d_m, float* d_v, float* d_grad, int64_t n,
                        float alpha, float beta1, float beta2, float eps, int clear_grad,
                        void* stream);

/* Dense ApplyAdam with gradient = d_grad_a + d_grad_b (added in fp32, one rounding); the
 * gradient buffers are read-only. */
int nrhip_adam_dense_tf2(float* d_var, float* d_m, float* d_v, const float* d_grad_a,
                         const float* d_grad_b, int64_t n, float alpha, float beta1, float beta2,
                         float eps, void* stream);
/* Dense ApplyAdam on up to 32 tensors in one launch (a model's weight matrices and biases:
 * util/learner.py:9-10 applied to every trainable of NGCF.py:91-110 / MultiVAE.py:47-70).  Host
 * arrays of device pointers and lengths; clear_grad_host (optional) as in nrhip_adam_dense_tf. */
int nrhip_adam_dense_tf_multi(int n_tensors, float* const* d_vars_host, float* const* d_ms_host,
                              float* const* d_vs_host, float* const* d_grads_host,
                              const int64_t* sizes_host, const int32_t* clear_grad_host, float alpha,
                              float beta1, float beta2, float eps, void* stream);
/* Row-sparse helpers over a list of row ids of a [*, d] buffer (repeats allowed):
 * dst[row] = src[row] / denom; and zeroing of the listed rows of up to four buffers plus a
 * per-row byte flag (any of them may be NULL).
 * Empty work is no error: with n_listed == 0 (these two, nrhip_rows_gather*, nrhip_rows_scatter_add,
 * nrhip_mark_rows), n == 0 (nrhip_gather_u8, nrhip_sort_u64, the Adam sweeps, a tensor of
 * nrhip_adam_dense_tf_multi) or batch == 0 (the id arrays of nrhip_pairwise_mf_grad / nrhip_pointwise_mf_grad) the
 * arrays of that length may be NULL — an empty device tensor has no storage. */
int nrhip_rows_div(const int32_t* d_rows, int n_listed, int d, const float* d_src, float denom,
                   float* d_dst, void* stream);
int nrhip_rows_clear(const int32_t* d_rows, int n_listed, int d, float* d_b0, float* d_b1,
                     float* d_b2, float* d_b3, uint8_t* d_flag, void* stream);

/* ---- sparse adjacency x embedding (LightGCN / NGCF propagation) ----------
 * Replaces tf.sparse_tensor_dense_matmul(adj, ego)
 * (model/general_recommender/LightGCN.py:140, NGCF.py:176) and its autodiff
 * transpose.  Y[r] = sum_j vals[j]*X[indices[j]] over the CSR row r in
 * ascending j (product and sum rounded separately), then
 *   Y[r] += addend[r]            if d_addend != NULL
 *   d_sum_out[r] = d_sum_in[r]+Y if d_sum_out != NULL (running layer sum,
 *                                LightGCN.py:146-147)
 * A plan splits long rows into segments; build it once per graph. */
int nrhip_spmm_plan_bytes(int64_t n_rows, int64_t nnz, size_t* bytes);
/* h_indptr is a HOST pointer (n_rows+1 entries): the segment plan is computed
 * on the host, uploaded into the caller's device buffer d_plan_buf, and a
 * host-side handle describing it is returned in *plan_out.  item_rows /
 * item_nnz bound the whole-row work items (0 = tuned defaults; at most 32 rows
 * and 256 non-zeros).  split_row (0 = none) is a locality hint for bipartite graphs: rows
 * below it (user nodes) and from it on (item nodes) gather from disjoint halves of X and are
 * scheduled on disjoint halves of the XCDs. */
int nrhip_spmm_plan_create(const int64_t* h_indptr, int64_t n_rows, int item_rows, int item_nnz,
                           int64_t split_row, void* d_plan_buf, size_t plan_bytes, void* stream,
                           void** plan_out);
int nrhip_spmm_plan_destroy(void* plan);
int nrhip_spmm_plan_info(const void* plan, int64_t* n_work_items, int64_t* n_split_rows);
int nrhip_spmm_workspace_bytes(const void* plan, int d, size_t* bytes);
/* d_Y may be NULL when only the running sum is wanted. */
int nrhip_spmm_csr(const void* plan, const int64_t* d_indptr, const int32_t* d_indices,
                   const float* d_vals, const float* d_X, int d, float* d_Y,
                   const float* d_addend, const float* d_sum_in, float* d_sum_out, void* d_ws,
                   size_t ws_bytes, void* stream);

/* The same product with work skipped (d >= 64; either mask may be NULL, not both):
 *   d_x_row_nonzero[c] == 0 promises X[c][:] == 0: those terms are skipped instead of
 *     gathered (first backward hop of a training step: dLoss/dE* is non-zero on the batch
 *     rows only);
 *   d_y_row_wanted[r] == 0 says output row r is not needed: it is left untouched (last
 *     forward hop of a training step: the loss reads E* on the batch rows only).
 * Produced rows are bit-identical to nrhip_spmm_csr's, with one exception: behind a lane-group schedule with
 * column blocks (block_bytes > 0: several phases) the d = 64 row-masked hop walks its own schedule, which cuts a
 * row of more than seg_len non-zeros into seg_len-long segments by position, while the full pass cuts it per column
 * block — such a row's partial sums are then added in another association (rows of <= seg_len non-zeros keep every
 * bit; engine.SpmmCSR never asks for column blocks). */
int nrhip_spmm_csr_masked(const void* plan, const int64_t* d_indptr, const int32_t* d_indices,
                          const float* d_vals, const float* d_X, const uint8_t* d_x_row_nonzero,
                          const uint8_t* d_y_row_wanted, int d, float* d_Y, const float* d_addend,
                          const float* d_sum_in, float* d_sum_out, void* d_ws, size_t ws_bytes,
                          void* stream);
/* Only the listed rows of A·X (+ epilogue) are produced; other rows of the outputs are left
 * untouched.  d_rows may repeat; d_sum_out must not alias d_sum_in.  d in {64,128,256}. */
/* Persistent lane-group schedule for d = 16 / 32 / 64 (128 / 256 on request) (spmm_blocked.hip): one workgroup per CU
 * owns a LIST of rows (4·d-byte accumulators in LDS) — since r05 the rows are dealt to the workgroups by cost
 * (longest first, each to the least-loaded workgroup with a free accumulator), so the balance does not depend on how
 * the nodes are numbered (r01-r04's contiguous runs carried 1.9x the mean cost in their slowest workgroup when
 * popular items cluster in id); a d/4-lane group walks one row with 16-byte
 * loads, so a load instruction moves 4 / 2 / 1 rows; sub-lists longer than seg_len are cut into segments whose
 * partials are added in segment order.  Optional column blocking (block_bytes) cuts the gathered
 * table into L2-sized windows walked phase by phase.  Same contract and masks as nrhip_spmm_csr /
 * _masked; rows of <= seg_len non-zeros are bit-identical to the sequential order.  Attach it to
 * an SpMM plan (per d) and nrhip_spmm_csr / _masked / the step drivers use it for that d.
 * 0 selects a default for block_bytes (no blocking), n_workgroups (one per CU),
 * waves_per_wg (16), seg_len (64), r_max / p_max (LDS accumulators).  NR_ERR_UNSUPPORTED when the
 * matrix does not fit the schedule (the work-item kernel remains). */
int nrhip_spmm_blocked_plan_bytes(int64_t n_rows, int64_t nnz, int d, size_t* bytes);
int nrhip_spmm_blocked_plan_create(const int64_t* h_indptr, const int32_t* h_indices,
                                   int64_t n_rows, int64_t split_row, int d, int64_t block_bytes,
                                   int n_workgroups, int waves_per_wg, int seg_len, int r_max,
                                   int p_max, void* d_plan_buf, size_t plan_bytes, void* stream,
                                   void** plan_out);
int nrhip_spmm_blocked_plan_destroy(void* plan);
int nrhip_spmm_blocked_plan_info(const void* plan, int* n_workgroups, int* n_phases,
                                 int64_t* n_entries, int64_t* n_split);
int nrhip_spmm_blocked_tune(int gathers_in_flight);
/* How the column-masked hop of a training step stores its output Y, process-wide, for tests and A/B runs: -1 the
 * built-in default, 0 plain, 1 nontemporal, 2 written through (the same bytes either way). */
int nrhip_spmm_blocked_tune_store(int masked_store);
/* The plan OWNS a copy of the matrix's (column, value) pairs in its own row order (a workgroup's pairs are one
 * contiguous slice): nrhip_spmm_blocked_pack fills it from the CSR arrays — once per matrix, again whenever the
 * values change (NGCF's node dropout rewrites them every step); a product call that hands in arrays that were not
 * packed packs them first, on its stream.  CONTRACT: freshness is decided by the identity of the two pointers — a
 * caller that rewrites d_vals IN PLACE must call nrhip_spmm_blocked_pack again before the next product
 * (engine.SpmmCSR.values_changed does; NGCF's node dropout is the one such caller). */
int nrhip_spmm_blocked_pack(void* plan, const int32_t* d_indices, const float* d_vals, void* stream);
/* nrhip_spmm_blocked_pack, and where the values factor also a 4-byte form of the same pairs, which
 * spmm_blocked_kernel (the full passes, the pass with ApplyAdam, the general masked form) then reads instead, half
 * the bytes: word = column | code << column bits, value = float32(factor of the row * table[code]).  The staged
 * masked hop and the wanted-rows hops keep reading (column, value) pairs.  h_row_factor [n_rows] / h_col_factor [n_cols] are HOST arrays
 * (graph.factor_values; both NULL: the plain pack) that promise float32(h_row_factor[r] * h_col_factor[c]) ==
 * value[r][c]; the promise is checked on the device for every non-zero, so results keep every bit.  *packed
 * (optional) / nrhip_spmm_blocked_is_packed say whether the words are in use.  They are not — the plan is exactly what
 * the plain pack leaves — when one product misses its value, when there are more than 1,024 distinct factors (the
 * table the kernels keep in LDS) or more than the word has bits for, or when n_cols > n_rows.  Synchronises the
 * stream.  nrhip_spmm_blocked_tune_packed(0), process-wide, for tests and A/B runs: read the two arrays of
 * a packed plan (1: the words again; NEUREC_SPMM_PACKED=0 in the environment of a plan's creation does the same). */
int nrhip_spmm_blocked_pack_factored(void* plan, const int32_t* d_indices, const float* d_vals,
                                     const float* h_row_factor, const float* h_col_factor, int64_t n_cols,
                                     void* stream, int* packed);
int nrhip_spmm_blocked_is_packed(const void* plan);
int nrhip_spmm_blocked_tune_packed(int on);
int nrhip_spmm_blocked(const void* plan, const int32_t* d_indices, const float* d_vals,
                       const float* d_X, float* d_Y, const float* d_addend, const float* d_sum_in,
                       float* d_sum_out, const uint8_t* d_x_row_nonzero,
                       const uint8_t* d_y_row_wanted, void* stream);
/* The unmasked product with a promise about a row-sparse addend: d_addend_row_flag[r] == 0 says row r of d_addend is
 * all zero, and the lane-group pass does not read it (the inner backward hops of a LightGCN step: H is non-zero on
 * the batch rows only, whose flags the batch-rows hop set).  NULL flags: nrhip_spmm_blocked / nrhip_spmm_csr.
 * Flags need an addend and no masks.  nrhip_spmm_csr_flagged: behind the matrix handle; a width without a lane-group
 * schedule reads the addend densely (same result).  _tune_addend_flag(0): ignore the flags process-wide (A/B runs). */
int nrhip_spmm_blocked_flagged(const void* plan, const int32_t* d_indices, const float* d_vals,
                               const float* d_X, float* d_Y, const float* d_addend,
                               const uint8_t* d_addend_row_flag, const float* d_sum_in, float* d_sum_out,
                               const uint8_t* d_x_row_nonzero, const uint8_t* d_y_row_wanted, void* stream);
int nrhip_spmm_csr_flagged(const void* plan, const int64_t* d_indptr, const int32_t* d_indices,
                           const float* d_vals, const float* d_X, int d, float* d_Y,
                           const float* d_addend, const uint8_t* d_addend_row_flag, const float* d_sum_in,
                           float* d_sum_out, void* d_ws, size_t ws_bytes, void* stream);
int nrhip_spmm_blocked_tune_addend_flag(int on);
int nrhip_spmm_plan_attach_blocked(void* plan, const void* blocked_plan, int d);

/* Last backward hop of a step and the optimiser in one pass (LightGCN.py:130,140 fused):
 * d_var / d_m / d_v <- TF-1.12 ApplyAdam with the dense gradient (A·X + d_addend) + d_grad_b; the
 * product itself is never stored.  Needs the d = 64 lane-group schedule attached to the plan
 * (nrhip_spmm_plan_has_blocked(plan, 64) != 0), NRHIP_ERR_UNSUPPORTED otherwise. */
/* clear_consumed != 0 additionally zeroes the non-zero entries of d_addend / d_grad_b and the set
 * bytes of d_row_flag (may be NULL) as they are read — what nrhip_rows_clear would do after the
 * step (both buffers are row-sparse there).  With clear_consumed and a d_row_flag, the flags are
 * also a promise: rows of d_addend / d_grad_b whose flag byte is 0 are all zero (they are not
 * read). */
int nrhip_spmm_csr_adam(const void* plan, const int32_t* d_indices, const float* d_vals,
                        const float* d_X, int d, float* d_addend, float* d_grad_b, float* d_var,
                        float* d_m, float* d_v, float alpha, float beta1, float beta2, float eps,
                        int clear_consumed, uint8_t* d_row_flag, void* stream);
int nrhip_spmm_blocked_adam(const void* plan, const int32_t* d_indices, const float* d_vals,
                            const float* d_X, float* d_addend, float* d_grad_b, float* d_var,
                            float* d_m, float* d_v, float alpha, float beta1, float beta2,
                            float eps, int clear_consumed, uint8_t* d_row_flag, void* stream);
int nrhip_spmm_plan_has_blocked(const void* plan, int d);   /* 1 / 0, not a status code */

/* Last forward hop of a step with the layer sum completed on the way (LightGCN.py:143-146 on the
 * batch rows): for rows with d_y_row_wanted[r] != 0,
 *   d_sum_out[r] = ((d_sum_in[r] + d_layer_a[r]) + d_layer_b[r]) + (A·X)[r]
 * (d_layer_a / d_layer_b optional, NULL = term absent; other rows of d_sum_out untouched).  The
 * full hops before it then need no running-sum streams.  Same additions in the same order as
 * nrhip_spmm_csr with sum_in / sum_out hop by hop.  Needs the d = 64 wanted-rows schedule
 * (nrhip_spmm_plan_has_wanted(plan, 64) != 0), NRHIP_ERR_UNSUPPORTED otherwise. */
int nrhip_spmm_csr_wanted_layers(const void* plan, const int32_t* d_indices, const float* d_vals,
                                 const float* d_X, int d, const float* d_sum_in,
                                 const float* d_layer_a, const float* d_layer_b, float* d_sum_out,
                                 const uint8_t* d_y_row_wanted, void* stream);
int nrhip_spmm_blocked_wanted_layers(const void* plan, const int32_t* d_indices, const float* d_vals,
                                     const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                     const float* d_layer_b, float* d_sum_out,
                                     const uint8_t* d_y_row_wanted, void* stream);
/* The same hop told the batch instead of flags: wanted rows = d_users | n_users + d_pos |
 * n_users + d_neg.  It does nrhip_lightgcn_mark_batch's job on the way (one launch less per step):
 * d_row_flag (zero on entry) gets 1 on those rows, d_rows_out (optional) the 3*batch rows.  Needs
 * nrhip_spmm_plan_has_wanted(plan, 64) == 2 (a matrix of <= 131072 rows: one bit per row in LDS). */
int nrhip_spmm_csr_wanted_batch(const void* plan, const int32_t* d_indices, const float* d_vals,
                                const float* d_X, int d, const float* d_sum_in, const float* d_layer_a,
                                const float* d_layer_b, float* d_sum_out, const int32_t* d_users,
                                const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                                uint8_t* d_row_flag, int32_t* d_rows_out, void* stream);
int nrhip_spmm_blocked_wanted_batch(const void* plan, const int32_t* d_indices, const float* d_vals,
                                    const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                    const float* d_layer_b, float* d_sum_out, const int32_t* d_users,
                                    const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                                    uint8_t* d_row_flag, int32_t* d_rows_out, void* stream);
/* 0: no wanted-rows schedule, 1: flag form only, 2: flag and batch forms (not status codes) */
int nrhip_spmm_plan_has_wanted(const void* plan, int d);
int nrhip_spmm_blocked_has_wanted(const void* blocked_plan);
/* The batch-rows hop from a per-batch work list made an epoch ahead (csrc/spmm_wanted_plan.h has the layout).
 * A batch is no run-time surprise: nrhip_bpr_plan leaves every batch's distinct rows, sorted, for the whole epoch
 * stream.  _epoch_plan turns them into one list of wave-sized items per batch (records of 16 bytes, *stride per
 * batch) in ONE launch without a host read; _wanted_planned is nrhip_spmm_csr_wanted_batch run from the batch's own
 * records d_batch_sched = d_sched + k * stride * 16: no bit set, no descriptor scan, one round per workgroup, the
 * same additions in the same order.  _has_wanted_planned: 1 when the matrix has it (d = 64, <= 2^19 rows,
 * NEUREC_SPMM_WANTED_PLANNED != 0).  d_plans: 3 * batch keys per batch, the last batch last_len triplets;
 * 3 * batch <= 16384.  d_indptr: the matrix's row offsets on the device. */
int nrhip_spmm_plan_has_wanted_planned(const void* plan, int d);
int nrhip_spmm_blocked_has_wanted_planned(const void* blocked_plan);
int nrhip_spmm_wanted_epoch_plan_bytes(const void* plan, int d, int batch, int64_t n_batches, size_t* bytes,
                                       int* stride);
int nrhip_spmm_blocked_wanted_epoch_plan_bytes(const void* blocked_plan, int batch, int64_t n_batches, size_t* bytes,
                                               int* stride);
int nrhip_spmm_wanted_epoch_plan(const void* plan, int d, const int64_t* d_indptr, const uint64_t* d_plans, int batch,
                                 int64_t n_batches, int last_len, void* d_sched, size_t sched_bytes, void* stream);
int nrhip_spmm_blocked_wanted_epoch_plan(const void* blocked_plan, const int64_t* d_indptr, const uint64_t* d_plans,
                                         int batch, int64_t n_batches, int last_len, void* d_sched, size_t sched_bytes,
                                         void* stream);
int nrhip_spmm_csr_wanted_planned(const void* plan, const int32_t* d_indices, const float* d_vals, const float* d_X,
                                  int d, const float* d_sum_in, const float* d_layer_a, const float* d_layer_b,
                                  float* d_sum_out, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                                  int batch, int n_users, uint8_t* d_row_flag, int32_t* d_rows_out,
                                  const void* d_batch_sched, int stride, void* stream);
int nrhip_spmm_blocked_wanted_planned(const void* blocked_plan, const int32_t* d_indices, const float* d_vals,
                                      const float* d_X, const float* d_sum_in, const float* d_layer_a,
                                      const float* d_layer_b, float* d_sum_out, const int32_t* d_users,
                                      const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                                      uint8_t* d_row_flag, int32_t* d_rows_out, const void* d_batch_sched, int stride,
                                      void* stream);

/* Chunked propagation hop of the row-sharded engine (neurec_amd/sharded.py; LightGCN.py:132-149 with the operand
 * arriving in rank-ordered chunks — SURVEY 8e "overlap layer-k comm with layer-k local SpMM").  One launch per
 * operand chunk (columns < x_split: the rank's own block d_X; the rest: the received chunk d_X2) carries every
 * (virtual) row's accumulator on, so a row's sum stays ONE ascending-column chain; the
 * finish pass combines a hub row's 256-non-zero segments in segment order and applies nrhip_spmm_csr's epilogue. */
int nrhip_spmm_csr_carry(const void* plan, const int64_t* d_indptr, const int32_t* d_indices, const float* d_vals,
                         const float* d_X, const float* d_X2, int x_split, int d, float* d_Yv, int has_carry,
                         const uint8_t* d_row_mask, void* stream);
int nrhip_spmm_chunks_finish(const int32_t* d_first_vrow, int64_t n_rows, const float* d_Yv, int d, float* d_Y,
                             const float* d_addend, const float* d_sum_in, float* d_sum_out,
                             const uint8_t* d_row_mask, void* stream);

/* Reduced-exchange hop of the row-sharded engine (neurec_amd/sharded.py hop="reduce"; LightGCN.py:132-149 with the
 * item rows' sums formed as per-rank partials over each rank's OWN user rows): d_parts[world][n_rows][d]
 * holds the partial rows an owner received, rank-major; Y[r] = parts[0][r] + parts[1][r] + ... in rank order (one
 * fixed association), then nrhip_spmm_csr's epilogue (addend, running sum).  d_row_mask (optional): 0 = row left
 * untouched.  d a multiple of 4. */
int nrhip_partials_sum_rows(const float* d_parts, int world, int64_t n_rows, int d, float* d_Y, const float* d_addend,
                            const float* d_sum_in, float* d_sum_out, const uint8_t* d_row_mask, void* stream);

int nrhip_spmm_csr_rows(const int64_t* d_indptr, const int32_t* d_indices, const float* d_vals,
                        const float* d_X, int d, const int32_t* d_rows, int n_listed, float* d_Y,
                        const float* d_addend, const float* d_sum_in, float* d_sum_out,
                        void* stream);

/* ---- LightGCN BPR head ----------------------------------------------------
 * Replaces the lookups + create_bpr_loss of LightGCN.py:99-104,156-166 and
 * their gradient.  d_Esum is the running layer sum (E* = Esum/(L+1));
 * user rows first, item rows offset by n_users.  Stores, on the rows the batch touches
 * (duplicates summed in batch order, see nrhip_bpr_plan; other rows are left alone),
 *   d_Gstar  = dLoss/dE*      (dense [N][d], zero elsewhere)
 *   d_Greg   = reg * E0 rows  (dense [N][d], zero elsewhere)
 * and writes the two scalars mf_loss, emb_loss into d_loss2[0..1] (d_loss2 may be NULL:
 * the reference never fetches LightGCN's loss during training, LightGCN.py:178).
 * d_work: 8*batch floats; d_plan: the batch's plan or NULL (sorted on the spot). */
int nrhip_lightgcn_bpr_grad(const float* d_Esum, const float* d_E0, int n_users, int d,
                            int n_layers, const int32_t* d_users, const int32_t* d_pos,
                            const int32_t* d_neg, int batch, float reg, float* d_Gstar,
                            float* d_Greg, float* d_work, float* d_loss2, const uint64_t* d_plan,
                            void* stream);

/* Same head, storing dLoss/dE* already divided by (n_layers+1) into d_H (zero elsewhere) —
 * the H = Gstar/(L+1) the backward hops start from.  Only for n_layers+1 a power of two, where
 * dividing every term is bit-identical to dividing the sum (NRHIP_ERR_ARG otherwise). */
int nrhip_lightgcn_bpr_grad_h(const float* d_Esum, const float* d_E0, int n_users, int d,
                              int n_layers, const int32_t* d_users, const int32_t* d_pos,
                              const int32_t* d_neg, int batch, float reg, float* d_H,
                              float* d_Greg, float* d_work, float* d_loss2, const uint64_t* d_plan,
                              void* stream);

/* Node rows touched by a batch: d_rows_out[3*batch] = users | n_users+pos | n_users+neg and
 * d_row_flag[those rows] = 1 (d_row_flag: n_nodes bytes, zero on entry). */
int nrhip_lightgcn_mark_batch(const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                              int batch, int n_users, int32_t* d_rows_out, uint8_t* d_row_flag,
                              void* stream);

/* ---- whole training steps issued natively -----------------------------------
 * One call enqueues every kernel of a step (the reference's sess.run(opt) is one
 * call into its native runtime too: LightGCN.py:178, MF.py:101).  The context only
 * records caller-owned device pointers; nothing is allocated on the device. */
typedef struct nrhip_lightgcn_buffers {
  const void* plan;          /* SpMM plan of the adjacency A              */
  const void* plan_t;        /* plan of A^T (== plan when A is symmetric) */
  const int64_t* indptr;  const int32_t* indices;  const float* vals;      /* A   */
  const int64_t* indptr_t; const int32_t* indices_t; const float* vals_t;  /* A^T */
  float* E0; float* m; float* v;            /* [n_nodes][d] embeddings + Adam moments */
  float* Ea; float* Eb; float* Esum; float* Esum_rows;   /* layer buffers          */
  float* Gstar; float* Greg; float* H; float* Ga; float* Gb;   /* gradient buffers   */
  int32_t* batch_rows;       /* 3*max_batch                      */
  uint8_t* row_flag;         /* n_nodes bytes, zero between steps */
  float* terms;              /* 8*max_batch floats (loss terms + room for a batch plan) */
  void* spmm_ws; size_t spmm_ws_bytes;
  int n_users; int n_nodes; int d; int n_layers; int max_batch;
  float reg;
} nrhip_lightgcn_buffers;
int nrhip_lightgcn_ctx_create(const nrhip_lightgcn_buffers* bufs, void** ctx_out);
int nrhip_lightgcn_ctx_destroy(void* ctx);
/* alpha = lr*sqrt(1-b2^t)/(1-b1^t) in fp32 (the caller keeps the running powers).
 * d_loss2 may be NULL (loss not fetched).  d_plan: this batch's nrhip_bpr_plan slice (keys built
 * with n_users = the context's) or NULL. */
int nrhip_lightgcn_step(void* ctx, const int32_t* d_users, const int32_t* d_pos,
                        const int32_t* d_neg, int batch, const uint64_t* d_plan, float alpha,
                        float beta1, float beta2, float eps, float* d_loss2, void* stream);
/* The same step with the batch-rows hop run from the batch's records of an nrhip_spmm_wanted_epoch_plan output
 * (d_hop_sched, hop_stride records; the context's forward matrix must have nrhip_spmm_plan_has_wanted_planned). */
int nrhip_lightgcn_step_planned(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                                int batch, const uint64_t* d_plan, const void* d_hop_sched, int hop_stride,
                                float alpha, float beta1, float beta2, float eps, float* d_loss2, void* stream);

/* Column-sharded tables (LightGCN.py:132-166 when every rank holds d of the D embedding columns — the propagation,
 * the gradient rows and ApplyAdam are column-wise, so the only quantity that needs all columns is the head's inner
 * products): the step cut there.  _fwd: forward hops + this rank's partial products d_partials[3*batch] =
 * (<e_u,e_i>, <e_u,e_j>, l2 term) per triplet; the caller all-gathers them, nrhip_partials_sum adds them in rank
 * order; _bwd: head with the summed d_given, backward hops, ApplyAdam.  Every rank steps on the SAME global batch. */
int nrhip_lightgcn_step_colshard_fwd(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                                     int batch, float* d_partials, void* stream);
int nrhip_lightgcn_step_colshard_fwd_planned(void* ctx, const int32_t* d_users, const int32_t* d_pos,
                                             const int32_t* d_neg, int batch, const void* d_hop_sched, int hop_stride,
                                             float* d_partials, void* stream);
int nrhip_lightgcn_step_colshard_bwd(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                                     int batch, const uint64_t* d_plan, const float* d_given, float alpha,
                                     float beta1, float beta2, float eps, float* d_loss2, void* stream);
int nrhip_lightgcn_partial_dots(const float* d_Esum, const float* d_E0, int n_users, int d, int n_layers,
                                const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int batch,
                                float* d_out, void* stream);
int nrhip_partials_sum(const float* d_parts, int world, int n, float* d_given, void* stream);
int nrhip_lightgcn_bpr_grad_given(const float* d_Esum, const float* d_E0, int n_users, int d, int n_layers,
                                  const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int batch,
                                  float reg, float* d_Gstar, float* d_Greg, float* d_work, float* d_loss2,
                                  const uint64_t* d_plan, const float* d_given, int divided, void* stream);
/* The same step cut at its one exchange point (multi-GPU): _grad leaves this rank's total
 * dLoss/dE0 in d_grad_out ([n_nodes][d]); the caller sums it over ranks (RCCL all-reduce);
 * _apply runs Adam on the summed gradient. */
int nrhip_lightgcn_step_grad(void* ctx, const int32_t* d_users, const int32_t* d_pos,
                             const int32_t* d_neg, int batch, const uint64_t* d_plan,
                             float* d_loss2, float* d_grad_out, void* stream);
int nrhip_lightgcn_step_apply(void* ctx, float* d_grad, float alpha, float beta1, float beta2,
                              float eps, void* stream);

typedef struct nrhip_mf_buffers {
  float* P; float* Q; float* mP; float* vP; float* mQ; float* vQ; float* GP; float* GQ;
  float* terms;              /* 8*max_batch floats */
  int n_users; int n_items; int d; int max_batch;
  float reg;
  /* lazy sparse Adam (nrhip_adam_sparse_tf_lazy): last != NULL selects it; needs P|Q, mP|mQ, vP|vQ,
   * GP|GQ each one [n_users + n_items][d] allocation */
  int32_t* last; int32_t* stamp; const float* alpha_tab; int alpha_len; int lazy_period;
  /* one-launch step (nrhip_bpr_mf_step_fused): tw != NULL selects it; P / mP / vP then each hold TWO
   * copies of the [n_users + n_items][d] array (copy 1 at + rows * d), tw = int32 [rows][2] ({0, -1} at start),
   * inb = int32 [rows] (zero at start); last / stamp / GP / GQ are not used */
  int32_t* tw; int32_t* inb;
} nrhip_mf_buffers;
int nrhip_mf_ctx_create(const nrhip_mf_buffers* bufs, void** ctx_out);
int nrhip_mf_ctx_destroy(void* ctx);
/* step_index: 1-based index of this optimiser step (lazy mode: alpha must equal alpha_tab[step_index]);
 * d_next_plan / next_batch: the following batch's plan and length, or NULL / 0 (lazy mode: its rows are
 * brought up to date by this step's optimiser launch) */
int nrhip_mf_step(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                  int batch, const uint64_t* d_plan, const uint64_t* d_next_plan, int next_batch,
                  int step_index, float alpha, float beta1, float beta2, float eps, float* d_loss2,
                  void* stream);
/* The batch loop of MF.train_model (model/general_recommender/MF.py:95-103) over the consecutive batches of
 * one epoch stream (n_total triplets, `batch` per step, the last one short): step k runs on triplets
 * [k*batch, ...), plan d_plans + 3*k*batch (layout of nrhip_bpr_plan(n_total, batch); NULL: sorted per step),
 * step index first_step_index + k, step size h_alpha[k] (HOST array), loss pair d_loss2[2k..2k+1].
 * d_terms_steps: NULL, or 2*batch floats per step — the one-launch form then leaves each step's per-triplet
 * loss terms there and one launch after the loop (nrhip_loss_reduce_steps) produces every pair: the same sums
 * bit for bit, no cross-workgroup hand-off inside the steps (MF.py:101 fetches the loss per step but only adds
 * it up, :103,110). */
int nrhip_mf_steps(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                   int64_t n_total, int batch, const uint64_t* d_plans, int first_step_index,
                   const float* h_alpha, float beta1, float beta2, float eps, float* d_loss2,
                   float* d_terms_steps, void* stream);
/* (sum of the BPR terms, reg * sum of the l2 terms) of n_steps steps from their per-triplet terms: step k's lie at
 * d_terms + k*2*batch ([n] terms, then [n] l2 terms; n = batch, the last step n_last). */
int nrhip_loss_reduce_steps(const float* d_terms, int n_steps, int batch, int n_last, float reg, float* d_loss2,
                            void* stream);
/* lazy mode: bring every row of both tables to step `steps_done` (no-op otherwise) */
int nrhip_mf_flush(void* ctx, int steps_done, float beta1, float beta2, float eps, void* stream);

/* ---- NGCF propagation layer, dense half (second-model coverage) ---------------
 * Replaces the per-layer TF ops of NGCF._create_ngcf_embed
 * (model/general_recommender/NGCF.py:181-198) and their gradient; the sparse half
 * (S = A·E, NGCF.py:174-179) is nrhip_spmm_csr.  Width d = 16 (conf/NGCF.properties).
 *   fwd: T1 = S·Wg+bg, T2 = (E⊙S)·Wb+bb, Z = lrelu(T1)+lrelu(T2), E' = Z/keep·mask,
 *        out = l2_normalize(E').  d_mask (n_rows*d bytes) is read when mask_given, else
 *        drawn from (seed, step, layer) and written (the backward pass needs it).
 *        d_out points at this layer's column block of the concatenated output, row
 *        stride ldo (NGCF.py:200).
 *   bwd: from dLoss/d out (d_dout, stride ldo) and dLoss/dE' coming from the next layer
 *        (d_dego_next, may be NULL): d_dS (to be pushed through A^T), d_dego_direct
 *        (= dBi ⊙ S), and the four weight gradients. */
int nrhip_ngcf_workspace_bytes(int64_t n_rows, size_t* bytes);
int nrhip_ngcf_layer_fwd(const float* d_ego, const float* d_S, const float* d_Wg,
                         const float* d_bg, const float* d_Wb, const float* d_bb, int64_t n_rows,
                         int d, float keep, uint8_t* d_mask, int mask_given, uint64_t seed,
                         uint64_t step, int layer, float* d_ego_out, float* d_out, int64_t ldo,
                         void* stream);
int nrhip_ngcf_layer_bwd(const float* d_ego, const float* d_S, const float* d_Wg,
                         const float* d_bg, const float* d_Wb, const float* d_bb, int64_t n_rows,
                         int d, float keep, const uint8_t* d_mask, const float* d_dout, int64_t ldo,
                         const float* d_dego_next, float* d_dS, float* d_dego_direct, float* d_dT1,
                         float* d_dT2, float* d_dWg, float* d_dbg, float* d_dWb, float* d_dbb,
                         void* d_ws, size_t ws_bytes, void* stream);

/* ---- Mult-VAE (second-model coverage) ------------------------------------------
 * Replaces the TF graph of model/general_recommender/MultiVAE.py:73-135 (q_graph, the
 * reparameterised sample, p_graph, log_softmax, neg-ELBO) and its gradient, for the
 * two-layer shape conf/MultiVAE.properties gives (p_dim=[z,h]: I -> h -> 2z | z -> h -> I)
 * with h <= 32 and 2z <= 32.  The multi-hot input batch is never densified: batch row r
 * is the CSR row d_rows[r] of the train matrix (MultiVAE.py:152-165 builds it densely on
 * the host).  W_p1 is kept item-major, [n_items][h] (the transpose of the TF variable).
 *
 *   nrhip_vae_encode   l2-normalise + dropout + h1 = act(x·W_q0+b) + [mu|logvar] + sample
 *                      + g1 = act(z·W_p0+b); per-row KL.  d_drop_given (per CSR position,
 *                      {0,1}) / d_eps_given ([batch][z]) replace the internal draws when
 *                      non-NULL (tests; eps ~ N(0,0.01²) as MultiVAE.py:108).  d_h0val
 *                      (per CSR position, may be NULL) receives the dropped-out input value.
 *   logits             = nrhip_score_gemm(P=g1, Q=W_p1) (+ b_p1, nrhip_add_row_bias or
 *                      fused below)
 *   nrhip_vae_decoder_loss_grad   d_S holds g1·W_p1ᵀ (bias NOT added) on entry (contents on exit
 *                      unspecified); writes nll[b] = -Σ_i log_softmax·x, dW_p1 ([n_items][h]),
 *                      db_p1, dg1 — both products on the fp32 matrix cores, dLoss/dlogits formed in
 *                      registers from the logits (never stored).  The slab's rows and the bias are
 *                      read 16 bytes at a time: d_S and d_bp1 16-byte aligned, ld a multiple of 4
 *                      (nrhip_score_gemm's buffers are), else NRHIP_ERR_ARG.
 *   nrhip_vae_mid_backward        the 16/32-wide layers' backward and weight gradients.
 *   batch == 0: every entry point of this block (nrhip_vae_step included) launches nothing, writes nothing
 *                      and returns NRHIP_OK.
 *   nrhip_vae_dwq0     scatter of h0ᵀ·da1 into a zeroed dense [n_items][h] gradient.
 * act: 0 tanh, 1 sigmoid, 2 relu, 3 identity (util/tool.py activation_function). */
int nrhip_vae_encode(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows,
                     int batch, int h, int z, const float* d_Wq0, const float* d_bq0,
                     const float* d_Wq1, const float* d_bq1, const float* d_Wp0,
                     const float* d_bp0, int act, float keep, const float* d_drop_given,
                     const float* d_eps_given, float is_training, uint64_t seed, uint64_t step,
                     float* d_h0val, float* d_H1, float* d_MU, float* d_LOGVAR, float* d_EPSSTD,
                     float* d_ZS, float* d_G1, float* d_KLb, void* stream);
int nrhip_add_row_bias(float* d_S, int64_t ld, int batch, int cols, const float* d_bias,
                       void* stream);
int nrhip_vae_workspace_bytes(int batch, int cols, size_t* bytes);
int nrhip_vae_decoder_loss_grad(float* d_S, int64_t ld, int batch, int cols, int h,
                                const float* d_bp1, const int64_t* d_indptr,
                                const int32_t* d_indices, const int32_t* d_rows,
                                const float* d_G1, const float* d_Wp1, float* d_nll,
                                float* d_dWp1, float* d_dbp1, float* d_dG1, void* d_ws,
                                size_t ws_bytes, void* stream);
/* The decoder's loss and gradients with NO [batch][cols] buffer (csrc/vae_fused.hip; MultiVAE.py:104-124):
 * logits tiles are recomputed by MFMA in two passes (statistics; gradients) and never leave the registers.
 * Same arguments as nrhip_vae_decoder_loss_grad minus the slab; d_G1 [batch][h], d_Wp1 [cols][h] item-major.
 * d_dbg_logits: NULL, or (tests) a [batch][cols] buffer that receives pass 1's logits (bias included). */
int nrhip_vae_decoder_fused_workspace_bytes(int batch, int cols, size_t* bytes);
int nrhip_vae_decoder_fused(int batch, int cols, int h, const float* d_G1, const float* d_Wp1,
                            const float* d_bp1, const int64_t* d_indptr, const int32_t* d_indices,
                            const int32_t* d_rows, float* d_nll, float* d_dWp1, float* d_dbp1,
                            float* d_dG1, void* d_ws, size_t ws_bytes, float* d_dbg_logits, void* stream);
int nrhip_vae_mid_backward(int batch, int h, int z, int act, float anneal, const float* d_dG1,
                           const float* d_G1, const float* d_H1, const float* d_MU,
                           const float* d_LOGVAR, const float* d_EPSSTD, const float* d_ZS,
                           const float* d_Wp0, const float* d_Wq1, float* d_DA3, float* d_DH2,
                           float* d_DA1, float* d_dWp0, float* d_dbp0, float* d_dWq1,
                           float* d_dbq1, float* d_dbq0, void* stream);
int nrhip_vae_dwq0(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows,
                   int batch, int h, const float* d_h0val, const float* d_DA1, float* d_dWq0,
                   void* stream);
/* y += a*x ; *d_out += sum(x*x) (fp64) ; *d_out = mean(x) */
int nrhip_axpy(float a, const float* d_x, float* d_y, int64_t n, void* stream);
int nrhip_sumsq_accumulate(const float* d_x, int64_t n, double* d_out, void* stream);
int nrhip_mean_f32(const float* d_x, int n, float* d_out, void* stream);
int nrhip_mean2_f32(const float* d_x, const float* d_y, int n, float* d_out, void* stream);   /* out[0], out[1]: two means, one launch */

/* The narrow Mult-VAE step (one sess.run((loss, optimizer)) of MultiVAE.py:73-139) as one call: nrhip_vae_encode,
 * nrhip_vae_decoder_fused, nrhip_vae_mid_backward, nrhip_vae_dwq0, [nrhip_mean2_f32 -> d_stats = (neg_ll, KL); the L2
 * terms into d_regsum] and nrhip_adam_dense_tf_multi issued back to back.  P / G / M / V / sizes: the eight variables in
 * the order W_q0, b_q0, W_q1, b_q1, W_p0, b_p0, W_p1^T (item-major), b_p1 (host arrays of device pointers).  The
 * per-batch buffers hold max_batch rows; d_drop_given / d_eps_given (tests) may be NULL. */
typedef struct nrhip_vae_step_args {
  const int64_t* d_indptr; const int32_t* d_indices;   /* train CSR: the users' rows are the network's input */
  int n_items, h, z, act;
  float* P[8]; float* G[8]; float* M[8]; float* V[8]; int64_t sizes[8];
  float *d_H1, *d_MU, *d_LOGVAR, *d_EPSSTD, *d_ZS, *d_G1, *d_KLb, *d_h0val;
  float *d_nll, *d_dG1, *d_DA3, *d_DH2, *d_DA1;
  float* d_stats; double* d_regsum;
  void* d_ws; size_t ws_bytes;                        /* nrhip_vae_decoder_fused_workspace_bytes(max_batch, n_items) */
  const float* d_drop_given; const float* d_eps_given;
  float reg, beta1, beta2, adam_eps;
  uint64_t seed;
} NrhipVaeStep;
int nrhip_vae_step(const NrhipVaeStep* args, const int32_t* d_rows, int batch, float anneal, float keep,
                   float adam_alpha, uint64_t step, int want_loss, int apply, void* stream);

/* BPR-MF step in ONE launch: the gradient of MF.py:57-72 + TF-1.12 sparse Adam (util/learner.py:9-10) by
 * exact lazy replay, bit-identical to nrhip_bpr_mf_grad + nrhip_adam_sparse_tf.  Two copies of every table
 * and a stamp per copy (d_tw int32 [rows][2], {0, -1} before step 1): readers of step t take the newer copy
 * older than t, the head of a row writes the other one.  d_inb int32 [rows] (zero before step 1) marks the
 * rows of the coming batch.  d_plan is required; batch_marked != 0 promises that the previous call (step
 * t - 1) received exactly this plan as its d_next_plan. */
int nrhip_bpr_mf_step_fused(float* d_W, float* d_M, float* d_V, int32_t* d_tw, int32_t* d_inb,
                            const float* d_alpha_tab, int t, float beta1, float beta2, float eps, int d,
                            int n_users, int n_items, const int32_t* d_users, const int32_t* d_pos,
                            const int32_t* d_neg, int batch, float reg, float* d_work, float* d_loss2,
                            const uint64_t* d_plan, int batch_marked, const uint64_t* d_next_plan,
                            int n_next_occ, int period, void* stream);
/* every row brought to step t, in copy 0 (copy 1 invalidated) */
int nrhip_bpr_mf_fused_flush(float* d_W, float* d_M, float* d_V, int32_t* d_tw, const float* d_alpha_tab,
                             int t, float beta1, float beta2, float eps, int d, int64_t n_rows, void* stream);
/* ---- the other losses and optimisers of util/learner.py (MF.py:62-76 with is_pairwise /
 * loss_function / learner other than bpr + adam) ----------------------------------------------
 * Same contract as nrhip_bpr_mf_grad (dense d_GP/d_GQ zero outside the batch rows, d_work scratch of
 * 8*batch floats, optional d_plan, d_loss2 = {data loss, reg * l2}).
 *   pairwise loss_kind  (learner.py:19-29):  0 bpr  1 hinge = sum max(y+1, 0)  2 square = sum (1-y)^2
 *   pointwise loss_kind (learner.py:31-41):  0 cross_entropy = tf.losses.sigmoid_cross_entropy (batch
 *                        MEAN)  1 square = sum (label - x)^2;  instances are (user, item, label) as
 *                        PointwiseSampler yields them (data/sampler.py:93-155); regulariser
 *                        l2_loss(p, q) (MF.py:71-72).
 * nrhip_optimizer_rows_tf applies the TF-1.12 *sparse* update of learner.py:2-16 to the rows flagged
 * in d_row_flag (set with nrhip_mark_rows; cleared again here, like the gradient rows):
 *   kind 0 gd; 1 adagrad (slot0 = accumulator, initialise to 1e-8); 2 rmsprop (slot0 = ms
 *   initialised to 1, slot1 = mom initialised to 0, hyper1 = decay 0.9, hyper2 = momentum 0,
 *   eps 1e-10); 3 momentum (slot0 = accumulator, hyper1 = momentum 0.9). */
int nrhip_pairwise_mf_grad(const float* d_P, const float* d_Q, int d, int n_users,
                           const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                           int batch, float reg, int loss_kind, float* d_GP, float* d_GQ,
                           float* d_work, float* d_loss2, const uint64_t* d_plan, void* stream);
int nrhip_pointwise_mf_grad(const float* d_P, const float* d_Q, int d, int n_users,
                            const int32_t* d_users, const int32_t* d_items, const float* d_labels,
                            int batch, float reg, int loss_kind, float* d_GP, float* d_GQ,
                            float* d_work, float* d_loss2, const uint64_t* d_plan, void* stream);
int nrhip_mark_rows(const int32_t* d_ids, int n, int offset, uint8_t* d_flag, void* stream);
/* d_dst[i] = d_src[d_index[i]]: a row flag per VIRTUAL row of the chunked hop (nrhip_spmm_csr_carry) */
int nrhip_gather_u8(const uint8_t* d_src, const int32_t* d_index, int64_t n, uint8_t* d_dst, void* stream);
/* Ordered sums of gradient rows that arrive from other ranks (row-sharded tables): sort the
 * keys (local row << 32 | global occurrence position; any n: one LDS workgroup up to 16384 keys, the
 * segmented multi-workgroup network beyond), then every row's run
 * is added in key order and stored, exactly the order of the single-process head on the global batch.
 * d_index_of_pos[position] = index of that occurrence's row in d_src. */
int nrhip_sort_u64(uint64_t* d_keys, int n, void* stream);
/* Routing of a batch's 3*batch row lookups over block-partitioned tables (neurec_amd/parallel.py:
 * BipartitePartition — rank r owns users [r*bu, (r+1)*bu) and items [r*bi, (r+1)*bi), bu + bi rows per rank):
 *   nrhip_route_batch   requests in owner order, stable in request order (users, then positives, then negatives):
 *                       d_packed[i] = (row in the owner's block, occurrence code = class*code_base + position in this
 *                       rank's batch), d_order[i] = the request (class*batch + b) routed at i, d_inv = its inverse,
 *                       d_counts[world] (optional) = requests per owner.  d_keys: scratch for 3*batch keys.
 *   nrhip_route_owner_keys   on the owner: sorted keys (row << 32 | position of the occurrence in the GLOBAL batch =
 *                       class*G + d_size_off[source rank] + position) of the n rows it was asked for (ordered by
 *                       source rank, d_recv_prefix[world+1] their offsets) and d_index_of_pos[position] = index of
 *                       that occurrence among the n — the inputs of nrhip_rows_sum_sorted, which then adds the
 *                       returning gradient rows in the order TF's unsorted_segment_sum walks the concatenated batch.
 * Nothing to route is a valid call: with batch == 0 nrhip_route_batch takes NULL for the three id arrays and for
 * d_keys / d_packed / d_order / d_inv, touches none of them and still ZEROES d_counts (an empty batch asks every owner
 * for nothing); with n == 0 nrhip_route_owner_keys takes NULL for d_rows / d_codes / d_keys_out and writes nothing, and
 * nrhip_rows_sum_sorted / nrhip_rows_sum_sorted2 take NULL for d_sorted_keys and the d_src arrays and write nothing. */
int nrhip_route_batch(const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int batch, int n_users,
                      int bu, int bi, int code_base, uint64_t* d_keys, int32_t* d_packed, int32_t* d_order,
                      int32_t* d_inv, int32_t* d_counts, int world, void* stream);
int nrhip_route_owner_keys(const int32_t* d_rows, const int32_t* d_codes, int n, const int32_t* d_recv_prefix,
                           const int32_t* d_size_off, int world, int global_batch, int code_base,
                           uint64_t* d_keys_out, int32_t* d_index_of_pos, void* stream);
/* The same two tables for EVERY batch of an epoch stream at once (the ids of an epoch are known when it starts —
 * data/sampler.py:196-213 draws them up front): a step then issues no routing launch at all.
 *   nrhip_sort_u64_segments        n_segs independent segments sorted in one launch (each <= 16384 keys)
 *   nrhip_route_epoch              batch k's requests live in slot [3*batch*k, 3*batch*(k+1)) of d_keys / d_packed /
 *                                  d_order / d_inv (d_seg_off[k] = 3*batch*k, d_seg_len[k] = 3 * that batch's length);
 *                                  d_counts [n_batches][world]
 *   nrhip_route_epoch_owner_keys   the received stream laid out [batch][source rank]: d_asked_off / d_asked_len per
 *                                  batch, d_batch_of[j], per batch d_recv_prefix [world + 1], d_size_off [world],
 *                                  d_global_len; d_index_of_pos has iop_stride entries per batch */
int nrhip_sort_u64_segments(uint64_t* d_keys, const int64_t* d_seg_off, const int32_t* d_seg_len, int n_segs,
                            int max_len, void* stream);
int nrhip_route_epoch(const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg, int64_t n, int batch,
                      int n_users, int bu, int bi, int code_base, int world, uint64_t* d_keys, int32_t* d_packed,
                      int32_t* d_order, int32_t* d_inv, int32_t* d_counts, const int64_t* d_seg_off,
                      const int32_t* d_seg_len, void* stream);
int nrhip_route_epoch_owner_keys(const int32_t* d_rows, const int32_t* d_codes, const int32_t* d_batch_of, int64_t n,
                                 const int64_t* d_asked_off, const int32_t* d_asked_len, int n_batches, int max_asked,
                                 const int32_t* d_recv_prefix, const int32_t* d_size_off,
                                 const int32_t* d_global_len, int world, int code_base, int64_t iop_stride,
                                 uint64_t* d_keys_out, int32_t* d_index_of_pos, void* stream);
int nrhip_rows_sum_sorted(const uint64_t* d_sorted_keys, int n, const int32_t* d_index_of_pos, int d,
                          const float* d_src, int64_t ld_src, float* d_dst, void* stream);
int nrhip_rows_sum_sorted2(const uint64_t* d_sorted_keys, int n, const int32_t* d_index_of_pos, int d,
                           const float* d_src_a, int64_t ld_a, float* d_dst_a, const float* d_src_b, int64_t ld_b,
                           float* d_dst_b, void* stream);                          /* two tables, same runs, one launch */
int nrhip_optimizer_rows_tf(int kind, float* d_var, float* d_slot0, float* d_slot1, float* d_grad,
                            uint8_t* d_row_flag, int64_t n_rows, int d, float lr, float hyper1,
                            float hyper2, float eps, void* stream);
/* The DENSE updates of learner.py:2-17 — a variable with a consumer that is not a gather (NGCF's and Mult-VAE's
 * tables and weights) gets TF-1.12's Apply* kernels (training_ops.cc): kinds, slots and hyper-parameters as above
 * (rmsprop in ApplyRMSProp's form: ms += (g² - ms)(1 - rho); mom = mom·momentum + g·lr / sqrt(eps + ms)).
 * clear_grad: zero the gradient once consumed. */
int nrhip_optimizer_dense_tf(int kind, float* d_var, float* d_slot0, float* d_slot1, float* d_grad, int64_t n,
                             float lr, float hyper1, float hyper2, float eps, int clear_grad, void* stream);

/* Row lookups of a row-sharded table (BASELINE config 4; the reference's tf.nn.embedding_lookup of
 * LightGCN.py:99-104 and its IndexedSlices gradient when the rows live on another rank):
 * d_dst[w][0..d) = d_src[d_rows[w]][0..d) (d_dst row stride ld_dst), and the reverse
 * d_dst[d_rows[w]] += d_src[w] (fp32 atomics, repeats summed). */
int nrhip_rows_gather(const int32_t* d_rows, int n_listed, int d, const float* d_src, float* d_dst,
                      int64_t ld_dst, void* stream);
int nrhip_rows_gather_ld(const int32_t* d_rows, int n_listed, int d, const float* d_src, int64_t ld_src,
                         float* d_dst, int64_t ld_dst, void* stream);
/* two tables, one row list, one launch: d_dst_a[w] = d_src_a[d_rows[w]], d_dst_b[w] = d_src_b[d_rows[w]] */
int nrhip_rows_gather2(const int32_t* d_rows, int n_listed, int d, const float* d_src_a, int64_t ld_a,
                       const float* d_src_b, int64_t ld_b, float* d_dst_a, int64_t ldd_a, float* d_dst_b,
                       int64_t ldd_b, void* stream);   /* d_src rows ld_src floats apart */
int nrhip_rows_scatter_add(const int32_t* d_rows, int n_listed, int d, const float* d_src,
                           int64_t ld_src, float* d_dst, void* stream);

/* y = a*x (+ y0)  elementwise helpers used between propagation passes. */
int nrhip_scale(const float* d_x, float a, float* d_y, int64_t n, void* stream);
int nrhip_add(const float* d_x, const float* d_y, float* d_out, int64_t n, void* stream);
int nrhip_div_scalar(const float* d_x, float denom, float* d_y, int64_t n, void* stream);
/* the same on row-strided [rows][cols] views (column blocks of a wider matrix) */
int nrhip_add2d(const float* d_x, int64_t ldx, const float* d_y, int64_t ldy, float* d_out,
                int64_t ldo, int64_t rows, int cols, void* stream);
int nrhip_copy2d(const float* d_x, int64_t ldx, float* d_out, int64_t ldo, int64_t rows, int cols,
                 void* stream);

/* ---- NGCF: forward pass and whole training step issued natively ----------------------------------
 * The launch sequence of NGCF._create_ngcf_embed + the BPR head + its gradient + Adam on every trainable
 * (model/general_recommender/NGCF.py:91-110,160-202) as ONE call each: a Python loop issues the ~27
 * launches of a step in ~270 us, more than they take on the GPU.  The context records caller-owned device
 * pointers only.  n_layers <= NRHIP_NGCF_MAX_LAYERS; layer width d = 16. */
#define NRHIP_NGCF_MAX_LAYERS 4
typedef struct nrhip_ngcf_buffers {
  const void* plan; const void* plan_t;                                     /* SpMM plans of A and A^T */
  const int64_t* indptr;  const int32_t* indices;  const float* vals;
  const int64_t* indptr_t; const int32_t* indices_t; const float* vals_t;
  void* spmm_ws; size_t spmm_ws_bytes;
  float* E0; float* mE; float* vE; float* gE0;                              /* [n_nodes][d] */
  float* Out; float* dOut;                                                  /* [n_nodes][d * (n_layers + 1)] */
  float* S[NRHIP_NGCF_MAX_LAYERS]; float* ego[NRHIP_NGCF_MAX_LAYERS + 1];   /* ego[0] == E0 */
  uint8_t* mask[NRHIP_NGCF_MAX_LAYERS];
  float* W[NRHIP_NGCF_MAX_LAYERS][4]; float* gW[NRHIP_NGCF_MAX_LAYERS][4];  /* W_gc, b_gc, W_bi, b_bi */
  float* mW[NRHIP_NGCF_MAX_LAYERS][4]; float* vW[NRHIP_NGCF_MAX_LAYERS][4];
  float* dS; float* dEd; float* dT1; float* dT2; float* dEgo[2];
  float* terms; int32_t* rows; uint8_t* flag; void* ws; size_t ws_bytes;
  int n_users; int n_nodes; int d; int n_layers; int max_batch;
  float reg; float keep;
} nrhip_ngcf_buffers;
int nrhip_ngcf_ctx_create(const nrhip_ngcf_buffers* bufs, void** ctx_out);
int nrhip_ngcf_ctx_destroy(void* ctx);
/* Out = concat(E0, out_1 .. out_L); masks drawn from (seed, step_counter, layer) unless mask_given */
int nrhip_ngcf_forward(void* ctx, uint64_t seed, uint64_t step_counter, int mask_given, void* stream);
/* forward + BPR head on the rows of Out + backward + dense TF Adam on E0 and the 4 * L weights */
int nrhip_ngcf_step(void* ctx, const int32_t* d_users, const int32_t* d_pos, const int32_t* d_neg,
                    int batch, const uint64_t* d_plan, uint64_t seed, uint64_t step_counter,
                    int mask_given, float alpha, float beta1, float beta2, float eps, float* d_loss2,
                    void* stream);

/* ---- NGCF layers of any width (NGCF.py:31-33,271-286; csrc/ngcf_wide.hip) — the row-wise pieces a layer needs next to
 * nrhip_spmm_csr and nrhip_gemm_kmajor; neurec_amd/ngcf_wide.py strings them (widths 1..256). */
int nrhip_ew_mul(const float* d_a, int64_t lda, const float* d_b, int64_t ldb, int64_t rows, int cols, float* d_out,
                 int64_t ldo, void* stream);                                            /* bi = E .* S (NGCF.py:185) */
int nrhip_ngcf_act_fwd(const float* d_T1, const float* d_T2, int64_t ldt, int64_t n_rows, int w, int w_pad,
                       float keep, uint8_t* d_mask_io, int mask_given, uint64_t seed, uint64_t step, int layer,
                       float* d_ego_out, int64_t lde, float* d_out, int64_t ldo, void* stream);   /* NGCF.py:181-198 */
int nrhip_ngcf_act_bwd(const float* d_dout, int64_t ldo, const float* d_dego_next, int64_t ldn,
                       const float* d_ego_next, int64_t lde, const float* d_T1, const float* d_T2, int64_t ldt,
                       const uint8_t* d_mask, int64_t n_rows, int w, float keep, float* d_dT1, float* d_dT2,
                       void* stream);
int nrhip_ngcf_mix_bwd(const float* d_Y1, const float* d_Y2, int64_t ldy, const float* d_ego, const float* d_S,
                       int64_t lde, int64_t n_rows, int w, int w_pad, float* d_dS, float* d_dego_direct,
                       void* stream);

/* NGCF's other conf-surface branches (r05): alg_type = gcn / gcmc (NGCF.py:204-248 — a layer is leaky_relu(S W_gc + b_gc)
 * with message dropout, gcmc adds a dense layer on top and concatenates only those) and node dropout of the adjacency
 * (NGCF.py:162-164,334-362).  The products are nrhip_spmm_csr / nrhip_gemm_f32; these are the element-wise pieces:
 *   nrhip_lrelu_drop_fwd   y = (flags & 1 ? leaky_relu(T) : T); (flags & 2): y = mask ? y / keep : 0 (mask read when
 *                          mask_given, else drawn from (seed, step, layer) and written); d_out_a [n_rows][lda] padded with
 *                          zeros to w_pad (the next hop's operand), d_out_b [n_rows][ldb] the w real columns; either NULL
 *   nrhip_lrelu_drop_bwd   dT[n_rows][w] = (d_a + d_b) through the same ops backwards (d_b optional)
 *   nrhip_edge_dropout     out[e] = keep_e ? vals[e] * (1 / keep) : 0 over the stored entries (sparse_retain + scale);
 *                          keep_e read (given) or drawn from (seed, step) and written
 *   nrhip_gather_f32       dst[e] = src[index[e]] (the transposed matrix takes the same draw) */
int nrhip_lrelu_drop_fwd(const float* d_T, int64_t ldt, int64_t n_rows, int w, int w_pad, float keep, uint8_t* d_mask_io,
                         int mask_given, uint64_t seed, uint64_t step, int layer, int flags, float* d_out_a, int64_t lda,
                         float* d_out_b, int64_t ldb, void* stream);
int nrhip_lrelu_drop_bwd(const float* d_da, int64_t lda, const float* d_db, int64_t ldb, const float* d_T, int64_t ldt,
                         const uint8_t* d_mask, int64_t n_rows, int w, float keep, int flags, float* d_dT, void* stream);
int nrhip_edge_dropout(const float* d_vals, int64_t n, float keep, uint8_t* d_keep_io, int given, uint64_t seed,
                       uint64_t step, float* d_out, void* stream);
int nrhip_gather_f32(const float* d_src, const int32_t* d_index, int64_t n, float* d_dst, void* stream);

/* The width-generic NGCF forward pass and training step as ONE call each (neurec_amd/ngcf_wide.py strung them from
 * ~70 Python-issued launches: 1.0 ms a step at 64 / [64, 64, 64], of which the GPU was busy 0.45).  The struct
 * records caller-owned device pointers; per layer k: widths w[k] -> w[k+1] (wp = padded to the SpMM's row widths),
 * off[k] = first column of layer k's block in the concatenated output. */
#define NRHIP_NGCF_WIDE_MAX_LAYERS 8
typedef struct {
  const void* plan; const int64_t* indptr; const int32_t* indices; const float* vals;           /* A_hat */
  const void* plan_t; const int64_t* indptr_t; const int32_t* indices_t; const float* vals_t;   /* A_hat^T */
  void* ws_fwd[NRHIP_NGCF_WIDE_MAX_LAYERS]; size_t ws_fwd_bytes[NRHIP_NGCF_WIDE_MAX_LAYERS];     /* SpMM scratch per layer */
  void* ws_bwd[NRHIP_NGCF_WIDE_MAX_LAYERS]; size_t ws_bwd_bytes[NRHIP_NGCF_WIDE_MAX_LAYERS];
  int n_users, n_nodes, n_layers, max_batch, dsum, splits;
  int w[NRHIP_NGCF_WIDE_MAX_LAYERS + 1], wp[NRHIP_NGCF_WIDE_MAX_LAYERS + 1], off[NRHIP_NGCF_WIDE_MAX_LAYERS + 2];
  float *E0p, *mE, *vE, *gE0, *Out, *dOut;
  float* ego[NRHIP_NGCF_WIDE_MAX_LAYERS + 1];
  float *S[NRHIP_NGCF_WIDE_MAX_LAYERS], *X2[NRHIP_NGCF_WIDE_MAX_LAYERS], *T1[NRHIP_NGCF_WIDE_MAX_LAYERS],
      *T2[NRHIP_NGCF_WIDE_MAX_LAYERS];
  uint8_t* mask[NRHIP_NGCF_WIDE_MAX_LAYERS];
  float *W[NRHIP_NGCF_WIDE_MAX_LAYERS][4], *gW[NRHIP_NGCF_WIDE_MAX_LAYERS][4], *mW[NRHIP_NGCF_WIDE_MAX_LAYERS][4],
      *vW[NRHIP_NGCF_WIDE_MAX_LAYERS][4];
  float *dS[NRHIP_NGCF_WIDE_MAX_LAYERS], *dEd[NRHIP_NGCF_WIDE_MAX_LAYERS], *dEgo[NRHIP_NGCF_WIDE_MAX_LAYERS];
  float *dT1, *dT2, *Y1, *Y2, *terms, *cs_ws;
  size_t cs_ws_bytes;
  int32_t* rows; uint8_t* flag;
  void* gemm_ws; size_t gemm_ws_bytes;
  float reg, keep;
} nrhip_ngcf_wide_buffers;
/* forward (NGCF.py:160-202): fills Out; masks_given != 0: mask[k] hold the dropout masks, else they are drawn
 * from (seed, step) and stored there */
int nrhip_ngcf_wide_forward(const nrhip_ngcf_wide_buffers* b, int masks_given, uint64_t seed, uint64_t step,
                            void* stream);
/* forward + BPR head (NGCF.py:91-110) + backward + dense TF-Adam on the ego table and every layer weight */
int nrhip_ngcf_wide_step(const nrhip_ngcf_wide_buffers* b, const int32_t* d_users, const int32_t* d_pos,
                         const int32_t* d_neg, int batch, const uint64_t* d_plan, int masks_given, uint64_t seed,
                         uint64_t step, float alpha, float beta1, float beta2, float eps, float* d_loss2,
                         void* stream);

/* ---- Mult-VAE for any p_dim (conf/MultiVAE.properties:3: [200, 600], [200]; MultiVAE.py:46-135 builds q / p networks
 * of arbitrary depth and width) — width-generic pieces (csrc/vae_wide.hip) + a general fp32-MFMA GEMM (csrc/gemm.hip).
 * act: 0 tanh, 1 sigmoid, 2 relu, 3 identity, -1 none.  neurec_amd/vae_wide.py strings them into a step. */
/* C[m][n] (+)= sum_k A[k][m] * B[k][n]; A [K][lda], B [K][ldb] (contraction index slow), C [M][ldc]; every element the
 * k-ascending fmaf chain (continued from C when accumulate); splits > 1 cuts K into ranges whose partial products
 * (d_ws: nrhip_gemm_workspace_bytes) are added in order.  Epilogue: + d_bias_n[n] (NULL: none), then `act` (-1: none) —
 * a dense layer y = act(x W + b) is one call with A = x^T.  lda, ldb < 2^24 elements (operand rows are addressed through
 * buffer resources with 32-bit byte offsets); K = 0 leaves C (+)= 0 followed by the epilogue. */
int nrhip_gemm_workspace_bytes(int M, int N, int splits, size_t* bytes);
/* the general form: either operand k-major ([K][ld], a_kminor / b_kminor = 0) or k-minor ([M][ld] / [N][ld], the
 * contraction index contiguous, = 1; such an operand must stay below 2 GB) — x W, x W^T, x^T g without a transposed
 * copy of anything */
int nrhip_gemm_f32(const float* d_A, int64_t lda, int a_kminor, const float* d_B, int64_t ldb, int b_kminor, int M,
                   int N, int K, float* d_C, int64_t ldc, int accumulate, const float* d_bias_n, int act, int splits,
                   void* d_ws, size_t ws_bytes, void* stream);
int nrhip_gemm_kmajor(const float* d_A, int64_t lda, const float* d_B, int64_t ldb, int M, int N, int K, float* d_C,
                      int64_t ldc, int accumulate, const float* d_bias_n, int act, int splits, void* d_ws,
                      size_t ws_bytes, void* stream);
int nrhip_transpose2d(const float* d_src, int64_t ld_src, int rows, int cols, float* d_dst, int64_t ld_dst,
                      void* stream);
/* first encoder layer straight from the train CSR (tf.nn.l2_normalize + tf.nn.dropout + the first tf.matmul of
 * q_graph, MultiVAE.py:76-80): Y[b] = act(sum over the row's items of (1/sqrt(n)/keep*mask) * W[item] + bias);
 * d_h0val (per CSR position, optional) keeps the values for nrhip_vae_dwq0_wide.  One grid row per batch row: this
 * call and nrhip_vae_dwq0_wide take batch <= 65535 (above: NRHIP_ERR_UNSUPPORTED, nothing is launched).  The kernel
 * entry points of this group and the row-wise ones of the NGCF group accept empty work (batch, n or rows = 0) with the
 * NULL pointers of empty tensors; nrhip_gemm_f32 reads neither A nor B when K = 0. */
int nrhip_vae_bag_fwd(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows, int batch,
                      int width, const float* d_W, const float* d_bias, int act, float keep,
                      const float* d_drop_given, uint64_t seed, uint64_t step, float* d_h0val, float* d_Y,
                      void* stream);
int nrhip_act_bwd(const float* d_dY, const float* d_Y, int64_t n, int act, float* d_dA, void* stream);
int nrhip_vae_sample(const float* d_H2, int batch, int z, const float* d_eps_given, float is_training, uint64_t seed,
                     uint64_t step, float* d_EPSSTD, float* d_ZS, float* d_KLb, void* stream);
int nrhip_vae_sample_bwd(const float* d_dZ, const float* d_H2, const float* d_EPSSTD, int batch, int z, float anneal,
                         float* d_dH2, void* stream);
int nrhip_vae_softmax_dlogits(float* d_S, int64_t ld, int batch, int cols, const int64_t* d_indptr,
                              const int32_t* d_indices, const int32_t* d_rows, float* d_nll, void* stream);
/* d_out[c] = sum_r d_X[r][c] (bias gradients), a fixed association; rows > 2048: d_ws of ceil(rows / 512) * cols floats */
int nrhip_colsum_rows(const float* d_X, int64_t ld, int rows, int cols, float* d_out, void* d_ws, size_t ws_bytes,
                      void* stream);
int nrhip_vae_dwq0_wide(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows, int batch,
                        int width, const float* d_h0val, const float* d_DA1, float* d_dWq0, void* stream);

/* ---- WRMF (implicit ALS) ---------------------------------------------------
 * Replaces: the per-row update_user / update_item solves of WRMF.py:47-59 (one tf.linalg.solve + scatter_update per
 * row, driven by train_model, WRMF.py:66-84).  A half-sweep solves, for every row u of one side, against the other
 * side's table Y [n_other][d]:
 *     (Y^T Y + alpha sum_{j in N(u)} y_j y_j^T + lambda I) x_u = (1 + alpha) sum_{j in N(u)} y_j
 * N(u) = the row's columns in the train CSR (only the pattern counts: Pui = 1, Cui = alpha).  A row without columns
 * gets x = 0.  d = 1..128 (above: NRHIP_ERR_UNSUPPORTED); lambda > 0 and alpha >= 0 (else NRHIP_ERR_ARG).  Every sum
 * is taken in a fixed order: results are bit-identical from run to run. */
#define NRHIP_WRMF_CHUNK 1024 /* neighbour lists longer than this are accumulated in chunks of this many */
/* Host-side chunk plan of a CSR (h_indptr: n_rows + 1 entries, host memory): h_row_chunk[r] = index of row r's first
 * chunk, or -1 for rows of at most NRHIP_WRMF_CHUNK columns; h_chunk_row[c] = the row of chunk c (a row's chunks are
 * consecutive, in list order).  Either array may be NULL (call once with both NULL to learn *n_chunks). */
int nrhip_wrmf_chunk_plan(const int64_t* h_indptr, int n_rows, int32_t* h_row_chunk, int32_t* h_chunk_row,
                          int* n_chunks);
/* Scratch for nrhip_wrmf_gram and for nrhip_wrmf_solve with n_chunks chunks (one buffer serves both). */
int nrhip_wrmf_workspace_bytes(int d, int n_chunks, size_t* bytes);
/* d_G [d][d] = d_Y^T d_Y over the n rows of d_Y [n][d] (YTY / XTX, WRMF.py:47 / 54). */
int nrhip_wrmf_gram(const float* d_Y, int n, int d, float* d_G, void* d_ws, size_t ws_bytes, void* stream);
/* The half-sweep: d_X [n_rows][d] row u = the solve above, rows u of the CSR (d_indptr int64, d_indices int32 column
 * ids < n_other), d_G from nrhip_wrmf_gram of the same d_Y; d_row_chunk / d_chunk_row: the chunk plan of this CSR
 * (device copies; may be NULL when n_chunks = 0).  d_X must not alias d_Y. */
int nrhip_wrmf_solve(const int64_t* d_indptr, const int32_t* d_indices, int n_rows, const float* d_Y, int n_other,
                     const float* d_G, int d, float alpha, float lambda, const int32_t* d_row_chunk,
                     const int32_t* d_chunk_row, int n_chunks, float* d_X, void* d_ws, size_t ws_bytes,
                     void* stream);

/* ---- ItemKNN (item-based nearest neighbours) ------------------------------
 * Replaces: Compute_Similarity_Python.compute_similarity (ItemKNN.py:395-547), Compute_Similarity_Euclidean.
 * compute_similarity (ItemKNN.py:60-214) and the dense scores `train_matrix.dot(W_sparse).toarray()` (ItemKNN.py:573).
 * The train matrix R (n_users x n_items) comes in CSR and CSC form (the same pattern; indptr int64, ids int32) with
 * the value arrays the similarity works on (raw ratings; mean-centred for adjusted / pearson; 1 for jaccard / dice /
 * tversky) and two per-item arrays:
 *     kind 0  cosine family   d_na = d_nb = sqrt(sumOfSquared); asymmetric: d_na = s^(2 alpha), d_nb = s^(2 (1 - alpha))
 *                             w = c / (na[i] nb[j] + shrink + 1e-6)                                (ItemKNN.py:478-484)
 *     kind 1  tanimoto        d_na = sumOfSquared;  w = c / (na[i] + na[j] - c + shrink + 1e-6)    (ItemKNN.py:488-490)
 *     kind 2  dice            d_na = sumOfSquared;  w = c / (na[i] + na[j] + shrink + 1e-6)        (ItemKNN.py:492-494)
 *     kind 3  tversky         d_na = sumOfSquared;  w = c / (c + (na[i] - c) ta + (na[j] - c) tb + shrink + 1e-6)
 *                                                                                                  (ItemKNN.py:496-500)
 *     kind 4  euclidean       d_na = sumOfSquared, d_nb = its square root;
 *                             w = 1 / (sqrt((na[i] + na[j] - 2 c) / (nb[i] nb[j])) + shrink + 1e-9) (ItemKNN.py:146-181)
 * with c = sum_u r_ui r_uj for column i (the diagonal is 0, ItemKNN.py:474 / 181).  The I x I matrix is never formed:
 * a column's accumulator lives in LDS when n_items <= NRHIP_ITEMKNN_LDS_ITEMS, in a row of the workspace slab
 * [block_cols][n_items] otherwise; columns are processed block_cols at a time.
 * Selection (ItemKNN.py:513-523): the min(neighbor, n_items) largest entries of the column, exact zeros dropped.
 * TIE RULE: the larger value wins; among equal values the LOWER item index wins (the reference's order among equal
 * values is whatever argpartition leaves).  A column's list is stored in that order.
 * Euclidean: a pair of items one or both of which have no interactions scores 0 (the reference: 0 and NaN) and is
 * never stored.
 * Output: d_w_idx / d_w_val [n_items][neighbor] (column i's neighbours j and W[j][i]; unused slots -1 / 0), d_w_cnt
 * [n_items]; and W^T in CSR form for the scoring: d_t_indptr [n_items + 1], d_t_cols / d_t_vals [n_items * neighbor]
 * (row j = the columns i whose list holds j, ascending i; the first d_t_indptr[n_items] entries are used).
 * neighbor = 1..NRHIP_ITEMKNN_MAX_NEIGHBOR and n_items * neighbor <= 2^29 (the transpose's key sort
 * keeps its padded count and strides in an int; above: NRHIP_ERR_UNSUPPORTED).  Every float sum is taken in a fixed
 * order: two builds are bit-identical, and so are two score calls. */
#define NRHIP_ITEMKNN_LDS_ITEMS 12288   /* the accumulator column stays in LDS up to this many items (48 KiB) */
#define NRHIP_ITEMKNN_MAX_NEIGHBOR 1024 /* conf/ItemKNN.properties names 5..800 */
int nrhip_itemknn_workspace_bytes(int n_items, int neighbor, int block_cols, size_t* bytes);
int nrhip_itemknn_build(const int64_t* d_csc_indptr, const int32_t* d_csc_users, const float* d_csc_vals,
                        const int64_t* d_csr_indptr, const int32_t* d_csr_items, const float* d_csr_vals,
                        const float* d_na, const float* d_nb, int n_users, int n_items, int kind, float shrink,
                        float tversky_alpha, float tversky_beta, int neighbor, int block_cols, int32_t* d_w_idx,
                        float* d_w_val, int32_t* d_w_cnt, int64_t* d_t_indptr, int32_t* d_t_cols, float* d_t_vals,
                        void* d_ws, size_t ws_bytes, void* stream);
/* d_S [batch][ld_s] (ld_s >= n_items, the leading dimension of the score slab), row b = sum_{j in N(u_b)} r_{u_b j}
 * W[j][:] (ItemKNN.py:573 for the users d_users only): the row is zeroed, then the history items are taken in CSR order
 * (d_csr_vals: the RAW ratings), each adding its row of W^T. */
int nrhip_itemknn_score(const int32_t* d_users, int batch, const int64_t* d_csr_indptr, const int32_t* d_csr_items,
                        const float* d_csr_vals, int n_users, int n_items, const int64_t* d_t_indptr,
                        const int32_t* d_t_cols, const float* d_t_vals, float* d_S, int64_t ld_s, void* stream);

/* ---- FISM (factored item similarity) ---------------------------------------
 * Replaces: FISM._create_inference / _create_loss / the optimizer's gradients (FISM.py:66-92) run by
 * `sess.run((self.loss, self.optimizer), feed_dict)` on histories padded to [B, Lmax] (FISM.py:119-139), and the
 * per-user `sess.run(self.output)` over num_items copies of the history in predict() (FISM.py:154-180).
 * An instance is (user u, item i, excluded item e or none, count n); H = the user's train row without e:
 *     p = sum_{h in H} c1[h]      out = n^-alpha (p . Q[i]) + bias[i]               (FISM.py:68-72)
 * The batch (d_users, d_items, d_third: `batch` entries each) expands as util/data_generator.py:29-54 states it:
 *     pointwise (d_third = float labels)  label 1: e = i, n = |R_u|;  label 0: e none, n = |R_u| + 1
 *         loss = pointwise_loss(kind, label, out) + reg_p l2_loss(p) + reg_q l2_loss(Q[i])        (FISM.py:86-88)
 *     pairwise  (d_third = int32 negatives j)  positive side (i, e = i, n = |R_u|), negative side (j, e none,
 *         n = |R_u| + 1); users with |R_u| <= 1 take no part (data_generator.py:13)
 *         loss = pairwise_loss(kind, out_pos - out_neg) + reg_p l2_loss(p_pos) + reg_q (l2_loss(Q[j]) + l2_loss(Q[i]))
 *                                                                                                 (FISM.py:79-83)
 * with l2_loss = sum(x^2) / 2 and the loss kinds of nrhip_pointwise_mf_grad / nrhip_pairwise_mf_grad.
 * Output: d_loss2 = (loss term, regulariser term); d_G_c1 [n_items][d] — EVERY row written, TF's gradient of c1 is
 * dense because c1 is read through tf.concat (FISM.py:61); d_G_Q [n_items][d] and d_G_bias [n_items] — the rows of the
 * batch's items only (sparse application, as embedding_lookup gives it), the other rows are left alone; d_flag_Q /
 * d_flag_bias (uint8 [n_items], may be NULL): set to 1 for those rows (nrhip_optimizer_rows_tf); d_flag_c1 (uint8
 * [n_items], may be NULL): set to 1 for every c1 row some instance of the batch pooled — for a caller that applies
 * c1 by rows instead.  A pair with a user or an item outside the tables takes no part, both sides.  batch <=
 * NRHIP_FISM_MAX_BATCH.
 * The train matrix comes twice: CSR (d_indptr int64 [n_users + 1], d_indices int32) and transposed (d_t_indptr
 * [n_items + 1], d_t_users ascending per item).  d_slot: int64 [n_users], zero before the first step; `step` >= 1 and
 * larger at every call on the same d_slot.  Work buffers for N = batch (pointwise) or 2 batch (pairwise) instances:
 * d_keys uint64 [2 N], d_inst int32 [4 N], d_n float [N], d_p / d_g float [N][d], d_scal float [8 N].
 * Any history length; d = 1..NRHIP_FISM_MAX_D (above: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed order
 * (the pooled sum in fp64 partials combined by a fixed tree), no floating-point atomics: two calls on the same
 * inputs are bit-identical. */
#define NRHIP_FISM_MAX_D 128
#define NRHIP_FISM_MAX_BATCH (1 << 24) /* 8 N work-buffer offsets stay inside an int for N = 2 batch */
typedef struct nrhip_fism_step_args {
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int64_t* d_t_indptr;
  const int32_t* d_t_users;
  const float* d_c1;
  const float* d_Q;
  const float* d_bias;
  float* d_G_c1;
  float* d_G_Q;
  float* d_G_bias;
  uint8_t* d_flag_Q;
  uint8_t* d_flag_bias;
  uint8_t* d_flag_c1;
  const int32_t* d_users;
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  int32_t* d_inst;
  float* d_n;
  float* d_p;
  float* d_g;
  float* d_scal;
  int64_t* d_slot;
  float* d_loss2;
  int n_users, n_items, d, batch, pairwise, loss_kind, step;
  float alpha, reg_p, reg_q;
} nrhip_fism_step_args;
int nrhip_fism_step(const nrhip_fism_step_args* args, void* stream);
/* The evaluation's user factors (FISM.py:154-180 scores every item against the user's WHOLE train row, n = |R_u|):
 * d_out [batch][ld] (ld >= d + 1), row b = [n^-alpha p_u | 1] for u = d_users[b] (d_users NULL: u = b), so that its
 * inner product with [Q[i] | bias[i]] is the reference's `output`.  A user without train items (or outside the
 * matrix) gets [0 | 1]: the bias alone (the reference raises KeyError there). */
int nrhip_fism_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, const float* d_c1, int d,
                            float alpha, const int32_t* d_users, int batch, float* d_out, int64_t ld, void* stream);

/* ---- NAIS (neural attentive item similarity) ---------------------------------
 * Replaces: NAIS._create_inference / _attention_mlp / _create_loss / the optimizer's gradients (NAIS.py:96-176) run by
 * `sess.run((self.loss, self.optimizer), feed_dict)` on histories padded to [B, Lmax] (NAIS.py:197-217), and the
 * per-user `sess.run(self.output)` over num_items copies of the history in predict() (NAIS.py:232-258).
 * Instances, batch fields, loss kinds, d_G_c1 / d_G_Q / d_G_bias, the flags, d_slot / step and the two forms of the
 * train matrix are nrhip_fism_step's; the rows of the CSR form must be ASCENDING.  With q = Q[i], per history item h_j:
 *     x_j = c1[h_j] (.) q (algorithm 0) or [c1[h_j], q] (algorithm 1)        z_j = x_j W + b      (NAIS.py:157)
 *     a_j = act(z_j) (activation 0 relu, 1 sigmoid, 2 tanh, other: identity)  (NAIS.py:158-163)
 *     e_j = exp(a_j . h)   S = sum e_j   A_j = e_j / S^beta   p = sum A_j c1[h_j]                 (NAIS.py:165-176)
 *     out = n^alpha (p . q) + bias[i]  — the exponent is +alpha                                  (NAIS.py:110-111)
 *     loss = the pointwise / pairwise loss + reg_p l2_loss(the gathered c1[h_j]) + reg_q l2_loss(Q[i]) (NAIS.py:121-128)
 * reference_mask != 0: an instance whose history is shorter than the longest of its side of the batch carries the
 * reference's padding term (sequence_mask(num_idx) covers one zero row): S += exp(h . act(b)) for algorithm 0,
 * exp(h . act(q W[d:2d] + b)) for algorithm 1, with its gradients.  reference_mask == 0: the softmax over H alone.
 * d_W [d][w] (algorithm 1: [2 d][w]), d_b [w], d_h [w]; d_G_W / d_G_b / d_G_h: their dense gradients.
 * Work buffers for N = batch (pointwise) or 2 batch (pairwise) instances: d_keys uint64 [2 N], d_inst int32 [4 N],
 * d_n float [N], d_p float [N][d], d_scal float [8 N], d_off int64 [N], d_dWp float [N][d w], d_dbp / d_dhp float
 * [N][w], d_dqp float [N][d], and d_rows float [row_cap][d]: the c1 row gradient of every history position of the
 * batch, row_cap >= the sum of the instances' train-row lengths.  d_need int64 [2]: the call stores that sum in
 * d_need[0] and keeps d_need[1] = the largest sum of any call (zero it once); positions beyond row_cap are not
 * written, so a caller that finds d_need[1] > row_cap has lost gradient rows and must treat it as an error.
 * c1_sort != 0: G_c1 is not taken by the walk over the transposed matrix but from d_pkeys uint64 [row_cap], the
 * (item | position) keys of the ragged buffer's rows, sorted, each item's run summed in position order (row_cap <
 * 2^31).  Both ways are fixed-order; their orders differ, so their sums may differ in the last bits.
 * d = 1..NRHIP_NAIS_MAX_D, w = 1..NRHIP_NAIS_MAX_W (above: NRHIP_ERR_UNSUPPORTED), beta >= 0.  Every sum is taken in a
 * fixed order, no floating-point atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_NAIS_MAX_D 128
#define NRHIP_NAIS_MAX_W 64
#define NRHIP_NAIS_MAX_BATCH (1 << 24)
typedef struct nrhip_nais_step_args {
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int64_t* d_t_indptr;
  const int32_t* d_t_users;
  const float* d_c1;
  const float* d_Q;
  const float* d_bias;
  const float* d_W;
  const float* d_b;
  const float* d_h;
  float* d_G_c1;
  float* d_G_Q;
  float* d_G_bias;
  float* d_G_W;
  float* d_G_b;
  float* d_G_h;
  uint8_t* d_flag_Q;
  uint8_t* d_flag_bias;
  uint8_t* d_flag_c1;
  const int32_t* d_users;
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  int32_t* d_inst;
  float* d_n;
  float* d_p;
  float* d_scal;
  int64_t* d_slot;
  int64_t* d_off;
  int64_t* d_need;
  uint64_t* d_pkeys;
  float* d_rows;
  float* d_dWp;
  float* d_dbp;
  float* d_dhp;
  float* d_dqp;
  float* d_loss2;
  int64_t row_cap;
  int n_users, n_items, d, w, batch, pairwise, loss_kind, step, algorithm, activation, reference_mask, c1_sort;
  float alpha, beta, reg_p, reg_q;
} nrhip_nais_step_args;
int nrhip_nais_step(const nrhip_nais_step_args* args, void* stream);
/* predict() (NAIS.py:232-258): d_out [batch][ld] (ld >= n_items), row b = the scores of every item for u = d_users[b]
 * on the user's WHOLE train row, the exact mask, n = |R_u|; a user without train items (or outside the matrix) gets
 * d_bias bit for bit (the reference raises KeyError).  e(i, h) does not depend on the user: per tile of `tile` target
 * items (a multiple of 256) e(i, h) and e(i, h)(c1[h] . Q[i]) are formed once for the distinct history items of the
 * block (at most h_cap: the caller's bound, min(n_items, the block's row lengths summed)) and summed per user in CSR
 * order.  Workspace: d_map / d_hs int32 [n_items], d_cnt int32 [1], d_E / d_F float [h_cap][tile]; algorithm 1:
 * d_cW / d_qW float [n_items][w] = c1 W[0:d] and Q W[d:2d] + b, made by the call when project != 0.
 * mfma != 0: the pair terms on the fp32 matrix cores (algorithm 0, d <= 16, w <= 16 only; else NRHIP_ERR_UNSUPPORTED). */
typedef struct nrhip_nais_scores_args {
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const float* d_c1;
  const float* d_Q;
  const float* d_bias;
  const float* d_W;
  const float* d_b;
  const float* d_h;
  const int32_t* d_users;
  float* d_out;
  int32_t* d_map;
  int32_t* d_hs;
  int32_t* d_cnt;
  float* d_E;
  float* d_F;
  float* d_cW;
  float* d_qW;
  int64_t ld;
  int n_users, n_items, d, w, algorithm, activation, batch, h_cap, tile, project, mfma;
  float alpha, beta;
} nrhip_nais_scores_args;
int nrhip_nais_scores(const nrhip_nais_scores_args* args, void* stream);

/* ---- FPMC (factorised personalised Markov chains) ------------------------------
 * Replaces: FPMC._create_inference / _create_loss / the optimizer's gradients (model/sequential_recommender/
 * FPMC.py:61-88) run by `sess.run((self.loss, self.optimizer), feed_dict)` (FPMC.py:111-128).
 * An instance is (user u, recent item l, item i[, negative j]):
 *     x(u, l, i) = <UI[u], IU[i]> + <IL[i], LI[l]>                                        (FPMC.py:64-69)
 *     pointwise (d_third = float labels)   loss = pointwise_loss(kind, label, x(u,l,i))
 *                                                 + reg l2_loss(UI[u], IU[i], IL[i], LI[l])              (FPMC.py:83-84)
 *     pairwise  (d_third = int32 negatives) loss = pairwise_loss(kind, x(u,l,i) - x(u,l,j))
 *                                                 + reg l2_loss(UI[u], IU[i], IL[i], LI[l], IU[j], IL[j]) (FPMC.py:77-80)
 * with l2_loss = sum(x^2) / 2 and the loss kinds of nrhip_pointwise_mf_grad / nrhip_pairwise_mf_grad (the pointwise
 * cross-entropy is the MEAN over `batch`).  UI[u] and LI[l] are regularised once per instance although the pairwise
 * graph looks them up in both inferences.
 * Output: d_loss2 = (loss term, regulariser term) of the tables as they come in; d_G_UI [n_users][d], d_G_IU / d_G_IL /
 * d_G_LI [n_items][d]: the rows the batch looked up are STORED (the others are left alone: keep them zero), each the
 * sum of its occurrences' gradients `g partner row + reg own row` in the order of nrhip_bpr_plan: by position in the
 * batch, the first inference's lookups (positions 0..batch) before the second's (batch..2 batch; UI and LI: the
 * gradient through the negative's score, without a regulariser term).  d_flag_* (uint8 per table row, may be NULL): set
 * to 1 for those rows (nrhip_optimizer_rows_tf).
 * A slot whose user is no row of UI or whose recent item, item or negative is outside [0, n_items) takes no part.
 * Work buffers: d_keys uint64 [3 N] for N = batch (pointwise) or 2 batch (pairwise), d_scal float [4 batch].
 * n_users + 2 n_items < 2^31; batch <= NRHIP_FPMC_MAX_BATCH; d = 1..NRHIP_FPMC_MAX_D (above: NRHIP_ERR_UNSUPPORTED).
 * Every sum is taken in a fixed order, no floating-point atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_FPMC_MAX_D 128
#define NRHIP_FPMC_MAX_BATCH (1 << 24)
typedef struct nrhip_fpmc_step_args {
  const float* d_UI;
  const float* d_IU;
  const float* d_IL;
  const float* d_LI;
  float* d_G_UI;
  float* d_G_IU;
  float* d_G_IL;
  float* d_G_LI;
  uint8_t* d_flag_UI;
  uint8_t* d_flag_IU;
  uint8_t* d_flag_IL;
  uint8_t* d_flag_LI;
  const int32_t* d_users;
  const int32_t* d_recent;
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  float* d_scal;
  float* d_loss2;
  int n_users, n_items, d, batch, pairwise, loss_kind;
  float reg;
} nrhip_fpmc_step_args;
int nrhip_fpmc_step(const nrhip_fpmc_step_args* args, void* stream);
/* The evaluation's user factors: d_out [batch][ld] (ld >= 2 d), row b = [UI[u] | LI[d_last[u]]] for u = d_users[b]
 * (d_users NULL: u = b), so that its inner product with [IU[i] | IL[i]] is x(u, last(u), i) (FPMC.py:140-152).
 * d_last int32 [n_users]: the user's most recent train item, -1 (or anything outside [0, n_items)): none — the second
 * half is zeros and the score <UI[u], IU[i]> alone.  A user outside [0, n_users) gets a row of zeros. */
int nrhip_fpmc_user_factors(const float* d_UI, const float* d_LI, int n_users, int n_items, int d,
                            const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                            void* stream);

/* ---- Fossil (FISM's long-term term + a personalised Markov term of order L) ------
 * Replaces: Fossil._create_inference / _create_loss / the optimizer's gradients (model/sequential_recommender/
 * Fossil.py:59-102) run by `sess.run((self.loss, self.optimizer), feed_dict)` on histories padded to [B, Lmax], and the
 * per-user `sess.run(self.output)` of predict() (Fossil.py:177-217).  These symbols are additions: no existing struct
 * changes and NRHIP_ABI_VERSION stays 4.
 * An instance is (user u, item i, excluded item e or none, count n, recents r_0..r_{L-1}); H = the train row without e:
 *     p = sum_{h in H} c1[h]     w_l = eta_bias[l] + eta[u][l]     s = sum_l w_l c1[r_l]
 *     out = n^-alpha (p . Q[i]) + (s . Q[i]) + bias[i]                                    (Fossil.py:76-85)
 * The batch (d_users, d_items, d_third: `batch` entries each; d_recents int32 [batch][L], MOST RECENT FIRST: column l
 * meets eta column l) expands as the reference's generators state it:
 *     pointwise (d_third = float labels)  label 1: e = i, n = |R_u| - 1;  label 0: e none, n = |R_u|
 *         loss = pointwise_loss(kind, label, out) + reg_p l2_loss(p) + reg_q l2_loss(Q[i], c1[r_.])
 *                + reg_eta l2_loss(eta[u], eta_bias)                                       (Fossil.py:99-102)
 *     pairwise  (d_third = int32 negatives j)  positive side (i, e = i, n = |R_u| - 1), negative side (j, e none,
 *         n = |R_u|), both on the slot's u and recents
 *         loss = pairwise_loss(kind, out_pos - out_neg) + reg_p l2_loss(p_pos) + reg_q l2_loss(Q[j], Q[i], c1[r_.])
 *                + reg_eta l2_loss(eta[u], eta_bias)                                       (Fossil.py:93-97)
 * c1[r_.] and eta[u] enter the regulariser once per pointwise instance / per pair, eta_bias once per CALL (also when
 * batch = 0).  A slot takes part only if its user and item(s) are table rows, |R_u| > L, and every one of its recents
 * is a train item of its user — a recent outside the user's train row (or outside [0, n_items)) takes the whole slot
 * out, both sides of a pair: the walk that sums G_c1 meets a recent through the train matrix, and no gradient is ever
 * dropped silently.  A recent may equal the slot's own item; one item may stand at several columns.
 * Tables: d_c1 / d_Q [n_items][d], d_bias [n_items], d_eta [n_users][L], d_eta_bias [L].  Output: d_loss2 = (loss term,
 * regulariser term); d_G_c1 — EVERY row written (dense, c1 is read through tf.concat), by both routes: the pooled
 * history and the recents; d_G_Q / d_G_bias — the rows of the batch's items, d_G_eta — the rows of the batch's users
 * (the other rows are left alone); d_G_eta_bias [L] written whole.  d_flag_Q / d_flag_bias (uint8 [n_items]) and
 * d_flag_eta (uint8 [n_users]), may be NULL: set to 1 for those rows; d_flag_c1 (may be NULL): every c1 row pooled or
 * read as a recent.
 * The train matrix, d_slot / step, and d_keys / d_inst / d_n / d_p / d_g / d_scal are nrhip_fism_step's; the rows of the
 * CSR form must be ASCENDING and free of duplicates.  Further work buffers for N instances: d_x float [N][d]
 * (n^-alpha p + s), d_dots float [N][L] (<c1[r_l], Q[i]>).  Neither a padded id matrix nor a [batch][L][d] block exists.
 * d = 1..NRHIP_FOSSIL_MAX_D, L = 1..NRHIP_FOSSIL_MAX_ORDER (outside: NRHIP_ERR_UNSUPPORTED); batch <=
 * NRHIP_FOSSIL_MAX_BATCH.  Every sum is taken in a fixed order, no floating-point atomics: two calls on the same
 * inputs are bit-identical. */
#define NRHIP_FOSSIL_MAX_D 128
#define NRHIP_FOSSIL_MAX_ORDER 16 /* high_order; one lane per eta column, 16 columns per reduction row */
#define NRHIP_FOSSIL_MAX_BATCH (1 << 24)
typedef struct nrhip_fossil_step_args {
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int64_t* d_t_indptr;
  const int32_t* d_t_users;
  const float* d_c1;
  const float* d_Q;
  const float* d_bias;
  const float* d_eta;
  const float* d_eta_bias;
  float* d_G_c1;
  float* d_G_Q;
  float* d_G_bias;
  float* d_G_eta;
  float* d_G_eta_bias;
  uint8_t* d_flag_Q;
  uint8_t* d_flag_bias;
  uint8_t* d_flag_c1;
  uint8_t* d_flag_eta;
  const int32_t* d_users;
  const int32_t* d_recents;
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  int32_t* d_inst;
  float* d_n;
  float* d_p;
  float* d_x;
  float* d_g;
  float* d_dots;
  float* d_scal;
  int64_t* d_slot;
  float* d_loss2;
  int n_users, n_items, d, L, batch, pairwise, loss_kind, step;
  float alpha, reg_p, reg_q, reg_eta;
} nrhip_fossil_step_args;
int nrhip_fossil_step(const nrhip_fossil_step_args* args, void* stream);
/* The evaluation's user factors: d_out [batch][ld] (ld >= d + 1), row b =
 * [ |R_u|^-alpha p_u + sum_l (eta_bias[l] + eta[u][l]) c1[d_last[u][l]] | 1 ] for u = d_users[b] (d_users NULL: u = b),
 * so that its inner product with [Q[i] | bias[i]] is predict()'s `output`.  d_last int32 [n_users][L]: the item that
 * meets eta column l, -1 (or anything outside [0, n_items)): the zero row.  A user outside the matrix gets [0 | 1]. */
int nrhip_fossil_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, int n_items,
                              const float* d_c1, const float* d_eta, const float* d_eta_bias, const int32_t* d_last,
                              int d, int L, float alpha, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                              void* stream);

/* ---- HRM (hierarchical representation model: max / avg pooling over the user and its recents) ------
 * Replaces: HRM._create_inference / _create_loss / the optimizer's gradients (model/sequential_recommender/
 * HRM.py:62-95) run by `sess.run((self.loss, self.optimizer), feed_dict)` (HRM.py:115-123).  These symbols are
 * additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * An instance is (user u, recents r_0..r_{L-1}, item i, label y) over d_P [n_users][d] and d_V [n_items][d]:
 *     s = session_agg over l of V[r_l]  (L >= 2: session_max ? column-wise max : mean;  L == 1: V[r_0])  (HRM.py:68-77)
 *     h = pre_agg over {P[u], s}        (pre_max ? column-wise max : the mean of the two)               (HRM.py:78-81)
 *     x = <h, V[i]>                                                                                     (HRM.py:82-83)
 *     loss = pointwise_loss(kind, y, x) + reg l2_loss(P[u], V[r_.], V[i])                               (HRM.py:90-91)
 * with l2_loss = sum(x^2) / 2 per occurrence and the loss kinds of nrhip_pointwise_mf_grad (the cross-entropy is the
 * MEAN over `batch`).  A max sends a column's derivative to the inputs equal to the maximum, in equal shares
 * (indicators / num_selected * grad); an item that stands twice among one instance's recents ties with itself.
 * Batch: d_users, d_items, d_labels (float): `batch` entries each; d_recents int32 [batch][L], in any order.
 * Output: d_loss2 = (loss term, regulariser term) of the tables as they come in; d_G_P / d_G_V: the rows the batch
 * looked up are STORED (the others are left alone: keep them zero), each the sum of its occurrences' gradients in the
 * order of its sort keys: a V row's target occurrences by batch slot, then its recent occurrences by (slot, column); a
 * P row's occurrences by batch slot.  d_flag_P / d_flag_V (uint8 per table row, may be NULL): set to 1 for those rows
 * (nrhip_optimizer_rows_tf).
 * A slot whose user is no row of P or whose item or any recent is outside [0, n_items) takes no part.
 * Work buffers: d_keys uint64 [batch (2 + L)], d_scal float [4 batch], d_s and d_ds float [batch][d] (the session row
 * and its already-divided derivative: the max's shares are decided once and read back by the row sums); no
 * [batch][L][d] block exists.
 * n_users + n_items < 2^31 - 1; batch <= NRHIP_HRM_MAX_BATCH; d = 1..NRHIP_HRM_MAX_D, L = 1..NRHIP_HRM_MAX_ORDER
 * (outside: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed order, no floating-point atomics: two calls on the
 * same inputs are bit-identical. */
#define NRHIP_HRM_MAX_D 128
#define NRHIP_HRM_MAX_ORDER 16 /* high_order; one lane per recent in the narrowest lane group */
#define NRHIP_HRM_MAX_BATCH (1 << 24)
typedef struct nrhip_hrm_step_args {
  const float* d_P;
  const float* d_V;
  float* d_G_P;
  float* d_G_V;
  uint8_t* d_flag_P;
  uint8_t* d_flag_V;
  const int32_t* d_users;
  const int32_t* d_recents;
  const int32_t* d_items;
  const float* d_labels;
  uint64_t* d_keys;
  float* d_scal;
  float* d_s;
  float* d_ds;
  float* d_loss2;
  int n_users, n_items, d, L, batch, pre_max, session_max, loss_kind;
  float reg;
} nrhip_hrm_step_args;
int nrhip_hrm_step(const nrhip_hrm_step_args* args, void* stream);
/* The evaluation's user factors: d_out [batch][ld] (ld >= d), row b = h_u for u = d_users[b] (d_users NULL: u = b), so
 * that its inner product with V[i] is predict()'s `output` (HRM.py:135-163).  d_last int32 [n_users][L]: the items the
 * user is pooled over, -1 (or anything outside [0, n_items)): a slot that takes no part — the session row is the max /
 * mean over the m slots that do, one item alone is that item, and with none h_u = P[u].  The pooling is the step's own
 * code.  A user outside [0, n_users) gets a row of zeros. */
int nrhip_hrm_user_factors(const float* d_P, const float* d_V, int n_users, int n_items, int d, int L, int pre_max,
                           int session_max, const int32_t* d_last, const int32_t* d_users, int batch, float* d_out,
                           int64_t ld, void* stream);

/* ---- NPE (neural personalized embedding: ReLU-gated user, context and item embeddings) ------
 * Replaces: NPE._create_inference / _create_loss / the optimizer's gradients (model/sequential_recommender/
 * NPE.py:54-75) run by `sess.run((self.loss, self.optimizer), feed_dict)` (NPE.py:94-102).  These symbols are
 * additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * An instance is (user u, recents r_0..r_{L-1}, item i, label y) over d_P [n_users][d], d_V [n_items][d] (the
 * reference's embeddings_IU) and d_W [n_items][d] (embeddings_IL, read only through the recents):
 *     s = sum over l of W[r_l]   (added in l order)                                                  (NPE.py:59-61)
 *     q = relu(P[u]) + relu(s)
 *     x = sum over c of relu(V[i])_c q_c                                                             (NPE.py:62-64)
 *     loss = pointwise_loss(kind, y, x) + reg l2_loss(P[u], V[i], W[r_.])                            (NPE.py:70-71)
 * with l2_loss = sum(x^2) / 2 per occurrence and the loss kinds of nrhip_pointwise_mf_grad (the cross-entropy is the
 * MEAN over `batch`).  The gates are strict, as TF's ReluGrad (features > 0): an input that is exactly 0, or -0,
 * passes nothing.
 * Batch: d_users, d_items, d_labels (float): `batch` entries each; d_recents int32 [batch][L].
 * Output: d_loss2 = (loss term, regulariser term) of the tables as they come in; d_G_P / d_G_V / d_G_W: the rows the
 * batch looked up are STORED (the others are left alone: keep them zero), each the sum of its occurrences' gradients
 * in the order of its sort keys: a P or V row's occurrences by batch slot, a W row's by (slot, column).  d_flag_P /
 * d_flag_V / d_flag_W (uint8 per table row, may be NULL): set to 1 for those rows (nrhip_optimizer_rows_tf).
 * A slot whose user is no row of P or whose item or any recent is outside [0, n_items) takes no part.
 * Work buffers: d_keys uint64 [batch (2 + L)], d_scal float [4 batch], d_s and d_ds float [batch][d] (the context sum
 * and the already-gated derivative with respect to it); no [batch][L][d] block exists.
 * The three tables share one key space: n_users + 2 n_items < 2^31 - 1; batch <= NRHIP_NPE_MAX_BATCH;
 * d = 1..NRHIP_NPE_MAX_D, L = 1..NRHIP_NPE_MAX_ORDER (outside: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed
 * order, no floating-point atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_NPE_MAX_D 128
#define NRHIP_NPE_MAX_ORDER 16 /* high_order; one lane per recent in the narrowest lane group */
#define NRHIP_NPE_MAX_BATCH (1 << 24)
typedef struct nrhip_npe_step_args {
  const float* d_P;
  const float* d_V;
  const float* d_W;
  float* d_G_P;
  float* d_G_V;
  float* d_G_W;
  uint8_t* d_flag_P;
  uint8_t* d_flag_V;
  uint8_t* d_flag_W;
  const int32_t* d_users;
  const int32_t* d_recents;
  const int32_t* d_items;
  const float* d_labels;
  uint64_t* d_keys;
  float* d_scal;
  float* d_s;
  float* d_ds;
  float* d_loss2;
  int n_users, n_items, d, L, batch, loss_kind;
  float reg;
} nrhip_npe_step_args;
int nrhip_npe_step(const nrhip_npe_step_args* args, void* stream);
/* The evaluation's user factors: d_out [batch][ld] (ld >= d), row b = h_u = relu(P[u]) + relu(sum of W[last[u][l]])
 * for u = d_users[b] (d_users NULL: u = b), so that its inner product with relu(V[i]) is predict()'s `output`
 * (NPE.py:114-142).  d_last int32 [n_users][L]: -1 (or anything outside [0, n_items)): a slot that takes no part; with
 * none h_u = relu(P[u]).  The sum and the gate are the step's own code.  A user outside [0, n_users) gets a row of
 * zeros. */
int nrhip_npe_user_factors(const float* d_P, const float* d_W, int n_users, int n_items, int d, int L,
                           const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                           void* stream);
/* The evaluation's item factors: d_out [n_items][d] = relu(d_V), element for element. */
int nrhip_npe_item_factors(const float* d_V, int n_items, int d, float* d_out, void* stream);

/* ---- FPMCplus (FPMC with an attention MLP over the user's last high_order items, per target item) ------
 * nrhip_fpmcplus_step replaces: FPMCplus._attention_mlp / _create_inference / _create_loss / the optimizer's gradients
 * (model/sequential_recommender/FPMCplus.py:73-119) run by `sess.run((self.loss, self.optimizer), feed_dict)`
 * (FPMCplus.py:154, 164).  nrhip_fpmcplus_scores replaces predict() (FPMCplus.py:177-205).  These symbols are
 * additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * An instance is (user u, recents r_0..r_{L-1}, item i[, negative j]) over d_UI [n_users][d], d_IU / d_IL / d_LI
 * [n_items][d], d_W [3 d][w] = [W_u; W_i; W_l], d_b [w], d_h [w]:
 *     a_l[k] = tanh(UI[u] . W_u[:,k] + IL[i] . W_i[:,k] + LI[r_l] . W_l[:,k] + b[k])            (FPMCplus.py:75-82)
 *     A_l = sum_k a_l[k] h[k];  alpha_l = exp(A_l) / sum_m exp(A_m)  (no max subtracted)          (FPMCplus.py:85-91)
 *     x(u, i) = <UI[u], IU[i]> + <IL[i], sum_l alpha_l LI[r_l]>                                   (FPMCplus.py:93-105)
 *     pairwise:  loss = pairwise_loss(kind, x(u,i) - x(u,j)) + reg_mf l2_loss(UI_u, IU_i, IL_i, LI_l, IU_j, IL_j)
 *                       + reg_w l2_loss(W, h)                                                     (FPMCplus.py:111-116)
 *     pointwise: loss = pointwise_loss(kind, y, x(u,i)) + reg_mf l2_loss(UI_u, IU_i, IL_i, LI_l)  (FPMCplus.py:118-119)
 * with l2_loss = sum(x^2) / 2 per occurrence and the loss kinds of nrhip_pairwise_mf_grad / nrhip_pointwise_mf_grad
 * (the cross-entropy is the MEAN over `batch`).  Pointwise mode has no reg_w term and b is never regularised, as the
 * class has it.  d_third: int32 negatives (pairwise) or float labels.
 * Stores (does not add) d_G_UI / d_G_IU / d_G_IL / d_G_LI rows of every looked-up row (each row's occurrences summed
 * along its run of the sorted keys, the regulariser's share per occurrence) and d_G_W / d_G_b / d_G_h whole (per-chunk
 * partials, then one ordered pass); sets d_flag_* (any may be NULL) of the looked-up rows; d_loss2 = (loss term,
 * regulariser term).  A slot whose user or item (or negative) is no table row takes no part; a RECENT outside
 * [0, n_items) takes no part in the softmax or in any gradient while the rest of its instance does (none present:
 * x = <UI[u], IU[i]>).
 * Work buffers, K = (pairwise ? 5 : 3) + L: d_keys uint64 [K batch], d_contrib float [K batch][d] (one gradient row per
 * lookup), d_scal float [4 batch], d_delta float [batch][(L + 4) w], d_partial float
 * [NRHIP_FPMCPLUS_MAX_CHUNKS][3 d w + 2 w].
 * The four tables share one key space: n_users + 3 n_items < 2^31 - 1; batch <= NRHIP_FPMCPLUS_MAX_BATCH; batch == 0
 * launches nothing, writes nothing and needs no pointer.  d = 1..NRHIP_FPMCPLUS_MAX_D, w = 1..NRHIP_FPMCPLUS_MAX_W,
 * L = 1..NRHIP_FPMCPLUS_MAX_L (outside: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed order, no floating-point
 * atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_FPMCPLUS_MAX_D 128
#define NRHIP_FPMCPLUS_MAX_W 64
#define NRHIP_FPMCPLUS_MAX_L 16
#define NRHIP_FPMCPLUS_MAX_BATCH (1 << 22)
#define NRHIP_FPMCPLUS_MAX_CHUNKS 64   /* partial sums of the dense gradients: min(ceil(batch / 32), this) chunks */
#define NRHIP_FPMCPLUS_SCORE_USERS 256 /* users a workgroup of nrhip_fpmcplus_scores walks per item tile */
typedef struct nrhip_fpmcplus_step_args {
  const float* d_UI;
  const float* d_IU;
  const float* d_IL;
  const float* d_LI;
  const float* d_W;
  const float* d_b;
  const float* d_h;
  float* d_G_UI;
  float* d_G_IU;
  float* d_G_IL;
  float* d_G_LI;
  float* d_G_W;
  float* d_G_b;
  float* d_G_h;
  uint8_t* d_flag_UI;
  uint8_t* d_flag_IU;
  uint8_t* d_flag_IL;
  uint8_t* d_flag_LI;
  const int32_t* d_users;
  const int32_t* d_recents; /* [batch][L] */
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  float* d_contrib;
  float* d_scal;
  float* d_delta;
  float* d_partial;
  float* d_loss2;
  int n_users, n_items, d, w, L, batch, pairwise, loss_kind;
  float reg_mf, reg_w;
} nrhip_fpmcplus_step_args;
int nrhip_fpmcplus_step(const nrhip_fpmcplus_step_args* args, void* stream);
/* predict(): d_out [batch][ld] (ld >= n_items), row n = x(u, i) for u = d_users[n] and every item i, the recents of u
 * the row d_last [n_users][L] (-1, or anything outside [0, n_items): a slot that takes no part; the softmax covers the
 * present slots alone; none: x = <UI[u], IU[i]>).  A user outside [0, n_users) gets a row of zeros.
 * Work buffers: d_c float [batch][L][w] and d_p float [n_items][w], the user-side and item-side halves of the
 * pre-activation; nothing of size batch x n_items x L exists. */
typedef struct nrhip_fpmcplus_scores_args {
  const float* d_UI;
  const float* d_IU;
  const float* d_IL;
  const float* d_LI;
  const float* d_W;
  const float* d_b;
  const float* d_h;
  const int32_t* d_last;
  const int32_t* d_users;
  float* d_c;
  float* d_p;
  float* d_out;
  int64_t ld;
  int n_users, n_items, d, w, L, batch;
} nrhip_fpmcplus_scores_args;
int nrhip_fpmcplus_scores(const nrhip_fpmcplus_scores_args* args, void* stream);

/* ---- TransRec (translation-based recommendation: one item table in three roles, a dense translation vector) ------
 * nrhip_transrec_step replaces: TransRec._create_inference / _create_loss / the optimizer's gradients
 * (model/sequential_recommender/TransRec.py:66-95) run by `sess.run((self.loss, self.optimizer), feed_dict)`
 * (TransRec.py:131, 140).  These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * An instance is (user u, recent item l, item i[, negative j]); P [n_users][d], Q [n_items][d], b [n_items], T [d]:
 *     v = P[u] + T + Q[l] - Q[i];   x(u, l, i) = b[i] - |v|^2   (the SQUARED distance)             (TransRec.py:75-77)
 *     pointwise (d_third = float labels)    loss = pointwise_loss(kind, label, x(u,l,i))
 *                                                  + reg l2_loss(P[u], Q[l], Q[i], b[i], T)               (TransRec.py:90-91)
 *     pairwise  (d_third = int32 negatives) loss = pairwise_loss(kind, x(u,l,i) - x(u,l,j))
 *                                                  + reg l2_loss(P[u], Q[l], Q[j], Q[i], b[i], b[j], T)   (TransRec.py:87-88)
 * with l2_loss = sum(x^2) / 2 and the loss kinds of nrhip_pointwise_mf_grad / nrhip_pairwise_mf_grad (the pointwise
 * cross-entropy is the MEAN over `batch`).  P[u] and Q[l] are regularised once per instance although the pairwise graph
 * looks them up in both inferences; T once per STEP.
 * Output: d_loss2 = (loss term, regulariser term) of the tables as they come in.  d_G_P [n_users][d], d_G_Q
 * [n_items][d]: the rows the batch looked up are STORED (the others are left alone: keep them zero), each the sum of
 * its occurrences' gradients — Q's over its occurrences as recent item, target and negative — in the order of the sorted
 * keys: by position in the batch, the first inference's lookups (positions 0..batch) before the second's
 * (batch..2 batch), at one position the recent item before the target / negative.  d_G_b [n_items]: stored for the
 * items that are a target or a negative (+-g + reg b per occurrence); an item that is a recent item only is left
 * alone.  d_G_T [d]: stored whole, the instances' sum in chunks of the batch plus reg T.  d_flag_P / d_flag_Q /
 * d_flag_b (uint8 per row, may be NULL): set to 1 for the rows nrhip_optimizer_rows_tf is to move.
 * A slot whose user is no row of P or whose recent item, item or negative is outside [0, n_items) takes no part.
 * Work buffers: d_keys uint64 [3 N] for N = batch (pointwise) or 2 batch (pairwise), d_scal float [4 batch],
 * d_partial float [min(ceil(batch / NRHIP_TRANSREC_CHUNK), NRHIP_TRANSREC_MAX_CHUNKS)][d].
 * n_users + n_items < 2^31 - 1; batch <= NRHIP_TRANSREC_MAX_BATCH; batch == 0 launches nothing, writes nothing and
 * needs no pointer; d = 1..NRHIP_TRANSREC_MAX_D (outside: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed
 * order, no floating-point atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_TRANSREC_MAX_D 128
#define NRHIP_TRANSREC_MAX_BATCH (1 << 24)
#define NRHIP_TRANSREC_CHUNK 32        /* instances per partial sum of G_T while there are at most MAX_CHUNKS chunks */
#define NRHIP_TRANSREC_MAX_CHUNKS 64
typedef struct nrhip_transrec_step_args {
  const float* d_P;
  const float* d_Q;
  const float* d_b;
  const float* d_T;
  float* d_G_P;
  float* d_G_Q;
  float* d_G_b;
  float* d_G_T;
  uint8_t* d_flag_P;
  uint8_t* d_flag_Q;
  uint8_t* d_flag_b;
  const int32_t* d_users;
  const int32_t* d_recent;
  const int32_t* d_items;
  const void* d_third;
  uint64_t* d_keys;
  float* d_scal;
  float* d_partial;
  float* d_loss2;
  int n_users, n_items, d, batch, pairwise, loss_kind;
  float reg;
} nrhip_transrec_step_args;
int nrhip_transrec_step(const nrhip_transrec_step_args* args, void* stream);
/* Replaces the query side of TransRec's prediction graph, `u_emb + global_embedding + last_i_emb` (TransRec.py:102-104):
 * d_out [batch][ld] (ld >= d), row n = P[u] + T + Q[d_last[u]] for u = d_users[n] (d_users NULL: u = n).  d_last int32
 * [n_users]: the user's most recent train item; -1 (or anything outside [0, n_items)): none — the row is P[u] + T.  A
 * user outside [0, n_users) gets a row of zeros. */
int nrhip_transrec_queries(const float* d_P, const float* d_Q, const float* d_T, int n_users, int n_items, int d,
                           const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                           void* stream);
/* Replaces `-l2_distance(pre_emb, j_emb) + item_biases` (TransRec.py:18-19, 105-107) and the per-batch
 * `sess.run(self.prediction)` of predict() (TransRec.py:153-161): d_out [n][ld] (ld >= n_items; the columns beyond
 * n_items are left alone), d_out[r][j] = d_b[j] - sqrt(sum_c (d_q[r][c] - d_Q[j][c])^2) for the query rows d_q [n][ldq]
 * (ldq >= d).  The DIRECT form: per output the difference, then a fused multiply-accumulate in fp32, columns
 * ascending; the expanded form |q|^2 + |Q_j|^2 - 2 q.Q_j cancels worst for the items nearest the query.  n, n_items
 * and d need not be multiples of anything; n <= 65535 * 64. */
int nrhip_transrec_scores(const float* d_q, int64_t ldq, const float* d_Q, const float* d_b, int n, int n_items, int d,
                          float* d_out, int64_t ld, void* stream);

/* ---- GRU4Rec (session-based recommendation with a stack of GRU cells; state carried across steps) ---------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * Variables: E_in [n_items][n_0], Q [n_items][n_last], b [n_items] (GRU4Rec.py:80-85) and per layer l, with input
 * width in_0 = n_0, in_l = n_(l-1): Wg_l [in_l + n_l][2 n_l], bg_l [2 n_l], Wc_l [in_l + n_l][n_l], bc_l [n_l]
 * (the variables of tf.nn.rnn_cell.GRUCell, GRU4Rec.py:111).  The cell [EXT: tensorflow r1.12 rnn_cell_impl.GRUCell]:
 *     [r, u] = sigmoid([x, s] Wg + bg)  (r the first n_l columns);  c = act([x, r * s] Wc + bc);  h = u s + (1 - u) c
 * nrhip_gru4rec_step replaces one `sess.run([self.update_opt, self.final_state], feed)` of GRU4Rec.py:160 up to the
 * optimiser: the graph of GRU4Rec.py:111-131 forward, the loss (GRU4Rec.py:87-101) and every gradient.  The states
 * d_state[l] [batch][n_l] are constants (placeholders, GRU4Rec.py:77: nothing flows back through them).
 *     x = E_in[X];  h_top = the stack's output;  Z[i][j] = h_top[i] . Q[Y[j]] + b[Y[j]];  A = final_act(Z)
 *     bpr   mean over all batch^2 entries of -log_sigmoid(A[i][i] - A[i][j])                       (GRU4Rec.py:87-92)
 *     top1  mean_i (mean_j sigmoid(A[i][j] - A[i][i]) + mean_j sigmoid(A[i][j]^2) - sigmoid(A[i][i]^2) / batch)
 *                                                                                                    (GRU4Rec.py:94-101)
 *     + reg (l2(E_in[X]) + l2(Q[Y]) + l2(b[Y])), l2 = sum of squares / 2, on the GATHERED rows      (GRU4Rec.py:130-131)
 * hidden_act: 0 tanh, 1 relu.  final_act: 0 linear, 1 relu, 2 leaky_relu (alpha 0.2).  loss_kind: 0 top1, 1 bpr.
 * Output: d_loss2 = (loss term, reg * regulariser sum); d_h_new[l] [batch][n_l] the new states; d_G_Wg / d_G_bg /
 * d_G_Wc / d_G_bc stored whole, every element the batch's sum in slot order; the rows of d_G_Ein the batch read and
 * the rows of d_G_Q / d_G_b it scored are STORED (the others are left alone: keep them zero), a row that occurs more
 * than once as the sum of its slots along a run of sorted keys (item << 32 | slot), slot order.  A slot whose X (Y)
 * is outside [0, n_items) reads a row of zeros and its gradient row is dropped.
 * Work buffers: d_keys uint64 [2 batch]; d_ws float [nrhip_gru4rec_workspace_floats].  1..NRHIP_GRU4REC_MAX_LAYERS
 * layers of width 1..NRHIP_GRU4REC_MAX_WIDTH (outside: NRHIP_ERR_UNSUPPORTED); batch <= NRHIP_GRU4REC_MAX_BATCH;
 * batch == 0 launches nothing and writes nothing.  fp32 throughout, every sum in a fixed order, no atomics: two calls
 * on the same inputs are bit-identical. */
#define NRHIP_GRU4REC_MAX_LAYERS 3
#define NRHIP_GRU4REC_MAX_WIDTH 128
#define NRHIP_GRU4REC_MAX_BATCH 4096
#define NRHIP_GRU4REC_TILE 16          /* users per workgroup of nrhip_gru4rec_user_states */
typedef struct nrhip_gru4rec_weights {
  const float* d_Wg[NRHIP_GRU4REC_MAX_LAYERS];
  const float* d_bg[NRHIP_GRU4REC_MAX_LAYERS];
  const float* d_Wc[NRHIP_GRU4REC_MAX_LAYERS];
  const float* d_bc[NRHIP_GRU4REC_MAX_LAYERS];
  int width[NRHIP_GRU4REC_MAX_LAYERS];
  int n_layers, hidden_act;
} nrhip_gru4rec_weights;
typedef struct nrhip_gru4rec_step_args {
  const float* d_Ein;
  const float* d_Q;
  const float* d_b;
  nrhip_gru4rec_weights w;
  float* d_G_Ein;
  float* d_G_Q;
  float* d_G_b;
  float* d_G_Wg[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_bg[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_Wc[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_bc[NRHIP_GRU4REC_MAX_LAYERS];
  const float* d_state[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_h_new[NRHIP_GRU4REC_MAX_LAYERS];
  const int32_t* d_X;
  const int32_t* d_Y;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  int n_items, batch, final_act, loss_kind;
  float reg;
} nrhip_gru4rec_step_args;
int nrhip_gru4rec_workspace_floats(int n_layers, const int* widths, int max_batch, size_t* floats);
int nrhip_gru4rec_step(const nrhip_gru4rec_step_args* args, void* stream);
/* Replaces `state = final_state` and `state[i][mask] = 0` of the session-parallel loop (GRU4Rec.py:160, 172-174) in
 * one launch: d_state[l][t] = d_reset[t] ? 0 : d_h_new[l][t] for every layer and slot (the hand-over first, then the
 * mask).  d_reset uint8 [batch], may be NULL (no slot ends). */
int nrhip_gru4rec_advance(float* const* d_state_host, const float* const* d_h_new_host, const int* widths,
                          int n_layers, int batch, const uint8_t* d_reset, void* stream);
/* Replaces GRU4Rec._get_user_embeddings (GRU4Rec.py:179-225), one `sess.run([self.u_emb, self.final_state])` per time
 * position on the host there: d_H[d_out_row ? d_out_row[k] : k] [n_last] (rows ldh apart) = the top layer's output
 * after user d_users[k]'s items d_seq[d_seq_ptr[u] .. d_seq_ptr[u + 1]) went through the stack from a zero state; a
 * user without items (or outside [0, n_users)) gets zeros.  One workgroup per NRHIP_GRU4REC_TILE consecutive entries
 * of d_users loops over the time positions up to the tile's longest sequence; the states stay in LDS, a user past its
 * end keeps its state.  Sort d_users by descending length for balance; a user's row does not depend on the tile it is
 * in: every output is one k-ascending chain over [x, s] (then [x, r * s]) whatever the tile holds.  An item outside
 * [0, n_items) feeds a zero input row. */
int nrhip_gru4rec_user_states(const int64_t* d_seq_ptr, const int32_t* d_seq, int n_users, int n_items,
                              const int32_t* d_users, const int32_t* d_out_row, int n_listed, const float* d_Ein,
                              const nrhip_gru4rec_weights* w, float* d_H, int64_t ldh, void* stream);
/* Replaces predict() (GRU4Rec.py:232-250): d_out[r][j] = final_act(d_H[r] . d_Q[j] + d_b[j]) for the rows d_H [n][ldh],
 * d_out [n][ld] (ld >= n_items; the columns beyond are left alone); the dot product is the k-ascending fmaf chain. */
int nrhip_gru4rec_scores(const float* d_H, int64_t ldh, const float* d_Q, const float* d_b, int n, int n_items, int d,
                         int final_act, float* d_out, int64_t ld, void* stream);

/* ---- GRU4RecPlus (GRU4Rec with shared sampled negatives and the softmax-weighted max losses) ----------------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * The variables, the cell, the states, nrhip_gru4rec_advance, nrhip_gru4rec_user_states and nrhip_gru4rec_scores are
 * GRU4Rec's: _get_user_embeddings and predict() of the two reference classes are the same computation.
 * nrhip_gru4recplus_step replaces one `sess.run([self.update_opt, self.final_state], feed_dict=feed)` of
 * GRU4RecPlus.py:186 up to the optimiser: the graph of GRU4RecPlus.py:130-150 forward, the loss
 * (GRU4RecPlus.py:91-120) and every gradient.  d_X holds batch items, d_Y holds M = batch + n_sample: the first batch
 * are the positives (the positive of row i is column i, tf.eye(b, size_y), GRU4RecPlus.py:93), the rest the sampled
 * negatives every row shares (GRU4RecPlus.py:178-180).
 *     Z[i][j] = h_top[i] . Q[Y[j]] + b[Y[j]], [batch][M];  A = final_act(Z);  p = A[i][i]
 *     hm_j = [j != i];  m = max_j (A[i][j] hm_j);  e_j = hm_j exp(A[i][j] hm_j - m);  s_j = e_j / sum_j e_j
 *                                                                                         (_softmax_neg, GRU4RecPlus.py:91-98)
 *     bpr_max   L_i = -log(sum_j s_j sigmoid(p - A[i][j]) + 1e-24) + bpr_reg sum_j s_j A[i][j]^2   (GRU4RecPlus.py:100-110)
 *     top1_max  L_i = sum_j s_j (sigmoid(A[i][j] - p) + sigmoid(A[i][j]^2))                        (GRU4RecPlus.py:112-120)
 *     loss = mean_i L_i + reg (l2(E_in[X]) + l2(Q[Y]) + l2(b[Y])), on the GATHERED rows, all M slots (GRU4RecPlus.py:149-150)
 * The softmax weights s are differentiated (they are no constants); the shift m cancels and is treated as one.
 * loss_kind: 0 top1_max, 1 bpr_max; hidden_act and final_act as in nrhip_gru4rec_step.
 * Output as nrhip_gru4rec_step's: d_loss2, d_h_new, the cells' gradients whole, the rows of d_G_Ein / d_G_Q / d_G_b the
 * batch touched STORED, a row that occurs in several slots as the sum of its slots in slot order.  A slot whose id is
 * outside [0, n_items) reads a row of zeros (it still takes part in the row's softmax as a zero logit) and its
 * gradient row is dropped.
 * Work buffers: d_keys uint64 [2 batch + n_sample]; d_ws float [nrhip_gru4recplus_workspace_floats].  Layers, widths and
 * batch within GRU4Rec's limits, n_sample 0..NRHIP_GRU4RECPLUS_MAX_SAMPLE (batch + n_sample floats then fit LDS);
 * outside: NRHIP_ERR_UNSUPPORTED.  n_sample == 0 is legal (GRU4RecPlus.py:178); batch + n_sample < 2 with batch > 0
 * is refused (NRHIP_ERR_UNSUPPORTED): the reference divides 0 by 0 there.  batch == 0 launches nothing and writes
 * nothing.  fp32 throughout (the two reported sums are added in double and rounded once), every sum in a fixed order,
 * no atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_GRU4RECPLUS_MAX_SAMPLE 8192
typedef struct nrhip_gru4recplus_step_args {
  const float* d_Ein;
  const float* d_Q;
  const float* d_b;
  nrhip_gru4rec_weights w;
  float* d_G_Ein;
  float* d_G_Q;
  float* d_G_b;
  float* d_G_Wg[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_bg[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_Wc[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_G_bc[NRHIP_GRU4REC_MAX_LAYERS];
  const float* d_state[NRHIP_GRU4REC_MAX_LAYERS];
  float* d_h_new[NRHIP_GRU4REC_MAX_LAYERS];
  const int32_t* d_X;
  const int32_t* d_Y;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  int n_items, batch, n_sample, final_act, loss_kind;
  float reg, bpr_reg;
} nrhip_gru4recplus_step_args;
/* Replaces the storage TensorFlow gives the intermediate tensors of the graph (GRU4RecPlus.py:130-150) and their
 * gradients: the size in floats of nrhip_gru4recplus_step's d_ws for batches up to max_batch with n_sample negatives. */
int nrhip_gru4recplus_workspace_floats(int n_layers, const int* widths, int max_batch, int n_sample, size_t* floats);
/* Replaces one `sess.run([self.update_opt, self.final_state], feed_dict=feed)` of GRU4RecPlus.py:186 up to the
 * optimiser; the head of this section has the graph, the outputs and the limits. */
int nrhip_gru4recplus_step(const nrhip_gru4recplus_step_args* args, void* stream);

/* ---- SASRec (causal multi-head self-attention blocks over padded item sequences) ----------------------------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * nrhip_sasrec_step replaces one `sess.run(self.train_opt, feed_dict=feed)` of SASRec.py:402 up to the optimiser: the
 * graph of SASRec.py:311-375 forward with training on, the loss and every gradient.  d_seq / d_pos_ids / d_neg_ids are
 * int32 [batch][L]; the padding item is id n_items (any id outside [0, n_items) reads the zero row, and its gradient is
 * dropped).
 *     table = concat(item, zeros[1, d]) sqrt(d);  x = (table[seq] + pos[0..L)) drop_0 * (seq != n_items)
 *     per block: q = ln1(x);  Q = q Wq + bq, K = x Wk + bk, V = x Wv + bv;  heads along the feature axis;
 *                logits Q K^T / sqrt(d / h), a key masked where sum(x_j) == 0 or j > i (value -2**32 + 1), softmax,
 *                * [sum(q_i) != 0], drop, . V;  y = that + q;  u = ln2(y);
 *                x = (drop(drop(relu(u W1 + b1)) W2 + b2) + u) * (seq != n_items)
 *     z = lnf(x);  ln(v) = gamma (v - mean) / sqrt(biased var + 1e-8) + beta
 *     loss = sum_t [pos_t != n_items] (-log(sigmoid(table[pos_t] . z_t) + 1e-24)
 *                                      - log(1 - sigmoid(table[neg_t] . z_t) + 1e-24)) / sum_t [pos_t != n_items]
 *            (+ l2_emb (sum item^2 + sum pos^2) / 2 when l2_emb != 0)
 * Variables of a block, in creation order (d_blk[i][k]): ln1 beta, ln1 gamma, Wq [d][d], bq, Wk, bk, Wv, bv, ln2 beta,
 * ln2 gamma, W1 [d][d] (the conv1d kernel [1][d][d]), b1, W2, b2.
 * Dropout: 1 + 3 n_blocks sites in evaluation order (the embedding [B][L][d]; per block the attention weights
 * [h B][L][L] head-major, the hidden layer and the output of the feed-forward net [B][L][d]).  d_mask[k] != NULL: the
 * uint8 {0, 1} keep mask of site k (all sites or none); otherwise a counter-based generator keyed by (seed, step, site,
 * element).  rate 0 applies none.
 * Output: d_loss2[0] the loss term, d_loss2[1] the regulariser term; every gradient STORED whole (d_G_item must be zero
 * on entry: only the rows the batch touches are written, a row that occurs in several slots as the sum of its slots in
 * slot order, plus l2_emb item on every row when l2_emb != 0).  A batch without any target yields gradients of exactly
 * zero and a loss term of zero.
 * Work buffers: d_keys uint64 [3 batch L]; d_ws float [nrhip_sasrec_workspace_floats].
 * Limits: hidden_units 1..NRHIP_SASREC_MAX_WIDTH, max_len 1..NRHIP_SASREC_MAX_LEN, blocks 1..NRHIP_SASREC_MAX_BLOCKS,
 * batch 0..NRHIP_SASREC_MAX_BATCH, num_heads * batch * max_len^2 <= NRHIP_SASREC_MAX_WEIGHTS (the saved attention
 * weights); outside: NRHIP_ERR_UNSUPPORTED.  num_heads must divide hidden_units (NRHIP_ERR_ARG).  batch == 0 launches
 * nothing and writes nothing.  fp32 throughout (the two reported sums are added in double and rounded once), every sum
 * in a fixed order, no atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_SASREC_MAX_BLOCKS 4
#define NRHIP_SASREC_MAX_WIDTH 128
#define NRHIP_SASREC_MAX_LEN 200
#define NRHIP_SASREC_MAX_BATCH 4096
#define NRHIP_SASREC_BLOCK_VARS 14
#define NRHIP_SASREC_MAX_SITES (1 + 3 * NRHIP_SASREC_MAX_BLOCKS)
#define NRHIP_SASREC_MAX_WEIGHTS (1ll << 30)
typedef struct nrhip_sasrec_weights {
  const float* d_item;
  const float* d_pos;
  const float* d_blk[NRHIP_SASREC_MAX_BLOCKS][NRHIP_SASREC_BLOCK_VARS];
  const float* d_lnf_beta;
  const float* d_lnf_gamma;
  int n_items, d, L, n_blocks, n_heads;
} nrhip_sasrec_weights;
typedef struct nrhip_sasrec_step_args {
  nrhip_sasrec_weights w;
  float* d_G_item;
  float* d_G_pos;
  float* d_G_blk[NRHIP_SASREC_MAX_BLOCKS][NRHIP_SASREC_BLOCK_VARS];
  float* d_G_lnf_beta;
  float* d_G_lnf_gamma;
  const int32_t* d_seq;
  const int32_t* d_pos_ids;
  const int32_t* d_neg_ids;
  const uint8_t* d_mask[NRHIP_SASREC_MAX_SITES];
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  uint64_t seed;
  int batch, step;
  float rate, l2_emb;
} nrhip_sasrec_step_args;
/* Replaces the storage TensorFlow gives the intermediate tensors of the graph and their gradients: the size in floats
 * of d_ws for batches up to max_batch (nrhip_sasrec_forward needs no more). */
int nrhip_sasrec_workspace_floats(int max_batch, int max_len, int hidden_units, int num_blocks, int num_heads,
                                  size_t* floats);
/* Replaces one `sess.run(self.train_opt, feed_dict=feed)` of SASRec.py:402 up to the optimiser; the head of this section
 * has the graph, the outputs and the limits. */
int nrhip_sasrec_step(const nrhip_sasrec_step_args* args, void* stream);
/* Replaces the forward half of `sess.run(self.all_logits, ...)` of SASRec.py:438: the graph with training off on d_seq
 * [batch][L]; d_out[b][0..d) = scale * z[b][L - 1] (row stride ld).  An all-padded row gives lnf's beta. */
int nrhip_sasrec_forward(const nrhip_sasrec_weights* weights, const int32_t* d_seq, int batch, float* d_ws, float scale,
                         float* d_out, int64_t ld, void* stream);

/* ---- Caser (vertical and horizontal convolutions over the L x d window of a user's last items) ---------------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * nrhip_caser_step replaces one `sess.run(self.train_opt, feed_dict=feed)` of Caser.py:139 up to the optimiser: the
 * graph of Caser.py:70-116 forward with training on, the loss and every gradient.  d_users int32 [batch], d_seq
 * [batch][L], d_pos [batch][T], d_neg [batch][N]; the padding item is id n_items (any id outside [0, n_items) reads a
 * zero row, and its gradient is dropped).  F = nv d + nh L.
 *     E = concat(seq_item, zeros[1, d])[seq]                                            [L][d]
 *     feature[j nv + c]            = conv_v_bias[c] + sum_t E[t][j] conv_v[t][c]        (no activation)
 *     feature[nv d + (i - 1) nh + c] = max_p relu(conv_h_bias[i][c] + sum_{t < i, j} E[p + t][j] conv_h[i][t][j][c]),
 *                                    heights i = 1..L, positions p = 0..L - i; the first maximum takes the gradient
 *     x = feature / (1 - rate) * mask;  z = relu(x fc + fc_bias);  p = concat(z, user[u])
 *     logit_k = p . item[tar_k] + item_bias[tar_k], the T positives, then the N negatives; a pad target has logit 0
 *     loss = mean_{batch T}(-log(sigmoid(pos) + 1e-24)) + mean_{batch N}(-log(1 - sigmoid(neg) + 1e-24))
 *            (+ l2_reg (sum user^2 + sum seq_item^2 + sum item^2 + sum item_bias^2) / 2 when l2_reg != 0)
 * written as the reference writes it, in fp32, with the sigmoid's derivative y (1 - y): a saturated term is exactly
 * -log(1e-24) with gradient 0.
 * Variables: d_user [U][d], d_seq_item [I][d], d_item [I][2 d], d_item_bias [I], d_conv_v [L][nv] (the Conv2D kernel
 * [L][1][1][nv]), d_conv_v_bias [nv], d_conv_h[i - 1] [i][d][nh] (the kernel [i][d][1][nh]), d_conv_h_bias[i - 1] [nh],
 * d_fc [F][d], d_fc_bias [d].
 * Dropout: d_mask != NULL is the uint8 {0, 1} keep mask [batch][F]; otherwise a counter-based generator keyed by (seed,
 * step, element).  rate 0 applies none.
 * Output: d_loss2[0] the loss term, d_loss2[1] the regulariser term; every gradient STORED (the four tables' buffers must
 * be zero on entry: only the rows the batch touches are written, a row that occurs in several slots as the sum of its
 * slots in slot order, plus l2_reg v on every row when l2_reg != 0; the conv and dense gradients are stored whole).
 * Work buffers: d_keys uint64 [batch (1 + L + T + N)]; d_ws float [nrhip_caser_workspace_floats].
 * Limits: factors_num 1..NRHIP_CASER_MAX_WIDTH, seq_L 1..NRHIP_CASER_MAX_LEN, nv 1..NRHIP_CASER_MAX_NV, nh
 * 1..NRHIP_CASER_MAX_NH, seq_T and neg_samples 1..NRHIP_CASER_MAX_TARGETS, batch 0..NRHIP_CASER_MAX_BATCH, n_users +
 * 2 n_items < 2^31 (the rows of one sort-key space); outside: NRHIP_ERR_UNSUPPORTED.  batch == 0 launches nothing and
 * writes nothing.  fp32 throughout (the reported sums are added in double and rounded once), every sum in a fixed
 * order, no atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_CASER_MAX_WIDTH 128
#define NRHIP_CASER_MAX_LEN 10
#define NRHIP_CASER_MAX_NV 16
#define NRHIP_CASER_MAX_NH 64
#define NRHIP_CASER_MAX_TARGETS 16
#define NRHIP_CASER_MAX_BATCH 4096
typedef struct nrhip_caser_weights {
  const float* d_user;
  const float* d_seq_item;
  const float* d_item;
  const float* d_item_bias;
  const float* d_conv_v;
  const float* d_conv_v_bias;
  const float* d_conv_h[NRHIP_CASER_MAX_LEN];
  const float* d_conv_h_bias[NRHIP_CASER_MAX_LEN];
  const float* d_fc;
  const float* d_fc_bias;
  int n_users, n_items, d, L, nv, nh;
} nrhip_caser_weights;
typedef struct nrhip_caser_step_args {
  nrhip_caser_weights w;
  float* d_G_user;
  float* d_G_seq_item;
  float* d_G_item;
  float* d_G_item_bias;
  float* d_G_conv_v;
  float* d_G_conv_v_bias;
  float* d_G_conv_h[NRHIP_CASER_MAX_LEN];
  float* d_G_conv_h_bias[NRHIP_CASER_MAX_LEN];
  float* d_G_fc;
  float* d_G_fc_bias;
  const int32_t* d_users;
  const int32_t* d_seq;
  const int32_t* d_pos;
  const int32_t* d_neg;
  const uint8_t* d_mask;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  uint64_t seed;
  int batch, T, N, step;
  float rate, l2_reg;
} nrhip_caser_step_args;
/* Replaces the storage TensorFlow gives the intermediate tensors of the graph and their gradients: the size in floats
 * of nrhip_caser_step's d_ws for batches up to max_batch. */
int nrhip_caser_workspace_floats(int max_batch, int seq_L, int factors_num, int nv, int nh, int seq_T, int neg_samples,
                                 size_t* floats);
/* Replaces one `sess.run(self.train_opt, feed_dict=feed)` of Caser.py:139 up to the optimiser; the head of this section
 * has the graph, the outputs and the limits. */
int nrhip_caser_step(const nrhip_caser_step_args* args, void* stream);
/* Replaces the forward half of `sess.run(self.all_logits, ...)` of Caser.py:202: the graph with training off on d_users
 * [n] and d_seq [n][L]; d_out[b][0..2 d) = concat(z, user[u]) (row stride ld).  d_ws is not read (the pass keeps a row
 * in LDS) and may be NULL. */
int nrhip_caser_forward(const nrhip_caser_weights* weights, const int32_t* d_users, const int32_t* d_seq, int n,
                        float* d_ws, float* d_out, int64_t ld, void* stream);
/* Replaces the matmul of `self.all_logits` (Caser.py:122) for rows wider than nrhip_gru4rec_scores takes (2 d > 128):
 * d_out[r][i] = d_H[r][0..width) . d_Q[i][0..width), no bias; width 1..2 NRHIP_CASER_MAX_WIDTH. */
int nrhip_caser_scores(const float* d_H, int64_t ldh, const float* d_Q, int n, int n_items, int width, float* d_out,
                       int64_t ld, void* stream);

/* ---- SRGNN (a gated graph network over each session's item graph, attention readout, full softmax) ---------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * nrhip_srgnn_step replaces one `sess.run(self.train_opt, feed_dict=feed)` of SRGNN.py:162 up to the optimiser: the
 * session graphs of SRGNN.py:176-205, the graph of SRGNN.py:75-136 forward, the loss and all 14 gradients.  d is
 * hidden_size, I num_items, L max_seq_len.
 * The feed, one of two forms (nrhip_srgnn_feed):
 *     d_seq int32 [batch][L] post-padded with id I — the first id outside [0, I) ends the session — and d_target
 *     int32 [batch]; or
 *     d_users, d_ends int32 [batch] over resident sequences (d_seq_ptr int64 [n_users + 1], d_seq_flat int32): the
 *     session is the last L of user u's first `end` items and the target the item at `end` (none when end is the
 *     user's item count: the forward pass).  A user or an end outside the data gives the empty session.
 * Per session, with items s_0 .. s_{len-1}:
 *     nodes = the distinct items ascending; alias[t] = the node of s_t; adj[alias[t]][alias[t + 1]] = 1
 *     A_in[i][j] = adj[i][j] / max(colsum_j, 1);  A_out[i][j] = adj[j][i] / max(rowsum_j, 1)   (both divisors by j)
 *     h = embedding[nodes];  `step` times:  x = [A_in (h W_in + b_in), A_out (h W_out + b_out)]
 *         [r, u] = sigmoid([x, h] gates_kernel + gates_bias);  c = tanh([x, r * h] candidate_kernel + candidate_bias)
 *         h = u h + (1 - u) c                                   (the gradient flows through the state h)
 *     last = h[alias[len - 1]] nasr_w1;  m_t = sigmoid(last + h[alias[t]] nasr_w2 + nasr_b)
 *     a = sum_t (m_t . nasrv) h[alias[t]];  sess = [a, last] B, or a when nonhybrid
 *     logits = sess . embedding^T [I];  loss = mean_b(log sum exp(logits - max) + max - logits[target])
 *            + l2 (sum over all 14 variables of sum v^2) / 2
 * The graph is never a dense n x n matrix: the distinct edges are two sorted lists with row pointers, and A_in . /
 * A_out . walk a node's edges.  The empty session has sess = 0.  A target outside [0, I) takes its session out of the
 * loss and the gradients (it stays in the mean's denominator).
 * Variables: d_nasr_w1, d_nasr_w2, d_W_in, d_W_out [d][d]; d_nasrv, d_nasr_b, d_b_in, d_b_out [d]; d_embedding [I][d]
 * (the pad row I is not stored and never written); d_B [2 d][d]; d_gates_kernel [3 d][2 d], d_gates_bias [2 d];
 * d_candidate_kernel [3 d][d], d_candidate_bias [d].
 * Output: d_loss2[0] the cross-entropy mean, d_loss2[1] the regulariser term; every gradient STORED whole (d_G_B is
 * l2 B when nonhybrid), l2 v included.
 * Work buffers: d_keys uint64 [batch L]; d_ws float [nrhip_srgnn_workspace_floats].
 * Limits: hidden_size 1..NRHIP_SRGNN_MAX_WIDTH, max_seq_len 1..NRHIP_SRGNN_MAX_LEN, step 1..NRHIP_SRGNN_MAX_STEP,
 * batch 0..NRHIP_SRGNN_MAX_BATCH, batch * num_items < 2^31; outside: NRHIP_ERR_UNSUPPORTED.  batch == 0 launches
 * nothing and writes nothing.  fp32 throughout (the reported sums are added in double and rounded once), every sum in
 * a fixed order, no atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_SRGNN_MAX_WIDTH 128
#define NRHIP_SRGNN_MAX_LEN 256
#define NRHIP_SRGNN_MAX_STEP 4
#define NRHIP_SRGNN_MAX_BATCH 4096
typedef struct nrhip_srgnn_weights {
  const float* d_nasr_w1;
  const float* d_nasr_w2;
  const float* d_nasrv;
  const float* d_nasr_b;
  const float* d_embedding;
  const float* d_W_in;
  const float* d_b_in;
  const float* d_W_out;
  const float* d_b_out;
  const float* d_B;
  const float* d_gates_kernel;
  const float* d_gates_bias;
  const float* d_candidate_kernel;
  const float* d_candidate_bias;
  int n_items, d, L, step, nonhybrid;
} nrhip_srgnn_weights;
typedef struct nrhip_srgnn_feed {
  const int32_t* d_seq;
  const int32_t* d_target;
  const int32_t* d_users;
  const int32_t* d_ends;
  const int64_t* d_seq_ptr;
  const int32_t* d_seq_flat;
  int n_users;
} nrhip_srgnn_feed;
typedef struct nrhip_srgnn_step_args {
  nrhip_srgnn_weights w;
  nrhip_srgnn_feed f;
  float* d_G_nasr_w1;
  float* d_G_nasr_w2;
  float* d_G_nasrv;
  float* d_G_nasr_b;
  float* d_G_embedding;
  float* d_G_W_in;
  float* d_G_b_in;
  float* d_G_W_out;
  float* d_G_b_out;
  float* d_G_B;
  float* d_G_gates_kernel;
  float* d_G_gates_bias;
  float* d_G_candidate_kernel;
  float* d_G_candidate_bias;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  int batch;
  float l2;
} nrhip_srgnn_step_args;
/* Replaces the storage TensorFlow gives the intermediate tensors of the graph and their gradients, the [batch][I]
 * logits included: the size in floats of d_ws for batches up to max_batch (nrhip_srgnn_forward needs no more). */
int nrhip_srgnn_workspace_floats(int max_batch, int max_seq_len, int hidden_size, int step, int num_items,
                                 size_t* floats);
/* Replaces one `sess.run(self.train_opt, feed_dict=feed)` of SRGNN.py:162 up to the optimiser; the head of this
 * section has the graph, the outputs and the limits. */
int nrhip_srgnn_step(const nrhip_srgnn_step_args* args, void* stream);
/* Replaces the forward half of `sess.run(self.all_logits, ...)` of SRGNN.py:230: d_out[b][0..d) = sess_b (row stride
 * ld) for the n sessions of `feed` (its d_target is not read), with the kernels of the step. */
int nrhip_srgnn_forward(const nrhip_srgnn_weights* weights, const nrhip_srgnn_feed* feed, int n, float* d_ws,
                        float* d_out, int64_t ld, void* stream);

/* ---- NeuMF / MLP (a relu layer stack over the concat of a user and an item row, plus a GMF dot product) -------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * nrhip_neumf_step replaces one `sess.run((self.loss, self.optimizer), feed_dict)` of NeuMF.py:146 / MLP.py up to the
 * optimiser, in pointwise mode.  d is embedding_size (0: MLP.py — no GMF branch, no mf_* tables), e = layers[0] / 2
 * (integer), w[k] = layers[k], n_layers of them.  Per instance (u, i, label):
 *     x = [mlp_user[u] | mlp_item[i]]  (2 e wide);  h_k = relu(h_{k-1} kernel_k + bias_k), h_{-1} = x
 *     y = sum_c mf_user[u][c] mf_item[i][c] + sum_j h_last[j]            (no output layer, no sigmoid)
 *     loss_kind 0: sigmoid cross-entropy of (label, y), the MEAN over the batch; 1: (label - y)^2, the sum
 *     regulariser: reg_mf (|mf_user[u]|^2 + |mf_item[i]|^2) / 2 + reg_mlp (|mlp_user[u]|^2 + |mlp_item[i]|^2) / 2 per
 *     instance — on the gathered rows: a row the batch holds twice counts twice
 * relu's gradient is 0 where the pre-activation is <= 0.  An instance with an id outside its table takes no part.
 * Variables: d_mf_user [U][d], d_mf_item [I][d], d_mlp_user [U][e], d_mlp_item [I][e]; d_kernel[k] [in_k][w_k] with
 * in_0 = 2 e and in_k = w_{k-1}; d_bias[k] [w_k].  A table or kernel of zero width may be a null pointer.
 * Output: d_loss2[0] the data term, d_loss2[1] the regulariser term; d_G_kernel / d_G_bias STORED whole; the rows of the
 * four tables' gradients that the batch touches STORED (duplicates of a row summed in slot order), other rows left as
 * they are; d_flag_* (optional, uint8 per row): set to 1 for the touched rows.
 * Work buffers: d_keys uint64 [2 batch]; d_ws float [nrhip_neumf_workspace_floats].
 * Limits: embedding_size 0..NRHIP_NEUMF_MAX_WIDTH, 1..NRHIP_NEUMF_MAX_LAYERS layers of width 1..NRHIP_NEUMF_MAX_WIDTH,
 * batch 0..NRHIP_NEUMF_MAX_BATCH, n_users + n_items < 2^31; outside: NRHIP_ERR_UNSUPPORTED.  batch == 0 launches nothing
 * and writes nothing.  fp32 throughout (the reported sums are added in double and rounded once), every sum in a fixed
 * order, no atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_NEUMF_MAX_WIDTH 128
#define NRHIP_NEUMF_MAX_LAYERS 4
#define NRHIP_NEUMF_MAX_BATCH 4096
typedef struct nrhip_neumf_weights {
  const float* d_mf_user;
  const float* d_mf_item;
  const float* d_mlp_user;
  const float* d_mlp_item;
  const float* d_kernel[NRHIP_NEUMF_MAX_LAYERS];
  const float* d_bias[NRHIP_NEUMF_MAX_LAYERS];
  int n_users, n_items, d, n_layers;
  int width[NRHIP_NEUMF_MAX_LAYERS];
} nrhip_neumf_weights;
typedef struct nrhip_neumf_step_args {
  nrhip_neumf_weights w;
  float* d_G_mf_user;
  float* d_G_mf_item;
  float* d_G_mlp_user;
  float* d_G_mlp_item;
  float* d_G_kernel[NRHIP_NEUMF_MAX_LAYERS];
  float* d_G_bias[NRHIP_NEUMF_MAX_LAYERS];
  uint8_t* d_flag_mf_user;
  uint8_t* d_flag_mf_item;
  uint8_t* d_flag_mlp_user;
  uint8_t* d_flag_mlp_item;
  const int32_t* d_users;
  const int32_t* d_items;
  const float* d_labels;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  int batch, loss_kind;
  float reg_mf, reg_mlp;
} nrhip_neumf_step_args;
/* Replaces the storage TensorFlow gives the intermediate tensors of the graph and their gradients: the size in floats
 * of nrhip_neumf_step's d_ws for batches up to max_batch (only the shape fields of `weights` are read). */
int nrhip_neumf_workspace_floats(const nrhip_neumf_weights* weights, int max_batch, size_t* floats);
/* Replaces one `sess.run((self.loss, self.optimizer), feed_dict)` of NeuMF.py:146 up to the optimiser; the head of this
 * section has the graph, the outputs and the limits. */
int nrhip_neumf_step(const nrhip_neumf_step_args* args, void* stream);
/* Replaces `sess.run(self.output, feed_dict)` of NeuMF.py:163 (candidate mode): d_out[k] = y(d_users[k], d_items[k])
 * for n pairs, through the step's own forward path; a pair with an id outside its table scores relu-of-biases alone. */
int nrhip_neumf_forward(const nrhip_neumf_weights* weights, const int32_t* d_users, const int32_t* d_items, int n,
                        float* d_out, void* stream);
/* The size in floats of nrhip_neumf_scores' d_ws for n users (only the shape fields of `weights` are read). */
int nrhip_neumf_scores_workspace_floats(const nrhip_neumf_weights* weights, int n, size_t* floats);
/* Replaces the per-user `sess.run(self.output, ...)` loop of NeuMF.py:165-168: d_out[r][i] = y(d_users[r], i) for every
 * item i < n_items (row stride ld >= n_items; nothing is written beyond column n_items or row n).  The first layer is
 * split, relu((m | n) W1 + b1) = relu((m W1u + b1) + n W1i), and made once per call for the n users and the I items; the
 * further layers run per pair on v_mfma_f32_32x32x2_f32 (exact fp32), relu, the row sum and the GMF dot product in the
 * epilogue; each score is written once.  At most 65535 tiles of users per call (NRHIP_ERR_UNSUPPORTED beyond). */
int nrhip_neumf_scores(const nrhip_neumf_weights* weights, const int32_t* d_users, int n, float* d_ws, float* d_out,
                       int64_t ld, void* stream);

/* ---- CDAE (collaborative denoising auto-encoder, Wu et al., WSDM 2016) ------------------------------
 * Replaces: the per-user batch loops of CDAE.train_model (model/general_recommender/CDAE.py:108-140), the graph of
 * CDAE._encoding / build_graph (CDAE.py:62-98) up to the optimiser, and the encoder half of predict() (CDAE.py:148-160).
 * A batch is `batch` slots, each a user u with the train row R_u.  Per slot the builder draws |R_u| num_neg items
 * outside R_u with replacement and keeps each once, ascending: N_s.  The slot's DECODER entries are R_u ascending
 * (label 1), then N_s (label 0); its INPUT entries are R_u and N_s merged, ascending, every value 1 (CDAE.py:118 writes the
 * negatives into the input row).  With keep_e = the corruption mask of input entry e and k = keep_prob:
 *     hidden_s = act(sum_e keep_e (1 / k) en[item_e]  +  user[u]  +  offset)       act: 0 identity, 1 sigmoid
 *     x_e      = <hidden_slot(e), de[item_e]> + bias[item_e]                       over the decoder entries
 *     loss     = sum_e pointwise_loss(kind, label_e, x_e)        kind 0: sigmoid cross-entropy, 1: square; a SUM
 *              + reg l2_loss(en[i], de[i], bias[i] for every item i of the batch ONCE (tf.unique, CDAE.py:83);
 *                            user[u] per slot; all of offset)
 *
 * nrhip_cdae_batch: draw (seed, user, q) is the q-th number of the sampler's counter-based stream (nrhip_sample_*):
 * independent of the batch around it.  The host passes what it knows from the CSR: d_pos_ptr [batch + 1], the prefix
 * sums of the slots' |R_u|, d_seg_off [batch + 1] = num_neg d_pos_ptr and d_seg_len [batch] = num_neg |R_u|.  The draws
 * are sorted per slot in LDS (nrhip_sort_u64_segments) while max_draws <= NRHIP_CDAE_SEGMENT_DRAWS, by one sort of
 * all (slot, item) keys (nrhip_sort_u64) beyond.  Output, all on the device: d_entry_ptr [batch + 1]; per entry
 * d_items, d_labels, d_slot and d_in_pos (the index in d_in_items of the entry's own item); d_in_items (the input
 * list; slot s holds the same range d_entry_ptr[s] .. d_entry_ptr[s + 1] in both lists).  The arrays hold
 * (1 + num_neg) d_pos_ptr[batch] entries at most.  d_keys: scratch, num_neg d_pos_ptr[batch] keys.  Users must be rows
 * of the CSR.  batch 0..NRHIP_CDAE_MAX_BATCH.
 *
 * nrhip_cdae_step: d_loss2 = (loss term, regulariser term); d_G_user / d_G_en / d_G_de / d_G_bias: the rows of the
 * batch are STORED (keep the others zero), d_G_offset whole.  A row's gradient is the sum over its run of the sorted
 * keys (row << 32 | entry, or slot), in key order, plus reg row once per item, once per occurrence per user.
 * d_keep uint8 per input entry: read (keep_given) or drawn from (seed, step, entry index) and written.  d_flag_*: as in
 * nrhip_fpmc_step.  Work buffers: d_keys uint64 and d_l2 float [entry_cap + batch], d_g float [entry_cap], d_hidden /
 * d_dz float [batch][d], d_scal float [4 batch].  entry_cap >= d_entry_ptr[batch], which stays on the device.
 * n_users + n_items < 2^31 - 1; d = 1..NRHIP_CDAE_MAX_D.  fp32, fixed summation orders, no atomics: bit-identical. */
#define NRHIP_CDAE_MAX_D 128
#define NRHIP_CDAE_MAX_BATCH 1024
#define NRHIP_CDAE_SEGMENT_DRAWS 16384 /* draws of one slot that nrhip_sort_u64_segments sorts in LDS */
typedef struct nrhip_cdae_batch_args {
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int32_t* d_users;
  const int64_t* d_pos_ptr;
  const int64_t* d_seg_off;
  const int32_t* d_seg_len;
  uint64_t* d_keys;
  int64_t* d_entry_ptr;
  int32_t* d_items;
  float* d_labels;
  int32_t* d_slot;
  int32_t* d_in_items;
  int32_t* d_in_pos;
  int64_t n_draws;
  uint64_t seed;
  int n_users, n_items, batch, num_neg, max_draws;
} nrhip_cdae_batch_args;
int nrhip_cdae_batch(const nrhip_cdae_batch_args* args, void* stream);
typedef struct nrhip_cdae_step_args {
  const float* d_user;
  const float* d_en;
  const float* d_offset;
  const float* d_de;
  const float* d_bias;
  float* d_G_user;
  float* d_G_en;
  float* d_G_offset;
  float* d_G_de;
  float* d_G_bias;
  uint8_t* d_flag_user;
  uint8_t* d_flag_en;
  uint8_t* d_flag_de;
  uint8_t* d_flag_bias;
  const int32_t* d_users;
  const int64_t* d_entry_ptr;
  const int32_t* d_items;
  const float* d_labels;
  const int32_t* d_slot;
  const int32_t* d_in_items;
  const int32_t* d_in_pos;
  uint8_t* d_keep;
  uint64_t* d_keys;
  float* d_g;
  float* d_hidden;
  float* d_dz;
  float* d_scal;
  float* d_l2;
  float* d_loss2;
  uint64_t seed, step;
  int n_users, n_items, d, batch, entry_cap, act, loss_kind, keep_given;
  float keep_prob, reg;
} nrhip_cdae_step_args;
int nrhip_cdae_step(const nrhip_cdae_step_args* args, void* stream);
/* The evaluation's user factors: d_out [batch][ld] (ld >= d + 1), row b = [hidden | 1] of u = d_users[b] (NULL: u = b)
 * from the train row alone, so that its inner product with [de[i] | bias[i]] is predict()'s score.  The mask of the
 * k-th entry of row b is d_keep_io[d_mask_ptr[b] + k] (d_mask_ptr: the prefix sums of the row lengths, batch + 1),
 * read or drawn as in nrhip_cdae_step; keep_prob >= 1 keeps everything and takes NULL for both.  A user outside
 * [0, n_users) gets [0 | 1]. */
int nrhip_cdae_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, int n_items,
                            const float* d_user, const float* d_en, const float* d_offset, int d, int act,
                            const int32_t* d_users, const int64_t* d_mask_ptr, int batch, uint8_t* d_keep_io,
                            int keep_given, float keep_prob, uint64_t seed, uint64_t step, float* d_out, int64_t ld,
                            void* stream);
/* Candidate mode: d_out[k] = <d_factors[d_rows[k]][0..d), de[d_items[k]]> + bias[d_items[k]] for n pairs; an item
 * outside [0, n_items) scores 0. */
int nrhip_cdae_pairs(const float* d_factors, int64_t ld, const float* d_de, const float* d_bias, int n_items, int d,
                     const int32_t* d_rows, const int32_t* d_items, int64_t n, float* d_out, void* stream);

/* ---- DeepICF (deep item-based collaborative filtering) -------------------------
 * Replaces: the graph of model/general_recommender/DeepICF.py:112-178 and one `sess.run((loss, optimizer))` per step,
 * and predict() (DeepICF.py:231-259).  NAIS's attention pooling (nrhip_nais_step: the same instances, mask, ragged
 * buffer and walks) gives p; then a tower over x0 = (n^alpha p) (.) Q[i]:
 *     per layer k  z = x W_k + b_k,  [batch norm],  relu;   out = x_L . w_out + b_out;   output = sigmoid(out + bias[i])
 *     loss = MEAN(-y log(output + 1e-7) - (1 - y) log(1 - output + 1e-7))                        (tf.losses.log_loss)
 *          + regs[0] l2(Q) + regs[1] l2(c1) + regs[2] l2(W) + sum_k regw[k] l2(W_k)   — WHOLE tables, so d_G_Q and d_G_c1
 *            are dense gradients (reg * table + the batch's rows); the call zeroes d_G_Q itself
 * Batch norm (batch_norm != 0) is the fused form of TF-1.12 on a rank-2 input, decay 0.9, epsilon 0.001: training
 * normalises with the batch mean and the BIASED batch variance; d_mm / d_mv move by v -= (v - batch) * 0.1, the variance
 * entering with Bessel's correction batch / max(batch - 1, 1) when bessel != 0.  The batch statistics are crossed at
 * kernel boundaries: per-tile partial sums combined in tile order, the mean first, then the centred squares; backward
 * likewise for sum dy and sum dy xhat.  With batch norm on, d_G_b[k] is written as exact zeros (it is zero in exact
 * arithmetic).  An instance outside the matrix takes part in the batch statistics as a zero row (and in the mean's
 * 1 / batch); it has no loss term and its d loss / d logit is zero, so it reaches no gradient but through those statistics.
 * `nais`: as for nrhip_nais_step with pairwise = 0, c1_sort = 0, reg_p = reg_q = 0; loss_kind is not
 * read.  d_ws: nrhip_deepicf_workspace_floats(tower, d, max_batch) floats.  Up to NRHIP_DEEPICF_MAX_LAYERS layers of up
 * to NRHIP_DEEPICF_MAX_WIDTH (beyond: NRHIP_ERR_UNSUPPORTED).  Every sum is taken in a fixed order, no atomics. */
#define NRHIP_DEEPICF_MAX_LAYERS 4
#define NRHIP_DEEPICF_MAX_WIDTH 128
typedef struct nrhip_deepicf_tower {
  const float* d_W[NRHIP_DEEPICF_MAX_LAYERS];      /* [in][width] */
  const float* d_b[NRHIP_DEEPICF_MAX_LAYERS];
  const float* d_gamma[NRHIP_DEEPICF_MAX_LAYERS];  /* batch_norm != 0 */
  const float* d_beta[NRHIP_DEEPICF_MAX_LAYERS];
  float* d_mm[NRHIP_DEEPICF_MAX_LAYERS];           /* moving mean / variance */
  float* d_mv[NRHIP_DEEPICF_MAX_LAYERS];
  const float* d_Wout;                             /* [width of the last layer] */
  const float* d_bout;                             /* [1] */
  int n_layers, batch_norm;
  int width[NRHIP_DEEPICF_MAX_LAYERS];
} nrhip_deepicf_tower;
typedef struct nrhip_deepicf_step_args {
  nrhip_nais_step_args nais;
  nrhip_deepicf_tower tower;
  float* d_G_W[NRHIP_DEEPICF_MAX_LAYERS];
  float* d_G_b[NRHIP_DEEPICF_MAX_LAYERS];
  float* d_G_gamma[NRHIP_DEEPICF_MAX_LAYERS];
  float* d_G_beta[NRHIP_DEEPICF_MAX_LAYERS];
  float* d_G_Wout;
  float* d_G_bout;
  float* d_ws;
  float regs[3];
  float regw[NRHIP_DEEPICF_MAX_LAYERS];            /* 0: the layer is not regularised */
  int bessel;
} nrhip_deepicf_step_args;
int nrhip_deepicf_workspace_floats(const nrhip_deepicf_tower* tower, int d, int max_batch, size_t* floats);
int nrhip_deepicf_step(const nrhip_deepicf_step_args* args, void* stream);
/* predict(): d_out [batch][ld], row b = sigmoid(tower(|R_u|^alpha v(u, i) (.) Q[i]) + bias[i]) for every item i, with
 * v(u, i) = sum_{h in R_u} e(i, h) c1[h] / (sum_{h in R_u} e(i, h))^beta pooled per (user, item) in registers — no
 * [batch][items][d] block exists.  `nais`: as for nrhip_nais_scores (its workspace, tile, h_cap and mfma); the e(i, h)
 * terms are nais.hip's.  d_wpad: the tower at inference as ONE affine map per layer (the caller folds the moving
 * statistics in): per layer the kernel [32 Kt][32 Mt] zero-padded then the bias [32 Mt], then w_out [32 Mt] and b_out;
 * tiles[k] = 32-tiles of the width in front of layer k (tiles[0]: of d) .. tiles[n_layers]: of the last width.
 * mfma != 0: the tower on v_mfma_f32_32x32x2_f32, a wavefront per (user, 32 items), widths up to 64 (beyond:
 * NRHIP_ERR_UNSUPPORTED); mfma == 0: one lane per pair, any width up to NRHIP_DEEPICF_MAX_WIDTH.  A user without train
 * items (or outside the matrix) scores through an empty pooling (v = 0).  Reads every table, writes d_out alone. */
typedef struct nrhip_deepicf_scores_args {
  nrhip_nais_scores_args nais;
  const float* d_wpad;
  int n_layers, mfma, wtotal;
  int tiles[NRHIP_DEEPICF_MAX_LAYERS + 1];
} nrhip_deepicf_scores_args;
int nrhip_deepicf_scores(const nrhip_deepicf_scores_args* args, void* stream);

/* ---- ConvNCF: the outer-product conv tower's step, the pairs' outputs and the all-items scorer (csrc/convncf.hip).
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * nrhip_convncf_step replaces one `sess.run((self.loss, self.optimizer), feed_dict)` of ConvNCF.py:177 up to the two
 * Adagrad applications: the graph of ConvNCF.py:87-125 on `batch` triplets (user, pos, neg) and its gradients.
 *   E = P[u] (x) Q[i] [d, d, 1]; n_layers layers tanh(conv2d(x, kernel_k [2, 2, c_in, c_out], strides 2, SAME) + bias_k)
 *   with d == 2^n_layers, so the last layer has one position; output = a_last . W + b (no sigmoid);
 *   loss = sum pairwise_loss(output(u, pos) - output(u, neg))  (loss_kind: 0 bpr, 1 hinge, 2 square)
 *   opt_loss = loss + reg_embed l2_loss(P[u], Q[neg], Q[pos]) + reg_head l2_loss(W, b)
 *              + reg_net (sum_k l2_loss(kernel_k, bias_k) + l2_loss(W, b)),  l2_loss = sum / 2, on the GATHERED rows: the
 *   user row counts once per triplet, each item row once per occurrence.
 * Outputs: d_G_kernel / d_G_bias / d_G_W / d_G_b in full (stored); of d_G_P / d_G_Q the rows the batch holds (stored: a
 * row's gradient is the sum over its occurrences in key order; other rows are left as they are); d_flag_P / d_flag_Q
 * (uint8 per row, may be NULL): set to 1 for those rows (nrhip_optimizer_rows_tf); d_loss2 = {loss, the reg_embed term}.
 * A triplet with an id outside its table takes no part.  Work buffers: d_keys uint64 [4 batch]; d_ws float
 * [nrhip_convncf_workspace_floats] (the activations of layers 2.. between the passes, the slots, the chunks' partials).
 * Limits: 1..NRHIP_CONVNCF_MAX_LAYERS layers of 1..NRHIP_CONVNCF_MAX_CHANNELS channels, d == 2^n_layers, batch
 * 0..NRHIP_CONVNCF_MAX_BATCH, n_users + n_items < 2^31; outside: NRHIP_ERR_UNSUPPORTED.  batch == 0 launches nothing and
 * writes nothing.  Sums run in a fixed order, no atomics: reruns are bit-identical. */
#define NRHIP_CONVNCF_MAX_LAYERS 6
#define NRHIP_CONVNCF_MAX_CHANNELS 32
#define NRHIP_CONVNCF_MAX_BATCH 4096
typedef struct nrhip_convncf_weights {
  const float* d_P;             /* embedding_P [n_users][d] */
  const float* d_Q;             /* embedding_Q [n_items][d] */
  const float* d_kernel[NRHIP_CONVNCF_MAX_LAYERS];   /* [2][2][c_in][c_out], c_in = 1 for the first */
  const float* d_bias[NRHIP_CONVNCF_MAX_LAYERS];
  const float* d_W;             /* [channel[n_layers - 1]] */
  const float* d_b;             /* [1] */
  int n_users, n_items, d, n_layers;
  int channel[NRHIP_CONVNCF_MAX_LAYERS];
} nrhip_convncf_weights;
typedef struct nrhip_convncf_step_args {
  nrhip_convncf_weights w;
  float* d_G_P;
  float* d_G_Q;
  float* d_G_kernel[NRHIP_CONVNCF_MAX_LAYERS];
  float* d_G_bias[NRHIP_CONVNCF_MAX_LAYERS];
  float* d_G_W;
  float* d_G_b;
  uint8_t* d_flag_P;
  uint8_t* d_flag_Q;
  const int32_t* d_users;
  const int32_t* d_pos;
  const int32_t* d_neg;
  uint64_t* d_keys;
  float* d_ws;
  float* d_loss2;
  int batch, loss_kind;
  float reg_embed, reg_head, reg_net;
} nrhip_convncf_step_args;
/* The size in floats of nrhip_convncf_step's d_ws for batches up to max_batch (only the shape fields are read). */
int nrhip_convncf_workspace_floats(const nrhip_convncf_weights* weights, int max_batch, size_t* floats);
int nrhip_convncf_step(const nrhip_convncf_step_args* args, void* stream);
/* d_out[k] = output(d_users[k], d_items[k]), k < n, through the step's forward path; a pair outside the tables gives 0 */
int nrhip_convncf_pairs(const nrhip_convncf_weights* weights, const int32_t* d_users, const int32_t* d_items, int n,
                        float* d_out, void* stream);
/* d_out[r * ld + i] = output(d_users[r], i) for r < n and every item i: predict() of ConvNCF.py:196-199; ld >= n_items,
 * the columns behind n_items are left as they are.  Any number of pairs: a launch holds at most 2^20 workgroups, each of
 * which takes its pairs in turn (nrhip_convncf_pairs likewise) */
int nrhip_convncf_scores(const nrhip_convncf_weights* weights, const int32_t* d_users, int n, float* d_out, int64_t ld,
                         void* stream);

/* ---- CFGAN: the per-epoch masks, the two adversarial steps and the scorer's row factors (csrc/cfgan.hip).
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * R is the train matrix in CSR ([n_rows][n_cols], ascending rows; already transposed in itemBased mode); c is a row of
 * it as a 0/1 vector.  Both networks are stacks of dense layers [in][out] with sigmoid hidden layers and an identity
 * output layer: G maps n_cols -> width[0..n_hidden) -> n_cols, D maps 2 n_cols -> width[0..n_hidden) -> 1 on [c | y].
 * A dense c, the [batch][2 n_cols] concatenation and a dense mask never exist: first layers pool rows of the kernel over
 * the CSR row, masks are bit rows of words = ceil(n_cols / 32) uint32, column 32 w + k at bit k of word w.
 *
 * nrhip_cfgan_masks: per batch row b and plane (0: d_zr, 1: d_pm) one bit row: the row's train columns plus the
 * d_n_sample[2 b + plane] other columns with the smallest (key, column) pairs, key = the upper word of
 * splitmix64(base + column), base a splitmix64 chain over (seed, epoch, plane, row id): a pure function of those four,
 * found by a radix select over 256-bin histograms in LDS, one workgroup per (row, plane); no key is ever stored.
 * A count outside [0, n_cols - deg] is clamped.
 *
 * nrhip_cfgan_d_step / nrhip_cfgan_g_step: the forward pass and the gradients of one sess.run(trainer_d) /
 * sess.run(trainer_g) of CFGAN.py:60-95 WITHOUT the regularisers and the optimiser (nrhip_cfgan_apply carries both).
 *   out = G(c), y_fake = out . pm
 *   D: mean softplus(-D([c | c])) + mean softplus(D([c | y_fake]))  -> d_loss3[0], d_loss3[1]; dis.d_G_* stored in full
 *   G: mean softplus(-D([c | y_fake])) + zr_coef mean sum_i out_i^2 zr_i -> d_loss3[0], d_loss3[2]; gen.d_G_* stored
 * The row gradients of the pooled kernel halves are summed along sorted (column << 32 | slot) keys in key order; every
 * float sum has a fixed order and nothing is accumulated with floating-point atomics: reruns are bit-identical.
 * d_ent_ptr [batch + 1]: the running sum of the batch rows' lengths (n_ent = its last entry); d_keys uint64 [n_ent];
 * d_ws / d_gemm_ws: nrhip_cfgan_workspace for max_batch.  batch == 0 launches nothing.
 *
 * nrhip_cfgan_apply: one pass over every kernel and bias of `net`: gradient = d_G + reg * variable, ApplyAdam (sgd == 0;
 * step = alpha) or ApplyGradientDescent (sgd != 0; step = the learning rate), the gradient zero afterwards, and
 * *d_reg_loss = reg * sum(variable^2) / 2 of the values BEFORE the update.  d_partials: NRHIP_CFGAN_APPLY_BLOCKS doubles.
 *
 * nrhip_cfgan_hidden: d_out [batch][ld] (ld >= width[n_hidden - 1]), row b = G's last hidden layer on row d_rows[b] of R
 * (NULL: row b); d_tmp: 2 * batch * NRHIP_CFGAN_MAX_WIDTH floats (unused with one hidden layer).
 * nrhip_cfgan_pairs: d_out[e] = sum_k d_F[d_rows[e]][k] * d_Q[d_items[e]][k], k < width.
 * Limits: 1..NRHIP_CFGAN_MAX_HIDDEN hidden layers of 1..NRHIP_CFGAN_MAX_WIDTH units, batch 0..NRHIP_CFGAN_MAX_BATCH,
 * n_cols < 2^24; outside: NRHIP_ERR_UNSUPPORTED. */
#define NRHIP_CFGAN_MAX_HIDDEN 3
#define NRHIP_CFGAN_MAX_WIDTH 512
#define NRHIP_CFGAN_MAX_BATCH 1024
#define NRHIP_CFGAN_APPLY_BLOCKS 2048
typedef struct nrhip_cfgan_net {
  float* d_W[NRHIP_CFGAN_MAX_HIDDEN + 1];     /* layer k's kernel [in][out]; layer n_hidden is the output layer */
  float* d_b[NRHIP_CFGAN_MAX_HIDDEN + 1];
  float* d_G_W[NRHIP_CFGAN_MAX_HIDDEN + 1];   /* the gradients */
  float* d_G_b[NRHIP_CFGAN_MAX_HIDDEN + 1];
  float* d_m_W[NRHIP_CFGAN_MAX_HIDDEN + 1];   /* Adam's moments (not read with sgd) */
  float* d_m_b[NRHIP_CFGAN_MAX_HIDDEN + 1];
  float* d_v_W[NRHIP_CFGAN_MAX_HIDDEN + 1];
  float* d_v_b[NRHIP_CFGAN_MAX_HIDDEN + 1];
  int n_hidden;
  int width[NRHIP_CFGAN_MAX_HIDDEN];
} nrhip_cfgan_net;
typedef struct nrhip_cfgan_step_args {
  nrhip_cfgan_net gen;
  nrhip_cfgan_net dis;
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int32_t* d_rows;          /* [batch] rows of R, repeats allowed */
  const int64_t* d_ent_ptr;       /* [batch + 1] */
  const uint32_t* d_zr;           /* [batch][words] */
  const uint32_t* d_pm;
  uint64_t* d_keys;
  float* d_ws;
  void* d_gemm_ws;
  size_t gemm_ws_bytes;
  float* d_loss3;
  int n_rows, n_cols, batch, n_ent, max_batch;
  float zr_coef;
} nrhip_cfgan_step_args;
/* the sizes of d_ws (floats) and d_gemm_ws (bytes) for batches up to max_batch (only the shape fields are read) */
int nrhip_cfgan_workspace(const nrhip_cfgan_step_args* shape, size_t* floats, size_t* gemm_bytes);
int nrhip_cfgan_masks(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows,
                      const int32_t* d_n_sample, int batch, int n_rows, int n_cols, uint64_t seed, uint64_t epoch,
                      uint32_t* d_zr, uint32_t* d_pm, void* stream);
int nrhip_cfgan_d_step(const nrhip_cfgan_step_args* args, void* stream);
int nrhip_cfgan_g_step(const nrhip_cfgan_step_args* args, void* stream);
int nrhip_cfgan_apply(const nrhip_cfgan_net* net, int n_in, int n_out, int sgd, float step, float beta1, float beta2,
                      float eps, float reg, double* d_partials, float* d_reg_loss, void* stream);
int nrhip_cfgan_hidden(const nrhip_cfgan_net* net, const int64_t* d_indptr, const int32_t* d_indices,
                       const int32_t* d_rows, int batch, int n_cols, float* d_tmp, float* d_out, int64_t ld,
                       void* stream);
int nrhip_cfgan_pairs(const float* d_F, int64_t ldf, const float* d_Q, int64_t ldq, int width, const int32_t* d_rows,
                      const int32_t* d_items, int64_t n, float* d_out, void* stream);

/* ---- IRGAN (two matrix-factorisation triples in a minimax game; the generator samples from its own softmax) --------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * Two triples (P [n_users][d], Q [n_items][d], b [n_items]): G and D, plain gradient descent with one lr.
 * Weights of a row of logits z at temperature tau: w_i = floor(exp((z_i - max z) / tau) 2^31) as uint32, W = sum w_i in
 * 64 bits.  A draw is a pure function of (seed, pass, phase, user, draw index) through nr::XorShift64s seeded with
 * (seed, ((pass << 2 | phase) << 32) | user, draw index), three words h0, h1, h2:
 *     phase 0 (D data, IRGAN.py:175-193): the smallest i whose inclusive prefix sum exceeds mulhi64(h0, W)
 *     phase 1 (G step, IRGAN.py:220-224): mulhi64(h0, 5) == 0 ? the positive at index mulhi64(h1, deg)
 *                                                              : the smallest i whose prefix sum exceeds mulhi64(h2, W) */
#define NRHIP_IRGAN_MAX_D 128
#define NRHIP_IRGAN_MAX_BATCH 1024
typedef struct nrhip_irgan_args {
  float* d_Pg; float* d_Qg; float* d_bg;          /* the generator */
  float* d_Pd; float* d_Qd; float* d_bd;          /* the discriminator */
  const int64_t* d_indptr;                        /* the train CSR, [n_users + 1] */
  const int32_t* d_indices;                       /* ascending per row */
  float* d_z;                                     /* [n_items]: the logits of the last G step's user */
  uint32_t* d_w;                                  /* [n_items]: the weights its draws were made from */
  int32_t* d_draw_items;                          /* [2][2 max_deg]: the draws as made, then sorted by (item, index) */
  float* d_draw_r;                                /* [2][2 max_deg]: their rewards times p / pn, same two orders */
  float* d_hdr;                                   /* [4]: max z, sum exp(z - max), R, S (an int) */
  float* d_ws; size_t ws_floats;                  /* nrhip_irgan_workspace */
  int n_users, n_items, d, max_deg, max_batch;
  float lr, g_reg, d_reg;
  uint64_t seed;
} nrhip_irgan_args;
int nrhip_irgan_workspace(int n_items, int d, int max_batch, size_t* floats);
/* d_z [rows][ld] logits -> the uint32 weights of each row over its first n entries, IN PLACE */
int nrhip_irgan_weights(float* d_z, int64_t ld, int rows, int n, double tau, void* stream);
/* row r of d_w belongs to user d_users[r].  phase 0: deg(u) draws; the interleaved (u, pos_k, 1), (u, draw_k, 0) go to
 * d_out_*[d_out_off[r] + 2 k (+ 1)].  phase 1: 2 deg(u) mixture draws to d_out_items[d_out_off[r] + k] */
int nrhip_irgan_draws(const uint32_t* d_w, int64_t ld, int rows, int n, const int32_t* d_users, const int64_t* d_indptr,
                      const int32_t* d_indices, const int64_t* d_out_off, int phase, uint64_t seed, uint64_t pass,
                      int32_t* d_out_users, int32_t* d_out_items, float* d_out_labels, void* stream);
/* Replaces the `sess.run(self.discriminator.d_updates, ...)` loop of IRGAN.py:207-211: ceil(n / batch) steps over the
 * triples d_users / d_items / d_labels [>= n] taken in the order d_order [n] (NULL: as they lie), the last step short.
 * d_loss (or NULL) [steps][3]: sum of the cross entropies, B d_reg / 2 (sum |P_u|^2 + sum |Q_i|^2), B d_reg / 2 sum
 * b_i^2 over the occurrences, all from before the step. */
int nrhip_irgan_d_pass(const nrhip_irgan_args* args, const int32_t* d_users, const int32_t* d_items,
                       const float* d_labels, const int32_t* d_order, int64_t n, int batch, float* d_loss, void* stream);
/* Replaces the loop of IRGAN.py:214-235 over h_users (a HOST array), one user step after the other: four launches per
 * user.  d_given (or NULL; one user only): 2 deg(u) recorded draws in place of made ones. */
int nrhip_irgan_g_pass(const nrhip_irgan_args* args, const int32_t* h_users, int n_users, const int32_t* d_given,
                       uint64_t pass, void* stream);

/* ---- SBPR (social BPR: a third, social item per positive; Zhao et al., CIKM 2014) ---------------------------------
 * These symbols are additions: no existing struct changes and NRHIP_ABI_VERSION stays 4.
 * Replaces model/social_recommender/SBPR.py: _get_SocialItemsSet (:40-49), _get_pairwise_all_data with the
 * DataIterator's permutation (:104-106, 122-148) and `sess.run((self.loss, self.optimizer), feed_dict)` (:115).
 * CSR inputs: int64 indptr [n_users + 1], int32 indices ascending per row; the trust CSR deduplicated.
 *
 * Social sets.  C_u = the distinct items k that some user f trusted by u has in their train row and u has not, with
 * count(u, k) = the number of such f (= suk - 1); users without train items have no set, trusted users without train
 * items add nothing.  nrhip_sbpr_expansion_sizes: d_sizes [n_users] = sum over f in S_u of |R_f| (0 for a user without
 * train items).  nrhip_sbpr_sets_block: the sets of the users [u0, u1), whose expansions lie one after the other at
 * d_pair_off [u1 - u0 + 1] (exclusive offsets, the last = n_pairs <= NRHIP_SBPR_MAX_PAIRS).  Output: d_indptr_out
 * [u1 - u0 + 1] offsets into d_items_out / d_counts_out [>= n_pairs] (items ascending per user), *d_total the number of
 * entries.  Work buffers: d_keys uint64 [n_pairs], d_cnt and d_pos int32 [n_pairs], d_chunk int64
 * [ceil(n_pairs / 1024) + 1].  The sort: a user's keys lie together, so with d_seg_len (the length of each user's
 * expansion, 0 for one above max_seg_len <= NRHIP_SBPR_SEGMENT_PAIRS) the users' segments are sorted on their own in
 * one launch, and the n_big larger ones, listed in the HOST arrays h_big_off / h_big_len, by one nrhip_sort_u64 each;
 * d_seg_len NULL: one sort of the whole block.  No atomics: the same result on every run. */
#define NRHIP_SBPR_SEGMENT_PAIRS 16384
#define NRHIP_SBPR_MAX_PAIRS (1ll << 30)
#define NRHIP_SBPR_MAX_D 128
#define NRHIP_SBPR_MAX_BATCH (1 << 24)
typedef struct nrhip_sbpr_sets_args {
  const int64_t* d_tr_indptr;
  const int32_t* d_tr_indices;
  const int64_t* d_s_indptr;
  const int32_t* d_s_indices;
  const int64_t* d_pair_off;
  uint64_t* d_keys;
  int32_t* d_cnt;
  int32_t* d_pos;
  int64_t* d_chunk;
  int32_t* d_items_out;
  int32_t* d_counts_out;
  int64_t* d_indptr_out;
  int64_t* d_total;
  const int32_t* d_seg_len;       /* [u1 - u0] or NULL: see above */
  const int64_t* h_big_off;       /* HOST arrays [n_big] */
  const int64_t* h_big_len;
  int n_users, n_items, u0, u1;
  int64_t n_pairs;
  int max_seg_len, n_big;
} nrhip_sbpr_sets_args;
int nrhip_sbpr_expansion_sizes(const int64_t* d_tr_indptr, const int64_t* d_s_indptr, const int32_t* d_s_indices,
                               int n_users, int64_t* d_sizes, void* stream);
int nrhip_sbpr_sets_block(const nrhip_sbpr_sets_args* args, void* stream);
/* One epoch's instances.  Slots: one per (eligible user, train item), eligible users d_elig [n_elig] ascending, slot s of
 * row r = d_slot_row[s] is train item s - d_slot_ptr[r] of user d_elig[r].  Output position p in [out_begin, out_begin +
 * out_count) carries slot perm(p) (shuffle != 0; the keyed bijection of nrhip_sample_instances_epoch) and writes entry
 * p - out_begin of the five outputs (u, i, k, j, suk).  The draws are a pure function of (seed, epoch, slot) through
 * nr::XorShift64s seeded with them: word 0, h: k = C_u[mulhi64(h, |C_u|)] and suk = count(u, k) + 1; words 1.. are the
 * attempts at j = mulhi64(h, n_items), rejected while j is in R_u or C_u; after 64 rejections j is the r-th id outside
 * both, r = mulhi64(next word, the number of such ids).  j = -1 when no id is outside both. */
typedef struct nrhip_sbpr_stream_args {
  const int64_t* d_tr_indptr;
  const int32_t* d_tr_indices;
  const int64_t* d_c_indptr;      /* [n_users + 1] */
  const int32_t* d_c_items;
  const int32_t* d_c_counts;
  const int64_t* d_slot_ptr;      /* [n_elig + 1] */
  const int32_t* d_slot_row;      /* [n_slots] */
  const int32_t* d_elig;          /* [n_elig] */
  int32_t* d_users_out;
  int32_t* d_items_out;
  int32_t* d_social_out;
  int32_t* d_neg_out;
  float* d_suk_out;
  int64_t n_slots, out_begin, out_count;
  uint64_t seed, epoch;
  int n_elig, n_users, n_items, shuffle;
} nrhip_sbpr_stream_args;
int nrhip_sbpr_stream(const nrhip_sbpr_stream_args* args, void* stream);
/* The step on slots (u, i, k, j, suk), P [n_users][d], Q [n_items][d], b [n_items]:
 *     x_a = P[u] . Q[a] + b[a];   y1 = (x_i - x_k) / suk,   y2 = x_k - x_j
 *     loss = pairwise_loss(kind, y1) + pairwise_loss(kind, y2) + reg l2_loss(P[u], Q[k], Q[i], Q[j], b[i], b[k], b[j])
 * with l2_loss = sum(x^2) / 2 per occurrence and the loss kinds of nrhip_pairwise_mf_grad.  i, k and j may coincide
 * within a slot and across slots.  Output: d_loss2 = (loss term, regulariser term) of the tables as they come in; the
 * rows of d_G_P / d_G_Q / d_G_b the batch looked up are STORED (the others are left alone: keep them zero), each the
 * sum over its occurrences in the order of the sorted keys: by slot, in one slot i before k before j.  d_flag_* (uint8
 * per row, may be NULL) are set for the rows nrhip_optimizer_rows_tf is to move.  A slot with an id that is no table
 * row takes no part.  Work buffers: d_keys uint64 [4 batch], d_scal float [4 batch].  batch == 0 launches nothing.
 * d = 1..NRHIP_SBPR_MAX_D.  Every sum is taken in a fixed order: two calls on the same inputs are bit-identical. */
typedef struct nrhip_sbpr_step_args {
  const float* d_P;
  const float* d_Q;
  const float* d_b;
  float* d_G_P;
  float* d_G_Q;
  float* d_G_b;
  uint8_t* d_flag_P;
  uint8_t* d_flag_Q;
  uint8_t* d_flag_b;
  const int32_t* d_users;
  const int32_t* d_items;
  const int32_t* d_social;
  const int32_t* d_neg;
  const float* d_suk;
  uint64_t* d_keys;
  float* d_scal;
  float* d_loss2;
  int n_users, n_items, d, batch, loss_kind;
  float reg;
} nrhip_sbpr_step_args;
int nrhip_sbpr_step(const nrhip_sbpr_step_args* args, void* stream);

/* ---- JCA (joint collaborative autoencoders on a block of the rating matrix; Zhu et al., WWW 2019) -----------------
 *
 * Replaces model/general_recommender/JCA.py.  A block is n_rows batch users d_rows and n_cols batch items d_cols (each
 * distinct, at most batch_size <= NRHIP_JCA_MAX_BATCH), H = hidden_neuron <= NRHIP_JCA_MAX_H:
 *     hu[a]  = g(sum over i in R[r_a,:] of UV[i,:] + Ub1)                              [n_rows, H]
 *     hi[b]  = g((sum over u in R[:,c_b] of IV[u,:] + Ib1) * IF[c_b])                  [n_cols, H]
 *     D[a,b] = (f(hu[a] . UW[:,c_b] + Ub2[c_b]) + f(hi[b] . IW[:,r_a] + Ib2[r_a])) / 2
 *     cost   = sum over pairs (a, bp, bn) of max(0, D[a,bn] - D[a,bp] + margin) + reg * 0.5 * sum over the eight
 *              tables of sum(w^2) / 2      (IF = I_factor_vector is not regularised)
 * Every variable, its two optimiser slots and its gradient live at the same offsets of four flat float arrays d_W, d_M,
 * d_V and d_G, in this order: UV [I][H], UWt [I][H] (UW transposed), IV [U][H], IWt [U][H] (IW transposed), Ub2 [I],
 * IF [I], Ib2 [U], Ub1 [H], Ib1 [H]: 2 (U + I) H + 2 I + U + 2 H floats.  d_flag (uint8 [4 I + 3 U]): the touched rows
 * of UV, UWt, IV, IWt, then of Ub2, IF, Ib2.  d_indptr / d_indices: the train CSR; d_t_indptr / d_t_users: its transpose
 * (users ascending per item).  d_rowslot int64 [U] and d_colslot int64 [I] (zero at first) map a batch row or column to
 * its position under `stamp`, which the caller raises by one per call (>= 1).  nrhip_jca_workspace fills out[4]: the
 * floats of d_wsf, the int32 of d_wsi, the doubles of d_wsd and the uint32 of d_pairs for (U, I, H, batch_size, num_neg).
 * The ids of d_rows / d_cols / users / items are the caller's to check: they index tables.
 *
 * nrhip_jca_pairs: the block's observed bit set (n_rows x n_cols bits, built in LDS a row per wavefront) and the pair
 * list, row-major over the stored entries of the block, num_neg pairs each, one uint32 a << 18 | bp << 9 | bn per pair;
 * *d_total = the number of pairs.  A block row with fewer than num_neg unobserved columns gives no pair.  Negative k of
 * the positive at (a, bp) is a pure function of (seed, epoch, block_i, block_j, a * 512 + bp, k, attempt): the
 * generator nr::XorShift64s seeded (seed ^ splitmix64(block_i << 32 | block_j), epoch, (a * 512 + bp) * 8 + k); each
 * attempt is mulhi64(next(), n_cols), rejected if observed or taken by an earlier k; after 64 rejections the
 * mulhi64(next(), free)-th free column in ascending order.
 *
 * nrhip_jca_step: the gradients of one block from n_pairs pairs (nrhip_jca_pairs' or the caller's): d_loss2[0] = the
 * hinge term; the touched rows of d_G are STORED and flagged (the rest of d_G must be zero).  dD is an integer count
 * per cell summed with integer atomics, every float sum is taken in a fixed order: reruns are bit-identical.  A pair is
 * active when D[a,bn] - D[a,bp] + margin > 0.
 *
 * nrhip_jca_apply: one sweep over all nine variables: g + 0.5 reg w on the eight tables, then Adam (adam != 0:
 * `step` = lr_t, TensorFlow's form with epsilon outside the root) or gradient descent (`step` = lr).  A gradient is
 * read only under its flag; d_G and d_flag are zero afterwards.  Under gd with reg == 0 only flagged rows are visited.
 * d_loss2[1] = reg * 0.5 * sum(w^2) / 2 of the variables as they come in (0 when reg == 0).
 *
 * nrhip_jca_encode: which = 0: d_out [n][H] = hu of the users d_ids (NULL: 0..n-1); which = 1: hi of the items.
 * nrhip_jca_score: d_out [n][ld] = D of the users d_users (hu d_hu [n][H]) against every item (d_hi [I][H]).
 * nrhip_jca_score_pairs: d_out [n] = D of (d_users[p], d_items[p]) with hu row d_slot[p] of d_hu. */
#define NRHIP_JCA_MAX_H 128
#define NRHIP_JCA_MAX_BATCH 512
#define NRHIP_JCA_MAX_NEG 8
#define NRHIP_JCA_ACT_SIGMOID 0
#define NRHIP_JCA_ACT_TANH 1
#define NRHIP_JCA_ACT_RELU 2
#define NRHIP_JCA_ACT_ELU 3
#define NRHIP_JCA_ACT_IDENTITY 4
typedef struct nrhip_jca_args {
  float* d_W;
  float* d_M;
  float* d_V;
  float* d_G;
  uint8_t* d_flag;
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const int64_t* d_t_indptr;
  const int32_t* d_t_users;
  int64_t* d_rowslot;
  int64_t* d_colslot;
  float* d_wsf;
  int32_t* d_wsi;
  double* d_wsd;
  const int32_t* d_rows;
  const int32_t* d_cols;
  uint32_t* d_pairs;
  int32_t* d_total;
  float* d_loss2;
  int64_t n_pairs, stamp;
  uint64_t seed, epoch;
  int n_users, n_items, H, batch_size, num_neg, n_rows, n_cols, f_act, g_act, block_i, block_j;
  float margin, reg;
} nrhip_jca_args;
int nrhip_jca_workspace(int n_users, int n_items, int H, int batch_size, int num_neg, int64_t* out);
int nrhip_jca_pairs(const nrhip_jca_args* args, void* stream);
int nrhip_jca_step(const nrhip_jca_args* args, void* stream);
int nrhip_jca_apply(const nrhip_jca_args* args, int adam, float step, float beta1, float beta2, float eps,
                    void* stream);
int nrhip_jca_encode(const nrhip_jca_args* args, int which, const int32_t* d_ids, int n, float* d_out, void* stream);
int nrhip_jca_score(const nrhip_jca_args* args, const int32_t* d_users, int n, const float* d_hu, const float* d_hi,
                    float* d_out, int64_t ld, void* stream);
int nrhip_jca_score_pairs(const nrhip_jca_args* args, const int32_t* d_users, const int32_t* d_items,
                          const int32_t* d_slot, int64_t n, const float* d_hu, const float* d_hi, float* d_out,
                          void* stream);

/* ---- APR (adversarial personalized ranking: BPR-MF with a perturbation of the batch's rows inside the step) ------
 * Replaces: APR._create_loss / _create_adversarial and the optimizer's gradients (model/general_recommender/
 * APR.py:73-118) run as `sess.run([update_P, update_Q])` then `sess.run((loss, opt_loss, minimize(opt_loss)))`.
 * For the triplets t = (u, i, j) over d_P [n_users][d] and d_Q [n_items][d]:
 *     x_t = <P[u], Q[i]> - <P[u], Q[j]>     loss = sum softplus(-x_t)     s_t = -sigmoid(-x_t)           (APR.py:76-80)
 *     Gamma_P[u] = sum_{u_t = u} s_t (Q[i_t] - Q[j_t])
 *     Gamma_Q[r] = sum_{i_t = r} s_t P[u_t] - sum_{j_t = r} s_t P[u_t]                                   (APR.py:110)
 * adversarial == 0:  d_G_* [row] = Gamma[row] (+ reg row, with_reg) for the batch's rows; d_loss2 = {loss, reg l2}.
 * adversarial != 0:  Delta[row] = eps Gamma[row] / sqrt(max(|Gamma[row]|^2, 1e-12))                     (APR.py:117-118)
 *                    (adv_random: Gamma replaced by a truncated normal of stddev 0.01, APR.py:99-104, drawn from
 *                    (seed, step, row, column); d_delta_given [n_users + n_items][d] non-NULL: Delta read from there)
 *     xa_t = <P[u] + Delta_P[u], Q[i] + Delta_Q[i]> - <P[u] + Delta_P[u], Q[j] + Delta_Q[j]>             (APR.py:63-71)
 *     loss_adv = sum softplus(-xa_t)     sa_t = -reg_adv sigmoid(-xa_t)     Delta constant (stop_gradient)
 *     d_G_P[u] = Gamma_P[u] + sum sa_t ((Q + Delta)[i_t] - (Q + Delta)[j_t]) (+ reg P[u])
 *     d_G_Q[r] = Gamma_Q[r] + sum_{i_t = r} sa_t (P + Delta)[u_t] - sum_{j_t = r} sa_t (P + Delta)[u_t] (+ reg Q[r])
 *     d_loss2 = {loss, reg l2 + reg_adv loss_adv}
 * with l2 = sum(P^2) / 2 + sum(Q^2) / 2 over the WHOLE tables (APR.py:83) when with_reg != 0 and reg != 0; then every
 * row of d_G_* outside the batch is additionally SET to reg row (the dense gradient), otherwise only the batch's rows
 * are stored and the others must be zero.  A row's sums run over its occurrences in the order of the sort keys
 * (row << 32 | slot * 4 + role; users, then items at n_users + item, the positive before the negative of a slot).
 * A triplet with an id outside its table takes no part in either pass.  i == j is allowed.
 * d_flag_* (uint8 per row, NULL for Adam): set to 1 for the batch's rows.
 * Work buffers: d_keys uint64 [3 batch], d_scal float [4 batch] (s, softplus, sa, softplus_adv per slot), d_where
 * int32 [3 batch] (per slot and role: the position of its row's run head), d_gamma / d_delta float [3 batch][d]
 * (indexed by that position), d_part double [NRHIP_APR_L2_BLOCKS].
 * n_users + n_items < 2^31 - 1; batch <= NRHIP_APR_MAX_BATCH; batch == 0 launches nothing and writes nothing (with the
 * dense regulariser: the table sweep and the loss kernel alone);
 * d = 1..NRHIP_APR_MAX_D (above: NRHIP_ERR_UNSUPPORTED).  fp32, the loss sums in double by a fixed tree, every sum in a
 * fixed order, no floating-point atomics: two calls on the same inputs are bit-identical. */
#define NRHIP_APR_MAX_D 128
#define NRHIP_APR_MAX_BATCH (1 << 24)
#define NRHIP_APR_L2_BLOCKS 256
typedef struct nrhip_apr_step_args {
  const float* d_P;
  const float* d_Q;
  float* d_G_P;
  float* d_G_Q;
  uint8_t* d_flag_P;
  uint8_t* d_flag_Q;
  const int32_t* d_users;
  const int32_t* d_pos;
  const int32_t* d_neg;
  const float* d_delta_given;
  uint64_t* d_keys;
  float* d_scal;
  int32_t* d_where;
  float* d_gamma;
  float* d_delta;
  double* d_part;
  float* d_loss2;
  uint64_t seed, step;
  int n_users, n_items, d, batch, adversarial, adv_random, with_reg;
  float reg, reg_adv, eps;
} nrhip_apr_step_args;
int nrhip_apr_step(const nrhip_apr_step_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUREC_HIP_H */
