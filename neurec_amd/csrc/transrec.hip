// transrec.hip — TransRec (He et al., RecSys 2017): the step and predict() of model/sequential_recommender/TransRec.py
// on gfx950.
//
// An instance is (user u, recent item l, item i[, negative j]).  Tables P [U][d], Q [I][d], b [I] and ONE dense
// translation vector T [d]:
//     v      = P[u] + T + Q[l] - Q[i]              (added in this order: (P[u] + T) + Q[l], then - Q[i])
//     x(u,l,i) = b[i] - |v|^2                       the training score is the SQUARED distance      TransRec.py:75-77
//     predict  = b[j] - |P[u] + T + Q[last(u)] - Q[j]|   the distance itself                         TransRec.py:102-107
// Q is looked up in three roles in one batch — as the recent item, as the target and as the negative — and a row's
// gradient is the sum over all of them; T takes a gradient from every instance.
//
//   transrec_forward_kernel   one lane group (DP lanes, DP = 16 / 32 / 64 by d) per batch slot: gathers the rows, v (and
//                             v'), the score(s), the loss and its derivative g, the l2 sum, the row flags and the 3 N
//                             sort keys of the slot's lookups — N = B (pointwise) or 2 B (pairwise) — over one key space
//                             of U + I rows, key = row << 32 | position << 2 | role:
//                                 keys [0, N)     P row u          at positions t and B + t          role 0
//                                 keys [N, 2N)    Q row U + l      at positions t and B + t          role 0 (recent)
//                                 keys [2N, 3N)   Q row U + i      at position  t                    role 1 (target)
//                                                 Q row U + j      at position  B + t                role 2 (negative)
//                             the role bits lie below the row: one row is one run, whatever its roles.  A slot that
//                             takes no part writes the sentinel key and g = 0
//   transrec_loss_kernel      one workgroup: the loss and regulariser sums in a fixed order, |T|^2 added once
//   nrhip_sort_u64            the keys, ascending
//   transrec_rows_kernel      one lane group per sorted key: the head of a run walks it and STORES the row's gradient,
//                             every occurrence recomputed from the gathered rows.  The order of the sum is the order of
//                             the sorted keys: by position (the first inference's lookups, positions 0..B, before the
//                             second's, B..2B), and at one position the recent before the target / the negative.
//                                 P[u], Q[l]   first inference  -2 g v + reg own row;   second  +2 g v'  (no reg)
//                                 Q[i]         +2 g v  + reg own row,   G_b[i] += +g + reg b[i]
//                                 Q[j]         -2 g v' + reg own row,   G_b[j] += -g + reg b[j]
//                             G_b[item] is stored by the head of a Q run that holds a target or negative occurrence
//   transrec_gt_kernel        G_T per chunk of the batch: one thread per column, the chunk's instances in batch order,
//                             -2 g v (+ 2 g v')
//   transrec_gt_reduce_kernel the chunks' partials in chunk order, + reg T (once per step), stored
//   transrec_queries_kernel   q = P[u] + T (+ Q[last(u)]) per user
//   transrec_scores_kernel    b[j] - sqrt(sum_c (q_c - Q_jc)^2) in the DIRECT form: subtract, then fused
//                             multiply-accumulate in fp32, ascending column order per output.  A 64 x 64 output tile per
//                             workgroup, 4 x 4 outputs per thread; the tiles of q and Q rows pass through LDS kColumns
//                             columns at a time, column-major with a leading dimension of 68 floats: a thread reads its
//                             4 q values and its 4 Q values of a column as one 16-byte read each (the 16 lanes of a row of
//                             threads read 64 consecutive floats, the 4 rows of a wavefront broadcast)
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

enum { ROLE_RECENT = 0, ROLE_TARGET = 1, ROLE_NEGATIVE = 2 };

__device__ __forceinline__ uint64_t row_key(int row, int pos, int role) {
  return nr::rowkey::row_key(row, ((uint32_t)pos << 2) | (uint32_t)role);
}

__host__ __device__ inline int chunks_of(int B) {
  const int n = (B + NRHIP_TRANSREC_CHUNK - 1) / NRHIP_TRANSREC_CHUNK;
  return B <= 0 ? 0 : n < NRHIP_TRANSREC_MAX_CHUNKS ? n : NRHIP_TRANSREC_MAX_CHUNKS;
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void transrec_forward_kernel(nrhip_transrec_step_args a) {
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
  float si = 0.f, sj = 0.f, sq = 0.f;
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col], ql = a.d_Q[(int64_t)l * d + col];
        const float qi = a.d_Q[(int64_t)i * d + col];
        const float base = p + a.d_T[col] + ql;
        const float v = base - qi;
        si += v * v;
        sq += p * p + ql * ql + qi * qi;
        if (a.pairwise) {
          const float qj = a.d_Q[(int64_t)j * d + col];
          const float w = base - qj;
          sj += w * w;
          sq += qj * qj;
        }
      }
    }
  }
  group_sum<DP>(si, sj, sq);
  if (!in || c != 0) return;
  float g = 0.f, loss = 0.f;
  if (ok) {
    const float bi = a.d_b[i];
    const float xi = bi - si;
    float xj = 0.f;
    sq += bi * bi;
    if (a.pairwise) {
      const float bj = a.d_b[j];
      xj = bj - sj;
      sq += bj * bj;
    }
    instance_loss_g(a.pairwise, a.loss_kind, B, a.d_third, t, xi, xj, loss, g);
    if (a.d_flag_P) a.d_flag_P[u] = 1;
    if (a.d_flag_Q) {
      a.d_flag_Q[l] = 1;
      a.d_flag_Q[i] = 1;
      if (a.pairwise) a.d_flag_Q[j] = 1;
    }
    if (a.d_flag_b) {
      a.d_flag_b[i] = 1;
      if (a.pairwise) a.d_flag_b[j] = 1;
    }
  }
  float* sc = a.d_scal + (int64_t)t * kScal;
  store_slot(sc, g, loss, sq, ok);
  sc[S_OK] = ok ? 1.f : 0.f;
  a.d_keys[t] = ok ? row_key(u, t, ROLE_RECENT) : kSentinel;
  a.d_keys[N + t] = ok ? row_key(U + l, t, ROLE_RECENT) : kSentinel;
  a.d_keys[2 * (int64_t)N + t] = ok ? row_key(U + i, t, ROLE_TARGET) : kSentinel;
  if (a.pairwise) {
    a.d_keys[B + t] = ok ? row_key(u, B + t, ROLE_RECENT) : kSentinel;
    a.d_keys[N + B + t] = ok ? row_key(U + l, B + t, ROLE_RECENT) : kSentinel;
    a.d_keys[2 * (int64_t)N + B + t] = ok ? row_key(U + j, B + t, ROLE_NEGATIVE) : kSentinel;
  }
}

__global__ __launch_bounds__(256) void transrec_loss_kernel(nrhip_transrec_step_args a) {
  double v[2] = {0.0, 0.0};
  slot_sums(a.d_scal, a.batch, v[0], v[1]);
  // l2_loss(..., global_embedding): T enters once per step (TransRec.py:88,91)
  for (int c = threadIdx.x; c < a.d; c += 256) v[1] += 0.5 * (double)a.d_T[c] * (double)a.d_T[c];
  block_sum(v);
  if (threadIdx.x == 0) {
    a.d_loss2[0] = (float)v[0];
    a.d_loss2[1] = (float)((double)a.reg * v[1]);
  }
}

// the sum of one run of the sorted keys: the row's occurrences in key order, each recomputed from the gathered rows
template <int DP, int CPL>
__global__ __launch_bounds__(256) void transrec_rows_kernel(nrhip_transrec_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int B = a.batch, d = a.d, U = a.n_users;
  const int64_t n_keys = 3 * (int64_t)(a.pairwise ? 2 * B : B);
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  const float reg = a.reg;
  const int32_t* negs = (const int32_t*)a.d_third;
  const bool is_user = row < U;
  const int r = is_user ? row : row - U;
  float own[CPL], acc[CPL] = {};
  load_row<DP, CPL>(is_user ? a.d_P : a.d_Q, r, d, c, own);
  float gb = 0.f;
  bool has_b = false;
  const float own_b = is_user ? 0.f : a.d_b[r];
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t low) {
    const int role = (int)(low & 3u), pos = (int)(low >> 2);
    const bool second = pos >= B;
    const int t = second ? pos - B : pos;
    const float g = a.d_scal[(int64_t)t * kScal + S_G];
    const int u = a.d_users[t], l = a.d_recent[t], x = second ? negs[t] : a.d_items[t];
    // d score / d row: -2 v for P[u], Q[l] and T, +2 v for the target's own row; the second inference's score enters
    // y = x - x' with a minus sign.  The regulariser reaches the first inference's P[u] and Q[l] and every target row
    float s;
    bool with_reg;
    if (role == ROLE_RECENT) {
      s = second ? 2.0f * g : -2.0f * g;
      with_reg = !second;
    } else {
      s = second ? -2.0f * g : 2.0f * g;
      with_reg = true;
      gb += (second ? -g : g) + reg * own_b;
      has_b = true;
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float base = a.d_P[(int64_t)u * d + col] + a.d_T[col] + a.d_Q[(int64_t)l * d + col];
        const float v = base - a.d_Q[(int64_t)x * d + col];
        acc[k] += with_reg ? s * v + reg * own[k] : s * v;
      }
    }
  });
  store_row<DP, CPL>(is_user ? a.d_G_P : a.d_G_Q, r, d, c, acc);
  if (has_b && c == 0) a.d_G_b[r] = gb;                  // a run of recents alone leaves G_b[r] as it is
}

// G_T of one chunk of the batch: thread = column, the chunk's instances in batch order
__global__ __launch_bounds__(NRHIP_TRANSREC_MAX_D) void transrec_gt_kernel(nrhip_transrec_step_args a, int chunks) {
  const int c = threadIdx.x, d = a.d, B = a.batch;
  if (c >= d) return;
  const int per = (B + chunks - 1) / chunks;
  const int t0 = blockIdx.x * per, t1 = min(B, t0 + per);
  const float tc = a.d_T[c];
  float acc = 0.f;
  for (int t = t0; t < t1; ++t) {
    const float* sc = a.d_scal + (int64_t)t * kScal;
    if (sc[S_OK] == 0.f) continue;
    const float g = sc[S_G];
    const float base = a.d_P[(int64_t)a.d_users[t] * d + c] + tc + a.d_Q[(int64_t)a.d_recent[t] * d + c];
    acc += -2.0f * g * (base - a.d_Q[(int64_t)a.d_items[t] * d + c]);
    if (a.pairwise) acc += 2.0f * g * (base - a.d_Q[(int64_t)((const int32_t*)a.d_third)[t] * d + c]);
  }
  a.d_partial[(int64_t)blockIdx.x * d + c] = acc;
}

__global__ __launch_bounds__(NRHIP_TRANSREC_MAX_D) void transrec_gt_reduce_kernel(nrhip_transrec_step_args a,
                                                                                  int chunks) {
  const int c = threadIdx.x, d = a.d;
  if (c >= d) return;
  float acc = 0.f;
  for (int y = 0; y < chunks; ++y) acc += a.d_partial[(int64_t)y * d + c];
  a.d_G_T[c] = acc + a.reg * a.d_T[c];                     // the regulariser reaches T once per step
}

__global__ __launch_bounds__(256) void transrec_queries_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                               const float* __restrict__ T, int n_users, int n_items,
                                                               int d, const int32_t* __restrict__ last,
                                                               const int32_t* __restrict__ users, int batch,
                                                               float* __restrict__ out, int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * d) return;
  const int b = (int)(idx / d), col = (int)(idx - (int64_t)b * d);
  const int u = users ? users[b] : b;
  float v = 0.f;
  if (u >= 0 && u < n_users) {
    v = P[(int64_t)u * d + col] + T[col];
    const int l = last[u];
    if (l >= 0 && l < n_items) v += Q[(int64_t)l * d + col];
  }
  out[(int64_t)b * ld + col] = v;
}

constexpr int kTile = 64;          // q rows and Q rows of a workgroup's output tile
constexpr int kColumns = 32;       // columns staged in LDS at a time
constexpr int kLd = kTile + 4;     // floats per staged column: 16-byte aligned, and the transposing writes of a
                                   // wavefront (32 columns of 2 rows) fall on 8 banks four deep instead of on one

// rows [r0, r0 + 64) x columns [c0, c0 + 32) of src [n_rows][ld] into dst [column][kLd], zeros beyond the edges
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int64_t ld, int n_rows, int d, int r0, int c0,
                                           float* dst) {
  for (int e = threadIdx.x; e < kTile * kColumns; e += 256) {
    const int rr = e / kColumns, cc = e % kColumns;
    const int row = r0 + rr, col = c0 + cc;
    dst[cc * kLd + rr] = (row < n_rows && col < d) ? src[(int64_t)row * ld + col] : 0.f;
  }
}

__global__ __launch_bounds__(256) void transrec_scores_kernel(const float* __restrict__ q, int64_t ldq,
                                                              const float* __restrict__ Q, const float* __restrict__ b,
                                                              int n, int n_items, int d, float* __restrict__ out,
                                                              int64_t ld) {
  __shared__ __attribute__((aligned(16))) float s_q[kColumns * kLd];
  __shared__ __attribute__((aligned(16))) float s_Q[kColumns * kLd];
  const int i0 = blockIdx.x * kTile, n0 = blockIdx.y * kTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;    // items i0 + 4 tx + (0..3), users n0 + 4 ty + (0..3)
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.f;
  for (int c0 = 0; c0 < d; c0 += kColumns) {
    __syncthreads();
    stage_tile(q, ldq, n, d, n0, c0, s_q);
    stage_tile(Q, d, n_items, d, i0, c0, s_Q);
    __syncthreads();
    // the columns beyond d hold zeros on both sides: their difference is 0 and leaves every sum as it is
#pragma unroll 8
    for (int cc = 0; cc < kColumns; ++cc) {
      const float4 qa = *reinterpret_cast<const float4*>(s_q + cc * kLd + 4 * ty);
      const float4 qb = *reinterpret_cast<const float4*>(s_Q + cc * kLd + 4 * tx);
      const float qv[4] = {qa.x, qa.y, qa.z, qa.w}, iv[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float diff = qv[r] - iv[s];
          acc[r][s] = __builtin_fmaf(diff, diff, acc[r][s]);
        }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int item = i0 + 4 * tx + s;
    if (item >= n_items) continue;
    const float bias = b[item];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + 4 * ty + r;
      if (row < n) out[(int64_t)row * ld + item] = bias - sqrtf(acc[r][s]);
    }
  }
}

}  // namespace

extern "C" {

int nrhip_transrec_step(const nrhip_transrec_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "transrec_step: null argument block");
  const nrhip_transrec_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_TRANSREC_MAX_D, NR_ERR_UNSUPPORTED,
             "transrec_step: embedding_size %d outside 1..%d", a.d, NRHIP_TRANSREC_MAX_D);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_TRANSREC_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG,
             "transrec_step: bad sizes");
  NR_TRY(check_loss_kind("transrec_step", a.pairwise, a.loss_kind));
  const int B = a.batch;
  if (B == 0) return NR_OK;                                // no work: nothing is launched, nothing is written
  NR_REQUIRE(a.d_P && a.d_Q && a.d_b && a.d_T && a.d_G_P && a.d_G_Q && a.d_G_b && a.d_G_T && a.d_users && a.d_recent &&
                 a.d_items && a.d_third && a.d_keys && a.d_scal && a.d_partial && a.d_loss2, NR_ERR_ARG,
             "transrec_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int n_keys = 3 * B * (a.pairwise ? 2 : 1), chunks = chunks_of(B);
  NR_BY_WIDTH(transrec_forward_kernel, a.d, B, st, a);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(a.d_keys, n_keys, stream));
  hipLaunchKernelGGL(transrec_loss_kernel, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  NR_BY_WIDTH(transrec_rows_kernel, a.d, n_keys, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(transrec_gt_kernel, dim3(chunks), dim3(NRHIP_TRANSREC_MAX_D), 0, st, a, chunks);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(transrec_gt_reduce_kernel, dim3(1), dim3(NRHIP_TRANSREC_MAX_D), 0, st, a, chunks);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_transrec_queries(const float* d_P, const float* d_Q, const float* d_T, int n_users, int n_items, int d,
                           const int32_t* d_last, const int32_t* d_users, int batch, float* d_out, int64_t ld,
                           void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_TRANSREC_MAX_D, NR_ERR_UNSUPPORTED,
             "transrec_queries: embedding_size %d outside 1..%d", d, NRHIP_TRANSREC_MAX_D);
  NR_REQUIRE(n_users >= 0 && n_items >= 0 && batch >= 0 && ld >= d && (d_users || batch <= n_users), NR_ERR_ARG,
             "transrec_queries: bad sizes");
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_P && (d_Q || n_items == 0) && d_T && d_last && d_out, NR_ERR_ARG,
             "transrec_queries: null pointer argument");
  const int64_t n = (int64_t)batch * d;
  hipLaunchKernelGGL(transrec_queries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_P,
                     d_Q, d_T, n_users, n_items, d, d_last, d_users, batch, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_transrec_scores(const float* d_q, int64_t ldq, const float* d_Q, const float* d_b, int n, int n_items, int d,
                          float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_TRANSREC_MAX_D, NR_ERR_UNSUPPORTED,
             "transrec_scores: embedding_size %d outside 1..%d", d, NRHIP_TRANSREC_MAX_D);
  NR_REQUIRE(n >= 0 && n_items >= 0 && ldq >= d && ld >= n_items && (n + kTile - 1) / kTile <= 65535, NR_ERR_ARG,
             "transrec_scores: bad sizes");
  if (n == 0 || n_items == 0) return NR_OK;
  NR_REQUIRE(d_q && d_Q && d_b && d_out, NR_ERR_ARG, "transrec_scores: null pointer argument");
  const dim3 grid((n_items + kTile - 1) / kTile, (n + kTile - 1) / kTile);
  hipLaunchKernelGGL(transrec_scores_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_q, ldq, d_Q, d_b, n, n_items, d,
                     d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
