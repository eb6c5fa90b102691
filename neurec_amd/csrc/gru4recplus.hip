// gru4recplus.hip — GRU4RecPlus (Hidasi & Karatzoglou, "Recurrent Neural Networks with Top-k Gains for Session-based
// Recommendations", CIKM 2018): the step of model/sequential_recommender/GRU4RecPlus.py on gfx950.  The stack, the
// states, the users' final states and predict() are GRU4Rec's (gru4rec_cell.h, gru4rec.hip); what is this model's own
// is the B x M logit block, M = B + n_sample, and its row loss.
//
// X holds B items, Y holds M: the first B are the positives (the positive of row i is column i, tf.eye(b, size_y)),
// the rest the sampled negatives every row shares.  Row i of the loss on A = final_act(Z), p = A_ii:
//     hm_j = [j != i];  m = max_j (A_ij hm_j) >= 0;  e_j = hm_j exp(A_ij hm_j - m);  s_j = e_j / sum e
//     bpr_max   f_j = sigmoid(p - A_ij);  P = sum_j s_j f_j;  R = sum_j s_j A_ij^2;  L_i = -log(P + 1e-24) + bpr_reg R
//     top1_max  g_j = sigmoid(A_ij - p) + sigmoid(A_ij^2);    L_i = sum_j s_j g_j
// and the loss is mean_i L_i.  The softmax weights are differentiated: with c_j = dL_i/ds_j and C = sum_k s_k c_k,
//     j != i:   dL_i/dA_ij = s_j (c_j - C) + (the direct terms through f_j or g_j and A_ij^2)
//     j == i:   dL_i/dp alone (the masked diagonal has weight 0)
//     bpr_max   c_j = -f_j / (P + eps) + bpr_reg A_ij^2;  direct: s_j f_j (1 - f_j) / (P + eps) + 2 bpr_reg s_j A_ij
//               dL_i/dp = -sum_j s_j f_j (1 - f_j) / (P + eps)
//     top1_max  c_j = g_j;  direct: s_j (e_j' + 2 A_ij q_j'), e' and q' the two sigmoids' derivatives
//               dL_i/dp = -sum_j s_j e_j'
// The shift m cancels and is a constant here.
//
// One step (nrhip_gru4recplus_step):
//   plus_gather_kernel    x0 = E_in[X] and the keys of X; Qy = Q[Y] [M][n], by = b[Y] [M] — gathered ONCE, contiguous —
//                         and the keys of Y
//   gru_gates_kernel, gru_cand_kernel            the stack (gru4rec_cell.h)
//   plus_tile_kernel      the three products, 64 x 64 outputs per workgroup, 4 x 4 per thread, both operands staged
//                         through LDS 32 reduction steps at a time; every output one k-ascending fmaf chain:
//                             Z [B][M]        = h_top Qy^T + by
//                             dh_top [B][n]   = dZ Qy        in chunks of >= 128 columns of dZ (few outputs, a long
//                                               sum: the chunks give the device work), then plus_chunksum_kernel adds
//                                               the chunks in ascending order
//                             sQ [M][n]       = dZ^T h_top + reg Qy    per SLOT
//   plus_lossrow_kernel   one workgroup per row: the row staged once in LDS, the max, the sum and the loss's sums by
//                         fixed-order trees, the max subtracted before any exp; dLoss/dZ of the row
//   plus_colsum_kernel    per slot j: sb = sum_i dZ[i][j] + reg by[j], and the slot's share of the regulariser
//   gru_cellbwd_kernel .. gru_dw_kernel          the stack's backward pass (gru4rec_cell.h)
//   nrhip_sort_u64        the two key lists (B and M keys)
//   gru_rows_kernel       duplicates summed in slot order and stored once (gru4rec_cell.h)
//   plus_loss_kernel      one workgroup: the two REPORTED sums, added in double and rounded to float once
// Everything that reaches a gradient, a state or a table is fp32.  No atomics anywhere: two runs are bit-identical.
#include "gru4rec_cell.h"

namespace {

enum { LOSS_TOP1_MAX = 0, LOSS_BPR_MAX = 1 };
constexpr int kMaxM = NRHIP_GRU4REC_MAX_BATCH + NRHIP_GRU4RECPLUS_MAX_SAMPLE;     // floats of a staged row: 48 KiB
constexpr float kEps = 1e-24f;     // inside the bpr_max log (GRU4RecPlus.py:107)
constexpr int kTile = 64;          // rows and columns of a workgroup's output tile
constexpr int kSteps = 32;         // reduction steps staged in LDS at a time
constexpr int kLd = kTile + 4;     // floats per staged step, 16-byte aligned
constexpr int kChunkMin = 128;     // columns of dZ per chunk of the dh_top product, at least
constexpr int kChunksMax = 32;     // and at most this many chunks (the partial sums are [chunks][B][n] floats)

// the float work buffer of a step: offsets in floats
struct Layout {
  size_t x0, gate[kL], c[kL], dpg[kL], dpc[kL], dhA, dhB, Qy, by, Z, dZ, rowloss, sQ, sb, part, l2, total;
};
// the chunk length for M columns, a multiple of kSteps, and the number of chunks: a function of M alone
inline int chunk_len(int M) {
  int n = (M + kChunkMin - 1) / kChunkMin;
  n = n < 1 ? 1 : (n > kChunksMax ? kChunksMax : n);
  return ((M + n - 1) / n + kSteps - 1) / kSteps * kSteps;
}
inline int chunks_of(int M) { return M > 0 ? (M + chunk_len(M) - 1) / chunk_len(M) : 1; }
Layout layout_of(int L, const int* w, int B, int n_sample) {
  Layout y;
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += (n + 3) / 4 * 4;
    return at;
  };
  const size_t b = (size_t)B, m = (size_t)B + (size_t)n_sample, nl = (size_t)w[L - 1];
  y.x0 = take(b * w[0]);
  for (int l = 0; l < kL; ++l) {
    const size_t n = l < L ? (size_t)w[l] : 0;
    y.gate[l] = take(b * 2 * n);
    y.c[l] = take(b * n);
    y.dpg[l] = take(b * 2 * n);
    y.dpc[l] = take(b * n);
  }
  y.dhA = take(b * kW);
  y.dhB = take(b * kW);
  y.Qy = take(m * nl);
  y.by = take(m);
  y.Z = take(b * m);
  y.dZ = take(b * m);
  y.rowloss = take(b);
  y.sQ = take(m * nl);
  y.sb = take(m);
  y.part = take((size_t)kChunksMax * b * nl);      // not chunks_of(m): every region grows with the batch, so the buffer
                                                   // sized for max_batch holds the layout of every smaller batch
  y.l2 = take(2 * m);              // M doubles (every offset is a multiple of 16 bytes)
  y.total = o;
  return y;
}

// out[t] = T[ids[t]] (a row of zeros for an id outside the table), the bias likewise, and the sort key of the slot
__global__ __launch_bounds__(256) void plus_gather_kernel(const float* __restrict__ T, const float* __restrict__ bias,
                                                          const int32_t* __restrict__ ids, int n_items, int n, int d,
                                                          float* __restrict__ out, float* __restrict__ bias_out,
                                                          uint64_t* __restrict__ keys) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n * d) return;
  const int t = (int)(idx / d), k = (int)(idx - (int64_t)t * d);
  const int id = ids[t];
  const bool ok = id >= 0 && id < n_items;
  out[idx] = ok ? T[(int64_t)id * d + k] : 0.0f;
  if (k == 0) {
    keys[t] = ok ? (((uint64_t)(uint32_t)id << 32) | (uint32_t)t) : kSentinel;
    if (bias) bias_out[t] = ok ? bias[id] : 0.0f;
  }
}

// An operand of plus_tile_kernel is read as op(o, k): o the output index (row or column of the tile), k the reduction
// index.  kAcross = false: src[o][k], k contiguous; true: src[k][o], o contiguous.  A thread holds kPerThread values of
// a block of kSteps reduction steps in registers (load_operand) and puts them into LDS k-major, dst[kk][o]
// (store_operand): the loads of the next block are in flight while the current one is multiplied.
// Beyond n_out or k_end: zeros, which leave every sum as it is.
constexpr int kPerThread = kTile * kSteps / 256;
template <bool kAcross>
__device__ __forceinline__ void load_operand(const float* __restrict__ src, int64_t ld, int n_out, int k_end, int o0,
                                             int k0, float (&reg)[kPerThread]) {
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int e = q * 256 + threadIdx.x;
    const int oo = kAcross ? e % kTile : e / kSteps, kk = kAcross ? e / kTile : e % kSteps;
    const int o = o0 + oo, k = k0 + kk;
    float v = 0.0f;
    if (o < n_out && k < k_end) v = kAcross ? src[(int64_t)k * ld + o] : src[(int64_t)o * ld + k];
    reg[q] = v;
  }
}
template <bool kAcross>
__device__ __forceinline__ void store_operand(const float (&reg)[kPerThread], float* dst) {
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int e = q * 256 + threadIdx.x;
    const int oo = kAcross ? e % kTile : e / kSteps, kk = kAcross ? e / kTile : e % kSteps;
    dst[kk * kLd + oo] = reg[q];
  }
}

// out[z][r][c] = sum_{k in chunk z} opA(r, k) opB(c, k)  (+ colbias[c])  (+ scale add[r][c]);  grid (column tiles, row
// tiles, chunks), a chunk kchunk reduction steps long
template <bool kAcrossA, bool kAcrossB>
__global__ __launch_bounds__(256) void plus_tile_kernel(const float* __restrict__ A, int64_t lda,
                                                        const float* __restrict__ Bm, int64_t ldb, int n_rows,
                                                        int n_cols, int K, int kchunk, const float* __restrict__ colbias,
                                                        const float* __restrict__ add, float scale,
                                                        float* __restrict__ out, int64_t ldo, int64_t chunk_stride) {
  __shared__ __attribute__((aligned(16))) float s_a[kSteps * kLd];
  __shared__ __attribute__((aligned(16))) float s_b[kSteps * kLd];
  const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
  const int k_begin = blockIdx.z * kchunk;
  const int k_end = k_begin + kchunk < K ? k_begin + kchunk : K;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.0f;
  float ga[kPerThread], gb[kPerThread];
  load_operand<kAcrossA>(A, lda, n_rows, k_end, r0, k_begin, ga);
  load_operand<kAcrossB>(Bm, ldb, n_cols, k_end, c0, k_begin, gb);
  for (int k0 = k_begin; k0 < k_end; k0 += kSteps) {
    __syncthreads();                                       // every read of the previous block is done
    store_operand<kAcrossA>(ga, s_a);
    store_operand<kAcrossB>(gb, s_b);
    __syncthreads();
    if (k0 + kSteps < k_end) {
      load_operand<kAcrossA>(A, lda, n_rows, k_end, r0, k0 + kSteps, ga);
      load_operand<kAcrossB>(Bm, ldb, n_cols, k_end, c0, k0 + kSteps, gb);
    }
#pragma unroll 8
    for (int kk = 0; kk < kSteps; ++kk) {
      const float4 ra = *reinterpret_cast<const float4*>(s_a + kk * kLd + 4 * ty);
      const float4 cb = *reinterpret_cast<const float4*>(s_b + kk * kLd + 4 * tx);
      const float av[4] = {ra.x, ra.y, ra.z, ra.w}, bv[4] = {cb.x, cb.y, cb.z, cb.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = __builtin_fmaf(av[r], bv[s], acc[r][s]);
    }
  }
  float* o = out + (int64_t)blockIdx.z * chunk_stride;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * ty + r;
    if (row >= n_rows) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int col = c0 + 4 * tx + s;
      if (col >= n_cols) continue;
      float v = acc[r][s];
      if (colbias) v += colbias[col];
      if (add) v += scale * add[(int64_t)row * ldo + col];
      o[(int64_t)row * ldo + col] = v;
    }
  }
}

// dst[e] = sum_z part[z][e], z ascending
__global__ __launch_bounds__(256) void plus_chunksum_kernel(const float* __restrict__ part, int n_chunks, int64_t n,
                                                            float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float acc = part[idx];
  for (int z = 1; z < n_chunks; ++z) acc += part[(int64_t)z * n + idx];
  dst[idx] = acc;
}

// fixed-order trees over the workgroup's 256 values; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    __syncthreads();
  }
  const float r = s[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_max(float v, float* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] = fmaxf(s[threadIdx.x], s[threadIdx.x + h]);
    __syncthreads();
  }
  const float r = s[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float dsigmoidf_(float x) { return sigmoidf_(x) * sigmoidf_(-x); }
// sigmoid(x) - sigmoid(y)
__device__ __forceinline__ float sigmoid_diff(float x, float y) {
  return (x > 0.0f && y > 0.0f) ? sigmoidf_(-y) - sigmoidf_(-x) : sigmoidf_(x) - sigmoidf_(y);
}

// row i of the B x M loss (the file's header has the formulas); every term of the mean carries 1 / B.
// c_j - C is taken against the row's largest negative, score a*:  c_j - C = (c_j - c*) - sum_k s_k (c_k - c*), with
// every difference formed from the differences of its parts (f_j - f*, (a_j - a*)(a_j + a*), ...).  When the softmax
// is close to one-hot c_j and C agree to many digits and their plain difference is all rounding; these keep their
// digits.  For the same reason sigmoid' is sigmoid(x) sigmoid(-x), never s (1 - s), and a difference of two sigmoids
// whose arguments are both positive is taken between the small tails.
__global__ __launch_bounds__(256) void plus_lossrow_kernel(const float* __restrict__ Z, int B, int M, int fin,
                                                           int loss_kind, float bpr_reg, float* __restrict__ dZ,
                                                           float* __restrict__ rowloss) {
  __shared__ float s_row[kMaxM];
  __shared__ float s_red[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* z = Z + (int64_t)i * M;
  float* dz = dZ + (int64_t)i * M;
  float mx = -INFINITY;
  for (int j = tid; j < M; j += 256) {
    const float a = final_act(fin, z[j]);
    s_row[j] = a;
    if (j != i) mx = fmaxf(mx, a);
  }
  const float astar = block_max(mx, s_red);                // its first barrier publishes s_row; M >= 2: a negative exists
  const float m = fmaxf(astar, 0.0f);                      // the masked diagonal's 0 takes part in the max
  const float p = s_row[i];
  float se = 0.0f;
  for (int j = tid; j < M; j += 256)
    if (j != i) se += expf(s_row[j] - m);
  const float S = block_sum(se, s_red);
  const bool bpr = loss_kind == LOSS_BPR_MAX;
  // bpr_max: f = sigmoid(p - a); top1_max: e = sigmoid(a - p), q = sigmoid(a^2)
  // t0: the loss's sum; t1: sum s a^2; t2: sum s sigmoid'; d0, d1: sum s (part of c - its value at a*)
  float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, d0 = 0.0f, d1 = 0.0f;
  for (int j = tid; j < M; j += 256) {
    if (j == i) continue;
    const float a = s_row[j], s = expf(a - m) / S;
    if (bpr) {
      const float f = sigmoidf_(p - a);
      t0 += s * f;
      t1 += s * (a * a);
      t2 += s * dsigmoidf_(p - a);
      d0 += s * sigmoid_diff(p - a, p - astar);
      d1 += s * ((a - astar) * (a + astar));
    } else {
      const float e = sigmoidf_(a - p), q = sigmoidf_(a * a);
      t0 += s * (e + q);
      t2 += s * dsigmoidf_(a - p);
      d0 += s * (sigmoid_diff(a - p, astar - p) + sigmoid_diff(a * a, astar * astar));
    }
  }
  t0 = block_sum(t0, s_red);
  t1 = block_sum(t1, s_red);
  t2 = block_sum(t2, s_red);
  d0 = block_sum(d0, s_red);
  d1 = block_sum(d1, s_red);
  const float inv = 1.0f / (float)B;
  const float den = t0 + kEps;                             // bpr_max: P + eps
  float loss, Cd, dp;                                      // Cd = C - c*
  if (bpr) {
    loss = -logf(den) + bpr_reg * t1;
    Cd = -d0 / den + bpr_reg * d1;
    dp = -t2 / den;
  } else {
    loss = t0;
    Cd = d0;
    dp = -t2;
  }
  for (int j = tid; j < M; j += 256) {
    const float a = s_row[j];
    float da;
    if (j == i) {
      da = dp;
    } else {
      const float s = expf(a - m) / S;
      if (bpr) {
        const float cd = -sigmoid_diff(p - a, p - astar) / den + bpr_reg * ((a - astar) * (a + astar));
        da = s * (cd - Cd) + s * dsigmoidf_(p - a) / den + bpr_reg * (s * (2.0f * a));
      } else {
        const float cd = sigmoid_diff(a - p, astar - p) + sigmoid_diff(a * a, astar * astar);
        da = s * (cd - Cd) + s * (dsigmoidf_(a - p) + 2.0f * a * dsigmoidf_(a * a));
      }
    }
    dz[j] = da * final_dact(fin, a) * inv;                 // a > 0 exactly where z > 0, for relu and leaky_relu alike
  }
  if (tid == 0) rowloss[i] = loss * inv;
}

// per SLOT j: sb[j] = sum_i dZ[i][j] + reg by[j] (i ascending);  l2[j] = |Qy[j]|^2 + by[j]^2 in double
__global__ __launch_bounds__(256) void plus_colsum_kernel(const float* __restrict__ dZ, const float* __restrict__ Qy,
                                                          const float* __restrict__ by, int B, int M, int n, float reg,
                                                          float* __restrict__ sb, double* __restrict__ l2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  float acc = 0.0f;
#pragma unroll 8
  for (int i = 0; i < B; ++i) acc += dZ[(int64_t)i * M + j];
  const float bj = by[j];
  sb[j] = acc + reg * bj;
  double q = (double)bj * (double)bj;
  for (int k = 0; k < n; ++k) q += (double)Qy[(int64_t)j * n + k] * (double)Qy[(int64_t)j * n + k];
  l2[j] = q;
}

__global__ __launch_bounds__(256) void plus_loss_kernel(const float* __restrict__ rowloss, const float* __restrict__ x0,
                                                        const double* __restrict__ l2, int B, int M, int n0, float reg,
                                                        float* __restrict__ loss2) {
  __shared__ double s_a[256], s_b[256];
  double la = 0.0, lb = 0.0;
  for (int t = threadIdx.x; t < B; t += 256) {
    la += (double)rowloss[t];
    double q = 0.0;
    for (int k = 0; k < n0; ++k) q += (double)x0[(int64_t)t * n0 + k] * (double)x0[(int64_t)t * n0 + k];
    lb += 0.5 * q;
  }
  for (int j = threadIdx.x; j < M; j += 256) lb += 0.5 * l2[j];
  s_a[threadIdx.x] = la;
  s_b[threadIdx.x] = lb;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_a[threadIdx.x] += s_a[threadIdx.x + s];
      s_b[threadIdx.x] += s_b[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss2[0] = (float)s_a[0];
    loss2[1] = (float)((double)reg * s_b[0]);
  }
}

int check_sizes(const char* who, int batch, int n_sample) {
  NR_REQUIRE(batch >= 0 && batch <= NRHIP_GRU4REC_MAX_BATCH, NR_ERR_UNSUPPORTED, "%s: batch %d outside 0..%d", who, batch,
             NRHIP_GRU4REC_MAX_BATCH);
  NR_REQUIRE(n_sample >= 0 && n_sample <= NRHIP_GRU4RECPLUS_MAX_SAMPLE, NR_ERR_UNSUPPORTED,
             "%s: n_sample %d outside 0..%d", who, n_sample, NRHIP_GRU4RECPLUS_MAX_SAMPLE);
  return NR_OK;
}

inline unsigned tiles_of(int n) { return (unsigned)((n + kTile - 1) / kTile); }

}  // namespace

extern "C" {

int nrhip_gru4recplus_workspace_floats(int n_layers, const int* widths, int max_batch, int n_sample, size_t* floats) {
  NR_REQUIRE(widths && floats, NR_ERR_ARG, "gru4recplus_workspace_floats: null argument");
  NR_REQUIRE(n_layers >= 1 && n_layers <= kL, NR_ERR_UNSUPPORTED,
             "gru4recplus_workspace_floats: %d layers outside 1..%d", n_layers, kL);
  for (int l = 0; l < n_layers; ++l)
    NR_REQUIRE(widths[l] >= 1 && widths[l] <= kW, NR_ERR_UNSUPPORTED,
               "gru4recplus_workspace_floats: layer width %d outside 1..%d", widths[l], kW);
  NR_TRY(check_sizes("gru4recplus_workspace_floats", max_batch, n_sample));
  *floats = layout_of(n_layers, widths, max_batch, n_sample).total;
  return NR_OK;
}

int nrhip_gru4recplus_step(const nrhip_gru4recplus_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "gru4recplus_step: null argument block");
  const nrhip_gru4recplus_step_args a = *args;
  NR_TRY(check_weights(a.w, "gru4recplus_step"));
  NR_TRY(check_sizes("gru4recplus_step", a.batch, a.n_sample));
  NR_REQUIRE(a.n_items >= 0, NR_ERR_ARG, "gru4recplus_step: bad sizes");
  NR_REQUIRE(a.final_act >= FIN_LINEAR && a.final_act <= FIN_LEAKY, NR_ERR_ARG,
             "gru4recplus_step: unknown final_act %d (0 linear, 1 relu, 2 leaky_relu)", a.final_act);
  NR_REQUIRE(a.loss_kind == LOSS_TOP1_MAX || a.loss_kind == LOSS_BPR_MAX, NR_ERR_ARG,
             "gru4recplus_step: unknown loss %d (0 top1_max, 1 bpr_max)", a.loss_kind);
  const int B = a.batch, L = a.w.n_layers, M = a.batch + a.n_sample;
  if (B == 0) return NR_OK;
  NR_REQUIRE(M >= 2, NR_ERR_UNSUPPORTED,
             "gru4recplus_step: batch + n_sample = %d: a row needs at least one negative (the softmax over none is 0 / 0)",
             M);
  NR_REQUIRE(a.d_Ein && a.d_Q && a.d_b && a.d_G_Ein && a.d_G_Q && a.d_G_b && a.d_X && a.d_Y && a.d_keys && a.d_ws &&
                 a.d_loss2, NR_ERR_ARG, "gru4recplus_step: null pointer argument");
  for (int l = 0; l < L; ++l)
    NR_REQUIRE(a.d_G_Wg[l] && a.d_G_bg[l] && a.d_G_Wc[l] && a.d_G_bc[l] && a.d_state[l] && a.d_h_new[l], NR_ERR_ARG,
               "gru4recplus_step: null pointer argument (layer %d)", l);
  hipStream_t st = (hipStream_t)stream;
  const int* w = a.w.width;
  const Layout y = layout_of(L, w, B, a.n_sample);
  float* ws = a.d_ws;
  float* x0 = ws + y.x0;
  float* Qy = ws + y.Qy;
  float* by = ws + y.by;
  float* Z = ws + y.Z;
  float* dZ = ws + y.dZ;
  double* l2 = reinterpret_cast<double*>(ws + y.l2);
  const int n0 = w[0], nl = w[L - 1];
  const dim3 blk(256);
  const float* none = nullptr;

  hipLaunchKernelGGL(plus_gather_kernel, dim3(blocks_of((int64_t)B * n0)), blk, 0, st, a.d_Ein, none, a.d_X, a.n_items,
                     B, n0, x0, (float*)nullptr, a.d_keys);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(plus_gather_kernel, dim3(blocks_of((int64_t)M * nl)), blk, 0, st, a.d_Q, a.d_b, a.d_Y, a.n_items, M,
                     nl, Qy, by, a.d_keys + B);
  NR_LAUNCH_CHECK();
  for (int l = 0; l < L; ++l) {
    const float* x = l ? a.d_h_new[l - 1] : x0;
    const int in = l ? w[l - 1] : n0, n = w[l];
    hipLaunchKernelGGL(gru_gates_kernel, dim3(blocks_of((int64_t)B * 2 * n)), blk, 0, st, x, in, a.d_state[l], n,
                       a.w.d_Wg[l], a.w.d_bg[l], B, ws + y.gate[l]);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_cand_kernel, dim3(blocks_of((int64_t)B * n)), blk, 0, st, x, in, a.d_state[l], n, a.w.d_Wc[l],
                       a.w.d_bc[l], ws + y.gate[l], a.w.hidden_act, B, ws + y.c[l], a.d_h_new[l]);
    NR_LAUNCH_CHECK();
  }
  const float* htop = a.d_h_new[L - 1];
  // Z [B][M] = h_top Qy^T + by
  hipLaunchKernelGGL((plus_tile_kernel<false, false>), dim3(tiles_of(M), tiles_of(B), 1), blk, 0, st, htop, (int64_t)nl,
                     (const float*)Qy, (int64_t)nl, B, M, nl, nl, (const float*)by, none, 0.0f, Z, (int64_t)M,
                     (int64_t)0);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(plus_lossrow_kernel, dim3(B), blk, 0, st, (const float*)Z, B, M, a.final_act, a.loss_kind,
                     a.bpr_reg, dZ, ws + y.rowloss);
  NR_LAUNCH_CHECK();
  float* dh = ws + y.dhA;
  float* dnext = ws + y.dhB;
  // dh_top [B][n] = dZ Qy, a chunk of dZ's columns per grid.z, then the chunks in ascending order
  const int n_chunks = chunks_of(M);
  hipLaunchKernelGGL((plus_tile_kernel<false, true>), dim3(tiles_of(nl), tiles_of(B), n_chunks), blk, 0, st,
                     (const float*)dZ, (int64_t)M, (const float*)Qy, (int64_t)nl, B, nl, M, chunk_len(M), none, none, 0.0f,
                     ws + y.part, (int64_t)nl, (int64_t)B * nl);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(plus_chunksum_kernel, dim3(blocks_of((int64_t)B * nl)), blk, 0, st, (const float*)(ws + y.part),
                     n_chunks, (int64_t)B * nl, dh);
  NR_LAUNCH_CHECK();
  // sQ [M][n] = dZ^T h_top + reg Qy, per slot
  hipLaunchKernelGGL((plus_tile_kernel<true, true>), dim3(tiles_of(nl), tiles_of(M), 1), blk, 0, st, (const float*)dZ,
                     (int64_t)M, htop, (int64_t)nl, M, nl, B, B, none, (const float*)Qy, a.reg, ws + y.sQ, (int64_t)nl,
                     (int64_t)0);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(plus_colsum_kernel, dim3(blocks_of(M)), blk, 0, st, (const float*)dZ, (const float*)Qy,
                     (const float*)by, B, M, nl, a.reg, ws + y.sb, l2);
  NR_LAUNCH_CHECK();
  for (int l = L - 1; l >= 0; --l) {
    const float* x = l ? a.d_h_new[l - 1] : x0;
    const int in = l ? w[l - 1] : n0, n = w[l];
    float* dpc = ws + y.dpc[l];
    float* dpg = ws + y.dpg[l];
    const float* gate = ws + y.gate[l];
    hipLaunchKernelGGL(gru_cellbwd_kernel, dim3(blocks_of((int64_t)B * n)), blk, 0, st, dh, a.d_state[l], gate,
                       ws + y.c[l], a.w.hidden_act, B, n, dpc, dpg);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_dr_kernel, dim3(blocks_of((int64_t)B * n)), blk, 0, st, dpc, a.w.d_Wc[l], a.d_state[l], gate,
                       in, B, n, dpg);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_dx_kernel, dim3(blocks_of((int64_t)B * in)), blk, 0, st, dpc, dpg, a.w.d_Wc[l], a.w.d_Wg[l],
                       in, B, n, l == 0 ? x0 : (const float*)nullptr, a.reg, dnext);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_dw_kernel, dim3(blocks_of((int64_t)(in + n + 1) * 3 * n)), blk, 0, st, x, in, a.d_state[l],
                       gate, dpg, dpc, B, n, a.d_G_Wg[l], a.d_G_bg[l], a.d_G_Wc[l], a.d_G_bc[l]);
    NR_LAUNCH_CHECK();
    float* tmp = dh;
    dh = dnext;
    dnext = tmp;
  }
  // dh now holds dLoss/dx0 + reg x0 per slot
  NR_TRY(nrhip_sort_u64(a.d_keys, B, stream));
  NR_TRY(nrhip_sort_u64(a.d_keys + B, M, stream));
  hipLaunchKernelGGL(gru_rows_kernel, dim3((B + 3) / 4), blk, 0, st, a.d_keys, B, n0, dh, a.d_G_Ein,
                     (const float*)nullptr, (float*)nullptr);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gru_rows_kernel, dim3((M + 3) / 4), blk, 0, st, a.d_keys + B, M, nl, ws + y.sQ, a.d_G_Q, ws + y.sb,
                     a.d_G_b);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(plus_loss_kernel, dim3(1), blk, 0, st, ws + y.rowloss, x0, (const double*)l2, B, M, n0, a.reg,
                     a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
