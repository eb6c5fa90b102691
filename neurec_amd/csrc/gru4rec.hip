// gru4rec.hip — GRU4Rec (Hidasi et al., ICLR 2016): the step, the state hand-over, the users' final states and
// predict() of model/sequential_recommender/GRU4Rec.py on gfx950.
//
// Variables: E_in [I][n_0], Q [I][n_last], b [I] and per layer Wg [in + n][2 n], bg [2 n], Wc [in + n][n], bc [n].
// The cell [EXT: tensorflow r1.12 rnn_cell_impl.GRUCell]:
//     [r, u] = sigmoid([x, s] Wg + bg)      r the first n columns, u the last n
//     c      = act([x, r * s] Wc + bc)      the reset gate multiplies the state BEFORE the product
//     h      = u s + (1 - u) c
// The states are constants of a step (placeholders in the reference): nothing flows back through them.
//
// One step (nrhip_gru4rec_step), every kernel one thread per output and one k-ascending fmaf chain per output (the
// cell's kernels and gru_rows_kernel live in gru4rec_cell.h, shared with gru4recplus.hip):
//   gru_prep_kernel       x0 = E_in[X]; the sort keys item << 32 | slot of X and of Y
//   gru_gates_kernel      per layer: the gates [B][2 n]
//   gru_cand_kernel       per layer: c and h (= the new state, = the next layer's input)
//   gru_logits_kernel     Z [B][B] = h_top Q[Y]^T + b[Y]
//   gru_lossrow_kernel    one workgroup per row i: A = final_act(Z), the row's loss, dLoss/dZ with the diagonal's share
//   gru_dhtop_kernel      dLoss/dh_top = dZ Q[Y]
//   gru_dq_kernel         per slot j: dZ^T h_top + reg Q[Y_j], and the bias slot sum + reg b[Y_j]
//   gru_cellbwd_kernel    per layer, top down: dc -> d(pre-candidate); du -> d(pre-update gate)
//   gru_dr_kernel         d(r * s) = d(pre-candidate) Wc[in:]^T -> dr -> d(pre-reset gate)
//   gru_dx_kernel         dx = d(pre-candidate) Wc[:in]^T + d(pre-gates) Wg[:in]^T (layer 0: + reg x0, per slot)
//   gru_dw_kernel         G_Wg, G_bg, G_Wc, G_bc whole: per element the slots' sum in slot order
//   nrhip_sort_u64        the two key lists
//   gru_rows_kernel       one wavefront per sorted key: the head of a run adds the run's slot rows in key order and
//                         STORES the table row's gradient once (E_in from dx of layer 0; Q and b from gru_dq_kernel)
//   gru_loss_kernel       one workgroup: the rows' losses and the regulariser in a fixed order.  These two REPORTED sums
//                         alone are added in double and rounded to float once (as the other models' loss kernels do);
//                         every value that reaches a gradient, a state or a table is fp32
// No atomics anywhere: two runs are bit-identical.
//
//   gru_advance_kernel    state = reset ? 0 : h_new, every layer, one launch
//   gru_user_states_kernel  NRHIP_GRU4REC_TILE users per workgroup, the states of all layers in LDS for the whole loop
//                         over time positions; thread = output column, 16 accumulators (one per user of the tile), a
//                         weight is read once per position and tile (through L2) and used 16 times; the inputs and
//                         states are read from LDS k-major as 16-byte broadcasts
//   gru_scores_kernel     final_act(H Q^T + b): 64 x 64 output tile per workgroup, 4 x 4 outputs per thread, operands
//                         staged through LDS 32 columns at a time
#include "gru4rec_cell.h"

namespace {

constexpr int kT = NRHIP_GRU4REC_TILE;
enum { LOSS_TOP1 = 0, LOSS_BPR = 1 };

// the float work buffer of a step: offsets in floats
struct Layout {
  size_t x0, gate[kL], c[kL], dpg[kL], dpc[kL], dhA, dhB, Z, dZ, rowloss, sQ, sb, total;
};
Layout layout_of(int L, const int* w, int B) {
  Layout y;
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += (n + 3) / 4 * 4;
    return at;
  };
  const size_t b = (size_t)B;
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
  y.Z = take(b * b);
  y.dZ = take(b * b);
  y.rowloss = take(b);
  y.sQ = take(b * w[L - 1]);
  y.sb = take(b);
  y.total = o;
  return y;
}

__global__ __launch_bounds__(256) void gru_prep_kernel(const float* __restrict__ Ein, const int32_t* __restrict__ X,
                                                       const int32_t* __restrict__ Y, int n_items, int B, int n0,
                                                       float* __restrict__ x0, uint64_t* __restrict__ keys) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n0) return;
  const int t = (int)(idx / n0), k = (int)(idx - (int64_t)t * n0);
  const int x = X[t];
  const bool okx = x >= 0 && x < n_items;
  x0[idx] = okx ? Ein[(int64_t)x * n0 + k] : 0.0f;
  if (k == 0) {
    const int y = Y[t];
    keys[t] = okx ? (((uint64_t)(uint32_t)x << 32) | (uint32_t)t) : kSentinel;
    keys[B + t] = (y >= 0 && y < n_items) ? (((uint64_t)(uint32_t)y << 32) | (uint32_t)t) : kSentinel;
  }
}

__global__ __launch_bounds__(256) void gru_logits_kernel(const float* __restrict__ h, const float* __restrict__ Q,
                                                         const float* __restrict__ b, const int32_t* __restrict__ Y,
                                                         int n_items, int B, int n, float* __restrict__ Z) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * B) return;
  const int i = (int)(idx / B), j = (int)(idx - (int64_t)i * B);
  const int y = Y[j];
  float acc = 0.0f, bias = 0.0f;
  if (y >= 0 && y < n_items) {
#pragma unroll 8
    for (int k = 0; k < n; ++k) acc = __builtin_fmaf(h[(int64_t)i * n + k], Q[(int64_t)y * n + k], acc);
    bias = b[y];
  }
  Z[idx] = acc + bias;
}

// row i of the B x B loss.  Every term of the mean carries 1 / B^2:
//   bpr   sum_j softplus(A_ij - p)                        p = A_ii; the diagonal term is part of the mean
//   top1  sum_j (sigmoid(A_ij - p) + sigmoid(A_ij^2)) - sigmoid(p^2)        (the last: `/ batch_size` of the reference)
// dLoss/dA_ij directly, dLoss/dp summed over the row in a fixed tree and added at the diagonal; then through final_act.
__global__ __launch_bounds__(256) void gru_lossrow_kernel(const float* __restrict__ Z, int B, int fin, int loss_kind,
                                                          float* __restrict__ dZ, float* __restrict__ rowloss) {
  __shared__ float s_l[256], s_e[256];
  __shared__ float s_diag;
  const int i = blockIdx.x;
  const float* z = Z + (int64_t)i * B;
  float* dz = dZ + (int64_t)i * B;
  const float inv = 1.0f / ((float)B * (float)B);
  const float zp = z[i], p = final_act(fin, zp);
  float sl = 0.0f, se = 0.0f;
  for (int j = threadIdx.x; j < B; j += 256) {
    const float zj = z[j], a = final_act(fin, zj);
    float da;
    if (loss_kind == LOSS_BPR) {
      const float e = sigmoidf_(a - p);
      sl += nr::tf_softplus(a - p);
      se += e;
      da = e * inv;
    } else {
      const float e = sigmoidf_(a - p), q = sigmoidf_(a * a);
      const float de = e * (1.0f - e);
      sl += e + q;
      se += de;
      da = (de + 2.0f * a * (q * (1.0f - q))) * inv;
    }
    if (j == i) s_diag = da;
    else dz[j] = da * final_dact(fin, zj);
  }
  s_l[threadIdx.x] = sl;
  s_e[threadIdx.x] = se;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_l[threadIdx.x] += s_l[threadIdx.x + s];
      s_e[threadIdx.x] += s_e[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float loss = s_l[0], dp = -s_e[0];
    if (loss_kind == LOSS_TOP1) {
      const float q = sigmoidf_(p * p);
      loss -= q;
      dp -= 2.0f * p * (q * (1.0f - q));
    }
    rowloss[i] = loss * inv;
    dz[i] = (s_diag + dp * inv) * final_dact(fin, zp);
  }
}

// dh[i][k] = sum_j dZ[i][j] Q[Y_j][k]
__global__ __launch_bounds__(256) void gru_dhtop_kernel(const float* __restrict__ dZ, const float* __restrict__ Q,
                                                        const int32_t* __restrict__ Y, int n_items, int B, int n,
                                                        float* __restrict__ dh) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n) return;
  const int i = (int)(idx / n), k = (int)(idx - (int64_t)i * n);
  float acc = 0.0f;
  for (int j = 0; j < B; ++j) {
    const int y = Y[j];
    if (y >= 0 && y < n_items) acc = __builtin_fmaf(dZ[(int64_t)i * B + j], Q[(int64_t)y * n + k], acc);
  }
  dh[idx] = acc;
}

// per SLOT j: sQ[j][k] = sum_i dZ[i][j] h[i][k] + reg Q[Y_j][k];  sb[j] = sum_i dZ[i][j] + reg b[Y_j]
__global__ __launch_bounds__(256) void gru_dq_kernel(const float* __restrict__ dZ, const float* __restrict__ h,
                                                     const float* __restrict__ Q, const float* __restrict__ b,
                                                     const int32_t* __restrict__ Y, int n_items, int B, int n, float reg,
                                                     float* __restrict__ sQ, float* __restrict__ sb) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n) return;
  const int j = (int)(idx / n), k = (int)(idx - (int64_t)j * n);
  const int y = Y[j];
  const bool ok = y >= 0 && y < n_items;
  float acc = 0.0f;
#pragma unroll 8
  for (int i = 0; i < B; ++i) acc = __builtin_fmaf(dZ[(int64_t)i * B + j], h[(int64_t)i * n + k], acc);
  sQ[idx] = ok ? acc + reg * Q[(int64_t)y * n + k] : 0.0f;
  if (k == 0) {
    float ab = 0.0f;
#pragma unroll 8
    for (int i = 0; i < B; ++i) ab += dZ[(int64_t)i * B + j];
    sb[j] = ok ? ab + reg * b[y] : 0.0f;
  }
}

__global__ __launch_bounds__(256) void gru_loss_kernel(const float* __restrict__ rowloss, const float* __restrict__ x0,
                                                       const float* __restrict__ Q, const float* __restrict__ b,
                                                       const int32_t* __restrict__ Y, int n_items, int B, int n0, int n,
                                                       float reg, float* __restrict__ loss2) {
  __shared__ double s_a[256], s_b[256];
  double la = 0.0, lb = 0.0;
  for (int t = threadIdx.x; t < B; t += 256) {
    la += (double)rowloss[t];
    double q = 0.0;
    for (int k = 0; k < n0; ++k) q += (double)x0[(int64_t)t * n0 + k] * (double)x0[(int64_t)t * n0 + k];
    const int y = Y[t];
    if (y >= 0 && y < n_items) {
      for (int k = 0; k < n; ++k) q += (double)Q[(int64_t)y * n + k] * (double)Q[(int64_t)y * n + k];
      q += (double)b[y] * (double)b[y];
    }
    lb += 0.5 * q;
  }
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

struct AdvanceArgs {
  float* state[kL];
  const float* h_new[kL];
  int width[kL];
  int n_layers, batch;
  const uint8_t* reset;
};

// the hand-over first, then the mask: a slot that ends starts its next session from zero
__global__ __launch_bounds__(256) void gru_advance_kernel(AdvanceArgs a) {
  const int l = blockIdx.y;
  const int n = a.width[l];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.batch * n) return;
  const int t = (int)(idx / n);
  const float v = a.h_new[l][idx];
  a.state[l][idx] = (a.reset && a.reset[t]) ? 0.0f : v;
}

// ------------------------------------------------------------------ the users' final states
__device__ __forceinline__ void tile_fma(const float* src_, float wv, float (&acc)[NRHIP_GRU4REC_TILE]) {
  const float4* src = reinterpret_cast<const float4*>(src_);
#pragma unroll
  for (int q = 0; q < NRHIP_GRU4REC_TILE / 4; ++q) {
    const float4 v = src[q];
    acc[4 * q + 0] = __builtin_fmaf(v.x, wv, acc[4 * q + 0]);
    acc[4 * q + 1] = __builtin_fmaf(v.y, wv, acc[4 * q + 1]);
    acc[4 * q + 2] = __builtin_fmaf(v.z, wv, acc[4 * q + 2]);
    acc[4 * q + 3] = __builtin_fmaf(v.w, wv, acc[4 * q + 3]);
  }
}

// acc[u] = the k-ascending fmaf chain over K = in + rest inputs of the tile's kT users: input k is s_a[k] for k < in and
// s_b[k - in] beyond (k-major, kT floats each), weight k is W[k][col]: per term one weight from global memory (through
// L2), four 16-byte LDS reads that every lane shares, and 16 multiply-adds.
__device__ __forceinline__ void tile_chain(const float* __restrict__ W, int ldw, int col, int K, int in,
                                           const float* s_a, const float* s_b, float (&acc)[NRHIP_GRU4REC_TILE]) {
#pragma unroll
  for (int u = 0; u < NRHIP_GRU4REC_TILE; ++u) acc[u] = 0.0f;
  const float* wp = W + col;
#pragma unroll 4
  for (int k = 0; k < K; ++k)
    tile_fma(k < in ? s_a + k * NRHIP_GRU4REC_TILE : s_b + (k - in) * NRHIP_GRU4REC_TILE, wp[(int64_t)k * ldw], acc);
}

// LDS, k-major with the kT users of the tile contiguous: a thread reads the 16 values of one k as four 16-byte reads
// that every lane of the wavefront shares (broadcast)
__global__ __launch_bounds__(256) void gru_user_states_kernel(const int64_t* __restrict__ seq_ptr,
                                                              const int32_t* __restrict__ seq, int n_users, int n_items,
                                                              const int32_t* __restrict__ users,
                                                              const int32_t* __restrict__ out_row, int n_listed,
                                                              const float* __restrict__ Ein, nrhip_gru4rec_weights w,
                                                              float* __restrict__ H, int64_t ldh) {
  __shared__ __attribute__((aligned(16))) float s_state[kL][kW * kT];
  __shared__ __attribute__((aligned(16))) float s_x[kW * kT];
  __shared__ __attribute__((aligned(16))) float s_g[2 * kW * kT];
  __shared__ int64_t s_beg[kT];
  __shared__ int s_len[kT], s_item[kT];
  __shared__ int s_max;
  const int tid = threadIdx.x;
  const int base = blockIdx.x * kT;
  const int L = w.n_layers, n0 = w.width[0];
  if (tid < kT) {
    const int e = base + tid;
    int len = 0;
    int64_t beg = 0;
    if (e < n_listed) {
      const int u = users[e];
      if (u >= 0 && u < n_users) {
        beg = seq_ptr[u];
        const int64_t m = seq_ptr[u + 1] - beg;
        len = m > 0 ? (int)m : 0;
      }
    }
    s_beg[tid] = beg;
    s_len[tid] = len;
  }
  for (int e = tid; e < kL * kW * kT; e += 256) (&s_state[0][0])[e] = 0.0f;
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int u = 0; u < kT; ++u) m = s_len[u] > m ? s_len[u] : m;
    s_max = m;
  }
  __syncthreads();
  const int max_len = s_max;
  for (int p = 0; p < max_len; ++p) {
    if (tid < kT) s_item[tid] = p < s_len[tid] ? seq[s_beg[tid] + p] : -1;
    __syncthreads();
    for (int e = tid; e < kT * n0; e += 256) {
      const int u = e / n0, k = e - u * n0;
      const int item = s_item[u];
      s_x[k * kT + u] = (item >= 0 && item < n_items) ? Ein[(int64_t)item * n0 + k] : 0.0f;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const int in = l ? w.width[l - 1] : n0, n = w.width[l], n2 = 2 * n;
      float* st = s_state[l];
      float acc[kT];
      if (tid < n2) {
        tile_chain(w.d_Wg[l], n2, tid, in + n, in, s_x, st, acc);
        const float bias = w.d_bg[l][tid];
#pragma unroll
        for (int u = 0; u < kT; ++u) s_g[tid * kT + u] = sigmoidf_(acc[u] + bias);
      }
      __syncthreads();
      for (int e = tid; e < n * kT; e += 256) s_g[e] *= st[e];          // r -> r * s, rows [0, n) of s_g
      __syncthreads();
      if (tid < n) {
        tile_chain(w.d_Wc[l], n, tid, in + n, in, s_x, s_g, acc);
        const float bias = w.d_bc[l][tid];
#pragma unroll
        for (int u = 0; u < kT; ++u) {
          const float cv = hidden_act(w.hidden_act, acc[u] + bias);
          const float ug = s_g[(n + tid) * kT + u], sv = st[tid * kT + u];
          acc[u] = ug * sv + (1.0f - ug) * cv;
        }
      }
      __syncthreads();                                    // every read of s_x and of the old state is done
      if (tid < n) {
#pragma unroll
        for (int u = 0; u < kT; ++u) {
          s_x[tid * kT + u] = acc[u];                     // the next layer's input
          if (p < s_len[u]) st[tid * kT + u] = acc[u];    // a user past its end keeps its state
        }
      }
      __syncthreads();
    }
  }
  const int nl = w.width[L - 1];
  for (int e = tid; e < kT * nl; e += 256) {
    const int u = e / nl, k = e - u * nl;
    const int entry = base + u;
    if (entry < n_listed) {
      const int64_t row = out_row ? out_row[entry] : entry;
      H[row * ldh + k] = s_state[L - 1][k * kT + u];
    }
  }
}

// ------------------------------------------------------------------ predict()
constexpr int kTile = 64;          // H rows and Q rows of a workgroup's output tile
constexpr int kColumns = 32;       // columns staged in LDS at a time
constexpr int kLd = kTile + 4;     // floats per staged column, 16-byte aligned

__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int64_t ld, int n_rows, int d, int r0, int c0,
                                           float* dst) {
  for (int e = threadIdx.x; e < kTile * kColumns; e += 256) {
    const int rr = e / kColumns, cc = e % kColumns;
    const int row = r0 + rr, col = c0 + cc;
    dst[cc * kLd + rr] = (row < n_rows && col < d) ? src[(int64_t)row * ld + col] : 0.0f;
  }
}

__global__ __launch_bounds__(256) void gru_scores_kernel(const float* __restrict__ Hm, int64_t ldh,
                                                         const float* __restrict__ Q, const float* __restrict__ b, int n,
                                                         int n_items, int d, int fin, float* __restrict__ out,
                                                         int64_t ld) {
  __shared__ __attribute__((aligned(16))) float s_h[kColumns * kLd];
  __shared__ __attribute__((aligned(16))) float s_q[kColumns * kLd];
  const int i0 = blockIdx.x * kTile, n0 = blockIdx.y * kTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.0f;
  for (int c0 = 0; c0 < d; c0 += kColumns) {
    __syncthreads();
    stage_tile(Hm, ldh, n, d, n0, c0, s_h);
    stage_tile(Q, d, n_items, d, i0, c0, s_q);
    __syncthreads();
    // the columns beyond d hold zeros on both sides: fmaf(0, 0, acc) leaves every sum as it is
#pragma unroll 8
    for (int cc = 0; cc < kColumns; ++cc) {
      const float4 ha = *reinterpret_cast<const float4*>(s_h + cc * kLd + 4 * ty);
      const float4 qa = *reinterpret_cast<const float4*>(s_q + cc * kLd + 4 * tx);
      const float hv[4] = {ha.x, ha.y, ha.z, ha.w}, qv[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = __builtin_fmaf(hv[r], qv[s], acc[r][s]);
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
      if (row < n) out[(int64_t)row * ld + item] = final_act(fin, acc[r][s] + bias);
    }
  }
}

}  // namespace

extern "C" {

int nrhip_gru4rec_workspace_floats(int n_layers, const int* widths, int max_batch, size_t* floats) {
  NR_REQUIRE(widths && floats, NR_ERR_ARG, "gru4rec_workspace_floats: null argument");
  NR_REQUIRE(n_layers >= 1 && n_layers <= kL, NR_ERR_UNSUPPORTED, "gru4rec_workspace_floats: %d layers outside 1..%d",
             n_layers, kL);
  for (int l = 0; l < n_layers; ++l)
    NR_REQUIRE(widths[l] >= 1 && widths[l] <= kW, NR_ERR_UNSUPPORTED,
               "gru4rec_workspace_floats: layer width %d outside 1..%d", widths[l], kW);
  NR_REQUIRE(max_batch >= 0 && max_batch <= NRHIP_GRU4REC_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "gru4rec_workspace_floats: max_batch %d outside 0..%d", max_batch, NRHIP_GRU4REC_MAX_BATCH);
  *floats = layout_of(n_layers, widths, max_batch).total;
  return NR_OK;
}

int nrhip_gru4rec_step(const nrhip_gru4rec_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "gru4rec_step: null argument block");
  const nrhip_gru4rec_step_args a = *args;
  NR_TRY(check_weights(a.w, "gru4rec_step"));
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_GRU4REC_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "gru4rec_step: batch %d outside 0..%d", a.batch, NRHIP_GRU4REC_MAX_BATCH);
  NR_REQUIRE(a.n_items >= 0, NR_ERR_ARG, "gru4rec_step: bad sizes");
  NR_REQUIRE(a.final_act >= FIN_LINEAR && a.final_act <= FIN_LEAKY, NR_ERR_ARG,
             "gru4rec_step: unknown final_act %d (0 linear, 1 relu, 2 leaky_relu)", a.final_act);
  NR_REQUIRE(a.loss_kind == LOSS_TOP1 || a.loss_kind == LOSS_BPR, NR_ERR_ARG,
             "gru4rec_step: unknown loss %d (0 top1, 1 bpr)", a.loss_kind);
  const int B = a.batch, L = a.w.n_layers;
  if (B == 0) return NR_OK;
  NR_REQUIRE(a.d_Ein && a.d_Q && a.d_b && a.d_G_Ein && a.d_G_Q && a.d_G_b && a.d_X && a.d_Y && a.d_keys && a.d_ws &&
                 a.d_loss2, NR_ERR_ARG, "gru4rec_step: null pointer argument");
  for (int l = 0; l < L; ++l)
    NR_REQUIRE(a.d_G_Wg[l] && a.d_G_bg[l] && a.d_G_Wc[l] && a.d_G_bc[l] && a.d_state[l] && a.d_h_new[l], NR_ERR_ARG,
               "gru4rec_step: null pointer argument (layer %d)", l);
  hipStream_t st = (hipStream_t)stream;
  const int* w = a.w.width;
  const Layout y = layout_of(L, w, B);
  float* ws = a.d_ws;
  float* x0 = ws + y.x0;
  const int n0 = w[0], nl = w[L - 1];
  const dim3 blk(256);

  hipLaunchKernelGGL(gru_prep_kernel, dim3(blocks_of((int64_t)B * n0)), blk, 0, st, a.d_Ein, a.d_X, a.d_Y, a.n_items, B,
                     n0, x0, a.d_keys);
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
  hipLaunchKernelGGL(gru_logits_kernel, dim3(blocks_of((int64_t)B * B)), blk, 0, st, htop, a.d_Q, a.d_b, a.d_Y,
                     a.n_items, B, nl, ws + y.Z);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gru_lossrow_kernel, dim3(B), blk, 0, st, ws + y.Z, B, a.final_act, a.loss_kind, ws + y.dZ,
                     ws + y.rowloss);
  NR_LAUNCH_CHECK();
  float* dh = ws + y.dhA;
  float* dnext = ws + y.dhB;
  hipLaunchKernelGGL(gru_dhtop_kernel, dim3(blocks_of((int64_t)B * nl)), blk, 0, st, ws + y.dZ, a.d_Q, a.d_Y, a.n_items,
                     B, nl, dh);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gru_dq_kernel, dim3(blocks_of((int64_t)B * nl)), blk, 0, st, ws + y.dZ, htop, a.d_Q, a.d_b, a.d_Y,
                     a.n_items, B, nl, a.reg, ws + y.sQ, ws + y.sb);
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
  NR_TRY(nrhip_sort_u64(a.d_keys + B, B, stream));
  hipLaunchKernelGGL(gru_rows_kernel, dim3((B + 3) / 4), blk, 0, st, a.d_keys, B, n0, dh, a.d_G_Ein,
                     (const float*)nullptr, (float*)nullptr);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gru_rows_kernel, dim3((B + 3) / 4), blk, 0, st, a.d_keys + B, B, nl, ws + y.sQ, a.d_G_Q, ws + y.sb,
                     a.d_G_b);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gru_loss_kernel, dim3(1), blk, 0, st, ws + y.rowloss, x0, a.d_Q, a.d_b, a.d_Y, a.n_items, B, n0, nl,
                     a.reg, a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_gru4rec_advance(float* const* d_state_host, const float* const* d_h_new_host, const int* widths, int n_layers,
                          int batch, const uint8_t* d_reset, void* stream) {
  NR_REQUIRE(n_layers >= 1 && n_layers <= kL, NR_ERR_UNSUPPORTED, "gru4rec_advance: %d layers outside 1..%d", n_layers,
             kL);
  NR_REQUIRE(batch >= 0 && batch <= NRHIP_GRU4REC_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "gru4rec_advance: batch %d outside 0..%d", batch, NRHIP_GRU4REC_MAX_BATCH);
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_state_host && d_h_new_host && widths, NR_ERR_ARG, "gru4rec_advance: null argument");
  AdvanceArgs a;
  int widest = 0;
  for (int l = 0; l < kL; ++l) {
    a.state[l] = nullptr;
    a.h_new[l] = nullptr;
    a.width[l] = 0;
  }
  for (int l = 0; l < n_layers; ++l) {
    NR_REQUIRE(widths[l] >= 1 && widths[l] <= kW, NR_ERR_UNSUPPORTED, "gru4rec_advance: layer width %d outside 1..%d",
               widths[l], kW);
    NR_REQUIRE(d_state_host[l] && d_h_new_host[l], NR_ERR_ARG, "gru4rec_advance: null pointer argument");
    a.state[l] = d_state_host[l];
    a.h_new[l] = d_h_new_host[l];
    a.width[l] = widths[l];
    widest = widths[l] > widest ? widths[l] : widest;
  }
  a.n_layers = n_layers;
  a.batch = batch;
  a.reset = d_reset;
  hipLaunchKernelGGL(gru_advance_kernel, dim3(blocks_of((int64_t)batch * widest), n_layers), dim3(256), 0,
                     (hipStream_t)stream, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_gru4rec_user_states(const int64_t* d_seq_ptr, const int32_t* d_seq, int n_users, int n_items,
                              const int32_t* d_users, const int32_t* d_out_row, int n_listed, const float* d_Ein,
                              const nrhip_gru4rec_weights* w, float* d_H, int64_t ldh, void* stream) {
  NR_REQUIRE(w, NR_ERR_ARG, "gru4rec_user_states: null weights");
  NR_TRY(check_weights(*w, "gru4rec_user_states"));
  NR_REQUIRE(n_users >= 0 && n_items >= 0 && n_listed >= 0 && ldh >= w->width[w->n_layers - 1], NR_ERR_ARG,
             "gru4rec_user_states: bad sizes");
  if (n_listed == 0) return NR_OK;
  NR_REQUIRE(d_seq_ptr && d_users && d_Ein && d_H, NR_ERR_ARG, "gru4rec_user_states: null pointer argument");
  hipLaunchKernelGGL(gru_user_states_kernel, dim3((n_listed + kT - 1) / kT), dim3(256), 0, (hipStream_t)stream,
                     d_seq_ptr, d_seq, n_users, n_items, d_users, d_out_row, n_listed, d_Ein, *w, d_H, ldh);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_gru4rec_scores(const float* d_H, int64_t ldh, const float* d_Q, const float* d_b, int n, int n_items, int d,
                         int final_act, float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(d >= 1 && d <= kW, NR_ERR_UNSUPPORTED, "gru4rec_scores: width %d outside 1..%d", d, kW);
  NR_REQUIRE(final_act >= FIN_LINEAR && final_act <= FIN_LEAKY, NR_ERR_ARG,
             "gru4rec_scores: unknown final_act %d (0 linear, 1 relu, 2 leaky_relu)", final_act);
  NR_REQUIRE(n >= 0 && n_items >= 0 && ldh >= d && ld >= n_items && (n + kTile - 1) / kTile <= 65535, NR_ERR_ARG,
             "gru4rec_scores: bad sizes");
  if (n == 0 || n_items == 0) return NR_OK;
  NR_REQUIRE(d_H && d_Q && d_b && d_out, NR_ERR_ARG, "gru4rec_scores: null pointer argument");
  const dim3 grid((n_items + kTile - 1) / kTile, (n + kTile - 1) / kTile);
  hipLaunchKernelGGL(gru_scores_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_H, ldh, d_Q, d_b, n, n_items, d,
                     final_act, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
