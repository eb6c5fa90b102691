// srgnn.hip — the SRGNN step (model/sequential_recommender/SRGNN.py:75-136 up to the optimiser) and its forward pass,
// fp32.  Notation: I items, d hidden_size, L max_seq_len, B sessions, n a session's distinct items (its nodes), R the
// batch's nodes laid end to end (session b's at rows OFF[b] .. OFF[b] + n_b), S the `step` iterations.
//
//   srgnn_graph_kernel     one workgroup per session, in LDS: the window (from the padded row, or gathered from the
//                          resident sequences by (user, end)), a rank sort of its ids -> the distinct nodes ascending,
//                          their occurrence counts and the alias map; a rank sort of the (alias[t], alias[t + 1]) pairs
//                          -> the deduplicated edge list by (source, target) with row pointers, and the same by (target,
//                          source).  A node's out-degree / in-degree is a row-pointer difference.  No n x n matrix.
//   srgnn_nodes_kernel     OFF (an integer prefix over the sessions' node counts), the node rows of the table into H_0,
//                          the sort key (item, row) of every node row
//   per iteration s:       srgnn_lin_kernel [h W_in + b_in | h W_out + b_out]; srgnn_prop_kernel x = [A_in . | A_out .]
//                          as a walk over the node's edges in list order; srgnn_gates_kernel; srgnn_cand_kernel
//                          (r first, u second, r * s before the product: the cell of gru4rec_cell.h, input width 2 d)
//   srgnn_q_kernel, srgnn_readout_kernel   h nasr_w2 per node; per session last, m, the coefficients (a node's coefficient
//                          times its occurrence count: positions of one node have equal m), a, sess
//   srgnn_logits_kernel    [B][I]: a 64-item tile of the table in LDS against 32 sessions
//   srgnn_softmax_kernel   per session: row maximum, log-sum-exp, the loss term, and (p - y) / B in place
//   srgnn_headg_kernel     G_embedding[i] = sum_b (p - y)_bi / B sess_b + L2 embedding[i], STORED for every row
//   srgnn_dsess_kernel / srgnn_dsess_sum_kernel   d sess_b: partials per chunk of 512 items, added in chunk order
//   srgnn_transpose_kernel the kernels' transposes, so that the backward row kernels read weights along their lanes
//   srgnn_readout_bwd_kernel, srgnn_dh_kernel     back through B, the attention and nasr_w1 / nasr_w2 to the nodes
//   per iteration, last first: srgnn_cellbwd_kernel, srgnn_dr_kernel (ds = dh u + d(r s) r), srgnn_dx_kernel (dx, and
//                          ds += d(pre-gates) Wg[2d:]^T), srgnn_propT_kernel, srgnn_linT_kernel (ds += through W_in, W_out)
//   srgnn_wgrad_kernel / srgnn_wsum_kernel   the 13 other variables: one thread per element and chunk of rows (or of
//                          sessions), iterations and rows ascending; the chunks added in order, + L2 v, STORED
//   nrhip_sort_u64, srgnn_rows_kernel        the node rows' gradient added to the table's rows in key order
//   srgnn_loss_kernel      the mean and the regulariser, in double, rounded once
//
// One ascending fmaf chain per output, fixed trees, no atomics: two calls on the same inputs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using nr::rowkey::kSentinel;
using nr::rowkey::row_key;

constexpr int kD = NRHIP_SRGNN_MAX_WIDTH;
constexpr int kLen = NRHIP_SRGNN_MAX_LEN;
constexpr int kS = NRHIP_SRGNN_MAX_STEP;
constexpr int kB = NRHIP_SRGNN_MAX_BATCH;
constexpr int kChunks = 64;                 // row / session chunks of the variable-gradient partials
constexpr int kItemChunk = 512;             // items per partial of d sess
constexpr int kVars = 13;                   // the variables besides the table
static_assert(kLen <= 256, "a node index is 8 bits of an edge word; one thread per position");

struct Ctx {
  nrhip_srgnn_weights w;
  nrhip_srgnn_feed f;
  uint64_t* keys;
  int *NODES, *ALIAS, *CNT, *EOUT, *EIN, *OPTR, *IPTR, *N, *LEN, *OFF, *TGT, *ROWB, *ROWI, *LASTROW;
  float *H, *X, *GATE, *CC, *FIO, *DFIO, *DPG, *DPC, *DX, *DHA, *DHB, *M, *DQ, *WN, *LAST, *MA, *SESS, *DSESS, *DLAST,
      *GV, *GNB, *DA, *DLASTH, *LOGITS, *LOSSB, *DSP, *part, *RS, *WgT, *WcT, *WinT, *WoutT, *w2T;
  double* l2part;
  int B;
  int64_t R;                                // B L: rows of the per-iteration buffers
};

struct Layout {
  size_t l2part, NODES, ALIAS, CNT, EOUT, EIN, OPTR, IPTR, N, LEN, OFF, TGT, ROWB, ROWI, LASTROW;
  size_t H, X, GATE, CC, FIO, DFIO, DPG, DPC, DX, DHA, DHB, M, DQ, WN, LAST, MA, SESS, DSESS, DLAST, GV, GNB, DA, DLASTH,
      LOGITS, LOSSB, DSP, part, RS, WT, total;
  int64_t nW, end[kVars];
  int head_blocks, w_blocks, item_chunks;
};

Layout layout_of(int B, int L, int d, int S, int I, bool train) {
  Layout y;
  const size_t b = (size_t)(B > 0 ? B : 1), R = b * L, dd = (size_t)d;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 3) / 4 * 4; return at; };
  const int64_t sizes[kVars] = {(int64_t)d * d, (int64_t)d * d, d, d, (int64_t)d * d, d, (int64_t)d * d, d,
                                2ll * d * d, 6ll * d * d, 2 * d, 3ll * d * d, d};
  int64_t run = 0;
  for (int k = 0; k < kVars; ++k) y.end[k] = run += sizes[k];
  y.nW = run;
  y.head_blocks = (I + 31) / 32;
  y.w_blocks = (int)((y.nW + 255) / 256);
  y.item_chunks = (I + kItemChunk - 1) / kItemChunk;
  y.l2part = take(2 * ((size_t)y.head_blocks + y.w_blocks));     // doubles
  y.NODES = take(R), y.ALIAS = take(R), y.CNT = take(R), y.EOUT = take(R), y.EIN = take(R);
  y.OPTR = take(b * (L + 1)), y.IPTR = take(b * (L + 1));
  y.N = take(b), y.LEN = take(b), y.OFF = take(b + 1), y.TGT = take(b), y.ROWB = take(R), y.ROWI = take(R);
  y.LASTROW = take(b);
  y.H = take((size_t)(S + 1) * R * dd);
  y.X = take((size_t)S * R * 2 * dd), y.GATE = take((size_t)S * R * 2 * dd), y.CC = take((size_t)S * R * dd);
  y.FIO = take(R * 2 * dd);
  y.M = take(R * dd), y.WN = take(R);
  y.LAST = take(b * dd), y.MA = take(b * 2 * dd), y.SESS = take(b * dd);
  if (train) {
    y.DFIO = take((size_t)S * R * 2 * dd), y.DPG = take((size_t)S * R * 2 * dd), y.DPC = take((size_t)S * R * dd);
    y.DX = take(R * 2 * dd), y.DHA = take(R * dd), y.DHB = take(R * dd), y.DQ = take(R * dd);
    y.DSESS = take(b * dd), y.DLAST = take(b * dd), y.GV = take(b * dd), y.GNB = take(b * dd), y.DA = take(b * dd);
    y.DLASTH = take(b * dd);
    y.LOGITS = take(b * (size_t)I), y.LOSSB = take(b);
    y.DSP = take((size_t)y.item_chunks * b * dd);
    y.part = take((size_t)kChunks * y.nW);
    y.RS = take((size_t)S * R * dd);
    y.WT = take(12 * dd * dd);
  } else {
    y.DFIO = y.DPG = y.DPC = y.DX = y.DHA = y.DHB = y.DQ = y.DSESS = y.DLAST = y.GV = y.GNB = y.DA = y.DLASTH =
        y.LOGITS = y.LOSSB = y.DSP = y.part = y.RS = y.WT = o;
  }
  y.total = o;
  return y;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// key[0..n) ranked ascending, ties by position; sorted[rank] = key; uidx[p] = the number of distinct keys below
// sorted[p].  Returns the number of distinct keys.  256 threads; every array holds kLen ints of LDS.
__device__ int sort_unique(const int* key, int n, int* sorted, int* rank, int* uidx) {
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += 256) {
    const int k = key[t];
    int r = 0;
    for (int u = 0; u < n; ++u) {
      const int ku = key[u];
      r += (ku < k || (ku == k && u < t)) ? 1 : 0;
    }
    rank[t] = r;
    sorted[r] = k;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < n; p += 256) {
    int c = 0;
    for (int q = 1; q <= p; ++q) c += sorted[q] != sorted[q - 1] ? 1 : 0;
    uidx[p] = c;
  }
  __syncthreads();
  return n > 0 ? uidx[n - 1] + 1 : 0;
}

// the distinct edge words of sorted[0..ne) to list[b L + .], and ptr[i] = the number of them whose upper node is below i
__device__ void store_edges(const int* sorted, const int* uidx, int ne, int n, int* list, int* ptr) {
  for (int p = threadIdx.x; p < ne; p += 256)
    if (p == 0 || sorted[p] != sorted[p - 1]) list[uidx[p]] = sorted[p];
  for (int i = threadIdx.x; i <= n; i += 256) {
    int c = 0;
    for (int p = 0; p < ne; ++p)
      if ((p == 0 || sorted[p] != sorted[p - 1]) && (sorted[p] >> 8) < i) ++c;
    ptr[i] = c;
  }
}

__global__ __launch_bounds__(256) void srgnn_graph_kernel(Ctx c) {
  const int b = blockIdx.x, tid = threadIdx.x, L = c.w.L, I = c.w.n_items;
  __shared__ int s_id[kLen], s_sorted[kLen], s_rank[kLen], s_u[kLen], s_alias[kLen], s_key[kLen];
  __shared__ int s_len;
  int target = -1;
  if (c.f.d_seq) {
    for (int t = tid; t < L; t += 256) s_id[t] = c.f.d_seq[(int64_t)b * L + t];
    if (c.f.d_target) target = c.f.d_target[b];
  } else {
    const int u = c.f.d_users[b], e = c.f.d_ends[b];
    int64_t base = 0;
    int cnt = 0, have = 0, lo = 0;
    if (u >= 0 && u < c.f.n_users) {
      base = c.f.d_seq_ptr[u];
      cnt = (int)(c.f.d_seq_ptr[u + 1] - base);
      if (e >= 0 && e <= cnt) {
        lo = e > L ? e - L : 0;
        have = e - lo;
        if (e < cnt) target = c.f.d_seq_flat[base + e];
      }
    }
    for (int t = tid; t < L; t += 256) s_id[t] = t < have ? c.f.d_seq_flat[base + lo + t] : -1;
  }
  __syncthreads();
  if (tid == 0) {
    int len = 0;
    while (len < L && s_id[len] >= 0 && s_id[len] < I) ++len;          // an id outside [0, I) ends the session
    s_len = len;
  }
  __syncthreads();
  const int len = s_len;
  int* NODES = c.NODES + (int64_t)b * L;
  const int n = sort_unique(s_id, len, s_sorted, s_rank, s_u);
  for (int p = tid; p < len; p += 256) {
    if (p == 0 || s_sorted[p] != s_sorted[p - 1]) {
      int q = p + 1;
      while (q < len && s_sorted[q] == s_sorted[p]) ++q;
      NODES[s_u[p]] = s_sorted[p];
      c.CNT[(int64_t)b * L + s_u[p]] = q - p;
    }
    const int al = s_u[s_rank[p]];
    s_alias[p] = al;
    c.ALIAS[(int64_t)b * L + p] = al;
  }
  __syncthreads();
  const int ne = len > 0 ? len - 1 : 0;
  for (int t = tid; t < ne; t += 256) s_key[t] = s_alias[t] << 8 | s_alias[t + 1];
  sort_unique(s_key, ne, s_sorted, s_rank, s_u);
  store_edges(s_sorted, s_u, ne, n, c.EOUT + (int64_t)b * L, c.OPTR + (int64_t)b * (L + 1));
  __syncthreads();
  for (int t = tid; t < ne; t += 256) s_key[t] = s_alias[t + 1] << 8 | s_alias[t];
  sort_unique(s_key, ne, s_sorted, s_rank, s_u);
  store_edges(s_sorted, s_u, ne, n, c.EIN + (int64_t)b * L, c.IPTR + (int64_t)b * (L + 1));
  if (c.keys)
    for (int t = tid; t < L; t += 256) c.keys[(int64_t)b * L + t] = kSentinel;
  if (tid == 0) {
    c.N[b] = n;
    c.LEN[b] = len;
    c.TGT[b] = target;
  }
}

__global__ __launch_bounds__(256) void srgnn_nodes_kernel(Ctx c) {
  const int b = blockIdx.x, tid = threadIdx.x, L = c.w.L, d = c.w.d;
  __shared__ int s_sum[256];
  int part = 0;
  for (int q = tid; q < b; q += 256) part += c.N[q];
  s_sum[tid] = part;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) s_sum[tid] += s_sum[tid + h];
    __syncthreads();
  }
  const int off = s_sum[0], n = c.N[b], len = c.LEN[b];
  if (tid == 0) {
    c.OFF[b] = off;
    if (b == c.B - 1) c.OFF[c.B] = off + n;
    c.LASTROW[b] = len > 0 ? off + c.ALIAS[(int64_t)b * L + len - 1] : -1;
  }
  const int* NODES = c.NODES + (int64_t)b * L;
  for (int e = tid; e < n * d; e += 256) {
    const int i = e / d, j = e - i * d;
    c.H[(int64_t)(off + i) * d + j] = c.w.d_embedding[(int64_t)NODES[i] * d + j];
  }
  for (int i = tid; i < n; i += 256) {
    c.ROWB[off + i] = b;
    c.ROWI[off + i] = i;
    if (c.keys) c.keys[off + i] = row_key(NODES[i], (uint32_t)(off + i));
  }
}

// the transposes the backward row kernels read along their lanes: WgT [2 d][3 d], WcT [d][3 d], W_inT, W_outT, nasr_w2T
__global__ __launch_bounds__(256) void srgnn_transpose_kernel(Ctx c) {
  const int d = c.w.d, dd = d * d;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 12 * dd) return;
  if (e < 6 * dd) {
    const int j = e / (3 * d), k = e - j * 3 * d;
    c.WgT[e] = c.w.d_gates_kernel[(int64_t)k * 2 * d + j];
  } else if (e < 9 * dd) {
    const int r = e - 6 * dd, j = r / (3 * d), k = r - j * 3 * d;
    c.WcT[r] = c.w.d_candidate_kernel[(int64_t)k * d + j];
  } else {
    const int which = (e - 9 * dd) / dd, r = e - 9 * dd - which * dd, j = r / d, k = r - j * d;
    const float* src = which == 0 ? c.w.d_W_in : which == 1 ? c.w.d_W_out : c.w.d_nasr_w2;
    (which == 0 ? c.WinT : which == 1 ? c.WoutT : c.w2T)[r] = src[(int64_t)k * d + j];
  }
}

// ---- the row kernels: thread (row, col) of [R][W]; rows beyond the batch's node count leave at once
#define SRGNN_ROW_COL(W)                                                   \
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;             \
  const int64_t row = idx / (W);                                           \
  const int col = (int)(idx - row * (W));                                  \
  if (row >= c.OFF[c.B]) return

__global__ __launch_bounds__(256) void srgnn_lin_kernel(Ctx c, const float* __restrict__ h) {
  const int d = c.w.d;
  SRGNN_ROW_COL(2 * d);
  const bool in = col < d;
  const int j = in ? col : col - d;
  const float* W = in ? c.w.d_W_in : c.w.d_W_out;
  const float* hr = h + row * d;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < d; ++k) acc = __builtin_fmaf(hr[k], W[(int64_t)k * d + j], acc);
  c.FIO[idx] = acc + (in ? c.w.d_b_in[j] : c.w.d_b_out[j]);
}

// x[i] = [sum_{i -> j} fin_in[j] / indeg(j), sum_{j -> i} fin_out[j] / outdeg(j)]
__global__ __launch_bounds__(256) void srgnn_prop_kernel(Ctx c, float* __restrict__ x) {
  const int d = c.w.d, L = c.w.L;
  SRGNN_ROW_COL(2 * d);
  const int b = c.ROWB[row], i = c.ROWI[row], off = c.OFF[b];
  const int* optr = c.OPTR + (int64_t)b * (L + 1);
  const int* iptr = c.IPTR + (int64_t)b * (L + 1);
  const bool in = col < d;
  const int* own = in ? optr : iptr;
  const int* other = in ? iptr : optr;
  const int* list = (in ? c.EOUT : c.EIN) + (int64_t)b * L;
  float acc = 0.0f;
  for (int e = own[i]; e < own[i + 1]; ++e) {
    const int j = list[e] & 255;
    const float coef = 1.0f / (float)(other[j + 1] - other[j]);
    acc = __builtin_fmaf(coef, c.FIO[(int64_t)(off + j) * 2 * d + col], acc);
  }
  x[idx] = acc;
}

__global__ __launch_bounds__(256) void srgnn_gates_kernel(Ctx c, const float* __restrict__ x, const float* __restrict__ h,
                                                          float* __restrict__ gate) {
  const int d = c.w.d, d2 = 2 * d;
  SRGNN_ROW_COL(d2);
  const float* Wg = c.w.d_gates_kernel;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < d2; ++k) acc = __builtin_fmaf(x[row * d2 + k], Wg[(int64_t)k * d2 + col], acc);
#pragma unroll 8
  for (int k = 0; k < d; ++k) acc = __builtin_fmaf(h[row * d + k], Wg[(int64_t)(d2 + k) * d2 + col], acc);
  gate[idx] = sigmoidf_(acc + c.w.d_gates_bias[col]);
}

__global__ __launch_bounds__(256) void srgnn_cand_kernel(Ctx c, const float* __restrict__ x, const float* __restrict__ h,
                                                         const float* __restrict__ gate, float* __restrict__ cc,
                                                         float* __restrict__ hn, float* __restrict__ rs) {
  const int d = c.w.d, d2 = 2 * d;
  SRGNN_ROW_COL(d);
  const float* Wc = c.w.d_candidate_kernel;
  const float* g = gate + row * d2;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < d2; ++k) acc = __builtin_fmaf(x[row * d2 + k], Wc[(int64_t)k * d + col], acc);
#pragma unroll 8
  for (int k = 0; k < d; ++k) acc = __builtin_fmaf(g[k] * h[row * d + k], Wc[(int64_t)(d2 + k) * d + col], acc);
  const float cv = tanhf(acc + c.w.d_candidate_bias[col]);
  const float u = g[d + col], sv = h[idx];
  cc[idx] = cv;
  hn[idx] = u * sv + (1.0f - u) * cv;
  if (rs) rs[idx] = g[col] * sv;                        // the candidate kernel's state input, for its gradient
}

__global__ __launch_bounds__(256) void srgnn_q_kernel(Ctx c, const float* __restrict__ h) {
  const int d = c.w.d;
  SRGNN_ROW_COL(d);
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < d; ++k) acc = __builtin_fmaf(h[row * d + k], c.w.d_nasr_w2[(int64_t)k * d + col], acc);
  c.M[idx] = acc;
}

// per session: last, m (over q, in place), the nodes' weights, a, ma and sess
__global__ __launch_bounds__(256) void srgnn_readout_kernel(Ctx c, const float* __restrict__ h, float* __restrict__ out,
                                                            int64_t ld) {
  const int b = blockIdx.x, tid = threadIdx.x, d = c.w.d;
  const int off = c.OFF[b], n = c.N[b], lr = c.LASTROW[b];
  __shared__ float s_last[kD], s_w[kLen], s_ma[2 * kD];
  if (tid < d) {
    float acc = 0.0f;
    if (lr >= 0)
      for (int k = 0; k < d; ++k) acc = __builtin_fmaf(h[(int64_t)lr * d + k], c.w.d_nasr_w1[(int64_t)k * d + tid], acc);
    s_last[tid] = acc;
  }
  __syncthreads();
  for (int e = tid; e < n * d; e += 256) {
    const int i = e / d, j = e - i * d;
    float* m = c.M + (int64_t)(off + i) * d + j;
    *m = sigmoidf_(s_last[j] + *m + c.w.d_nasr_b[j]);
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float* m = c.M + (int64_t)(off + i) * d;
    float acc = 0.0f;
    for (int j = 0; j < d; ++j) acc = __builtin_fmaf(m[j], c.w.d_nasrv[j], acc);
    const float w = (float)c.CNT[(int64_t)b * c.w.L + i] * acc;
    s_w[i] = w;
    c.WN[off + i] = w;
  }
  __syncthreads();
  if (tid < d) {
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) acc = __builtin_fmaf(s_w[i], h[(int64_t)(off + i) * d + tid], acc);
    s_ma[tid] = acc;
    s_ma[d + tid] = s_last[tid];
  }
  __syncthreads();
  if (tid < d) {
    float acc = s_ma[tid];
    if (!c.w.nonhybrid) {
      acc = 0.0f;
      for (int k = 0; k < 2 * d; ++k) acc = __builtin_fmaf(s_ma[k], c.w.d_B[(int64_t)k * d + tid], acc);
    }
    c.SESS[(int64_t)b * d + tid] = acc;
    c.MA[(int64_t)b * 2 * d + tid] = s_ma[tid];
    c.MA[(int64_t)b * 2 * d + d + tid] = s_ma[d + tid];
    if (out) out[(int64_t)b * ld + tid] = acc;
  }
}

// grid (I / 64, B / 32): a 64-item tile of the table in LDS (row stride odd: no bank conflicts), item along the lanes
__global__ __launch_bounds__(256) void srgnn_logits_kernel(Ctx c) {
  const int d = c.w.d, I = c.w.n_items, ld = d | 1, tid = threadIdx.x;
  const int i0 = blockIdx.x * 64;
  __shared__ float s_e[64 * (kD + 1)];
  for (int e = tid; e < 64 * d; e += 256) {
    const int il = e / d, k = e - il * d;
    s_e[il * ld + k] = i0 + il < I ? c.w.d_embedding[(int64_t)(i0 + il) * d + k] : 0.0f;
  }
  __syncthreads();
  const int il = tid & 63;
  const float* er = s_e + il * ld;
  for (int bb = tid >> 6; bb < 32; bb += 4) {
    const int b = blockIdx.y * 32 + bb;
    if (b >= c.B) break;
    const float* s = c.SESS + (int64_t)b * d;
    float acc = 0.0f;
#pragma unroll 8
    for (int k = 0; k < d; ++k) acc = __builtin_fmaf(s[k], er[k], acc);
    if (i0 + il < I) c.LOGITS[(int64_t)b * I + i0 + il] = acc;
  }
}

template <bool MAX>
__device__ __forceinline__ float block_tree(float x, float* s) {
  __syncthreads();
  s[threadIdx.x] = x;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] = MAX ? fmaxf(s[threadIdx.x], s[threadIdx.x + h]) : s[threadIdx.x] + s[threadIdx.x + h];
    __syncthreads();
  }
  return s[0];
}

// per session: the maximum, the sum of exp(logit - maximum), the loss term, then (p - y) / B over the logits
__global__ __launch_bounds__(256) void srgnn_softmax_kernel(Ctx c) {
  const int b = blockIdx.x, tid = threadIdx.x, I = c.w.n_items;
  float* z = c.LOGITS + (int64_t)b * I;
  __shared__ float s[256];
  float mx = -__builtin_huge_valf();
  for (int i = tid; i < I; i += 256) mx = fmaxf(mx, z[i]);
  mx = block_tree<true>(mx, s);
  float sum = 0.0f;
  for (int i = tid; i < I; i += 256) sum += expf(z[i] - mx);
  sum = block_tree<false>(sum, s);
  const int tgt = c.TGT[b];
  const bool real = tgt >= 0 && tgt < I;                    // a session without a target takes no part
  if (tid == 0) c.LOSSB[b] = real ? logf(sum) - (z[tgt] - mx) : 0.0f;
  __syncthreads();
  const float inv_b = 1.0f / (float)c.B;
  for (int i = tid; i < I; i += 256) {
    const float p = expf(z[i] - mx) / sum;
    z[i] = real ? (p - (i == tgt ? 1.0f : 0.0f)) * inv_b : 0.0f;
  }
}

// 32 items per workgroup, 8 per wavefront, the columns along the lanes: G[i] = sum_b dl[b][i] sess[b] + L2 embedding[i]
__global__ __launch_bounds__(256) void srgnn_headg_kernel(Ctx c, float* __restrict__ G, float l2) {
  const int d = c.w.d, I = c.w.n_items, lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * 32 + (threadIdx.x >> 6) * 8;
  float acc[8][2];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m][0] = acc[m][1] = 0.0f;
  for (int b = 0; b < c.B; ++b) {
    const float* s = c.SESS + (int64_t)b * d;
    const float s0 = lane < d ? s[lane] : 0.0f, s1 = lane + 64 < d ? s[lane + 64] : 0.0f;
    const float* dl = c.LOGITS + (int64_t)b * I;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float g = i0 + m < I ? dl[i0 + m] : 0.0f;
      acc[m][0] = __builtin_fmaf(g, s0, acc[m][0]);
      acc[m][1] = __builtin_fmaf(g, s1, acc[m][1]);
    }
  }
  double v[1] = {0.0};
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (i0 + m >= I) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int col = lane + 64 * q;
      if (col < d) {
        const float e = c.w.d_embedding[(int64_t)(i0 + m) * d + col];
        G[(int64_t)(i0 + m) * d + col] = __builtin_fmaf(l2, e, acc[m][q]);
        v[0] += (double)e * (double)e;
      }
    }
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) c.l2part[blockIdx.x] = v[0];
}

// grid (item chunks, B / 4): one wavefront per session and chunk, items ascending
__global__ __launch_bounds__(256) void srgnn_dsess_kernel(Ctx c) {
  const int d = c.w.d, I = c.w.n_items, lane = threadIdx.x & 63;
  const int b = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (b >= c.B) return;
  const int i0 = blockIdx.x * kItemChunk, i1 = i0 + kItemChunk < I ? i0 + kItemChunk : I;
  const float* dl = c.LOGITS + (int64_t)b * I;
  float a0 = 0.0f, a1 = 0.0f;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) {
    const float g = dl[i];
    const float* e = c.w.d_embedding + (int64_t)i * d;
    if (lane < d) a0 = __builtin_fmaf(g, e[lane], a0);
    if (lane + 64 < d) a1 = __builtin_fmaf(g, e[lane + 64], a1);
  }
  float* dst = c.DSP + ((int64_t)blockIdx.x * c.B + b) * d;
  if (lane < d) dst[lane] = a0;
  if (lane + 64 < d) dst[lane + 64] = a1;
}

__global__ __launch_bounds__(256) void srgnn_dsess_sum_kernel(Ctx c, int chunks) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)c.B * c.w.d;
  if (idx >= n) return;
  float acc = 0.0f;
  for (int q = 0; q < chunks; ++q) acc += c.DSP[(int64_t)q * n + idx];
  c.DSESS[idx] = acc;
}

// per session: d ma = d sess B^T, d a, d last; per node d(coefficient), DQ = d(pre-sigmoid); the session's shares of the
// nasrv and nasr_b gradients; d last_h
__global__ __launch_bounds__(256) void srgnn_readout_bwd_kernel(Ctx c, const float* __restrict__ h) {
  const int b = blockIdx.x, tid = threadIdx.x, d = c.w.d;
  const int off = c.OFF[b], n = c.N[b];
  __shared__ float s_ds[kD], s_dma[2 * kD], s_dcn[kLen], s_dl[kD];
  if (tid < d) s_ds[tid] = c.DSESS[(int64_t)b * d + tid];
  __syncthreads();
  if (tid < 2 * d) {
    float acc;
    if (c.w.nonhybrid) {
      acc = tid < d ? s_ds[tid] : 0.0f;
    } else {
      acc = 0.0f;
      for (int j = 0; j < d; ++j) acc = __builtin_fmaf(s_ds[j], c.w.d_B[(int64_t)tid * d + j], acc);
    }
    s_dma[tid] = acc;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float* hr = h + (int64_t)(off + i) * d;
    float acc = 0.0f;
    for (int j = 0; j < d; ++j) acc = __builtin_fmaf(hr[j], s_dma[j], acc);
    s_dcn[i] = (float)c.CNT[(int64_t)b * c.w.L + i] * acc;
  }
  __syncthreads();
  for (int e = tid; e < n * d; e += 256) {
    const int i = e / d, j = e - i * d;
    const float m = c.M[(int64_t)(off + i) * d + j];
    c.DQ[(int64_t)(off + i) * d + j] = s_dcn[i] * c.w.d_nasrv[j] * (m * (1.0f - m));
  }
  if (tid < d) {
    const float v = c.w.d_nasrv[tid];
    float gnb = 0.0f, gv = 0.0f;
    for (int i = 0; i < n; ++i) {
      const float m = c.M[(int64_t)(off + i) * d + tid];
      gnb += s_dcn[i] * v * (m * (1.0f - m));
      gv = __builtin_fmaf(s_dcn[i], m, gv);
    }
    const float dl = s_dma[d + tid] + gnb;
    s_dl[tid] = dl;
    c.GNB[(int64_t)b * d + tid] = gnb;
    c.GV[(int64_t)b * d + tid] = gv;
    c.DLAST[(int64_t)b * d + tid] = dl;
    c.DA[(int64_t)b * d + tid] = s_dma[tid];
  }
  __syncthreads();
  if (tid < d) {
    float acc = 0.0f;
    for (int j = 0; j < d; ++j) acc = __builtin_fmaf(s_dl[j], c.w.d_nasr_w1[(int64_t)tid * d + j], acc);
    c.DLASTH[(int64_t)b * d + tid] = acc;
  }
}

// dh[row] = weight da + DQ nasr_w2^T (+ d last_h on the session's last node)
__global__ __launch_bounds__(256) void srgnn_dh_kernel(Ctx c, float* __restrict__ dh) {
  const int d = c.w.d;
  SRGNN_ROW_COL(d);
  const int b = c.ROWB[row];
  const float* dq = c.DQ + row * d;
  const float* w2 = c.w2T + col;
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(dq[j], w2[(int64_t)j * d], acc);
  acc = __builtin_fmaf(c.WN[row], c.DA[(int64_t)b * d + col], acc);
  if (row == c.LASTROW[b]) acc += c.DLASTH[(int64_t)b * d + col];
  dh[idx] = acc;
}

// h' = u s + (1 - u) c:  dpc = dh (1 - u) (1 - c^2);  dpg[:, d + j] = dh (s - c) u (1 - u)
__global__ __launch_bounds__(256) void srgnn_cellbwd_kernel(Ctx c, const float* __restrict__ dh,
                                                            const float* __restrict__ s, const float* __restrict__ gate,
                                                            const float* __restrict__ cc, float* __restrict__ dpc,
                                                            float* __restrict__ dpg) {
  const int d = c.w.d;
  SRGNN_ROW_COL(d);
  const float g = dh[idx], u = gate[row * 2 * d + d + col], cv = cc[idx], sv = s[idx];
  dpc[idx] = g * (1.0f - u) * (1.0f - cv * cv);
  dpg[row * 2 * d + d + col] = g * (sv - cv) * (u * (1.0f - u));
}

// d(r s)[k] = sum_j dpc[j] Wc[2 d + k][j];  dpg[:, k] = d(r s) s r (1 - r);  ds = dh u + d(r s) r
__global__ __launch_bounds__(256) void srgnn_dr_kernel(Ctx c, const float* __restrict__ dh, const float* __restrict__ s,
                                                       const float* __restrict__ gate, const float* __restrict__ dpc,
                                                       float* __restrict__ dpg, float* __restrict__ ds) {
  const int d = c.w.d;
  SRGNN_ROW_COL(d);
  const float* w = c.WcT + 2 * d + col;
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(dpc[row * d + j], w[(int64_t)j * 3 * d], acc);
  const float r = gate[row * 2 * d + col], u = gate[row * 2 * d + d + col];
  dpg[row * 2 * d + col] = acc * s[idx] * (r * (1.0f - r));
  ds[idx] = __builtin_fmaf(acc, r, dh[idx] * u);
}

// columns k < 2 d: dx[k] = dpc Wc[k]^T + dpg Wg[k]^T;  columns 2 d + k: ds[k] += dpg Wg[2 d + k]^T
__global__ __launch_bounds__(256) void srgnn_dx_kernel(Ctx c, const float* __restrict__ dpc,
                                                       const float* __restrict__ dpg, float* __restrict__ ds) {
  const int d = c.w.d, d2 = 2 * d;
  SRGNN_ROW_COL(3 * d);
  const int d3 = 3 * d;
  const float* wg = c.WgT + col;
  float acc = 0.0f;
  if (col < d2) {
    const float* wc = c.WcT + col;
#pragma unroll 8
    for (int j = 0; j < d; ++j) acc = __builtin_fmaf(dpc[row * d + j], wc[(int64_t)j * d3], acc);
  }
#pragma unroll 8
  for (int j = 0; j < d2; ++j) acc = __builtin_fmaf(dpg[row * d2 + j], wg[(int64_t)j * d3], acc);
  if (col < d2) c.DX[row * d2 + col] = acc;
  else ds[row * d + (col - d2)] += acc;
}

// d fin_in[j] = sum_{i -> j} dx_in[i] / indeg(j);  d fin_out[j] = sum_{j -> i} dx_out[i] / outdeg(j)
__global__ __launch_bounds__(256) void srgnn_propT_kernel(Ctx c, float* __restrict__ dfio) {
  const int d = c.w.d, L = c.w.L;
  SRGNN_ROW_COL(2 * d);
  const int b = c.ROWB[row], i = c.ROWI[row], off = c.OFF[b];
  const bool in = col < d;
  const int* own = (in ? c.IPTR : c.OPTR) + (int64_t)b * (L + 1);
  const int* list = (in ? c.EIN : c.EOUT) + (int64_t)b * L;
  const int e0 = own[i], e1 = own[i + 1];
  const float coef = e1 > e0 ? 1.0f / (float)(e1 - e0) : 0.0f;
  float acc = 0.0f;
  for (int e = e0; e < e1; ++e) acc = __builtin_fmaf(coef, c.DX[(int64_t)(off + (list[e] & 255)) * 2 * d + col], acc);
  dfio[idx] = acc;
}

__global__ __launch_bounds__(256) void srgnn_linT_kernel(Ctx c, const float* __restrict__ dfio, float* __restrict__ ds) {
  const int d = c.w.d;
  SRGNN_ROW_COL(d);
  const float* g = dfio + row * 2 * d;
  const float* wi = c.WinT + col;
  const float* wo = c.WoutT + col;
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(g[j], wi[(int64_t)j * d], acc);
#pragma unroll 8
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(g[d + j], wo[(int64_t)j * d], acc);
  ds[idx] += acc;
}

struct WArgs {
  int64_t nW, end[kVars];
  const float* W[kVars];
  float* G[kVars];
  float l2;
  int head_blocks;
};

enum { V_W1, V_W2, V_NV, V_NB, V_WIN, V_BIN, V_WOUT, V_BOUT, V_B, V_WG, V_BG, V_WC, V_BC };

__device__ __forceinline__ int var_of(const WArgs& a, int64_t e, int64_t& at) {
  int k = 0;
  while (e >= a.end[k]) ++k;
  at = e - (k ? a.end[k - 1] : 0);
  return k;
}

// grid (elements / 256, chunks): element e of the 13 variables laid end to end, over the sessions or the node rows of
// chunk blockIdx.y, iterations ascending, rows ascending
__global__ __launch_bounds__(256) void srgnn_wgrad_kernel(Ctx c, WArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.nW) return;
  const int d = c.w.d, d2 = 2 * d, S = c.w.step, chunk = blockIdx.y;
  const int total = c.OFF[c.B];
  const int rpc = (total + kChunks - 1) / kChunks, bpc = (c.B + kChunks - 1) / kChunks;
  const int r0 = chunk * rpc, r1 = r0 + rpc < total ? r0 + rpc : total;
  const int b0 = chunk * bpc, b1 = b0 + bpc < c.B ? b0 + bpc : c.B;
  const int64_t Rd = c.R * d, Rd2 = c.R * d2;
  const float* hf = c.H + (int64_t)S * Rd;
  int64_t at;
  const int var = var_of(a, e, at);
  float acc = 0.0f;
  // a matrix over the node rows: sum over (iteration, row) of in[row][k] g[row][j]; a bias: the same with in = 1
  const float *in = nullptr, *gr = nullptr;
  int in_ld = 0, g_ld = 0;
  int64_t in_it = 0, g_it = 0;                 // the buffers' strides between iterations (0: the final state only)
  int its = S;
  switch (var) {
    case V_W1: {
      const int k = (int)(at / d), j = (int)(at % d);
      for (int b = b0; b < b1; ++b) {
        const int lr = c.LASTROW[b];
        if (lr >= 0) acc = __builtin_fmaf(hf[(int64_t)lr * d + k], c.DLAST[(int64_t)b * d + j], acc);
      }
    } break;
    case V_W2:
      in = hf + at / d, in_ld = d, gr = c.DQ + at % d, g_ld = d, its = 1;
      break;
    case V_NV:
      for (int b = b0; b < b1; ++b) acc += c.GV[(int64_t)b * d + at];
      break;
    case V_NB:
      for (int b = b0; b < b1; ++b) acc += c.GNB[(int64_t)b * d + at];
      break;
    case V_WIN:
    case V_WOUT:
      in = c.H + at / d, in_ld = d, in_it = Rd;
      gr = c.DFIO + at % d + (var == V_WOUT ? d : 0), g_ld = d2, g_it = Rd2;
      break;
    case V_BIN:
    case V_BOUT:
      gr = c.DFIO + at + (var == V_BOUT ? d : 0), g_ld = d2, g_it = Rd2;
      break;
    case V_B: {
      const int k = (int)(at / d), j = (int)(at % d);
      if (!c.w.nonhybrid)
        for (int b = b0; b < b1; ++b) acc = __builtin_fmaf(c.MA[(int64_t)b * d2 + k], c.DSESS[(int64_t)b * d + j], acc);
    } break;
    case V_WG: {
      const int k = (int)(at / d2);
      if (k < d2) in = c.X + k, in_ld = d2, in_it = Rd2;
      else in = c.H + (k - d2), in_ld = d, in_it = Rd;
      gr = c.DPG + at % d2, g_ld = d2, g_it = Rd2;
    } break;
    case V_BG:
      gr = c.DPG + at, g_ld = d2, g_it = Rd2;
      break;
    case V_WC: {
      const int k = (int)(at / d);
      if (k < d2) in = c.X + k, in_ld = d2, in_it = Rd2;
      else in = c.RS + (k - d2), in_ld = d, in_it = Rd;
      gr = c.DPC + at % d, g_ld = d, g_it = Rd;
    } break;
    default:
      gr = c.DPC + at, g_ld = d, g_it = Rd;
      break;
  }
  if (gr) {
    for (int s = 0; s < its; ++s) {
      const float* g = gr + s * g_it;
      if (in) {
        const float* x = in + s * in_it;
#pragma unroll 8
        for (int r = r0; r < r1; ++r) acc = __builtin_fmaf(x[(int64_t)r * in_ld], g[(int64_t)r * g_ld], acc);
      } else {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) acc += g[(int64_t)r * g_ld];
      }
    }
  }
  c.part[(int64_t)chunk * a.nW + e] = acc;
}

// the chunks in chunk order, + L2 v, stored; sum v^2 per workgroup
__global__ __launch_bounds__(256) void srgnn_wsum_kernel(Ctx c, WArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[1] = {0.0};
  if (e < a.nW) {
    float acc = 0.0f;
    for (int q = 0; q < kChunks; ++q) acc += c.part[(int64_t)q * a.nW + e];
    int64_t at;
    const int var = var_of(a, e, at);
    const float x = a.W[var][at];
    a.G[var][at] = __builtin_fmaf(a.l2, x, acc);
    v[0] = (double)x * (double)x;
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) c.l2part[a.head_blocks + blockIdx.x] = v[0];
}

// one wavefront per sorted key: the head of a run adds the run's node rows in key order to the table row's gradient
__global__ __launch_bounds__(256) void srgnn_rows_kernel(Ctx c, const float* __restrict__ dh, float* __restrict__ G) {
  const int lane = threadIdx.x & 63, d = c.w.d;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = nr::rowkey::head_row(c.keys, c.R, w);
  if (row < 0) return;
  float a0 = 0.0f, a1 = 0.0f;
  nr::rowkey::for_run(c.keys, c.R, w, row, [&](uint32_t slot) {
    const float* src = dh + (int64_t)slot * d;
    if (lane < d) a0 += src[lane];
    if (lane + 64 < d) a1 += src[lane + 64];
  });
  float* dst = G + (int64_t)row * d;
  if (lane < d) dst[lane] += a0;
  if (lane + 64 < d) dst[lane + 64] += a1;
}

__global__ __launch_bounds__(256) void srgnn_loss_kernel(Ctx c, int parts, float l2, float* __restrict__ loss2) {
  double v[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < c.B; b += 256) v[0] += (double)c.LOSSB[b];
  for (int i = threadIdx.x; i < parts; i += 256) v[1] += c.l2part[i];
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) {
    loss2[0] = (float)(v[0] / (double)c.B);
    loss2[1] = (float)(0.5 * (double)l2 * v[1]);
  }
}

int check_shape(const char* who, const nrhip_srgnn_weights& w, int B) {
  NR_REQUIRE(w.d >= 1 && w.d <= kD, NR_ERR_UNSUPPORTED, "%s: hidden_size %d outside 1..%d", who, w.d, kD);
  NR_REQUIRE(w.L >= 1 && w.L <= kLen, NR_ERR_UNSUPPORTED, "%s: max_seq_len %d outside 1..%d", who, w.L, kLen);
  NR_REQUIRE(w.step >= 1 && w.step <= kS, NR_ERR_UNSUPPORTED, "%s: step %d outside 1..%d", who, w.step, kS);
  NR_REQUIRE(B >= 0 && B <= kB, NR_ERR_UNSUPPORTED, "%s: batch_size %d outside 0..%d", who, B, kB);
  NR_REQUIRE(w.n_items >= 0, NR_ERR_ARG, "%s: negative num_items", who);
  NR_REQUIRE((int64_t)(B > 0 ? B : 1) * w.n_items < (1ll << 31), NR_ERR_UNSUPPORTED,
             "%s: batch_size * num_items = %lld is not supported (below 2^31)", who,
             (long long)((int64_t)B * w.n_items));
  return NR_OK;
}

int check_pointers(const char* who, const nrhip_srgnn_weights& w, const nrhip_srgnn_feed& f) {
  NR_REQUIRE(w.d_nasr_w1 && w.d_nasr_w2 && w.d_nasrv && w.d_nasr_b && w.d_embedding && w.d_W_in && w.d_b_in &&
                 w.d_W_out && w.d_b_out && w.d_B && w.d_gates_kernel && w.d_gates_bias && w.d_candidate_kernel &&
                 w.d_candidate_bias, NR_ERR_ARG, "%s: null weight pointer", who);
  NR_REQUIRE(f.d_seq || (f.d_users && f.d_ends && f.d_seq_ptr && f.d_seq_flat && f.n_users >= 0), NR_ERR_ARG,
             "%s: the feed is neither padded rows (d_seq) nor (user, end) pairs over resident sequences", who);
  return NR_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

Ctx context_of(const nrhip_srgnn_weights& w, const nrhip_srgnn_feed& f, int B, float* ws, uint64_t* keys,
               const Layout& y) {
  Ctx c = {};
  c.w = w, c.f = f, c.keys = keys, c.B = B, c.R = (int64_t)B * w.L;
  int* wi = (int*)ws;
  c.l2part = (double*)(ws + y.l2part);
  c.NODES = wi + y.NODES, c.ALIAS = wi + y.ALIAS, c.CNT = wi + y.CNT, c.EOUT = wi + y.EOUT, c.EIN = wi + y.EIN;
  c.OPTR = wi + y.OPTR, c.IPTR = wi + y.IPTR, c.N = wi + y.N, c.LEN = wi + y.LEN, c.OFF = wi + y.OFF;
  c.TGT = wi + y.TGT, c.ROWB = wi + y.ROWB, c.ROWI = wi + y.ROWI, c.LASTROW = wi + y.LASTROW;
  c.H = ws + y.H, c.X = ws + y.X, c.GATE = ws + y.GATE, c.CC = ws + y.CC, c.FIO = ws + y.FIO, c.DFIO = ws + y.DFIO;
  c.DPG = ws + y.DPG, c.DPC = ws + y.DPC, c.DX = ws + y.DX, c.DHA = ws + y.DHA, c.DHB = ws + y.DHB, c.M = ws + y.M;
  c.DQ = ws + y.DQ, c.WN = ws + y.WN, c.LAST = ws + y.LAST, c.MA = ws + y.MA, c.SESS = ws + y.SESS;
  c.DSESS = ws + y.DSESS, c.DLAST = ws + y.DLAST, c.GV = ws + y.GV, c.GNB = ws + y.GNB, c.DA = ws + y.DA;
  c.DLASTH = ws + y.DLASTH, c.LOGITS = ws + y.LOGITS, c.LOSSB = ws + y.LOSSB, c.DSP = ws + y.DSP, c.part = ws + y.part;
  const size_t dd = (size_t)w.d * w.d;
  c.RS = ws + y.RS, c.WgT = ws + y.WT, c.WcT = c.WgT + 6 * dd, c.WinT = c.WcT + 3 * dd, c.WoutT = c.WinT + dd;
  c.w2T = c.WoutT + dd;
  return c;
}

// the graph, the S iterations and the readout; out (row stride ld) may be NULL
int forward_pass(const Ctx& c, float* out, int64_t ld, bool train, hipStream_t st) {
  const int B = c.B, d = c.w.d, S = c.w.step;
  const int64_t R = c.R, Rd = R * d, Rd2 = 2 * Rd;
  const dim3 blk(256);
  hipLaunchKernelGGL(srgnn_graph_kernel, dim3(B), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_nodes_kernel, dim3(B), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  for (int s = 0; s < S; ++s) {
    float *h = c.H + s * Rd, *x = c.X + s * Rd2, *gate = c.GATE + s * Rd2;
    hipLaunchKernelGGL(srgnn_lin_kernel, dim3(blocks_of(Rd2)), blk, 0, st, c, (const float*)h);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_prop_kernel, dim3(blocks_of(Rd2)), blk, 0, st, c, x);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_gates_kernel, dim3(blocks_of(Rd2)), blk, 0, st, c, (const float*)x, (const float*)h, gate);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_cand_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, (const float*)x, (const float*)h,
                       (const float*)gate, c.CC + s * Rd, h + Rd, train ? c.RS + s * Rd : nullptr);
    NR_LAUNCH_CHECK();
  }
  const float* hf = c.H + S * Rd;
  hipLaunchKernelGGL(srgnn_q_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, hf);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_readout_kernel, dim3(B), blk, 0, st, c, hf, out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_srgnn_workspace_floats(int max_batch, int max_seq_len, int hidden_size, int step, int num_items,
                                 size_t* floats) {
  NR_REQUIRE(floats, NR_ERR_ARG, "srgnn_workspace_floats: null argument");
  nrhip_srgnn_weights w = {};
  w.d = hidden_size, w.L = max_seq_len, w.step = step, w.n_items = num_items;
  NR_TRY(check_shape("srgnn_workspace_floats", w, max_batch));
  *floats = layout_of(max_batch, max_seq_len, hidden_size, step, num_items, true).total;
  return NR_OK;
}

int nrhip_srgnn_step(const nrhip_srgnn_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "srgnn_step: null argument block");
  const nrhip_srgnn_step_args a = *args;
  const nrhip_srgnn_weights& w = a.w;
  NR_TRY(check_shape("srgnn_step", w, a.batch));
  NR_TRY(check_pointers("srgnn_step", w, a.f));
  const int B = a.batch, d = w.d, S = w.step, I = w.n_items;
  if (B == 0) return NR_OK;
  NR_REQUIRE(I >= 1, NR_ERR_ARG, "srgnn_step: no items");
  NR_REQUIRE(a.d_G_nasr_w1 && a.d_G_nasr_w2 && a.d_G_nasrv && a.d_G_nasr_b && a.d_G_embedding && a.d_G_W_in &&
                 a.d_G_b_in && a.d_G_W_out && a.d_G_b_out && a.d_G_B && a.d_G_gates_kernel && a.d_G_gates_bias &&
                 a.d_G_candidate_kernel && a.d_G_candidate_bias && a.d_keys && a.d_ws && a.d_loss2, NR_ERR_ARG,
             "srgnn_step: null pointer argument");
  NR_REQUIRE(a.f.d_seq == nullptr || a.f.d_target, NR_ERR_ARG, "srgnn_step: padded rows without targets");
  hipStream_t st = (hipStream_t)stream;
  const Layout y = layout_of(B, w.L, d, S, I, true);
  const Ctx c = context_of(w, a.f, B, a.d_ws, a.d_keys, y);
  const int64_t R = c.R, Rd = R * d, Rd2 = 2 * Rd;
  const dim3 blk(256);
  NR_TRY(forward_pass(c, nullptr, 0, true, st));

  hipLaunchKernelGGL(srgnn_logits_kernel, dim3((unsigned)((I + 63) / 64), (unsigned)((B + 31) / 32)), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_softmax_kernel, dim3(B), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_headg_kernel, dim3(y.head_blocks), blk, 0, st, c, a.d_G_embedding, a.l2);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_dsess_kernel, dim3(y.item_chunks, (unsigned)((B + 3) / 4)), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_dsess_sum_kernel, dim3(blocks_of((int64_t)B * d)), blk, 0, st, c, y.item_chunks);
  NR_LAUNCH_CHECK();

  hipLaunchKernelGGL(srgnn_transpose_kernel, dim3(blocks_of(12ll * d * d)), blk, 0, st, c);
  NR_LAUNCH_CHECK();
  const float* hf = c.H + S * Rd;
  hipLaunchKernelGGL(srgnn_readout_bwd_kernel, dim3(B), blk, 0, st, c, hf);
  NR_LAUNCH_CHECK();
  float *dh = c.DHA, *ds = c.DHB;
  hipLaunchKernelGGL(srgnn_dh_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, dh);
  NR_LAUNCH_CHECK();
  for (int s = S - 1; s >= 0; --s) {
    const float *h = c.H + s * Rd, *gate = c.GATE + s * Rd2, *cc = c.CC + s * Rd;
    float *dpc = c.DPC + s * Rd, *dpg = c.DPG + s * Rd2, *dfio = c.DFIO + s * Rd2;
    hipLaunchKernelGGL(srgnn_cellbwd_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, (const float*)dh, h, gate, cc, dpc, dpg);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_dr_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, (const float*)dh, h, gate, (const float*)dpc,
                       dpg, ds);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_dx_kernel, dim3(blocks_of(3 * Rd)), blk, 0, st, c, (const float*)dpc, (const float*)dpg, ds);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_propT_kernel, dim3(blocks_of(Rd2)), blk, 0, st, c, dfio);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(srgnn_linT_kernel, dim3(blocks_of(Rd)), blk, 0, st, c, (const float*)dfio, ds);
    NR_LAUNCH_CHECK();
    float* t = dh;
    dh = ds;
    ds = t;
  }

  WArgs g = {};
  g.nW = y.nW;
  for (int k = 0; k < kVars; ++k) g.end[k] = y.end[k];
  const float* W[kVars] = {w.d_nasr_w1, w.d_nasr_w2, w.d_nasrv, w.d_nasr_b, w.d_W_in, w.d_b_in, w.d_W_out, w.d_b_out,
                           w.d_B, w.d_gates_kernel, w.d_gates_bias, w.d_candidate_kernel, w.d_candidate_bias};
  float* G[kVars] = {a.d_G_nasr_w1, a.d_G_nasr_w2, a.d_G_nasrv, a.d_G_nasr_b, a.d_G_W_in, a.d_G_b_in, a.d_G_W_out,
                     a.d_G_b_out, a.d_G_B, a.d_G_gates_kernel, a.d_G_gates_bias, a.d_G_candidate_kernel,
                     a.d_G_candidate_bias};
  for (int k = 0; k < kVars; ++k) g.W[k] = W[k], g.G[k] = G[k];
  g.l2 = a.l2;
  g.head_blocks = y.head_blocks;
  hipLaunchKernelGGL(srgnn_wgrad_kernel, dim3(y.w_blocks, kChunks), blk, 0, st, c, g);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_wsum_kernel, dim3(y.w_blocks), blk, 0, st, c, g);
  NR_LAUNCH_CHECK();

  NR_TRY(nrhip_sort_u64(a.d_keys, (int)R, stream));
  hipLaunchKernelGGL(srgnn_rows_kernel, dim3((unsigned)((R + 3) / 4)), blk, 0, st, c, (const float*)dh, a.d_G_embedding);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(srgnn_loss_kernel, dim3(1), blk, 0, st, c, y.head_blocks + y.w_blocks, a.l2, a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_srgnn_forward(const nrhip_srgnn_weights* weights, const nrhip_srgnn_feed* feed, int n, float* d_ws,
                        float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(weights && feed, NR_ERR_ARG, "srgnn_forward: null argument block");
  const nrhip_srgnn_weights w = *weights;
  NR_TRY(check_shape("srgnn_forward", w, n));
  NR_TRY(check_pointers("srgnn_forward", w, *feed));
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_ws && d_out && ld >= w.d, NR_ERR_ARG, "srgnn_forward: null pointer argument or ld < hidden_size");
  nrhip_srgnn_feed f = *feed;
  f.d_target = nullptr;
  const Layout y = layout_of(n, w.L, w.d, w.step, w.n_items, false);
  const Ctx c = context_of(w, f, n, d_ws, nullptr, y);
  return forward_pass(c, d_out, ld, false, (hipStream_t)stream);
}

}  // extern "C"
