// neumf.hip — the NeuMF / MLP step (model/general_recommender/NeuMF.py:69-100, MLP.py up to the optimiser), the pairs'
// forward pass and the all-items scorer, fp32.  Notation: U users, I items, d embedding_size (0: MLP, no GMF branch),
// e = layers[0] / 2 (integer), nL layers of widths w[k]; layer k reads in[k] = 2 e (k = 0) or w[k - 1] values.
//
//   neumf_row_kernel<TRAIN, STAGED>  one workgroup per chunk of batch rows, eight rows at a time.  STAGED: the whole layer
//                            stack lies in LDS (odd row strides: the forward pass walks a kernel by columns, the backward
//                            pass by rows), when it fits kStage floats — the shipped [64,32,16] does; wider stacks are
//                            read through the caches.  A row's activations stay in LDS from the gathers to its
//                            dL/d(embedding rows): relu layers, y = sum(p q) + sum(h_last), the loss and g = dL/dy, then
//                            per layer from the top the chunk's share of the kernel and bias gradients (added into the
//                            chunk's own partials, rows ascending), and dz of the layer below IN PLACE over its
//                            activations (0 where the pre-activation was <= 0, i.e. the activation is not > 0).  The L2
//                            terms' gradients ride with the rows' slots
//   neumf_reduce_kernel      the chunks' partials added in chunk order and stored
//   nrhip_sort_u64           the keys, ascending: one key space of U + I rows (user, item), low word = the batch slot
//   neumf_rows_kernel        one wavefront per sorted key: the head of a run adds the run's slots in key order and STORES
//                            the row's gradients of the mf_* and mlp_* tables (rowkey_common.h)
//   neumf_loss_kernel        one workgroup: data term and regulariser, in double, rounded once
//
//   neumf_proj_kernel        A = M[users] W1u + b1 [n, w0] and Bm = N W1i [I, w0]: the first layer is linear in the concat
//   neumf_pack_kernel        layers 2.. zero-padded to multiples of 32 in both dimensions
//   neumf_pairs_kernel<STAGE, MAXT>  a workgroup per (32 items, TU users) tile, a wavefront per (user, 32 items): h1 =
//                            relu(A_u + Bm_i) in registers, then every further layer on v_mfma_f32_32x32x2_f32 in the
//                            transposed form D[output][pair] = W^T h: a lane then holds, of ONE pair, the outputs
//                            (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) — exactly the k values it must feed the next
//                            layer's MFMAs as their B operand.  The chain never leaves the registers; relu, the row sum,
//                            and the GMF dot are the epilogue, one store per score.  STAGE: the padded layers lie in LDS
//                            beside the tiles; MAXT: the 32-tiles of the widest layer (DESIGN 6q has the measurements)
//
// Every float sum is taken in a fixed order, no atomics: two calls on the same inputs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using nr::rowkey::kSentinel;
using nr::rowkey::row_key;

constexpr int kW = NRHIP_NEUMF_MAX_WIDTH;
constexpr int kLayers = NRHIP_NEUMF_MAX_LAYERS;
constexpr int kB = NRHIP_NEUMF_MAX_BATCH;
constexpr int kR = 8;                                // batch rows a workgroup holds at a time
constexpr int kStage = 8192;                         // floats of LDS for the staged layer stack
constexpr int kChunks = 32;                          // row chunks of the dense variables' partials
constexpr int kPairLds = 65536;                      // bytes of LDS a workgroup of the pairs kernel may take
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Shape {
  int nL, d, e;
  int in[kLayers], w[kLayers];
  int ldw[kLayers], soffW[kLayers], soffB[kLayers];   // staged: odd row stride, offsets into s_w
  int64_t offW[kLayers], offB[kLayers], nW;           // the dense variables laid end to end
  int staged;
};

Shape shape_of(const nrhip_neumf_weights& w) {
  Shape s = {};
  s.nL = w.n_layers, s.d = w.d, s.e = w.width[0] / 2;
  int64_t o = 0;
  int so = 0;
  for (int k = 0; k < s.nL; ++k) {
    s.w[k] = w.width[k];
    s.in[k] = k ? w.width[k - 1] : 2 * s.e;
    s.ldw[k] = s.w[k] | 1;
    s.offW[k] = o, o += (int64_t)s.in[k] * s.w[k];
    s.offB[k] = o, o += s.w[k];
    s.soffW[k] = so, so += s.in[k] * s.ldw[k];
    s.soffB[k] = so, so += s.w[k];
  }
  s.nW = o;
  s.staged = so <= kStage;
  return s;
}

struct Layout {
  size_t TERM, REG, DP, DQ, DM, DN, part, total;
  int chunks, rpc;
};

Layout layout_of(int B, const Shape& s) {
  Layout y;
  const size_t b = (size_t)(B > 0 ? B : 1);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 3) / 4 * 4; return at; };
  y.TERM = take(b);
  y.REG = take(b);
  y.DP = take(b * s.d);
  y.DQ = take(b * s.d);
  y.DM = take(b * s.e);
  y.DN = take(b * s.e);
  y.chunks = (int)((b + kR - 1) / kR < (size_t)kChunks ? (b + kR - 1) / kR : (size_t)kChunks);
  y.rpc = (int)((b + y.chunks - 1) / y.chunks);
  y.part = take((size_t)y.chunks * s.nW);
  y.total = o;
  return y;
}

struct RowArgs {
  nrhip_neumf_weights w;
  Shape s;
  const int32_t* users;
  const int32_t* items;
  const float* labels;
  uint64_t* keys;
  uint8_t *flag_mf_user, *flag_mf_item, *flag_mlp_user, *flag_mlp_item;
  float *TERM, *REG, *DP, *DQ, *DM, *DN, *part;
  float* out;
  int B, rpc, loss_kind;
  float reg_mf, reg_mlp;
};

template <bool TRAIN, bool STAGED>
__global__ __launch_bounds__(256) void neumf_row_kernel(RowArgs a) {
  __shared__ float s_w[STAGED ? kStage : 1];
  __shared__ float s_act[(kLayers + 1) * kR * kW];
  __shared__ float s_g[kR];
  __shared__ int s_u[kR], s_i[kR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Shape& s = a.s;
  const int nL = s.nL, d = s.d, e = s.e, U = a.w.n_users, I = a.w.n_items, B = a.B;
  if (STAGED) {
    for (int k = 0; k < nL; ++k) {
      const int w = s.w[k], n = s.in[k] * w;
      for (int idx = tid; idx < n; idx += 256) {
        const int i = idx / w, j = idx - i * w;
        s_w[s.soffW[k] + i * s.ldw[k] + j] = a.w.d_kernel[k][idx];
      }
      for (int j = tid; j < w; j += 256) s_w[s.soffB[k] + j] = a.w.d_bias[k][j];
    }
  }
  const int b_begin = blockIdx.x * a.rpc, b_end = b_begin + a.rpc < B ? b_begin + a.rpc : B;
  float* part = TRAIN ? a.part + (int64_t)blockIdx.x * s.nW : nullptr;
  if (TRAIN && b_begin >= b_end) {                    // a chunk without rows adds nothing
    for (int64_t x = tid; x < s.nW; x += 256) part[x] = 0.0f;
    return;
  }
  bool first = true;
  for (int b0 = b_begin; b0 < b_end; b0 += kR) {
    const int nr = b_end - b0 < kR ? b_end - b0 : kR;
    __syncthreads();                                  // the staged stack; the round before
    if (tid < nr) {
      const int u = a.users[b0 + tid], i = a.items[b0 + tid];
      const bool ok = u >= 0 && u < U && i >= 0 && i < I;   // an instance takes part as a whole or not at all
      s_u[tid] = ok ? u : -1;
      s_i[tid] = ok ? i : -1;
    }
    __syncthreads();
    // the concat [m_u | n_i]
    for (int idx = tid; idx < nr * 2 * e; idx += 256) {
      const int r = idx / (2 * e), c = idx - r * 2 * e;
      float v = 0.0f;
      if (s_u[r] >= 0)
        v = c < e ? a.w.d_mlp_user[(int64_t)s_u[r] * e + c] : a.w.d_mlp_item[(int64_t)s_i[r] * e + (c - e)];
      s_act[r * kW + c] = v;
    }
    __syncthreads();
    for (int k = 0; k < nL; ++k) {
      const int w = s.w[k], in = s.in[k];
      const float* W = STAGED ? s_w + s.soffW[k] : a.w.d_kernel[k];
      const float* bias = STAGED ? s_w + s.soffB[k] : a.w.d_bias[k];
      const int ldw = STAGED ? s.ldw[k] : w;
      const float* x = s_act + k * kR * kW;
      float* y = s_act + (k + 1) * kR * kW;
      for (int idx = tid; idx < nr * w; idx += 256) {
        const int r = idx / w, j = idx - r * w;
        float acc = bias[j];
        for (int i = 0; i < in; ++i) acc = __builtin_fmaf(x[r * kW + i], W[i * ldw + j], acc);
        y[r * kW + j] = fmaxf(acc, 0.0f);
      }
      __syncthreads();
    }
    // y = sum(p q) + sum(h_last), the loss and g; the GMF rows' gradients
    float* top = s_act + nL * kR * kW;
    const int wL = s.w[nL - 1];
    for (int r = wave; r < nr; r += 4) {
      const int b = b0 + r, u = s_u[r], i = s_i[r];
      const bool ok = u >= 0;
      float sum = 0.0f, gm = 0.0f, sq_mf = 0.0f, sq_mlp = 0.0f;
      for (int c = lane; c < wL; c += 64) sum += top[r * kW + c];
      if (ok) {
        for (int c = lane; c < d; c += 64) {
          const float p = a.w.d_mf_user[(int64_t)u * d + c], q = a.w.d_mf_item[(int64_t)i * d + c];
          gm = __builtin_fmaf(p, q, gm);
          sq_mf += p * p + q * q;
        }
        for (int c = lane; c < 2 * e; c += 64) sq_mlp += s_act[r * kW + c] * s_act[r * kW + c];
      }
      sum = nr_wave_sum_f32(sum);
      gm = nr_wave_sum_f32(gm);
      const float yv = gm + sum;
      if (!TRAIN) {
        if (lane == 0) a.out[b] = yv;
        continue;
      }
      sq_mf = nr_wave_sum_f32(sq_mf);
      sq_mlp = nr_wave_sum_f32(sq_mlp);
      float loss = 0.0f, g = 0.0f;
      if (ok) nr::rowkey::pointwise_loss_g(a.loss_kind, B, a.labels[b], yv, loss, g);
      if (lane == 0) {
        a.TERM[b] = loss;
        a.REG[b] = ok ? 0.5f * (a.reg_mf * sq_mf + a.reg_mlp * sq_mlp) : 0.0f;
        s_g[r] = g;
        a.keys[b] = ok ? row_key(u, (uint32_t)b) : kSentinel;
        a.keys[B + b] = ok ? row_key(U + i, (uint32_t)b) : kSentinel;
        if (ok) {
          if (a.flag_mf_user) a.flag_mf_user[u] = 1;
          if (a.flag_mf_item) a.flag_mf_item[i] = 1;
          if (a.flag_mlp_user) a.flag_mlp_user[u] = 1;
          if (a.flag_mlp_item) a.flag_mlp_item[i] = 1;
        }
      }
      for (int c = lane; c < d; c += 64) {
        float gp = 0.0f, gq = 0.0f;
        if (ok) {
          const float p = a.w.d_mf_user[(int64_t)u * d + c], q = a.w.d_mf_item[(int64_t)i * d + c];
          gp = __builtin_fmaf(g, q, a.reg_mf * p);
          gq = __builtin_fmaf(g, p, a.reg_mf * q);
        }
        a.DP[(int64_t)b * d + c] = gp;
        a.DQ[(int64_t)b * d + c] = gq;
      }
    }
    if (!TRAIN) continue;
    __syncthreads();
    // dz of the last layer in place: relu passes g where the activation is > 0
    for (int idx = tid; idx < nr * wL; idx += 256) {
      const int r = idx / wL, j = idx - r * wL;
      top[r * kW + j] = top[r * kW + j] > 0.0f ? s_g[r] : 0.0f;
    }
    __syncthreads();
    for (int k = nL - 1; k >= 0; --k) {
      const int w = s.w[k], in = s.in[k];
      const float* W = STAGED ? s_w + s.soffW[k] : a.w.d_kernel[k];
      const int ldw = STAGED ? s.ldw[k] : w;
      float* x = s_act + k * kR * kW;
      const float* dz = s_act + (k + 1) * kR * kW;
      // this chunk's share of the kernel's and the bias's gradient, rows ascending
      float* pW = part + s.offW[k];
      for (int idx = tid; idx < in * w; idx += 256) {
        const int i = idx / w, j = idx - i * w;
        float acc = first ? 0.0f : pW[idx];
        for (int r = 0; r < nr; ++r) acc = __builtin_fmaf(x[r * kW + i], dz[r * kW + j], acc);
        pW[idx] = acc;
      }
      float* pB = part + s.offB[k];
      for (int j = tid; j < w; j += 256) {
        float acc = first ? 0.0f : pB[j];
        for (int r = 0; r < nr; ++r) acc += dz[r * kW + j];
        pB[j] = acc;
      }
      // the input's gradient: at most kR kW / 256 = 4 values per thread, held back until every thread has read x
      float tmp[kR * kW / 256];
#pragma unroll
      for (int q = 0; q < kR * kW / 256; ++q) {
        const int idx = tid + 256 * q;
        tmp[q] = 0.0f;
        if (idx < nr * in) {
          const int r = idx / in, i = idx - r * in;
          float acc = 0.0f;
          for (int j = 0; j < w; ++j) acc = __builtin_fmaf(dz[r * kW + j], W[i * ldw + j], acc);
          tmp[q] = acc;
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kR * kW / 256; ++q) {
        const int idx = tid + 256 * q;
        if (idx < nr * in) {
          const int r = idx / in, i = idx - r * in;
          const float v = x[r * kW + i];
          if (k > 0) {
            x[r * kW + i] = v > 0.0f ? tmp[q] : 0.0f;
          } else {                                     // the slot's m_u / n_i gradient, its L2 term included
            const float gv = __builtin_fmaf(a.reg_mlp, v, tmp[q]);
            if (i < e) a.DM[(int64_t)(b0 + r) * e + i] = gv;
            else a.DN[(int64_t)(b0 + r) * e + (i - e)] = gv;
          }
        }
      }
      __syncthreads();
    }
    first = false;
  }
}

struct ReduceArgs {
  const float* part;
  float* G_kernel[kLayers];
  float* G_bias[kLayers];
  int64_t offW[kLayers], offB[kLayers], nW;
  int nL, chunks;
};

__global__ __launch_bounds__(256) void neumf_reduce_kernel(ReduceArgs a) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= a.nW) return;
  float acc = 0.0f;
  for (int c = 0; c < a.chunks; ++c) acc += a.part[(int64_t)c * a.nW + x];
  int k = 0;
  while (k + 1 < a.nL && x >= a.offW[k + 1]) ++k;
  if (x < a.offB[k]) a.G_kernel[k][x - a.offW[k]] = acc;
  else a.G_bias[k][x - a.offB[k]] = acc;
}

struct RowsArgs {
  const uint64_t* keys;
  const float *DP, *DQ, *DM, *DN;
  float *G_mf_user, *G_mf_item, *G_mlp_user, *G_mlp_item;
  int64_t n_keys;
  int d, e, U;
};

// one wavefront per sorted key, lanes over the columns (widths <= 128: two per lane)
__global__ __launch_bounds__(256) void neumf_rows_kernel(RowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = nr::rowkey::head_row(a.keys, a.n_keys, w);
  if (row < 0) return;
  const bool user = row < a.U;
  const int r = user ? row : row - a.U, d = a.d, e = a.e;
  const float* src_mf = user ? a.DP : a.DQ;
  const float* src_mlp = user ? a.DM : a.DN;
  float acc_mf[2] = {0.0f, 0.0f}, acc_mlp[2] = {0.0f, 0.0f};
  nr::rowkey::for_run(a.keys, a.n_keys, w, row, [&](uint32_t slot) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int c = lane + 64 * m;
      if (c < d) acc_mf[m] += src_mf[(int64_t)slot * d + c];
      if (c < e) acc_mlp[m] += src_mlp[(int64_t)slot * e + c];
    }
  });
  float* dst_mf = user ? a.G_mf_user : a.G_mf_item;
  float* dst_mlp = user ? a.G_mlp_user : a.G_mlp_item;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int c = lane + 64 * m;
    if (c < d) dst_mf[(int64_t)r * d + c] = acc_mf[m];
    if (c < e) dst_mlp[(int64_t)r * e + c] = acc_mlp[m];
  }
}

__global__ __launch_bounds__(256) void neumf_loss_kernel(const float* __restrict__ term, const float* __restrict__ reg,
                                                         int B, float* __restrict__ loss2) {
  double v[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += 256) {
    v[0] += (double)term[b];
    v[1] += (double)reg[b];
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) {
    loss2[0] = (float)v[0];
    loss2[1] = (float)v[1];
  }
}

// ---------------------------------------------------------------------------------------------- all-items scoring
// out[r][j] = bias[j] + table[id_r][0..e) . W[row_off .. row_off + e)[j]; id_r = ids[r], or r when ids is null
__global__ __launch_bounds__(256) void neumf_proj_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                                         int rows, int n_table, int e, const float* __restrict__ W,
                                                         int row_off, int w0, const float* __restrict__ bias,
                                                         float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * w0) return;
  const int r = (int)(idx / w0), j = (int)(idx - (int64_t)r * w0);
  const int id = ids ? ids[r] : r;
  float acc = bias ? bias[j] : 0.0f;
  if (id >= 0 && id < n_table)
    for (int i = 0; i < e; ++i) acc = __builtin_fmaf(table[(int64_t)id * e + i], W[(int64_t)(row_off + i) * w0 + j], acc);
  out[idx] = acc;
}

struct PairShape {
  int nM;                       // MFMA layers: n_layers - 1
  int Kt[kLayers - 1], Mt[kLayers - 1];     // 32-tiles of the layer's input and output
  int woff[kLayers - 1], boff[kLayers - 1]; // offsets of the padded kernel [32 Kt][32 Mt] and bias [32 Mt] in wpad
  int wtotal;
};

PairShape pair_shape_of(const Shape& s) {
  PairShape p = {};
  p.nM = s.nL - 1;
  int o = 0;
  for (int k = 1; k < s.nL; ++k) {
    p.Kt[k - 1] = (s.w[k - 1] + 31) / 32, p.Mt[k - 1] = (s.w[k] + 31) / 32;
    p.woff[k - 1] = o, o += 32 * p.Kt[k - 1] * 32 * p.Mt[k - 1];
    p.boff[k - 1] = o, o += 32 * p.Mt[k - 1];
  }
  p.wtotal = o;
  return p;
}

struct PackArgs {
  const float* kernel[kLayers - 1];
  const float* bias[kLayers - 1];
  int in[kLayers - 1], w[kLayers - 1];
  PairShape p;
  float* wpad;
};

__global__ __launch_bounds__(256) void neumf_pack_kernel(PackArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= a.p.wtotal) return;
  int k = 0;
  while (k + 1 < a.p.nM && x >= a.p.woff[k + 1]) ++k;
  const int Mp = 32 * a.p.Mt[k];
  float v = 0.0f;
  if (x < a.p.boff[k]) {
    const int y = x - a.p.woff[k], i = y / Mp, j = y - i * Mp;
    if (i < a.in[k] && j < a.w[k]) v = a.kernel[k][(int64_t)i * a.w[k] + j];
  } else {
    const int j = x - a.p.boff[k];
    if (j < a.w[k]) v = a.bias[k][j];
  }
  a.wpad[x] = v;
}

struct PairArgs {
  const float* A;               // [n][w0]
  const float* Bm;              // [I][w0]
  const float* P;               // mf_embedding_user
  const float* Q;               // mf_embedding_item
  const int32_t* users;
  const float* wpad;
  float* out;
  int64_t ld;
  int n, I, U, d, w0, TU;
  PairShape p;
};

// this lane's 16 values of one 32-tile: value `reg` belongs to index (reg & 3) + 8 (reg >> 2) + 4 half
__device__ __forceinline__ int tile_index(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// h <- relu(W^T h + bias) for this lane's pair: W [32 Kt][32 Mt] zero-padded, so pad inputs and outputs are exact zeros
template <int MAXT>
__device__ __forceinline__ void mlp_layer(float (&h)[MAXT][16], const float* W, const float* bias, int Kt, int Mt, int nl,
                                          int half) {
  const int Mp = 32 * Mt;
  float o[MAXT][16];
#pragma unroll
  for (int mt = 0; mt < MAXT; ++mt) {
    if (mt < Mt) {
      f32x16 acc;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = bias[mt * 32 + tile_index(v, half)];
#pragma unroll
      for (int nt = 0; nt < MAXT; ++nt) {
        if (nt < Kt) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float wv = W[(nt * 32 + tile_index(v, half)) * Mp + mt * 32 + nl];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, h[nt][v], acc, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) o[mt][v] = fmaxf(acc[v], 0.0f);
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) o[mt][v] = 0.0f;
    }
  }
#pragma unroll
  for (int mt = 0; mt < MAXT; ++mt)
#pragma unroll
    for (int v = 0; v < 16; ++v) h[mt][v] = o[mt][v];
}

// grid (item tiles of 32, user tiles of TU); dynamic LDS: Bm tile [32][ldb], Q tile [32][ldq], A tile [TU][w0], P tile
// [TU][d], and with STAGE the padded layers.  MAXT: the 32-tiles of the widest layer (1, 2 or 4) — a pair's activations are
// 16 MAXT registers per lane, twice (in and out of a layer), and the narrower instances leave room for more wavefronts
template <bool STAGE, int MAXT>
__global__ __launch_bounds__(256) void neumf_pairs_kernel(PairArgs a) {
  extern __shared__ float s_dyn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, half = lane >> 5;
  const int w0 = a.w0, d = a.d, TU = a.TU, ldb = w0 | 1, ldq = d | 1;
  float* sB = s_dyn;
  float* sQ = sB + 32 * ldb;
  float* sA = sQ + 32 * ldq;
  float* sP = sA + TU * w0;
  float* sW = sP + TU * d;
  const int i0 = blockIdx.x * 32, u0 = blockIdx.y * TU;
  for (int idx = tid; idx < 32 * w0; idx += 256) {
    const int r = idx / w0, c = idx - r * w0;
    sB[r * ldb + c] = i0 + r < a.I ? a.Bm[(int64_t)(i0 + r) * w0 + c] : 0.0f;
  }
  for (int idx = tid; idx < 32 * d; idx += 256) {
    const int r = idx / d, c = idx - r * d;
    sQ[r * ldq + c] = i0 + r < a.I ? a.Q[(int64_t)(i0 + r) * d + c] : 0.0f;
  }
  for (int idx = tid; idx < TU * w0; idx += 256) {
    const int r = idx / w0;
    sA[idx] = u0 + r < a.n ? a.A[(int64_t)u0 * w0 + idx] : 0.0f;
  }
  for (int idx = tid; idx < TU * d; idx += 256) {
    const int r = idx / d, c = idx - r * d;
    float v = 0.0f;
    if (u0 + r < a.n) {
      const int u = a.users[u0 + r];
      if (u >= 0 && u < a.U) v = a.P[(int64_t)u * d + c];
    }
    sP[idx] = v;
  }
  if (STAGE)
    for (int idx = tid; idx < a.p.wtotal; idx += 256) sW[idx] = a.wpad[idx];
  __syncthreads();
  const float* W = STAGE ? sW : a.wpad;
  const int T0 = (w0 + 31) / 32;
  for (int t = wave; t < TU; t += 4) {
    if (u0 + t >= a.n) break;
    float h[MAXT][16];
#pragma unroll
    for (int nt = 0; nt < MAXT; ++nt)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int k = nt * 32 + tile_index(v, half);
        h[nt][v] = nt < T0 && k < w0 ? fmaxf(sA[t * w0 + k] + sB[nl * ldb + k], 0.0f) : 0.0f;
      }
    if (a.p.nM > 0) mlp_layer<MAXT>(h, W + a.p.woff[0], W + a.p.boff[0], a.p.Kt[0], a.p.Mt[0], nl, half);
    if (a.p.nM > 1) mlp_layer<MAXT>(h, W + a.p.woff[1], W + a.p.boff[1], a.p.Kt[1], a.p.Mt[1], nl, half);
    if (a.p.nM > 2) mlp_layer<MAXT>(h, W + a.p.woff[2], W + a.p.boff[2], a.p.Kt[2], a.p.Mt[2], nl, half);
    float sum = 0.0f;
#pragma unroll
    for (int mt = 0; mt < MAXT; ++mt)
#pragma unroll
      for (int v = 0; v < 16; ++v) sum += h[mt][v];
    float gm = 0.0f;
    for (int c = half; c < d; c += 2) gm = __builtin_fmaf(sP[t * d + c], sQ[nl * ldq + c], gm);
    sum += gm;
    sum += __shfl_xor(sum, 32, NR_WAVE);
    if (half == 0 && i0 + nl < a.I) a.out[(int64_t)(u0 + t) * a.ld + i0 + nl] = sum;
  }
}

int check_weights(const nrhip_neumf_weights& w, const char* who) {
  NR_REQUIRE(w.n_layers >= 1 && w.n_layers <= kLayers, NR_ERR_UNSUPPORTED, "%s: %d layers outside 1..%d", who,
             w.n_layers, kLayers);
  NR_REQUIRE(w.d >= 0 && w.d <= kW, NR_ERR_UNSUPPORTED, "%s: embedding_size %d outside 0..%d", who, w.d, kW);
  for (int k = 0; k < w.n_layers; ++k)
    NR_REQUIRE(w.width[k] >= 1 && w.width[k] <= kW, NR_ERR_UNSUPPORTED, "%s: layers[%d] = %d outside 1..%d", who, k,
               w.width[k], kW);
  NR_REQUIRE(w.n_users >= 0 && w.n_items >= 0 && (int64_t)w.n_users + (int64_t)w.n_items < (1ll << 31),
             NR_ERR_UNSUPPORTED, "%s: n_users + n_items = %lld does not fit the 31-bit row of a sort key", who,
             (long long)((int64_t)w.n_users + (int64_t)w.n_items));
  return NR_OK;
}

int check_pointers(const nrhip_neumf_weights& w, const char* who) {
  const int e = w.width[0] / 2;
  NR_REQUIRE(w.d == 0 || (w.d_mf_user && w.d_mf_item), NR_ERR_ARG, "%s: null mf_embedding pointer", who);
  NR_REQUIRE(e == 0 || (w.d_mlp_user && w.d_mlp_item), NR_ERR_ARG, "%s: null mlp_embedding pointer", who);
  for (int k = 0; k < w.n_layers; ++k)
    NR_REQUIRE((w.d_kernel[k] || (k == 0 && e == 0)) && w.d_bias[k], NR_ERR_ARG, "%s: null pointer (layer %d)", who, k);
  return NR_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// the pairs kernel's tile of users and whether the padded layers fit the LDS beside the tiles
void pair_tiling(const Shape& s, const PairShape& p, int* TU, int* stage, size_t* lds_bytes) {
  const int w0 = s.w[0], d = s.d;
  auto fixed = [&](int tu) { return (size_t)4 * (32 * (w0 | 1) + 32 * (d | 1) + tu * (w0 + d)); };
  int tu = 32;
  while (tu > 4 && fixed(tu) > (size_t)kPairLds * 3 / 4) tu /= 2;
  *TU = tu;
  *stage = p.wtotal > 0 && fixed(tu) + (size_t)4 * p.wtotal <= (size_t)kPairLds;
  *lds_bytes = fixed(tu) + (*stage ? (size_t)4 * p.wtotal : 0);
}

}  // namespace

extern "C" {

int nrhip_neumf_workspace_floats(const nrhip_neumf_weights* weights, int max_batch, size_t* floats) {
  NR_REQUIRE(weights && floats, NR_ERR_ARG, "neumf_workspace_floats: null argument");
  NR_TRY(check_weights(*weights, "neumf_workspace_floats"));
  NR_REQUIRE(max_batch >= 0 && max_batch <= kB, NR_ERR_UNSUPPORTED, "neumf_workspace_floats: batch %d outside 0..%d",
             max_batch, kB);
  *floats = layout_of(max_batch, shape_of(*weights)).total;
  return NR_OK;
}

int nrhip_neumf_step(const nrhip_neumf_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "neumf_step: null argument block");
  const nrhip_neumf_step_args a = *args;
  const nrhip_neumf_weights& w = a.w;
  NR_TRY(check_weights(w, "neumf_step"));
  NR_REQUIRE(a.batch >= 0 && a.batch <= kB, NR_ERR_UNSUPPORTED, "neumf_step: batch %d outside 0..%d", a.batch, kB);
  NR_TRY(nr::rowkey::check_loss_kind("neumf_step", 0, a.loss_kind));
  const int B = a.batch;
  if (B == 0) return NR_OK;
  NR_TRY(check_pointers(w, "neumf_step"));
  const Shape s = shape_of(w);
  NR_REQUIRE(s.d == 0 || (a.d_G_mf_user && a.d_G_mf_item), NR_ERR_ARG, "neumf_step: null mf gradient pointer");
  NR_REQUIRE(s.e == 0 || (a.d_G_mlp_user && a.d_G_mlp_item), NR_ERR_ARG, "neumf_step: null mlp gradient pointer");
  for (int k = 0; k < s.nL; ++k)
    NR_REQUIRE((a.d_G_kernel[k] || s.in[k] == 0) && a.d_G_bias[k], NR_ERR_ARG,
               "neumf_step: null gradient pointer (layer %d)", k);
  NR_REQUIRE(a.d_users && a.d_items && a.d_labels && a.d_keys && a.d_ws && a.d_loss2, NR_ERR_ARG,
             "neumf_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const Layout y = layout_of(B, s);
  float* ws = a.d_ws;

  RowArgs r = {};
  r.w = w, r.s = s;
  r.users = a.d_users, r.items = a.d_items, r.labels = a.d_labels, r.keys = a.d_keys;
  r.flag_mf_user = a.d_flag_mf_user, r.flag_mf_item = a.d_flag_mf_item;
  r.flag_mlp_user = a.d_flag_mlp_user, r.flag_mlp_item = a.d_flag_mlp_item;
  r.TERM = ws + y.TERM, r.REG = ws + y.REG, r.DP = ws + y.DP, r.DQ = ws + y.DQ, r.DM = ws + y.DM, r.DN = ws + y.DN;
  r.part = ws + y.part;
  r.B = B, r.rpc = y.rpc, r.loss_kind = a.loss_kind;
  r.reg_mf = a.reg_mf, r.reg_mlp = a.reg_mlp;
  if (s.staged) hipLaunchKernelGGL((neumf_row_kernel<true, true>), dim3(y.chunks), dim3(256), 0, st, r);
  else hipLaunchKernelGGL((neumf_row_kernel<true, false>), dim3(y.chunks), dim3(256), 0, st, r);
  NR_LAUNCH_CHECK();

  ReduceArgs g = {};
  g.part = r.part;
  for (int k = 0; k < s.nL; ++k) {
    g.G_kernel[k] = a.d_G_kernel[k], g.G_bias[k] = a.d_G_bias[k];
    g.offW[k] = s.offW[k], g.offB[k] = s.offB[k];
  }
  g.nW = s.nW, g.nL = s.nL, g.chunks = y.chunks;
  hipLaunchKernelGGL(neumf_reduce_kernel, dim3(blocks_of(s.nW)), dim3(256), 0, st, g);
  NR_LAUNCH_CHECK();

  const int64_t n_keys = 2 * (int64_t)B;
  NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
  RowsArgs q = {};
  q.keys = a.d_keys;
  q.DP = r.DP, q.DQ = r.DQ, q.DM = r.DM, q.DN = r.DN;
  q.G_mf_user = a.d_G_mf_user, q.G_mf_item = a.d_G_mf_item;
  q.G_mlp_user = a.d_G_mlp_user, q.G_mlp_item = a.d_G_mlp_item;
  q.n_keys = n_keys, q.d = s.d, q.e = s.e, q.U = w.n_users;
  hipLaunchKernelGGL(neumf_rows_kernel, dim3((unsigned)((n_keys + 3) / 4)), dim3(256), 0, st, q);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(neumf_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)r.TERM, (const float*)r.REG, B,
                     a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_neumf_forward(const nrhip_neumf_weights* weights, const int32_t* d_users, const int32_t* d_items, int n,
                        float* d_out, void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "neumf_forward: null argument block");
  const nrhip_neumf_weights w = *weights;
  NR_TRY(check_weights(w, "neumf_forward"));
  NR_REQUIRE(n >= 0, NR_ERR_ARG, "neumf_forward: negative count");
  if (n == 0) return NR_OK;
  NR_TRY(check_pointers(w, "neumf_forward"));
  NR_REQUIRE(d_users && d_items && d_out, NR_ERR_ARG, "neumf_forward: null pointer argument");
  RowArgs r = {};
  r.w = w, r.s = shape_of(w);
  r.users = d_users, r.items = d_items, r.out = d_out;
  r.B = n, r.rpc = kR;
  const dim3 grid((unsigned)((n + kR - 1) / kR));
  if (r.s.staged) hipLaunchKernelGGL((neumf_row_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, r);
  else hipLaunchKernelGGL((neumf_row_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, r);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_neumf_scores_workspace_floats(const nrhip_neumf_weights* weights, int n, size_t* floats) {
  NR_REQUIRE(weights && floats, NR_ERR_ARG, "neumf_scores_workspace_floats: null argument");
  NR_TRY(check_weights(*weights, "neumf_scores_workspace_floats"));
  NR_REQUIRE(n >= 0, NR_ERR_ARG, "neumf_scores_workspace_floats: negative count");
  const Shape s = shape_of(*weights);
  const PairShape p = pair_shape_of(s);
  *floats = ((size_t)n + (size_t)weights->n_items) * s.w[0] + (size_t)p.wtotal + 4;
  return NR_OK;
}

int nrhip_neumf_scores(const nrhip_neumf_weights* weights, const int32_t* d_users, int n, float* d_ws, float* d_out,
                       int64_t ld, void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "neumf_scores: null argument block");
  const nrhip_neumf_weights w = *weights;
  NR_TRY(check_weights(w, "neumf_scores"));
  NR_REQUIRE(n >= 0 && ld >= w.n_items, NR_ERR_ARG, "neumf_scores: negative count or ld < n_items");
  if (n == 0 || w.n_items == 0) return NR_OK;
  NR_TRY(check_pointers(w, "neumf_scores"));
  NR_REQUIRE(d_users && d_ws && d_out, NR_ERR_ARG, "neumf_scores: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const Shape s = shape_of(w);
  const PairShape p = pair_shape_of(s);
  const int w0 = s.w[0], I = w.n_items;
  float* A = d_ws;
  float* Bm = A + (size_t)n * w0;
  float* wpad = Bm + (size_t)I * w0;
  // the first layer, split: W1 = [W1u ; W1i], relu((m | n) W1 + b1) = relu((m W1u + b1) + n W1i)
  hipLaunchKernelGGL(neumf_proj_kernel, dim3(blocks_of((int64_t)n * w0)), dim3(256), 0, st, w.d_mlp_user, d_users, n,
                     w.n_users, s.e, w.d_kernel[0], 0, w0, w.d_bias[0], A);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(neumf_proj_kernel, dim3(blocks_of((int64_t)I * w0)), dim3(256), 0, st, w.d_mlp_item,
                     (const int32_t*)nullptr, I, I, s.e, w.d_kernel[0], s.e, w0, (const float*)nullptr, Bm);
  NR_LAUNCH_CHECK();
  if (p.wtotal > 0) {
    PackArgs k = {};
    for (int m = 0; m < p.nM; ++m) {
      k.kernel[m] = w.d_kernel[m + 1], k.bias[m] = w.d_bias[m + 1];
      k.in[m] = s.in[m + 1], k.w[m] = s.w[m + 1];
    }
    k.p = p, k.wpad = wpad;
    hipLaunchKernelGGL(neumf_pack_kernel, dim3(blocks_of(p.wtotal)), dim3(256), 0, st, k);
    NR_LAUNCH_CHECK();
  }
  int TU, stage;
  size_t lds;
  pair_tiling(s, p, &TU, &stage, &lds);
  const int64_t tiles_u = ((int64_t)n + TU - 1) / TU;
  NR_REQUIRE(tiles_u <= 65535, NR_ERR_UNSUPPORTED, "neumf_scores: %d users in one call (at most %d)", n, 65535 * TU);
  PairArgs q = {};
  q.A = A, q.Bm = Bm, q.P = w.d_mf_user, q.Q = w.d_mf_item, q.users = d_users, q.wpad = wpad;
  q.out = d_out, q.ld = ld;
  q.n = n, q.I = I, q.U = w.n_users, q.d = s.d, q.w0 = w0, q.TU = TU;
  q.p = p;
  const dim3 grid((unsigned)((I + 31) / 32), (unsigned)tiles_u);
  int widest = 0;
  for (int k = 0; k < s.nL; ++k) widest = s.w[k] > widest ? s.w[k] : widest;
#define NEUMF_PAIRS(MAXT)                                                                                \
  do {                                                                                                   \
    if (stage) hipLaunchKernelGGL((neumf_pairs_kernel<true, MAXT>), grid, dim3(256), lds, st, q);        \
    else hipLaunchKernelGGL((neumf_pairs_kernel<false, MAXT>), grid, dim3(256), lds, st, q);             \
  } while (0)
  if (widest <= 32) NEUMF_PAIRS(1);
  else if (widest <= 64) NEUMF_PAIRS(2);
  else NEUMF_PAIRS(4);
#undef NEUMF_PAIRS
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
