// convncf.hip — the ConvNCF step (model/general_recommender/ConvNCF.py:87-145 up to the optimisers), the pairs' outputs
// and the all-items scorer, fp32.  Notation: U users, I items, d embedding_size = 2^L, L layers of c[k] channels
// (c[0] = 1), E = p_u (x) q_i [d, d]; layer k is tanh(conv2d(2x2, stride 2) + bias): position (a, b) of layer k reads the
// 2x2 patch (2a + i, 2b + j) of layer k - 1 as a row of 4 c[k-1] values (corner (i, j) major, channel minor) against the
// kernel [4 c[k-1]][c[k]]; side of layer k: d >> k.
//
// A pair is worked block by block: a block is a Bs x Bs square of E, Bs = min(d, 32), and is an independent subtree down to
// ONE position of layer Db = log2(Bs) (at most 8192 + 2048 + 512 + 128 + 32 activations, in LDS).  d = 64 has 2 x 2 blocks,
// whose four layer-5 positions feed layer 6.
//
//   convncf_forward_kernel<TRAIN>  a workgroup takes pairs in turn (at most 2^20 workgroups a launch, so any number of
//                            pairs): per block layer 1 from p and q (4 multiply-adds per output, a thread keeps its channel's
//                            kernel entries in registers, never stored), then every further layer on
//                            v_mfma_f32_16x16x4_f32 in the transposed form D[output][position] = K^T x^T, the layer's kernel
//                            staged in LDS (row stride 33), the activations at an odd position stride; the head output =
//                            a_L . W + b, one store per pair.  TRAIN: the activations of layers 2..L go to the work space
//                            (layer 1 is 128 KB per pair at the defaults and is recomputed instead)
//   convncf_backward_kernel  one workgroup per chunk of pairs, pairs ascending: g = +-dloss(out_pos - out_neg); per block
//                            layer 1 again, layers 2..Db read back, then from the top per layer the chunk's share of the
//                            kernel gradient as D[row][output] = x^T dz over the positions and of the bias gradient (each
//                            entry added by one fixed thread into the chunk's partials), and dz of the layer below IN PLACE
//                            over its activations, per patch corner D[channel][position] = K_corner dz^T, dz = da (1 - a^2),
//                            all three on the same matrix instruction; at layer 1 dE = dz1 K1^T [Bs, Bs], dp = dE q and
//                            dq = dE^T p summed over the blocks in block order.  The regs[0] terms ride with the pair's
//                            slots: p once per triplet (the positive pair), q per pair
//   convncf_reduce_kernel    the chunks' partials added in chunk order, plus the dense variables' L2 terms, and stored
//   nrhip_sort_u64           the keys, ascending: one key space of U + I rows, low word = the pair (2 triplet + side)
//   convncf_rows_kernel      one wavefront per sorted key: the head of a run adds the run's slots in key order and STORES
//                            the row's gradient (rowkey_common.h)
//   convncf_loss_kernel      one workgroup: data term and embedding regulariser, in double, rounded once
//
// Every float sum is taken in a fixed order, no atomics: two calls on the same inputs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using nr::rowkey::kSentinel;
using nr::rowkey::row_key;

constexpr int kC = NRHIP_CONVNCF_MAX_CHANNELS;
constexpr int kL = NRHIP_CONVNCF_MAX_LAYERS;
constexpr int kB = NRHIP_CONVNCF_MAX_BATCH;
constexpr int kD = 1 << kL;                          // the widest embedding
constexpr int kDb = 5;                               // the depth of the widest block of E, 32 x 32
constexpr int kChunks = 512;                         // pair chunks of the dense variables' partials
constexpr int64_t kGrid = 1 << 20;                   // workgroups of a forward launch: HIP takes fewer than 2^32 threads
constexpr int kLdK = kC + 1;                         // row stride of the staged kernel
constexpr int kActLds = (256 + 64 + 16 + 4 + 1) * (kC + 1);   // a block's activations, layers 1..5, odd position stride

struct Shape {
  int L, d, Bs, Db, nbs;                             // nbs: blocks per side
  int c[kL + 1];
  int soff[kL + 1];                                  // LDS offset of layer k within a block, k = 1..Db
  int poff[kL + 1], ld[kL + 1];                      // the forward kernel's: a position's channels at the odd stride ld
  int aoff[kL + 1], afloats;                         // work-space offset of layer k's activations of a pair, k = 2..L
  int offK[kL + 1], offB[kL + 1], offW, offb, nW;    // the dense variables laid end to end
};

Shape shape_of(const nrhip_convncf_weights& w) {
  Shape s = {};
  s.L = w.n_layers, s.d = w.d;
  s.Db = s.L < kDb ? s.L : kDb;
  s.Bs = 1 << s.Db;
  s.nbs = s.d / s.Bs;
  s.c[0] = 1;
  int so = 0, ao = 0, o = 0, po = 0;
  for (int k = 1; k <= s.L; ++k) {
    s.c[k] = w.channel[k - 1];
    s.ld[k] = s.c[k] | 1;
    if (k <= s.Db) s.soff[k] = so, so += (s.Bs >> k) * (s.Bs >> k) * s.c[k];
    if (k <= s.Db) s.poff[k] = po, po += (s.Bs >> k) * (s.Bs >> k) * s.ld[k];
    if (k >= 2) s.aoff[k] = ao, ao += (s.d >> k) * (s.d >> k) * s.c[k];
    s.offK[k] = o, o += 4 * s.c[k - 1] * s.c[k];
    s.offB[k] = o, o += s.c[k];
  }
  s.afloats = (ao + 3) / 4 * 4;
  s.offW = o, o += s.c[s.L];
  s.offb = o, o += 1;
  s.nW = o;
  return s;
}

struct Layout {
  size_t OUT, TERM, REG, DP, DQ, ACT, part, total;
  int chunks, ppc;                                   // pairs per chunk
};

Layout layout_of(int B, const Shape& s) {
  Layout y;
  const size_t n = (size_t)2 * (B > 0 ? B : 1);
  size_t o = 0;
  auto take = [&](size_t f) { const size_t at = o; o += (f + 3) / 4 * 4; return at; };
  y.OUT = take(n);
  y.TERM = take(n);
  y.REG = take(n);
  y.DP = take(n * s.d);
  y.DQ = take(n * s.d);
  y.ACT = take(n * s.afloats);
  y.chunks = (int)(n < (size_t)kChunks ? n : (size_t)kChunks);
  y.ppc = (int)((n + y.chunks - 1) / y.chunks);
  y.part = take((size_t)y.chunks * s.nW);
  y.total = o;
  return y;
}

// ---------------------------------------------------------------------------------------------- a layer in LDS
// K [rows][cout] -> s_K with row stride kLdK
__device__ __forceinline__ void stage_kernel(const float* __restrict__ K, int rows, int cout, float* s_K) {
  for (int idx = threadIdx.x; idx < rows * cout; idx += 256) {
    const int r = idx / cout, o = idx - r * cout;
    s_K[r * kLdK + o] = K[idx];
  }
}

// layer 1 of a block: y[a][b][o] = tanh(b1[o] + sum_ij K1[ij][o] p[r0 + 2a + i] q[s0 + 2b + j]), m = Bs / 2 positions a side
// (ld: the stride of a position in y)
__device__ __forceinline__ void first_forward(const float* s_p, const float* s_q, int r0, int s0, int m, int cout,
                                              const float* s_K, const float* __restrict__ bias, float* y, int ld) {
  // a thread keeps one channel: its four kernel entries and its bias in registers; m is a power of two
  const int o = threadIdx.x % cout, p0 = threadIdx.x / cout, step = 256 / cout, lm = __ffs(m) - 1;
  if (p0 >= step) return;
  const float k0 = s_K[o], k1 = s_K[kLdK + o], k2 = s_K[2 * kLdK + o], k3 = s_K[3 * kLdK + o], bo = bias[o];
  for (int pos = p0; pos < m * m; pos += step) {
    const int a = pos >> lm, b = pos & (m - 1);
    const float pa = s_p[r0 + 2 * a], pb = s_p[r0 + 2 * a + 1], qa = s_q[s0 + 2 * b], qb = s_q[s0 + 2 * b + 1];
    float acc = __builtin_fmaf(pa * qa, k0, bo);
    acc = __builtin_fmaf(pa * qb, k1, acc);
    acc = __builtin_fmaf(pb * qa, k2, acc);
    acc = __builtin_fmaf(pb * qb, k3, acc);
    y[pos * ld + o] = tanhf(acc);
  }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The layers from the second on run on v_mfma_f32_16x16x4_f32 (exact fp32): D[16 x 16] += A[16 x 4] B[4 x 16], lane l gives
// A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds D[4 (l >> 4) + v][l & 15], v = 0..3.  A workgroup's four wavefronts
// take the 16 x 16 tiles of a product in turn (tile t: wavefront t & 3); entries beyond a shape's edge are fed as zeros.

// y[a][b][o] = tanh(bias[o] + sum_{ij, c} x[2a + i][2b + j][c] K[ij cin + c][o]), m positions a side, as D[o][position] =
// K^T x^T; gy (may be null): the pair's activations of this layer in the work space, side gn, this block at (ga, gb)
// ldx, ldy: the stride of a position in x and in y (odd: the 16 positions of a tile then lie in different banks)
__device__ __forceinline__ void conv_forward(const float* x, int ldx, int m, int cin, int cout, const float* s_K,
                                             const float* __restrict__ bias, float* y, int ldy, float* __restrict__ gy,
                                             int gn, int ga, int gb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int npos = m * m, Mt = (cout + 15) >> 4, Nt = (npos + 15) >> 4;
  for (int t = wave; t < Mt * Nt; t += 4) {
    const int mt = t % Mt, nt = t / Mt;
    const int o = mt * 16 + lo, pos = nt * 16 + lo, a = pos / m, b = pos - a * m;
    const bool o_ok = o < cout, p_ok = pos < npos;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ij = 0; ij < 4; ++ij) {
      const float* xr = x + ((2 * a + (ij >> 1)) * (2 * m) + 2 * b + (ij & 1)) * ldx;
      const float* kr = s_K + ij * cin * kLdK + o;
      for (int c0 = 0; c0 < cin; c0 += 16)                // every lane takes every step: c >= cin feeds zeros
#pragma unroll
      for (int q = 0; q < 4; ++q) {                       // four steps' loads in flight
        const int c = c0 + 4 * q + hi;
        const bool c_ok = c < cin;
        const float av = (c_ok && o_ok) ? kr[c * kLdK] : 0.0f;
        const float bv = (c_ok && p_ok) ? xr[c] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
    }
    if (p_ok) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int ov = mt * 16 + 4 * hi + v;
        if (ov < cout) {
          const float val = tanhf(acc[v] + bias[ov]);
          y[pos * ldy + ov] = val;
          if (gy) gy[((int64_t)(ga + a) * gn + gb + b) * cout + ov] = val;
        }
      }
    }
  }
}

struct PairArgs {
  nrhip_convncf_weights w;
  Shape s;
  const int32_t* users;          // [n]; all_items: the block's users, pair x is (users[x / I], x % I)
  const int32_t* items;          // step: null — the pair's item is pos[t] / neg[t]
  const int32_t* pos;
  const int32_t* neg;
  float* out;
  float* act;
  int64_t ld;                    // all-items mode: the row stride of out
  int64_t n;                     // pairs
  int all_items;
};

// the ids of pair x, -1 where one lies outside its table; *at: where the pair's output goes
__device__ __forceinline__ void pair_ids(const PairArgs& a, int64_t x, int& u, int& i, int64_t& at) {
  if (a.all_items) {
    const int64_t r = x / a.w.n_items;
    u = a.users[r], i = (int)(x - r * a.w.n_items), at = r * a.ld + i;
  } else if (a.items) {
    u = a.users[x], i = a.items[x], at = x;
  } else {
    u = a.users[x >> 1], i = (x & 1) ? a.neg[x >> 1] : a.pos[x >> 1], at = x;
  }
  if (u < 0 || u >= a.w.n_users || i < 0 || i >= a.w.n_items) u = i = -1;
}

// grid: any number of workgroups up to kGrid; workgroup w takes the pairs w, w + gridDim.x, ..
template <bool TRAIN>
__global__ __launch_bounds__(256) void convncf_forward_kernel(PairArgs a) {
  __shared__ float s_act[kActLds];
  __shared__ float s_K[4 * kC * kLdK];
  __shared__ float s_K1[4 * kLdK];                    // the first layer's kernel: staged once for all the workgroup's pairs
  __shared__ float s_top[4 * kC], s_a6[kC];
  __shared__ float s_p[kD], s_q[kD];
  const int tid = threadIdx.x;
  const Shape& s = a.s;
  const int d = s.d, L = s.L;
  stage_kernel(a.w.d_kernel[0], 4, s.c[1], s_K1);
  for (int64_t x = blockIdx.x; x < a.n; x += gridDim.x) {
    int u, it;
    int64_t at;
    pair_ids(a, x, u, it, at);
    if (u < 0) {                                      // a pair outside the tables scores 0 and takes no part
      if (tid == 0) a.out[at] = 0.0f;
      continue;
    }
    __syncthreads();                                  // the pair before
    for (int c = tid; c < d; c += 256) {
      s_p[c] = a.w.d_P[(int64_t)u * d + c];
      s_q[c] = a.w.d_Q[(int64_t)it * d + c];
    }
    float* gact = TRAIN ? a.act + x * s.afloats : nullptr;
    for (int blk = 0; blk < s.nbs * s.nbs; ++blk) {
      const int bi = blk / s.nbs, bj = blk - bi * s.nbs;
      __syncthreads();
      first_forward(s_p, s_q, bi * s.Bs, bj * s.Bs, s.Bs >> 1, s.c[1], s_K1, a.w.d_bias[0], s_act + s.poff[1], s.ld[1]);
      for (int k = 2; k <= s.Db; ++k) {
        const int m = s.Bs >> k;
        __syncthreads();
        stage_kernel(a.w.d_kernel[k - 1], 4 * s.c[k - 1], s.c[k], s_K);
        __syncthreads();
        conv_forward(s_act + s.poff[k - 1], s.ld[k - 1], m, s.c[k - 1], s.c[k], s_K, a.w.d_bias[k - 1], s_act + s.poff[k],
                     s.ld[k], TRAIN ? gact + s.aoff[k] : nullptr, d >> k, bi * m, bj * m);
      }
      if (L > s.Db) {
        __syncthreads();
        for (int c = tid; c < s.c[s.Db]; c += 256) s_top[blk * s.c[s.Db] + c] = s_act[s.poff[s.Db] + c];
      }
    }
    const float* top = s_act + s.poff[s.Db];
    if (L > s.Db) {                                   // layer 6 over the four blocks' layer-5 positions
      __syncthreads();
      stage_kernel(a.w.d_kernel[L - 1], 4 * s.c[L - 1], s.c[L], s_K);
      __syncthreads();
      conv_forward(s_top, s.c[L - 1], 1, s.c[L - 1], s.c[L], s_K, a.w.d_bias[L - 1], s_a6, s.c[L],
                   TRAIN ? gact + s.aoff[L] : nullptr, 1, 0, 0);
      top = s_a6;
    }
    __syncthreads();
    if (tid == 0) {
      float acc = a.w.d_b[0];
      for (int c = 0; c < s.c[L]; ++c) acc = __builtin_fmaf(top[c], a.w.d_W[c], acc);
      a.out[at] = acc;
    }
  }
}

struct BackArgs {
  nrhip_convncf_weights w;
  Shape s;
  const int32_t* users;
  const int32_t* pos;
  const int32_t* neg;
  const float* out;              // [2 B]
  const float* act;
  uint64_t* keys;                // [4 B]: the pairs' user rows, then their item rows
  uint8_t *flag_P, *flag_Q;
  float *TERM, *REG, *DP, *DQ, *part;
  int B, ppc, loss_kind;
  float reg_embed;
};

// dK[r][o] += sum_pos x[pos's patch][r] dz[pos][o] as D[r][o] = x^T dz over the positions, and dbias[o] += sum_pos
// dz[pos][o]: every entry is added by one fixed thread of the workgroup
__device__ __forceinline__ void conv_weight_grad(const float* x, const float* dz, int m, int cin, int cout, float* pK,
                                                 float* pB) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int npos = m * m, rows = 4 * cin, Mt = (rows + 15) >> 4, Nt = (cout + 15) >> 4;
  for (int t = wave; t < Mt * Nt; t += 4) {
    const int mt = t / Nt, nt = t - mt * Nt;
    const int r = mt * 16 + lo, o = nt * 16 + lo, ij = r / cin, c = r - ij * cin;
    const bool r_ok = r < rows, o_ok = o < cout;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int pos0 = 0; pos0 < npos; pos0 += 16)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pos = pos0 + 4 * q + hi;
      const bool p_ok = pos < npos;
      const int a = pos / m, b = pos - a * m;
      const float av = (p_ok && r_ok) ? x[((2 * a + (ij >> 1)) * (2 * m) + 2 * b + (ij & 1)) * cin + c] : 0.0f;
      const float bv = (p_ok && o_ok) ? dz[pos * cout + o] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    if (o_ok) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int rv = mt * 16 + 4 * hi + v;
        if (rv < rows) pK[rv * cout + o] += acc[v];
      }
    }
  }
  for (int o = threadIdx.x; o < cout; o += 256) {
    float acc = 0.0f;
    for (int pos = 0; pos < npos; ++pos) acc += dz[pos * cout + o];
    pB[o] += acc;
  }
}

// x <- dz of the layer below, in place: (sum_o dz[parent][o] K[ij cin + c][o]) (1 - x^2), per corner ij as D[c][parent] =
// K_ij dz^T; m: the side of dz's layer.  An entry of x is read and written by one lane alone
__device__ __forceinline__ void conv_input_grad(float* x, const float* dz, int m, int cin, int cout, const float* s_K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int npos = m * m, Mt = (cin + 15) >> 4, Nt = (npos + 15) >> 4;
  for (int t = wave; t < 4 * Mt * Nt; t += 4) {
    const int ij = t & 3, mt = (t >> 2) % Mt, nt = (t >> 2) / Mt;
    const int c = mt * 16 + lo, pos = nt * 16 + lo, a = pos / m, b = pos - a * m;
    const bool c_ok = c < cin, p_ok = pos < npos;
    const float* kr = s_K + (ij * cin + c) * kLdK;
    const float* dr = dz + pos * cout;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int o0 = 0; o0 < cout; o0 += 16)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = o0 + 4 * q + hi;
      const bool o_ok = o < cout;
      const float av = (o_ok && c_ok) ? kr[o] : 0.0f;
      const float bv = (o_ok && p_ok) ? dr[o] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    if (p_ok) {
      float* xr = x + ((2 * a + (ij >> 1)) * (2 * m) + 2 * b + (ij & 1)) * cin;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int cv = mt * 16 + 4 * hi + v;
        if (cv < cin) {
          const float xv = xr[cv];
          xr[cv] = acc[v] * (1.0f - xv * xv);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void convncf_backward_kernel(BackArgs a) {
  __shared__ float s_act[kActLds];
  __shared__ float s_K[4 * kC * kLdK];
  __shared__ float s_top[4 * kC], s_a6[kC];
  __shared__ float s_p[kD], s_q[kD], s_dp[kD], s_dq[kD];
  float* s_dE = s_K + 4 * kLdK;                      // [Bs][Bs] behind the four rows of the first kernel
  const int tid = threadIdx.x;
  const Shape& s = a.s;
  const int d = s.d, L = s.L, U = a.w.n_users, I = a.w.n_items, n_pairs = 2 * a.B;
  float* part = a.part + (int64_t)blockIdx.x * s.nW;
  // the partials are zeroed here and added to by other threads: the barrier at the head of the pair loop lies between
  for (int x = tid; x < s.nW; x += 256) part[x] = 0.0f;
  const int p_begin = blockIdx.x * a.ppc, p_end = p_begin + a.ppc < n_pairs ? p_begin + a.ppc : n_pairs;
  for (int pr = p_begin; pr < p_end; ++pr) {
    const int t = pr >> 1, side = pr & 1;
    const int u = a.users[t], ip = a.pos[t], in = a.neg[t], it = side ? in : ip;
    const bool ok = u >= 0 && u < U && ip >= 0 && ip < I && in >= 0 && in < I;   // a triplet takes part whole or not
    __syncthreads();                                   // the pair before
    if (!ok) {
      for (int c = tid; c < d; c += 256) a.DP[(int64_t)pr * d + c] = 0.0f, a.DQ[(int64_t)pr * d + c] = 0.0f;
      if (tid == 0) {
        a.TERM[pr] = 0.0f, a.REG[pr] = 0.0f;
        a.keys[pr] = kSentinel, a.keys[n_pairs + pr] = kSentinel;
      }
      continue;
    }
    const float y = a.out[2 * t] - a.out[2 * t + 1];
    const float g = (side ? -1.0f : 1.0f) * nr::pairwise_dloss(a.loss_kind, y);
    for (int c = tid; c < d; c += 256) {
      s_p[c] = a.w.d_P[(int64_t)u * d + c];
      s_q[c] = a.w.d_Q[(int64_t)it * d + c];
      s_dp[c] = 0.0f, s_dq[c] = 0.0f;
    }
    const float* gact = a.act + (int64_t)pr * s.afloats;
    const int cL = s.c[L];
    if (L > s.Db) {                                    // the head and layer 6; s_top <- dz5 of the four blocks
      const int c5 = s.c[L - 1];
      for (int idx = tid; idx < 4 * c5; idx += 256) s_top[idx] = gact[s.aoff[L - 1] + idx];
      for (int o = tid; o < cL; o += 256) s_a6[o] = gact[s.aoff[L] + o];
      stage_kernel(a.w.d_kernel[L - 1], 4 * c5, cL, s_K);
      __syncthreads();
      if (tid < cL) {
        const float v = s_a6[tid];
        part[s.offW + tid] += v * g;
        s_a6[tid] = g * a.w.d_W[tid] * (1.0f - v * v);
      }
      if (tid == 0) part[s.offb] += g;
      __syncthreads();
      conv_weight_grad(s_top, s_a6, 1, c5, cL, part + s.offK[L], part + s.offB[L]);
      __syncthreads();
      conv_input_grad(s_top, s_a6, 1, c5, cL, s_K);
    }
    for (int blk = 0; blk < s.nbs * s.nbs; ++blk) {
      const int bi = blk / s.nbs, bj = blk - bi * s.nbs, r0 = bi * s.Bs, s0 = bj * s.Bs;
      __syncthreads();
      stage_kernel(a.w.d_kernel[0], 4, s.c[1], s_K);
      for (int k = 2; k <= s.Db; ++k) {
        const int m = s.Bs >> k, gn = d >> k, ck = s.c[k];
        float* dst = s_act + s.soff[k];
        for (int idx = tid; idx < m * m * ck; idx += 256) {
          const int pos = idx / ck, o = idx - pos * ck, aa = pos / m, bb = pos - aa * m;
          dst[idx] = gact[s.aoff[k] + ((int64_t)(bi * m + aa) * gn + bj * m + bb) * ck + o];
        }
      }
      __syncthreads();
      first_forward(s_p, s_q, r0, s0, s.Bs >> 1, s.c[1], s_K, a.w.d_bias[0], s_act + s.soff[1], s.c[1]);
      __syncthreads();
      // the block's top position becomes dz
      float* top = s_act + s.soff[s.Db];
      if (L > s.Db) {
        for (int c = tid; c < s.c[s.Db]; c += 256) top[c] = s_top[blk * s.c[s.Db] + c];
      } else {
        if (tid < cL) {
          const float v = top[tid];
          part[s.offW + tid] += v * g;
          top[tid] = g * a.w.d_W[tid] * (1.0f - v * v);
        }
        if (tid == 0) part[s.offb] += g;
      }
      for (int k = s.Db; k >= 2; --k) {
        const int m = s.Bs >> k;
        __syncthreads();
        stage_kernel(a.w.d_kernel[k - 1], 4 * s.c[k - 1], s.c[k], s_K);
        conv_weight_grad(s_act + s.soff[k - 1], s_act + s.soff[k], m, s.c[k - 1], s.c[k], part + s.offK[k],
                         part + s.offB[k]);
        __syncthreads();
        conv_input_grad(s_act + s.soff[k - 1], s_act + s.soff[k], m, s.c[k - 1], s.c[k], s_K);
      }
      // layer 1: E's patches are products of p and q
      {
        const int m = s.Bs >> 1, c1 = s.c[1], Bs = s.Bs;
        const float* dz = s_act + s.soff[1];
        __syncthreads();
        stage_kernel(a.w.d_kernel[0], 4, c1, s_K);
        for (int idx = tid; idx < 4 * c1; idx += 256) {
          const int ij = idx / c1, o = idx - ij * c1;
          float acc = 0.0f;
          for (int aa = 0; aa < m; ++aa) {
            const float pv = s_p[r0 + 2 * aa + (ij >> 1)];
            for (int bb = 0; bb < m; ++bb)
              acc = __builtin_fmaf(pv * s_q[s0 + 2 * bb + (ij & 1)], dz[(aa * m + bb) * c1 + o], acc);
          }
          part[s.offK[1] + idx] += acc;
        }
        for (int o = tid; o < c1; o += 256) {
          float acc = 0.0f;
          for (int pos = 0; pos < m * m; ++pos) acc += dz[pos * c1 + o];
          part[s.offB[1] + o] += acc;
        }
        __syncthreads();
        for (int idx = tid; idx < Bs * Bs; idx += 256) {   // dE[r][c] = sum_o dz1[r / 2][c / 2][o] K1[corner][o]
          const int r = idx / Bs, cc = idx - r * Bs;
          const float* dr = dz + ((r >> 1) * m + (cc >> 1)) * c1;
          const float* kr = s_K + ((r & 1) * 2 + (cc & 1)) * kLdK;
          float acc = 0.0f;
          for (int o = 0; o < c1; ++o) acc = __builtin_fmaf(dr[o], kr[o], acc);
          s_dE[idx] = acc;
        }
        __syncthreads();
        if (tid < Bs) {                                    // dp[r0 + r] += sum_c dE[r][c] q[s0 + c]
          float acc = 0.0f;
          for (int cc = 0; cc < Bs; ++cc) acc = __builtin_fmaf(s_dE[tid * Bs + cc], s_q[s0 + cc], acc);
          s_dp[r0 + tid] += acc;
        } else if (tid >= 64 && tid < 64 + Bs) {           // dq[s0 + c] += sum_r dE[r][c] p[r0 + r]
          const int cc = tid - 64;
          float acc = 0.0f;
          for (int r = 0; r < Bs; ++r) acc = __builtin_fmaf(s_dE[r * Bs + cc], s_p[r0 + r], acc);
          s_dq[s0 + cc] += acc;
        }
      }
    }
    __syncthreads();
    // the pair's slots, the regs[0] terms with them: p1 only (the positive pair), q1 and q2
    float sq = 0.0f;
    if (tid < 64) {
      float gp = 0.0f, gq = 0.0f;
      if (tid < d) {
        const float pv = s_p[tid], qv = s_q[tid];
        gp = side ? s_dp[tid] : __builtin_fmaf(a.reg_embed, pv, s_dp[tid]);
        gq = __builtin_fmaf(a.reg_embed, qv, s_dq[tid]);
        sq = qv * qv + (side ? 0.0f : pv * pv);
        a.DP[(int64_t)pr * d + tid] = gp;
        a.DQ[(int64_t)pr * d + tid] = gq;
      }
      sq = nr_wave_sum_f32(sq);
    }
    if (tid == 0) {
      a.TERM[pr] = side ? 0.0f : nr::pairwise_loss(a.loss_kind, y);
      a.REG[pr] = 0.5f * a.reg_embed * sq;
      a.keys[pr] = row_key(u, (uint32_t)pr);
      a.keys[n_pairs + pr] = row_key(U + it, (uint32_t)pr);
      if (a.flag_P) a.flag_P[u] = 1;
      if (a.flag_Q) a.flag_Q[it] = 1;
    }
  }
}

struct ReduceArgs {
  const float* part;
  const float* V_kernel[kL];
  const float* V_bias[kL];
  const float *V_W, *V_b;
  float* G_kernel[kL];
  float* G_bias[kL];
  float *G_W, *G_b;
  Shape s;
  int chunks;
  float reg_head, reg_net;
};

__global__ __launch_bounds__(256) void convncf_reduce_kernel(ReduceArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const Shape& s = a.s;
  if (x >= s.nW) return;
  float acc = 0.0f;
  for (int c = 0; c < a.chunks; ++c) acc += a.part[(int64_t)c * s.nW + x];
  // regs[1] l2(W, b) + regs[2] (sum_k l2(K_k, bias_k) + l2(W, b))
  if (x >= s.offW) {
    const float* V = x == s.offb ? a.V_b : a.V_W + (x - s.offW);
    float* G = x == s.offb ? a.G_b : a.G_W + (x - s.offW);
    G[0] = acc + a.reg_head * V[0] + a.reg_net * V[0];
    return;
  }
  int k = 1;
  while (k < s.L && x >= s.offK[k + 1]) ++k;
  if (x < s.offB[k]) a.G_kernel[k - 1][x - s.offK[k]] = acc + a.reg_net * a.V_kernel[k - 1][x - s.offK[k]];
  else a.G_bias[k - 1][x - s.offB[k]] = acc + a.reg_net * a.V_bias[k - 1][x - s.offB[k]];
}

struct RowsArgs {
  const uint64_t* keys;
  const float *DP, *DQ;
  float *G_P, *G_Q;
  int64_t n_keys;
  int d, U;
};

// one wavefront per sorted key, a lane per column (d <= 64)
__global__ __launch_bounds__(256) void convncf_rows_kernel(RowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = nr::rowkey::head_row(a.keys, a.n_keys, w);
  if (row < 0) return;
  const bool user = row < a.U;
  const int r = user ? row : row - a.U, d = a.d;
  const float* src = user ? a.DP : a.DQ;
  float acc = 0.0f;
  nr::rowkey::for_run(a.keys, a.n_keys, w, row, [&](uint32_t slot) {
    if (lane < d) acc += src[(int64_t)slot * d + lane];
  });
  float* dst = user ? a.G_P : a.G_Q;
  if (lane < d) dst[(int64_t)r * d + lane] = acc;
}

__global__ __launch_bounds__(256) void convncf_loss_kernel(const float* __restrict__ term, const float* __restrict__ reg,
                                                           int n, float* __restrict__ loss2) {
  double v[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < n; b += 256) {
    v[0] += (double)term[b];
    v[1] += (double)reg[b];
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) {
    loss2[0] = (float)v[0];
    loss2[1] = (float)v[1];
  }
}

int check_weights(const nrhip_convncf_weights& w, const char* who) {
  NR_REQUIRE(w.n_layers >= 1 && w.n_layers <= kL, NR_ERR_UNSUPPORTED, "%s: net_channel has %d layers, outside 1..%d", who,
             w.n_layers, kL);
  NR_REQUIRE(w.d == (1 << w.n_layers), NR_ERR_UNSUPPORTED,
             "%s: embedding_size %d is not 2^len(net_channel) = %d", who, w.d, 1 << w.n_layers);
  for (int k = 0; k < w.n_layers; ++k)
    NR_REQUIRE(w.channel[k] >= 1 && w.channel[k] <= kC, NR_ERR_UNSUPPORTED, "%s: net_channel[%d] = %d outside 1..%d", who,
               k, w.channel[k], kC);
  NR_REQUIRE(w.n_users >= 0 && w.n_items >= 0 && (int64_t)w.n_users + (int64_t)w.n_items < (1ll << 31),
             NR_ERR_UNSUPPORTED, "%s: n_users + n_items = %lld does not fit the 31-bit row of a sort key", who,
             (long long)((int64_t)w.n_users + (int64_t)w.n_items));
  return NR_OK;
}

int check_pointers(const nrhip_convncf_weights& w, const char* who) {
  NR_REQUIRE(w.d_P && w.d_Q && w.d_W && w.d_b, NR_ERR_ARG, "%s: null variable pointer", who);
  for (int k = 0; k < w.n_layers; ++k)
    NR_REQUIRE(w.d_kernel[k] && w.d_bias[k], NR_ERR_ARG, "%s: null pointer (layer %d)", who, k + 1);
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_convncf_workspace_floats(const nrhip_convncf_weights* weights, int max_batch, size_t* floats) {
  NR_REQUIRE(weights && floats, NR_ERR_ARG, "convncf_workspace_floats: null argument");
  NR_TRY(check_weights(*weights, "convncf_workspace_floats"));
  NR_REQUIRE(max_batch >= 0 && max_batch <= kB, NR_ERR_UNSUPPORTED, "convncf_workspace_floats: batch %d outside 0..%d",
             max_batch, kB);
  *floats = layout_of(max_batch, shape_of(*weights)).total;
  return NR_OK;
}

int nrhip_convncf_step(const nrhip_convncf_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "convncf_step: null argument block");
  const nrhip_convncf_step_args a = *args;
  const nrhip_convncf_weights& w = a.w;
  NR_TRY(check_weights(w, "convncf_step"));
  NR_REQUIRE(a.batch >= 0 && a.batch <= kB, NR_ERR_UNSUPPORTED, "convncf_step: batch %d outside 0..%d", a.batch, kB);
  NR_TRY(nr::rowkey::check_loss_kind("convncf_step", 1, a.loss_kind));
  const int B = a.batch;
  if (B == 0) return NR_OK;
  NR_TRY(check_pointers(w, "convncf_step"));
  NR_REQUIRE(a.d_G_P && a.d_G_Q && a.d_G_W && a.d_G_b, NR_ERR_ARG, "convncf_step: null gradient pointer");
  for (int k = 0; k < w.n_layers; ++k)
    NR_REQUIRE(a.d_G_kernel[k] && a.d_G_bias[k], NR_ERR_ARG, "convncf_step: null gradient pointer (layer %d)", k + 1);
  NR_REQUIRE(a.d_users && a.d_pos && a.d_neg && a.d_keys && a.d_ws && a.d_loss2, NR_ERR_ARG,
             "convncf_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const Shape s = shape_of(w);
  const Layout y = layout_of(B, s);
  float* ws = a.d_ws;
  const int n_pairs = 2 * B;

  PairArgs f = {};
  f.w = w, f.s = s;
  f.users = a.d_users, f.pos = a.d_pos, f.neg = a.d_neg;
  f.out = ws + y.OUT, f.act = ws + y.ACT, f.n = n_pairs;
  hipLaunchKernelGGL((convncf_forward_kernel<true>), dim3(n_pairs), dim3(256), 0, st, f);
  NR_LAUNCH_CHECK();

  BackArgs r = {};
  r.w = w, r.s = s;
  r.users = a.d_users, r.pos = a.d_pos, r.neg = a.d_neg;
  r.out = ws + y.OUT, r.act = ws + y.ACT, r.keys = a.d_keys;
  r.flag_P = a.d_flag_P, r.flag_Q = a.d_flag_Q;
  r.TERM = ws + y.TERM, r.REG = ws + y.REG, r.DP = ws + y.DP, r.DQ = ws + y.DQ, r.part = ws + y.part;
  r.B = B, r.ppc = y.ppc, r.loss_kind = a.loss_kind, r.reg_embed = a.reg_embed;
  hipLaunchKernelGGL(convncf_backward_kernel, dim3(y.chunks), dim3(256), 0, st, r);
  NR_LAUNCH_CHECK();

  ReduceArgs g = {};
  g.part = r.part;
  for (int k = 0; k < s.L; ++k) {
    g.V_kernel[k] = w.d_kernel[k], g.V_bias[k] = w.d_bias[k];
    g.G_kernel[k] = a.d_G_kernel[k], g.G_bias[k] = a.d_G_bias[k];
  }
  g.V_W = w.d_W, g.V_b = w.d_b, g.G_W = a.d_G_W, g.G_b = a.d_G_b;
  g.s = s, g.chunks = y.chunks, g.reg_head = a.reg_head, g.reg_net = a.reg_net;
  hipLaunchKernelGGL(convncf_reduce_kernel, dim3((unsigned)((s.nW + 255) / 256)), dim3(256), 0, st, g);
  NR_LAUNCH_CHECK();

  const int64_t n_keys = 2 * (int64_t)n_pairs;
  NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
  RowsArgs q = {};
  q.keys = a.d_keys, q.DP = r.DP, q.DQ = r.DQ, q.G_P = a.d_G_P, q.G_Q = a.d_G_Q;
  q.n_keys = n_keys, q.d = s.d, q.U = w.n_users;
  hipLaunchKernelGGL(convncf_rows_kernel, dim3((unsigned)((n_keys + 3) / 4)), dim3(256), 0, st, q);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(convncf_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)r.TERM, (const float*)r.REG, n_pairs,
                     a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_convncf_pairs(const nrhip_convncf_weights* weights, const int32_t* d_users, const int32_t* d_items, int n,
                        float* d_out, void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "convncf_pairs: null argument block");
  const nrhip_convncf_weights w = *weights;
  NR_TRY(check_weights(w, "convncf_pairs"));
  NR_REQUIRE(n >= 0, NR_ERR_ARG, "convncf_pairs: negative count");
  if (n == 0) return NR_OK;
  NR_TRY(check_pointers(w, "convncf_pairs"));
  NR_REQUIRE(d_users && d_items && d_out, NR_ERR_ARG, "convncf_pairs: null pointer argument");
  PairArgs f = {};
  f.w = w, f.s = shape_of(w);
  f.users = d_users, f.items = d_items, f.out = d_out, f.n = n;
  hipLaunchKernelGGL((convncf_forward_kernel<false>), dim3((unsigned)(n < kGrid ? n : kGrid)), dim3(256), 0,
                     (hipStream_t)stream, f);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_convncf_scores(const nrhip_convncf_weights* weights, const int32_t* d_users, int n, float* d_out, int64_t ld,
                         void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "convncf_scores: null argument block");
  const nrhip_convncf_weights w = *weights;
  NR_TRY(check_weights(w, "convncf_scores"));
  NR_REQUIRE(n >= 0 && ld >= w.n_items, NR_ERR_ARG, "convncf_scores: negative count or ld < n_items");
  if (n == 0 || w.n_items == 0) return NR_OK;
  NR_TRY(check_pointers(w, "convncf_scores"));
  NR_REQUIRE(d_users && d_out, NR_ERR_ARG, "convncf_scores: null pointer argument");
  const int64_t pairs = (int64_t)n * w.n_items;
  PairArgs f = {};
  f.w = w, f.s = shape_of(w);
  f.users = d_users, f.out = d_out, f.ld = ld, f.n = pairs, f.all_items = 1;
  hipLaunchKernelGGL((convncf_forward_kernel<false>), dim3((unsigned)(pairs < kGrid ? pairs : kGrid)), dim3(256), 0,
                     (hipStream_t)stream, f);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
