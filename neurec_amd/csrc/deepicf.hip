// deepicf.hip — DeepICF (Xue et al., TOIS 2019): NAIS's attention pooling, then a batch-normalised relu tower over
// (n^alpha p) (.) q, its loss, its gradients and predict() on gfx950.
//
// Replaces the graph of model/general_recommender/DeepICF.py:112-178 run on padded [B, Lmax] feeds, and the per-user
// sess.run over num_items copies of the history in predict() (DeepICF.py:231-259).  The instances, the reference's
// mask, the ragged position buffer and the walks are nais.hip's (nais_kernels.h); the backward walk runs in its VEC
// form: what reaches p is a vector per instance.
//
// The tower of a batch of B instances, in row tiles of kTB; a batch statistic is crossed at a KERNEL BOUNDARY: every
// tile leaves its partial sum, the next kernel adds the tiles' partials in tile order (every workgroup the same sum):
//   dicf_fwd_kernel(k)     [the statistics of layer k-1 -> its batch norm, relu] -> z_k = x W_k + b_k, the tile's sum z_k;
//                          workgroup 0 moves the moving statistics of layer k-1
//   dicf_var_kernel(k)     the mean of z_k from the tiles' sums, then the tile's sum (z_k - mean)^2
//   dicf_head_kernel       the last batch norm and relu, out, output = sigmoid(out + bias[i]), the instance's loss term
//                          and d loss / d logit
//   dicf_sumsq_kernel      the square sums of the regularised tables (64 workgroups each, combined in order)
//   dicf_loss_kernel       one workgroup: the batch's loss terms and the regulariser
//   dicf_bwd_a_kernel(k)   dy = dx (y > 0), the tile's sum dy and sum dy xhat (k = L-1: dx = dlogit w_out, and the
//                          tile's parts of d w_out, d b_out)
//   dicf_bwd_b_kernel(k)   the two batch sums from the tiles' parts; dz = gamma rstd (dy - mean dy - xhat mean(dy xhat));
//                          the tile's part of d W_k; dx_{k-1} = dz W_k^T (k = 0: the vectors that reach p and Q[i])
//   dicf_reduce_kernel     d W_k, d b_k, d gamma_k, d beta_k, d w_out, d b_out: the tiles' parts in tile order
//   dicf_axpy_kernel       G += reg * table (the whole-table regularisers of Q, c1, W)
// predict(): nais.hip's e(i, h) tiles, then per (user, 32 items) the pooled vector and the tower in registers:
//   dicf_pairs_mfma_kernel every layer on v_mfma_f32_32x32x2_f32 in the transposed form of neumf_pairs_kernel
//   dicf_pairs_valu_kernel one lane per pair, activations in LDS: the widths the matrix-core instance does not take
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "nais_kernels.h"

namespace {

constexpr int kL = NRHIP_DEEPICF_MAX_LAYERS, kMaxN = NRHIP_DEEPICF_MAX_WIDTH;
constexpr int kTB = 32;                                   // rows of a tile
constexpr int kLd = kMaxN + 1;                            // odd row stride of a tile in LDS
constexpr int kRegBlocks = 64;                            // workgroups per square sum
constexpr int kRegTables = 3 + kL;
constexpr float kBnEps = 0.001f, kBnMove = 0.1f, kLogEps = 1e-7f;

struct Tw {
  int L, bn, B, T, bessel;
  int n[kL + 1];                                          // n[0] = d, n[k + 1] = width of layer k
  const float *W[kL], *b[kL], *gamma[kL], *beta[kL];
  float *mm[kL], *mv[kL];
  const float *Wout, *bout;
  float *Z[kL], *psum[kL], *pvar[kL], *pdy[kL], *pdyx[kL], *pW[kL];
  float *pWout, *pbout, *DX, *DY, *lossi, *gp, *gq;
  double* regpart;                                        // [kRegTables][kRegBlocks]
  float *G_W[kL], *G_b[kL], *G_gamma[kL], *G_beta[kL], *G_Wout, *G_bout;
  float regs[3], regw[kL];
  // the pooling's side
  const float *p, *Q, *bias, *labels;
  float* scal;
  const int32_t* inst;
  float* loss2;
  int d;
};

struct Layout {
  size_t Z[kL], psum[kL], pvar[kL], pdy[kL], pdyx[kL], pW[kL], pWout, pbout, DX, DY, lossi, gp, gq, regpart, total;
  int T;
};

Layout layout_of(const nrhip_deepicf_tower& t, int d, int B) {
  Layout y = {};
  const size_t T = (size_t)((B + kTB - 1) / kTB > 0 ? (B + kTB - 1) / kTB : 1), Bs = (size_t)(B > 0 ? B : 1);
  y.T = (int)T;
  size_t o = 0;
  int n_in = d;
  for (int k = 0; k < t.n_layers; ++k) {
    const size_t n = (size_t)t.width[k];
    y.Z[k] = o, o += Bs * n;
    y.psum[k] = o, o += T * n;
    y.pvar[k] = o, o += T * n;
    y.pdy[k] = o, o += T * n;
    y.pdyx[k] = o, o += T * n;
    y.pW[k] = o, o += T * (size_t)n_in * n;
    n_in = t.width[k];
  }
  y.pWout = o, o += T * kMaxN;
  y.pbout = o, o += T;
  y.DX = o, o += Bs * kMaxN;
  y.DY = o, o += Bs * kMaxN;
  y.lossi = o, o += Bs;
  y.gp = o, o += Bs * (size_t)d;
  y.gq = o, o += Bs * (size_t)d;
  o += o & 1;                                             // doubles
  y.regpart = o, o += 2 * (size_t)kRegTables * kRegBlocks;
  y.total = o;
  return y;
}

// mean and 1 / sqrt(var + eps) of layer k from the tiles' partials, in tile order; every workgroup takes the same sums
__device__ __forceinline__ void stats_of(const Tw& t, int k, float* s_mean, float* s_rstd, bool move) {
  const int n = t.n[k + 1];
  for (int j = threadIdx.x; j < n; j += 256) {
    float s = 0.f, v = 0.f;
    for (int tile = 0; tile < t.T; ++tile) s += t.psum[k][(int64_t)tile * n + j];
    for (int tile = 0; tile < t.T; ++tile) v += t.pvar[k][(int64_t)tile * n + j];
    const float mean = s / (float)t.B, var = v / (float)t.B;
    s_mean[j] = mean;
    s_rstd[j] = 1.0f / sqrtf(var + kBnEps);
    if (move && blockIdx.x == 0) {
      const float unbiased = t.bessel ? var * ((float)t.B / (float)max(t.B - 1, 1)) : var;
      t.mm[k][j] = t.mm[k][j] - (t.mm[k][j] - mean) * kBnMove;
      t.mv[k][j] = t.mv[k][j] - (t.mv[k][j] - unbiased) * kBnMove;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float bn_of(const Tw& t, int k, int j, float z, const float* s_mean, const float* s_rstd,
                                       float* xhat) {
  if (!t.bn) return z;
  const float xh = (z - s_mean[j]) * s_rstd[j];
  if (xhat) *xhat = xh;
  return t.gamma[k][j] * xh + t.beta[k][j];
}

// the tile's input of layer k: x0 = (n^alpha p) (.) Q[i] for k = 0, else relu(batch norm(z_{k-1})) — the statistics of
// layer k-1 in s_mean / s_rstd; rows beyond the batch are zero
__device__ __forceinline__ void load_x(const Tw& t, int k, int r0, float* sx, const float* s_mean, const float* s_rstd) {
  const int n_in = t.n[k];
  for (int e = threadIdx.x; e < kTB * n_in; e += 256) {
    const int r = e / n_in, c = e - r * n_in, b = r0 + r;
    float v = 0.f;
    if (b < t.B) {
      if (k == 0) {
        if (t.inst[4 * b + 3] & F_VALID) {
          const int item = t.inst[4 * b + 1];
          v = (t.scal[(int64_t)b * kScal + S_COEFF] * t.p[(int64_t)b * t.d + c]) * t.Q[(int64_t)item * t.d + c];
        }
      } else {
        v = fmaxf(bn_of(t, k - 1, c, t.Z[k - 1][(int64_t)b * n_in + c], s_mean, s_rstd, nullptr), 0.f);
      }
    }
    sx[r * kLd + c] = v;
  }
  __syncthreads();
}

// the tile's column sums of s[r][j], rows in order -> out[tile][j]
__device__ __forceinline__ void column_sums(const float* s, int rows, int n, float* out) {
  for (int j = threadIdx.x; j < n; j += 256) {
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += s[r * kLd + j];
    out[(int64_t)blockIdx.x * n + j] = acc;
  }
}

__global__ __launch_bounds__(256) void dicf_fwd_kernel(Tw t, int k) {
  __shared__ float sx[kTB * kLd], sz[kTB * kLd];
  __shared__ float s_mean[kMaxN], s_rstd[kMaxN];
  const int r0 = blockIdx.x * kTB, rows = min(kTB, t.B - r0), n_in = t.n[k], n = t.n[k + 1];
  if (k > 0 && t.bn) stats_of(t, k - 1, s_mean, s_rstd, true);
  load_x(t, k, r0, sx, s_mean, s_rstd);
  const float* W = t.W[k];
  for (int e = threadIdx.x; e < kTB * n; e += 256) {
    const int r = e / n, j = e - r * n;
    float acc = 0.f;
    if (r < rows) {
      for (int c = 0; c < n_in; ++c) acc += sx[r * kLd + c] * W[(int64_t)c * n + j];
      acc += t.b[k][j];
      t.Z[k][(int64_t)(r0 + r) * n + j] = acc;
    }
    sz[r * kLd + j] = acc;
  }
  __syncthreads();
  if (t.bn) column_sums(sz, rows, n, t.psum[k]);
}

__global__ __launch_bounds__(256) void dicf_var_kernel(Tw t, int k) {
  __shared__ float sz[kTB * kLd];
  __shared__ float s_mean[kMaxN];
  const int r0 = blockIdx.x * kTB, rows = min(kTB, t.B - r0), n = t.n[k + 1];
  for (int j = threadIdx.x; j < n; j += 256) {
    float s = 0.f;
    for (int tile = 0; tile < t.T; ++tile) s += t.psum[k][(int64_t)tile * n + j];
    s_mean[j] = s / (float)t.B;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kTB * n; e += 256) {
    const int r = e / n, j = e - r * n;
    float c = 0.f;
    if (r < rows) {
      c = t.Z[k][(int64_t)(r0 + r) * n + j] - s_mean[j];
      c = c * c;
    }
    sz[r * kLd + j] = c;
  }
  __syncthreads();
  column_sums(sz, rows, n, t.pvar[k]);
}

__global__ __launch_bounds__(256) void dicf_head_kernel(Tw t) {
  __shared__ float sx[kTB * kLd];
  __shared__ float s_mean[kMaxN], s_rstd[kMaxN];
  const int r0 = blockIdx.x * kTB, n = t.n[t.L];
  if (t.bn) stats_of(t, t.L - 1, s_mean, s_rstd, true);
  load_x(t, t.L, r0, sx, s_mean, s_rstd);
  const int r = threadIdx.x, b = r0 + r;
  if (r >= kTB || b >= t.B) return;
  float out = 0.f;
  for (int j = 0; j < n; ++j) out += sx[r * kLd + j] * t.Wout[j];
  out += t.bout[0];
  const bool valid = t.inst[4 * b + 3] & F_VALID;
  if (!valid) {                                           // a zero row of the batch statistics: no loss term, no gradient
    t.lossi[b] = 0.f;
    t.scal[(int64_t)b * kScal + S_DOUT] = 0.f;
    return;
  }
  const float logit = out + t.bias[t.inst[4 * b + 1]];
  const float prob = 1.0f / (1.0f + expf(-logit)), y = t.labels[b], scale = 1.0f / (float)t.B;
  // tf.losses.log_loss: -y log(p + eps) - (1 - y) log(1 - p + eps), its MEAN; the derivative of THAT form
  t.lossi[b] = scale * (-y * logf(prob + kLogEps) - (1.0f - y) * logf(1.0f - prob + kLogEps));
  const float dprob = scale * (-y / (prob + kLogEps) + (1.0f - y) / (1.0f - prob + kLogEps));
  t.scal[(int64_t)b * kScal + S_DOUT] = dprob * (prob * (1.0f - prob));
}

struct SumsqArgs {
  const float* table[kRegTables];
  int64_t size[kRegTables];
  double* part;
};

__global__ __launch_bounds__(256) void dicf_sumsq_kernel(SumsqArgs a) {
  const int tab = blockIdx.y;
  double v[1] = {0.0};
  if (a.table[tab])
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.size[tab]; e += (int64_t)kRegBlocks * 256) {
      const float x = a.table[tab][e];
      v[0] += (double)(x * x);
    }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) a.part[tab * kRegBlocks + blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void dicf_loss_kernel(Tw t) {
  double v[1] = {0.0};
  for (int b = threadIdx.x; b < t.B; b += 256) v[0] += (double)t.lossi[b];
  nr::rowkey::block_sum(v);
  if (threadIdx.x != 0) return;
  double reg = 0.0;
  for (int tab = 0; tab < kRegTables; ++tab) {
    const float r = tab < 3 ? t.regs[tab] : t.regw[tab - 3];
    if (r == 0.f) continue;
    double s = 0.0;
    for (int k = 0; k < kRegBlocks; ++k) s += t.regpart[tab * kRegBlocks + k];
    reg += (double)r * (0.5 * s);
  }
  t.loss2[0] = (float)v[0];
  t.loss2[1] = (float)reg;
}

__global__ __launch_bounds__(256) void dicf_bwd_a_kernel(Tw t, int k) {
  __shared__ float s1[kTB * kLd], s2[kTB * kLd];
  __shared__ float s_mean[kMaxN], s_rstd[kMaxN];
  const int r0 = blockIdx.x * kTB, rows = min(kTB, t.B - r0), n = t.n[k + 1];
  const bool top = k == t.L - 1;
  if (t.bn) stats_of(t, k, s_mean, s_rstd, false);
  for (int e = threadIdx.x; e < kTB * n; e += 256) {
    const int r = e / n, j = e - r * n, b = r0 + r;
    float dy = 0.f, dyx = 0.f, xo = 0.f;
    if (r < rows) {
      float xh = 0.f;
      const float y = bn_of(t, k, j, t.Z[k][(int64_t)b * n + j], s_mean, s_rstd, &xh);
      const float dlogit = top ? t.scal[(int64_t)b * kScal + S_DOUT] : 0.f;
      const float dx = top ? dlogit * t.Wout[j] : t.DX[(int64_t)b * kMaxN + j];
      dy = y > 0.f ? dx : 0.f;
      dyx = dy * xh;
      xo = fmaxf(y, 0.f) * dlogit;
      t.DY[(int64_t)b * kMaxN + j] = dy;
    }
    s1[r * kLd + j] = dy;
    s2[r * kLd + j] = t.bn ? dyx : xo;
  }
  __syncthreads();
  column_sums(s1, rows, n, t.pdy[k]);
  if (t.bn) column_sums(s2, rows, n, t.pdyx[k]);
  if (!top) return;
  if (t.bn) {                                             // the tile's part of d w_out needs a pass of its own
    __syncthreads();
    for (int e = threadIdx.x; e < kTB * n; e += 256) {
      const int r = e / n, j = e - r * n, b = r0 + r;
      float xo = 0.f;
      if (r < rows)
        xo = fmaxf(bn_of(t, k, j, t.Z[k][(int64_t)b * n + j], s_mean, s_rstd, nullptr), 0.f) *
             t.scal[(int64_t)b * kScal + S_DOUT];
      s2[r * kLd + j] = xo;
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < n; j += 256) {
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += s2[r * kLd + j];
    t.pWout[(int64_t)blockIdx.x * kMaxN + j] = acc;
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += t.scal[(int64_t)(r0 + r) * kScal + S_DOUT];
    t.pbout[blockIdx.x] = acc;
  }
}

__global__ __launch_bounds__(256) void dicf_bwd_b_kernel(Tw t, int k) {
  __shared__ float sx[kTB * kLd], sdz[kTB * kLd];
  __shared__ float s_mean[2][kMaxN], s_rstd[2][kMaxN], s_c1[kMaxN], s_c2[kMaxN];
  const int r0 = blockIdx.x * kTB, rows = min(kTB, t.B - r0), n_in = t.n[k], n = t.n[k + 1];
  if (t.bn) {
    stats_of(t, k, s_mean[0], s_rstd[0], false);
    if (k > 0) stats_of(t, k - 1, s_mean[1], s_rstd[1], false);
    for (int j = threadIdx.x; j < n; j += 256) {
      float a = 0.f, c = 0.f;
      for (int tile = 0; tile < t.T; ++tile) a += t.pdy[k][(int64_t)tile * n + j];
      for (int tile = 0; tile < t.T; ++tile) c += t.pdyx[k][(int64_t)tile * n + j];
      s_c1[j] = a / (float)t.B;
      s_c2[j] = c / (float)t.B;
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < kTB * n; e += 256) {
    const int r = e / n, j = e - r * n, b = r0 + r;
    float dz = 0.f;
    if (r < rows) {
      const float dy = t.DY[(int64_t)b * kMaxN + j];
      if (t.bn) {
        const float xh = (t.Z[k][(int64_t)b * n + j] - s_mean[0][j]) * s_rstd[0][j];
        dz = (t.gamma[k][j] * s_rstd[0][j]) * ((dy - s_c1[j]) - xh * s_c2[j]);
      } else {
        dz = dy;
      }
    }
    sdz[r * kLd + j] = dz;
  }
  load_x(t, k, r0, sx, s_mean[1], s_rstd[1]);             // ends in a barrier
  float* pW = t.pW[k] + (int64_t)blockIdx.x * n_in * n;
  for (int e = threadIdx.x; e < n_in * n; e += 256) {
    const int c = e / n, j = e - c * n;
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += sx[r * kLd + c] * sdz[r * kLd + j];
    pW[e] = acc;
  }
  const float* W = t.W[k];
  for (int e = threadIdx.x; e < kTB * n_in; e += 256) {
    const int r = e / n_in, c = e - r * n_in, b = r0 + r;
    if (r >= rows) continue;
    float dx = 0.f;
    for (int j = 0; j < n; ++j) dx += sdz[r * kLd + j] * W[(int64_t)c * n + j];
    if (k > 0) {
      t.DX[(int64_t)b * kMaxN + c] = dx;
    } else {
      float gp = 0.f, gq = 0.f;
      if (t.inst[4 * b + 3] & F_VALID) {
        const float coeff = t.scal[(int64_t)b * kScal + S_COEFF];
        gp = coeff * (dx * t.Q[(int64_t)t.inst[4 * b + 1] * t.d + c]);
        gq = dx * (coeff * t.p[(int64_t)b * t.d + c]);
      }
      t.gp[(int64_t)b * t.d + c] = gp;
      t.gq[(int64_t)b * t.d + c] = gq;
    }
  }
}

__global__ __launch_bounds__(256) void dicf_reduce_kernel(Tw t, int total) {
  int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  for (int k = 0; k < t.L; ++k) {
    const int n_in = t.n[k], n = t.n[k + 1], nw = n_in * n;
    if (e < nw) {
      float acc = 0.f;
      for (int tile = 0; tile < t.T; ++tile) acc += t.pW[k][(int64_t)tile * nw + e];
      if (t.regw[k] != 0.f) acc += t.regw[k] * t.W[k][e];
      t.G_W[k][e] = acc;
      return;
    }
    e -= nw;
    if (e < n) {
      float a = 0.f, c = 0.f;
      for (int tile = 0; tile < t.T; ++tile) a += t.pdy[k][(int64_t)tile * n + e];
      if (t.bn) {
        for (int tile = 0; tile < t.T; ++tile) c += t.pdyx[k][(int64_t)tile * n + e];
        t.G_gamma[k][e] = c;
        t.G_beta[k][e] = a;
        t.G_b[k][e] = 0.f;                                // zero in exact arithmetic: rounding noise is not written
      } else {
        t.G_b[k][e] = a;
      }
      return;
    }
    e -= n;
  }
  const int n = t.n[t.L];
  float acc = 0.f;
  if (e < n) {
    for (int tile = 0; tile < t.T; ++tile) acc += t.pWout[(int64_t)tile * kMaxN + e];
    t.G_Wout[e] = acc;
  } else {
    for (int tile = 0; tile < t.T; ++tile) acc += t.pbout[tile];
    t.G_bout[0] = acc;
  }
}

__global__ __launch_bounds__(256) void dicf_axpy_kernel(float* __restrict__ G, const float* __restrict__ X, float reg,
                                                        int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) G[e] += reg * X[e];
}

template <int WP, int CPL>
__global__ __launch_bounds__(256) void dicf_backward_kernel(nrhip_nais_step_args a, int N, const float* gp,
                                                            const float* gq) {
  __shared__ NaisLds L;
  nais_backward_body<WP, CPL, true>(L, a, N, gp, gq);
}

// ------------------------------------------------------------------ predict()
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ScoreArgs {
  nrhip_nais_scores_args s;
  const float* wpad;
  int L, wtotal, stage;
  int tiles[kL + 1], woff[kL], boff[kL], ooff;            // ooff: w_out [32 tiles[L]], then b_out
};

// this lane's 16 values of one 32-tile: value `reg` belongs to index (reg & 3) + 8 (reg >> 2) + 4 half
__device__ __forceinline__ int tile_index(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// h <- relu(W^T h + bias) for this lane's pair: W [32 Kt][32 Mt] zero-padded, so pad inputs and outputs are exact zeros
template <int MAXT>
__device__ __forceinline__ void tower_layer(float (&h)[MAXT][16], const float* W, const float* bias, int Kt, int Mt,
                                            int nl, int half) {
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

constexpr int kTU = 8;                                    // users of a workgroup of the matrix-core pair kernel

// grid (32-item tiles of the e(i, h) tile, groups of kTU users); a wavefront per (user, 32 items): lane (nl, half)
// holds of item nl the features tile_index(v, half) — the pooled vector is summed in that form, which is the B operand
// of the first layer, and every layer's result is the B operand of the next
template <int MAXT>
__global__ __launch_bounds__(256) void dicf_pairs_mfma_kernel(ScoreArgs a, int i0, int ti) {
  extern __shared__ float s_w[];
  const nrhip_nais_scores_args& s = a.s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, half = lane >> 5;
  if (a.stage) {
    for (int e = tid; e < a.wtotal; e += 256) s_w[e] = a.wpad[e];
    __syncthreads();
  }
  const float* W = a.stage ? s_w : a.wpad;
  const int d = s.d, il = blockIdx.x * 32 + nl, i = i0 + il;
  const bool on = il < ti && i < s.n_items;
  const float bias = on ? s.d_bias[i] : 0.f;
  for (int t = wave; t < kTU; t += 4) {
    const int b = blockIdx.y * kTU + t;
    if (b >= s.batch) break;
    const int u = s.d_users[b];
    const bool user = u >= 0 && u < s.n_users;
    const int64_t b0 = user ? s.d_indptr[u] : 0, e0 = user ? s.d_indptr[u + 1] : 0;
    float h[MAXT][16];
#pragma unroll
    for (int nt = 0; nt < MAXT; ++nt)
#pragma unroll
      for (int v = 0; v < 16; ++v) h[nt][v] = 0.f;
    double den = 0.0;
    for (int64_t k = b0; k < e0; ++k) {
      const int hh = s.d_indices[k];
      const int idx = (hh >= 0 && hh < s.n_items) ? s.d_map[hh] : -1;
      if (idx < 0) continue;
      const float e = on ? s.d_E[(int64_t)idx * ti + il] : 0.f;
      den += (double)e;
      const float* c = s.d_c1 + (int64_t)hh * d;
#pragma unroll
      for (int nt = 0; nt < MAXT; ++nt)
        if (nt < a.tiles[0]) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int col = nt * 32 + tile_index(v, half);
            if (col < d) h[nt][v] += e * c[col];
          }
        }
    }
    const float denf = (float)den, coeff = nais_pow((float)(e0 - b0), s.alpha);
    const float SB = denf > 0.f ? nais_pow(denf, s.beta) : 1.f;
#pragma unroll
    for (int nt = 0; nt < MAXT; ++nt)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int col = nt * 32 + tile_index(v, half);
        const float q = (on && nt < a.tiles[0] && col < d) ? s.d_Q[(int64_t)i * d + col] : 0.f;
        h[nt][v] = (coeff * (denf > 0.f ? h[nt][v] / SB : 0.f)) * q;
      }
#pragma unroll 1
    for (int k = 0; k < a.L; ++k)
      tower_layer<MAXT>(h, W + a.woff[k], W + a.boff[k], a.tiles[k], a.tiles[k + 1], nl, half);
    float sum = 0.f;
#pragma unroll
    for (int mt = 0; mt < MAXT; ++mt)
      if (mt < a.tiles[a.L]) {
#pragma unroll
        for (int v = 0; v < 16; ++v) sum += h[mt][v] * W[a.ooff + mt * 32 + tile_index(v, half)];
      }
    sum += __shfl_xor(sum, 32, NR_WAVE);
    const float logit = (sum + W[a.ooff + 32 * a.tiles[a.L]]) + bias;
    if (half == 0 && on) s.d_out[(int64_t)b * s.ld + i] = 1.0f / (1.0f + expf(-logit));
  }
}

// grid (32-item tiles, users), 32 lanes: one lane per pair, the activations of the 32 pairs in LDS [feature][lane]
__global__ __launch_bounds__(32) void dicf_pairs_valu_kernel(ScoreArgs a, int i0, int ti) {
  __shared__ float sx[2][kMaxN][32];
  const nrhip_nais_scores_args& s = a.s;
  const int lane = threadIdx.x, d = s.d, il = blockIdx.x * 32 + lane, i = i0 + il, b = blockIdx.y;
  const bool on = il < ti && i < s.n_items;
  const int u = s.d_users[b];
  const bool user = u >= 0 && u < s.n_users;
  const int64_t b0 = user ? s.d_indptr[u] : 0, e0 = user ? s.d_indptr[u + 1] : 0;
  for (int c = 0; c < 32 * a.tiles[0]; ++c) sx[0][c][lane] = 0.f;
  double den = 0.0;
  for (int64_t k = b0; k < e0; ++k) {
    const int hh = s.d_indices[k];
    const int idx = (hh >= 0 && hh < s.n_items) ? s.d_map[hh] : -1;
    if (idx < 0) continue;
    const float e = on ? s.d_E[(int64_t)idx * ti + il] : 0.f;
    den += (double)e;
    const float* c1 = s.d_c1 + (int64_t)hh * d;
    for (int c = 0; c < d; ++c) sx[0][c][lane] += e * c1[c];
  }
  const float denf = (float)den, coeff = nais_pow((float)(e0 - b0), s.alpha);
  const float SB = denf > 0.f ? nais_pow(denf, s.beta) : 1.f;
  for (int c = 0; c < d; ++c)
    sx[0][c][lane] = (coeff * (denf > 0.f ? sx[0][c][lane] / SB : 0.f)) * (on ? s.d_Q[(int64_t)i * d + c] : 0.f);
  int cur = 0;
  for (int k = 0; k < a.L; ++k) {
    const int Kp = 32 * a.tiles[k], Mp = 32 * a.tiles[k + 1];
    const float* W = a.wpad + a.woff[k];
    const float* bias = a.wpad + a.boff[k];
    for (int j = 0; j < Mp; ++j) {
      float acc = bias[j];
      for (int c = 0; c < Kp; ++c) acc = fmaf(sx[cur][c][lane], W[c * Mp + j], acc);
      sx[cur ^ 1][j][lane] = fmaxf(acc, 0.f);
    }
    cur ^= 1;
  }
  float sum = 0.f;
  for (int j = 0; j < 32 * a.tiles[a.L]; ++j) sum += sx[cur][j][lane] * a.wpad[a.ooff + j];
  const float logit = (sum + a.wpad[a.ooff + 32 * a.tiles[a.L]]) + (on ? s.d_bias[i] : 0.f);
  if (on) s.d_out[(int64_t)b * s.ld + i] = 1.0f / (1.0f + expf(-logit));
}

int check_tower(const nrhip_deepicf_tower& t, int d, const char* who) {
  NR_REQUIRE(t.n_layers >= 1 && t.n_layers <= kL, NR_ERR_UNSUPPORTED, "%s: %d layers outside 1..%d", who, t.n_layers,
             kL);
  for (int k = 0; k < t.n_layers; ++k)
    NR_REQUIRE(t.width[k] >= 1 && t.width[k] <= kMaxN, NR_ERR_UNSUPPORTED, "%s: layers[%d] = %d outside 1..%d", who, k,
               t.width[k], kMaxN);
  NR_REQUIRE(d >= 1 && d <= kMaxN, NR_ERR_UNSUPPORTED, "%s: embedding_size %d outside 1..%d", who, d, kMaxN);
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_deepicf_workspace_floats(const nrhip_deepicf_tower* tower, int d, int max_batch, size_t* floats) {
  NR_REQUIRE(tower && floats, NR_ERR_ARG, "deepicf_workspace_floats: null argument");
  NR_TRY(check_tower(*tower, d, "deepicf_workspace_floats"));
  NR_REQUIRE(max_batch >= 0 && max_batch <= NRHIP_NAIS_MAX_BATCH, NR_ERR_ARG, "deepicf_workspace_floats: bad batch");
  *floats = layout_of(*tower, d, max_batch).total;
  return NR_OK;
}

int nrhip_deepicf_step(const nrhip_deepicf_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "deepicf_step: null argument block");
  const nrhip_deepicf_step_args A = *args;
  const nrhip_nais_step_args a = A.nais;
  const nrhip_deepicf_tower& tw = A.tower;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_NAIS_MAX_D, NR_ERR_UNSUPPORTED, "deepicf_step: embedding_size %d outside 1..%d",
             a.d, NRHIP_NAIS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_NAIS_MAX_W, NR_ERR_UNSUPPORTED, "deepicf_step: weight_size %d outside 1..%d", a.w,
             NRHIP_NAIS_MAX_W);
  NR_TRY(check_tower(tw, a.d, "deepicf_step"));
  NR_REQUIRE(a.beta >= 0.f && (a.algorithm == 0 || a.algorithm == 1), NR_ERR_ARG, "deepicf_step: bad beta / algorithm");
  NR_REQUIRE(!a.pairwise && !a.c1_sort && a.reg_p == 0.f && a.reg_q == 0.f, NR_ERR_ARG,
             "deepicf_step: the pooling runs pointwise, by the walk, without a regulariser of its own");
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_t_indptr && a.d_t_users && a.d_c1 && a.d_Q && a.d_bias && a.d_W &&
                 a.d_b && a.d_h && a.d_G_c1 && a.d_G_Q && a.d_G_bias && a.d_G_W && a.d_G_b && a.d_G_h && a.d_users &&
                 a.d_items && a.d_third && a.d_keys && a.d_inst && a.d_n && a.d_p && a.d_scal && a.d_slot &&
                 a.d_off && a.d_need && a.d_rows && a.d_dWp && a.d_dbp && a.d_dhp && a.d_dqp && a.d_loss2 && A.d_ws &&
                 tw.d_Wout && tw.d_bout && A.d_G_Wout && A.d_G_bout, NR_ERR_ARG, "deepicf_step: null pointer argument");
  for (int k = 0; k < tw.n_layers; ++k)
    NR_REQUIRE(tw.d_W[k] && tw.d_b[k] && A.d_G_W[k] && A.d_G_b[k] &&
                   (!tw.batch_norm || (tw.d_gamma[k] && tw.d_beta[k] && tw.d_mm[k] && tw.d_mv[k] && A.d_G_gamma[k] &&
                                       A.d_G_beta[k])), NR_ERR_ARG, "deepicf_step: null pointer (layer %d)", k);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_NAIS_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 && a.step >= 1 &&
                 a.row_cap >= 0 && a.row_cap < ((int64_t)1 << 31) &&
                 (int64_t)a.n_users + a.n_items < ((int64_t)1 << 31), NR_ERR_ARG, "deepicf_step: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const int N = a.batch, d = a.d, L = tw.n_layers;
  const Layout y = layout_of(tw, d, N);
  float* ws = A.d_ws;
  Tw t = {};
  t.L = L, t.bn = tw.batch_norm != 0, t.B = N, t.T = y.T, t.bessel = A.bessel;
  t.n[0] = d;
  for (int k = 0; k < L; ++k) {
    t.n[k + 1] = tw.width[k];
    t.W[k] = tw.d_W[k], t.b[k] = tw.d_b[k], t.gamma[k] = tw.d_gamma[k], t.beta[k] = tw.d_beta[k];
    t.mm[k] = tw.d_mm[k], t.mv[k] = tw.d_mv[k];
    t.Z[k] = ws + y.Z[k], t.psum[k] = ws + y.psum[k], t.pvar[k] = ws + y.pvar[k], t.pdy[k] = ws + y.pdy[k];
    t.pdyx[k] = ws + y.pdyx[k], t.pW[k] = ws + y.pW[k];
    t.G_W[k] = A.d_G_W[k], t.G_b[k] = A.d_G_b[k], t.G_gamma[k] = A.d_G_gamma[k], t.G_beta[k] = A.d_G_beta[k];
    t.regw[k] = A.regw[k];
  }
  t.Wout = tw.d_Wout, t.bout = tw.d_bout, t.G_Wout = A.d_G_Wout, t.G_bout = A.d_G_bout;
  t.pWout = ws + y.pWout, t.pbout = ws + y.pbout, t.DX = ws + y.DX, t.DY = ws + y.DY, t.lossi = ws + y.lossi;
  t.gp = ws + y.gp, t.gq = ws + y.gq, t.regpart = (double*)(ws + y.regpart);
  for (int k = 0; k < 3; ++k) t.regs[k] = A.regs[k];
  t.p = a.d_p, t.Q = a.d_Q, t.bias = a.d_bias, t.labels = (const float*)a.d_third;
  t.scal = a.d_scal, t.inst = a.d_inst, t.loss2 = a.d_loss2, t.d = d;
  const int attW_size = (a.algorithm == 1 ? 2 * d : d) * a.w;    // the attention's W

  // the whole-table square sums do not depend on the batch
  SumsqArgs q = {};
  q.table[0] = A.regs[0] != 0.f ? a.d_Q : nullptr, q.size[0] = (int64_t)a.n_items * d;
  q.table[1] = A.regs[1] != 0.f ? a.d_c1 : nullptr, q.size[1] = (int64_t)a.n_items * d;
  q.table[2] = A.regs[2] != 0.f ? a.d_W : nullptr, q.size[2] = attW_size;
  for (int k = 0; k < L; ++k)
    q.table[3 + k] = A.regw[k] != 0.f ? tw.d_W[k] : nullptr, q.size[3 + k] = (int64_t)t.n[k] * t.n[k + 1];
  q.part = t.regpart;
  hipLaunchKernelGGL(dicf_sumsq_kernel, dim3(kRegBlocks, kRegTables), dim3(256), 0, st, q);
  NR_LAUNCH_CHECK();
  NR_CHECK_HIP(hipMemsetAsync(a.d_G_Q, 0, sizeof(float) * (size_t)a.n_items * d, st));
  if (N > 0) {
    hipLaunchKernelGGL(prepare_kernel<nrhip_nais_step_args>, dim3((N + 255) / 256), dim3(256), 0, st, a, N);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nais_scan_kernel, dim3(1), dim3(256), 0, st, a, N);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, 2 * N, stream));
    NR_NAIS_BY_SHAPE(nais_forward_kernel, dim3((N + 3) / 4), st, a, N);
    NR_LAUNCH_CHECK();
    const dim3 tiles(y.T);
    for (int k = 0; k < L; ++k) {
      hipLaunchKernelGGL(dicf_fwd_kernel, tiles, dim3(256), 0, st, t, k);
      NR_LAUNCH_CHECK();
      if (t.bn) {
        hipLaunchKernelGGL(dicf_var_kernel, tiles, dim3(256), 0, st, t, k);
        NR_LAUNCH_CHECK();
      }
    }
    hipLaunchKernelGGL(dicf_head_kernel, tiles, dim3(256), 0, st, t);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dicf_loss_kernel, dim3(1), dim3(256), 0, st, t);
  NR_LAUNCH_CHECK();
  int total = t.n[L] + 1;
  for (int k = 0; k < L; ++k) total += t.n[k] * t.n[k + 1] + t.n[k + 1];
  if (N > 0) {
    const dim3 tiles(y.T);
    for (int k = L - 1; k >= 0; --k) {
      hipLaunchKernelGGL(dicf_bwd_a_kernel, tiles, dim3(256), 0, st, t, k);
      NR_LAUNCH_CHECK();
      hipLaunchKernelGGL(dicf_bwd_b_kernel, tiles, dim3(256), 0, st, t, k);
      NR_LAUNCH_CHECK();
    }
  } else {
    t.T = 0;                                              // no tile has written its parts: the sums are empty
  }
  hipLaunchKernelGGL(dicf_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, t, total);
  NR_LAUNCH_CHECK();
  if (N > 0) {
    NR_NAIS_BY_SHAPE(dicf_backward_kernel, dim3((N + 3) / 4), st, a, N, (const float*)t.gp, (const float*)t.gq);
    NR_LAUNCH_CHECK();
    const dim3 grid((2 * N + 3) / 4);
    NR_HIST_BY_CPL(nais_rows_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  if (a.n_items > 0) {
    const dim3 grid((a.n_items + 3) / 4);
    NR_HIST_BY_CPL(nais_walk_kernel, d, grid, st, a, N);
    NR_LAUNCH_CHECK();
  }
  const int entries = attW_size + 2 * a.w;
  hipLaunchKernelGGL(nais_reduce_kernel, dim3((entries + 255) / 256), dim3(256), 0, st, a, N);
  NR_LAUNCH_CHECK();
  const int64_t nq = (int64_t)a.n_items * d;
  if (A.regs[0] != 0.f && nq > 0) {
    hipLaunchKernelGGL(dicf_axpy_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, a.d_G_Q, a.d_Q,
                       A.regs[0], nq);
    NR_LAUNCH_CHECK();
  }
  if (A.regs[1] != 0.f && nq > 0) {
    hipLaunchKernelGGL(dicf_axpy_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, a.d_G_c1, a.d_c1,
                       A.regs[1], nq);
    NR_LAUNCH_CHECK();
  }
  if (A.regs[2] != 0.f) {
    hipLaunchKernelGGL(dicf_axpy_kernel, dim3((attW_size + 255) / 256), dim3(256), 0, st, a.d_G_W, a.d_W, A.regs[2],
                       (int64_t)attW_size);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_deepicf_scores(const nrhip_deepicf_scores_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "deepicf_scores: null argument block");
  const nrhip_deepicf_scores_args A = *args;
  const nrhip_nais_scores_args a = A.nais;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_NAIS_MAX_D, NR_ERR_UNSUPPORTED, "deepicf_scores: embedding_size %d outside 1..%d",
             a.d, NRHIP_NAIS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_NAIS_MAX_W, NR_ERR_UNSUPPORTED, "deepicf_scores: weight_size %d outside 1..%d",
             a.w, NRHIP_NAIS_MAX_W);
  NR_REQUIRE(A.n_layers >= 1 && A.n_layers <= kL, NR_ERR_UNSUPPORTED, "deepicf_scores: %d layers outside 1..%d",
             A.n_layers, kL);
  NR_REQUIRE(a.beta >= 0.f && (a.algorithm == 0 || a.algorithm == 1), NR_ERR_ARG, "deepicf_scores: bad beta / algorithm");
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_c1 && a.d_Q && a.d_bias && a.d_W && a.d_b && a.d_h && a.d_users &&
                 a.d_out && a.d_map && a.d_hs && a.d_cnt && a.d_E && a.d_F && (a.algorithm == 0 || (a.d_cW && a.d_qW)) &&
                 A.d_wpad, NR_ERR_ARG, "deepicf_scores: null pointer argument");
  NR_REQUIRE(a.batch >= 0 && a.batch <= 65535 && a.n_users >= 0 && a.n_items >= 0 && a.ld >= a.n_items &&
                 a.h_cap >= 1 && a.tile >= 256 && a.tile % 256 == 0, NR_ERR_ARG, "deepicf_scores: bad sizes");
  NR_REQUIRE(!a.mfma || (a.algorithm == 0 && a.d <= 16 && a.w <= 16), NR_ERR_UNSUPPORTED,
             "deepicf_scores: the matrix-core e(i, h) kernel takes algorithm 0 with d <= 16 and w <= 16");
  ScoreArgs s = {};
  s.s = a, s.wpad = A.d_wpad, s.L = A.n_layers;
  int o = 0, maxt = 0;
  for (int k = 0; k <= A.n_layers; ++k) {
    NR_REQUIRE(A.tiles[k] >= 1 && A.tiles[k] <= kMaxN / 32, NR_ERR_UNSUPPORTED,
               "deepicf_scores: a width of %d 32-tiles outside 1..%d", A.tiles[k], kMaxN / 32);
    s.tiles[k] = A.tiles[k];
    maxt = A.tiles[k] > maxt ? A.tiles[k] : maxt;
  }
  NR_REQUIRE(32 * A.tiles[0] >= a.d, NR_ERR_ARG, "deepicf_scores: tiles[0] does not hold embedding_size");
  for (int k = 0; k < A.n_layers; ++k) {
    s.woff[k] = o, o += 32 * A.tiles[k] * 32 * A.tiles[k + 1];
    s.boff[k] = o, o += 32 * A.tiles[k + 1];
  }
  s.ooff = o, o += 32 * A.tiles[A.n_layers] + 1;
  NR_REQUIRE(o == A.wtotal, NR_ERR_ARG, "deepicf_scores: the packed tower holds %d floats, its shape asks %d", A.wtotal,
             o);
  s.wtotal = o;
  NR_REQUIRE(!A.mfma || maxt <= 2, NR_ERR_UNSUPPORTED,
             "deepicf_scores: the matrix-core tower takes widths (and embedding_size) up to 64");
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
  NR_REQUIRE((hmax + kHC - 1) / kHC <= 65535, NR_ERR_UNSUPPORTED, "deepicf_scores: %d history items in one block", hmax);
  s.stage = (size_t)4 * s.wtotal <= 48 * 1024;
  const size_t lds = s.stage ? (size_t)4 * s.wtotal : 0;
  for (int i0 = 0; i0 < a.n_items; i0 += a.tile) {
    const int ti = a.tile;
    const dim3 grid(ti / 256, (hmax + kHC - 1) / kHC);
    if (a.mfma) hipLaunchKernelGGL(nais_pairs_mfma_kernel, grid, dim3(256), 0, st, a, i0, ti);
    else if (a.d <= 16) launch_pairs_w<16>(a, i0, ti, grid, st);
    else if (a.d <= 32) launch_pairs_w<32>(a, i0, ti, grid, st);
    else if (a.d <= 64) launch_pairs_w<64>(a, i0, ti, grid, st);
    else launch_pairs_w<128>(a, i0, ti, grid, st);
    NR_LAUNCH_CHECK();
    const int rest = a.n_items - i0 < ti ? a.n_items - i0 : ti;
    if (A.mfma) {
      const dim3 g2((rest + 31) / 32, (a.batch + kTU - 1) / kTU);
      if (maxt <= 1) hipLaunchKernelGGL((dicf_pairs_mfma_kernel<1>), g2, dim3(256), lds, st, s, i0, ti);
      else hipLaunchKernelGGL((dicf_pairs_mfma_kernel<2>), g2, dim3(256), lds, st, s, i0, ti);
    } else {
      hipLaunchKernelGGL(dicf_pairs_valu_kernel, dim3((rest + 31) / 32, a.batch), dim3(32), 0, st, s, i0, ti);
    }
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

}  // extern "C"
