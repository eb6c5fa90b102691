// caser.hip — the Caser step (model/sequential_recommender/Caser.py:70-118 up to the optimiser) and its evaluation-mode
// forward pass, fp32.  Notation: I items, d factors_num, L seq_L, T seq_T, N neg_samples, F = nv d + nh L.
//
//   caser_row_kernel<TRAIN>  one workgroup per batch row, the row's L x d window in LDS from end to end:
//                            vertical conv (feature j nv + c: the reshape of (b, 1, d, nv) is column-major in the
//                            embedding dimension), the L horizontal convs (ReLU, then the max over the L - i + 1 'valid'
//                            positions with the FIRST maximum's position saved), dropout over the F features, the dense
//                            layer, p = concat(z, user row); evaluation stops here.  Training goes on with the T + N
//                            logits, the loss terms as the reference writes them (sigmoid, + 1e-24, log; TF's y (1 - y)),
//                            and the row's whole backward pass: dp, dz, the features' gradient, the window's gradient,
//                            and the sort keys of the row's slots
//   caser_wgrad_kernel       the conv and dense variables: one thread per element and chunk of batch rows, rows ascending
//                            (the vertical conv's from the rows' shares, which the row kernel sums over d)
//   caser_reduce_kernel      ... the chunks added in chunk order and stored
//   nrhip_sort_u64           the keys, ascending: one key space of U + 2 I rows (user, sequence item, target item)
//   caser_rows_kernel        one wavefront per sorted key: the head of a run adds the run's slots in key order and STORES
//                            the row's gradient (rowkey_common.h); the item bias rides with the target rows
//   caser_l2_kernel          l2_reg != 0 only: G += l2_reg v over the four tables, and sum v^2 per workgroup
//   caser_loss_kernel        one workgroup: the two means and the regulariser, in double, rounded once
//
// First argmax for reduce_max.  TF splits the gradient evenly between tied positions.  Positions tie exactly only when
// their windows hold identical inputs (all-pad windows, whose value is relu(bias); a repeated item under height 1) or
// when ReLU clamps several to 0, where the gradient is 0 anyway.  For identical windows the kernel, bias and row
// gradients are sums of (share) x (the same window), so any split of the shares adds up to the same sums: the first
// position taking all of it is the even split.  tests/test_caser_cpu.py asserts it on both kinds of tie.
//
// One ascending fmaf chain per output, no atomics: two calls on the same inputs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using nr::rowkey::kSentinel;
using nr::rowkey::row_key;

constexpr int kD = NRHIP_CASER_MAX_WIDTH;
constexpr int kLen = NRHIP_CASER_MAX_LEN;
constexpr int kNV = NRHIP_CASER_MAX_NV;
constexpr int kNH = NRHIP_CASER_MAX_NH;
constexpr int kTN = NRHIP_CASER_MAX_TARGETS;
constexpr int kB = NRHIP_CASER_MAX_BATCH;
constexpr int kF = kNV * kD + kNH * kLen;            // 2688 features at most
constexpr int kPos = kLen * (kLen + 1) / 2;          // 55 (height, position) pairs at most
constexpr int kChunks = 32;                          // row chunks of the variable-gradient partials
constexpr int kL2Blocks = 2048;                      // workgroups of the regulariser sweep, one partial sum each
static_assert(kF <= kPos * kNH, "the features' gradient reuses the conv outputs' LDS");

struct Layout {
  size_t l2part, E, X, DF, ARG, P, DZ, DU, DE, GT, TERM, KV, part, total;
  int chunks, rpc;
  int64_t nW, off_fcb, off_kv, off_bv, off_kh, off_bh;
};

Layout layout_of(int B, int L, int d, int nv, int nh, int T, int N) {
  Layout y;
  const size_t b = (size_t)(B > 0 ? B : 1), F = (size_t)nv * d + (size_t)nh * L;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 3) / 4 * 4; return at; };
  y.l2part = take(2 * kL2Blocks);                    // doubles
  y.E = take(b * L * d);
  y.X = take(b * F);
  y.DF = take(b * F);
  y.ARG = take(b * L * nh);
  y.P = take(b * 2 * d);
  y.DZ = take(b * d);
  y.DU = take(b * d);
  y.DE = take(b * L * d);
  y.GT = take(b * (T + N));
  y.TERM = take(b * (T + N));
  y.KV = take(b * ((size_t)L * nv + nv));
  y.off_fcb = (int64_t)F * d;
  y.off_kv = y.off_fcb + d;
  y.off_bv = y.off_kv + (int64_t)L * nv;
  y.off_kh = y.off_bv + nv;
  y.off_bh = y.off_kh + (int64_t)d * nh * L * (L + 1) / 2;
  y.nW = y.off_bh + (int64_t)L * nh;
  y.chunks = (int)((b + 7) / 8 < (size_t)kChunks ? (b + 7) / 8 : (size_t)kChunks);
  y.rpc = (int)((b + y.chunks - 1) / y.chunks);
  y.part = take((size_t)y.chunks * y.nW);
  y.total = o;
  return y;
}

struct RowArgs {
  nrhip_caser_weights w;
  const int32_t* users;
  const int32_t* seq;
  const int32_t* pos;
  const int32_t* neg;
  const uint8_t* mask;
  uint64_t* keys;
  float *E, *X, *DF, *ARG, *P, *DZ, *DU, *DE, *GT, *TERM, *KV;
  float* out;
  int64_t ld;
  uint64_t seed;
  int step, B, T, N, drop_on;
  float keep, inv_keep;
};

// splitmix64 over (seed, step, element): a uniform in [0, 1) from the top 24 bits
__device__ __forceinline__ float drop_uniform(uint64_t seed, int step, int64_t idx) {
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * ((uint64_t)(uint32_t)step + 1u);
  z ^= (uint64_t)idx * 0xd1342543de82ef95ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}
// mask / (1 - rate) of feature idx = b F + f
__device__ __forceinline__ float drop_factor(const RowArgs& a, int64_t idx) {
  if (!a.drop_on) return 1.0f;
  const bool kept = a.mask ? a.mask[idx] != 0 : drop_uniform(a.seed, a.step, idx) < a.keep;
  return kept ? a.inv_keep : 0.0f;
}

// positions of the heights below i: sum_{h < i} (L - h + 1)
__device__ __forceinline__ int pos_base(int L, int i) { return (i - 1) * (L + 1) - (i - 1) * i / 2; }

template <bool TRAIN>
__global__ __launch_bounds__(256) void caser_row_kernel(RowArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = a.w.L, d = a.w.d, nv = a.w.nv, nh = a.w.nh, I = a.w.n_items, U = a.w.n_users;
  const int nvd = nv * d, F = nvd + nh * L, B = a.B, TN = a.T + a.N;
  __shared__ float s_E[kLen * kD];
  __shared__ float s_x[kF];
  __shared__ float s_h[kPos * kNH];
  __shared__ int s_arg[kLen * kNH];
  __shared__ float s_part[256];
  __shared__ float s_p[2 * kD];
  __shared__ float s_dz[kD];
  __shared__ float s_g[2 * kTN];
  __shared__ int s_id[2 * kTN];

  // the window: row t of the table, zeros for the pad id (any id outside [0, I))
  for (int e = tid; e < L * d; e += 256) {
    const int t = e / d, j = e - t * d;
    const int id = a.seq[(int64_t)b * L + t];
    const bool real = id >= 0 && id < I;
    const float v = real ? a.w.d_seq_item[(int64_t)id * d + j] : 0.0f;
    s_E[e] = v;
    if (TRAIN) {
      a.E[(int64_t)b * L * d + e] = v;
      if (j == 0) a.keys[B + (int64_t)b * L + t] = real ? row_key(U + id, (uint32_t)(B + b * L + t)) : kSentinel;
    }
  }
  __syncthreads();
  // vertical conv, no activation: feature j nv + c
  for (int f = tid; f < nvd; f += 256) {
    const int j = f / nv, c = f - j * nv;
    float acc = a.w.d_conv_v_bias[c];
    for (int t = 0; t < L; ++t) acc = __builtin_fmaf(s_E[t * d + j], a.w.d_conv_v[t * nv + c], acc);
    s_x[f] = acc;
  }
  // horizontal convs: every (height, position, filter), ReLU'd
  const int nq = L * (L + 1) / 2 * nh;
  for (int q = tid; q < nq; q += 256) {
    const int pp = q / nh, c = q - pp * nh;
    int i = 1, p = pp;
    while (p >= L - i + 1) {
      p -= L - i + 1;
      ++i;
    }
    const float* K = a.w.d_conv_h[i - 1];
    float acc = a.w.d_conv_h_bias[i - 1][c];
    for (int t = 0; t < i; ++t) {
      const float* e = s_E + (p + t) * d;
      const float* k = K + (int64_t)t * d * nh + c;
      for (int j = 0; j < d; ++j) acc = __builtin_fmaf(e[j], k[(int64_t)j * nh], acc);
    }
    s_h[q] = fmaxf(acc, 0.0f);
  }
  __syncthreads();
  // max over the positions, the first maximum's position saved
  for (int q = tid; q < L * nh; q += 256) {
    const int i = q / nh + 1, c = q - (i - 1) * nh;
    const float* h = s_h + pos_base(L, i) * nh + c;
    float best = h[0];
    int arg = 0;
    for (int p = 1; p <= L - i; ++p) {
      const float v = h[p * nh];
      if (v > best) {
        best = v;
        arg = p;
      }
    }
    s_x[nvd + q] = best;
    s_arg[q] = arg;
    if (TRAIN) a.ARG[(int64_t)b * L * nh + q] = (float)arg;
  }
  __syncthreads();
  // dropout over the F features
  if (TRAIN) {
    for (int f = tid; f < F; f += 256) {
      const float x = s_x[f] * drop_factor(a, (int64_t)b * F + f);
      s_x[f] = x;
      a.X[(int64_t)b * F + f] = x;
    }
    __syncthreads();
  }
  // dense layer: `parts` slices of the features per output, added in slice order
  {
    const int parts = 256 / d, per = (F + parts - 1) / parts;
    if (tid < parts * d) {
      const int part = tid / d, k = tid - part * d;
      const int f1 = (part + 1) * per < F ? (part + 1) * per : F;
      float acc = 0.0f;
      for (int f = part * per; f < f1; ++f) acc = __builtin_fmaf(s_x[f], a.w.d_fc[(int64_t)f * d + k], acc);
      s_part[tid] = acc;
    }
    __syncthreads();
    const int u = a.users[b];
    const bool real_u = u >= 0 && u < U;
    if (tid < d) {
      float acc = a.w.d_fc_bias[tid];
      for (int part = 0; part < parts; ++part) acc += s_part[part * d + tid];
      s_p[tid] = fmaxf(acc, 0.0f);
      s_p[d + tid] = real_u ? a.w.d_user[(int64_t)u * d + tid] : 0.0f;
    }
    if (TRAIN && tid == 0) a.keys[b] = real_u ? row_key(u, (uint32_t)b) : kSentinel;
  }
  __syncthreads();
  if (!TRAIN) {
    for (int c = tid; c < 2 * d; c += 256) a.out[(int64_t)b * a.ld + c] = s_p[c];
    return;
  }
  // logits, loss terms and their derivatives: one wavefront per target, the T positives first.  A pad target (an id
  // outside [0, I)) has logit 0 and no gradient, and stays in the mean
  for (int k = wave; k < TN; k += 4) {
    const bool positive = k < a.T;
    const int id = positive ? a.pos[(int64_t)b * a.T + k] : a.neg[(int64_t)b * a.N + (k - a.T)];
    const bool real = id >= 0 && id < I;
    float dot = 0.0f;
    if (real) {
      const float* q = a.w.d_item + (int64_t)id * 2 * d;
      for (int c = lane; c < 2 * d; c += 64) dot = __builtin_fmaf(s_p[c], q[c], dot);
    }
    dot = nr_wave_sum_f32(dot);
    if (lane == 0) {
      const float x = real ? dot + a.w.d_item_bias[id] : 0.0f;
      const float y = 1.0f / (1.0f + expf(-x));
      const float dy = y * (1.0f - y);                                   // TF's SigmoidGrad
      float term, g;
      if (positive) {
        const float arg = y + 1e-24f;
        term = -logf(arg);
        g = -(dy / arg) / (float)((int64_t)B * a.T);
      } else {
        const float arg = (1.0f - y) + 1e-24f;
        term = -logf(arg);
        g = (dy / arg) / (float)((int64_t)B * a.N);
      }
      if (!real) g = 0.0f;
      s_g[k] = g;
      s_id[k] = real ? id : -1;
      a.GT[(int64_t)b * TN + k] = g;
      a.TERM[(int64_t)b * TN + k] = term;
      a.keys[B + (int64_t)B * L + (int64_t)b * TN + k] =
          real ? row_key(U + I + id, (uint32_t)(B + B * L + b * TN + k)) : kSentinel;
    }
  }
  __syncthreads();
  // dp = sum_k g_k Q[tar_k]; its upper half is the user row's gradient, its lower half gated by z > 0 is dz
  for (int c = tid; c < 2 * d; c += 256) {
    float acc = 0.0f;
    for (int k = 0; k < TN; ++k)
      if (s_id[k] >= 0) acc = __builtin_fmaf(s_g[k], a.w.d_item[(int64_t)s_id[k] * 2 * d + c], acc);
    a.P[(int64_t)b * 2 * d + c] = s_p[c];
    if (c >= d) {
      a.DU[(int64_t)b * d + (c - d)] = acc;
    } else {
      const float dz = s_p[c] > 0.0f ? acc : 0.0f;
      s_dz[c] = dz;
      a.DZ[(int64_t)b * d + c] = dz;
    }
  }
  __syncthreads();
  // the features' gradient, through dropout; a pooled feature passes it on only where ReLU did (x > 0)
  for (int f = tid; f < F; f += 256) {
    const float* wrow = a.w.d_fc + (int64_t)f * d;
    float acc = 0.0f;
    for (int k = 0; k < d; ++k) acc = __builtin_fmaf(s_dz[k], wrow[k], acc);
    acc *= drop_factor(a, (int64_t)b * F + f);
    if (f >= nvd && !(s_x[f] > 0.0f)) acc = 0.0f;
    s_h[f] = acc;
    a.DF[(int64_t)b * F + f] = acc;
  }
  __syncthreads();
  // this row's share of the vertical kernel's and bias's gradients (L nv + nv <= 176 sums over the d columns)
  if (tid < L * nv + nv) {
    float acc = 0.0f;
    if (tid < L * nv) {
      const int t = tid / nv, c = tid - t * nv;
      for (int j = 0; j < d; ++j) acc = __builtin_fmaf(s_E[t * d + j], s_h[j * nv + c], acc);
    } else {
      const int c = tid - L * nv;
      for (int j = 0; j < d; ++j) acc += s_h[j * nv + c];
    }
    a.KV[(int64_t)b * (L * nv + nv) + tid] = acc;
  }
  // the window's gradient: the vertical filters, then per height and filter the window of the saved position
  for (int e = tid; e < L * d; e += 256) {
    const int t = e / d, j = e - t * d;
    float acc = 0.0f;
    for (int c = 0; c < nv; ++c) acc = __builtin_fmaf(s_h[j * nv + c], a.w.d_conv_v[t * nv + c], acc);
    for (int i = 1; i <= L; ++i) {
      const float* K = a.w.d_conv_h[i - 1];
      for (int c = 0; c < nh; ++c) {
        const float g = s_h[nvd + (i - 1) * nh + c];
        const int rel = t - s_arg[(i - 1) * nh + c];
        if (g != 0.0f && rel >= 0 && rel < i) acc = __builtin_fmaf(g, K[((int64_t)rel * d + j) * nh + c], acc);
      }
    }
    a.DE[(int64_t)b * L * d + e] = acc;
  }
}

struct WArgs {
  const float *E, *X, *DF, *ARG, *DZ, *KV;
  float* part;
  float* G_fc;
  float* G_fc_bias;
  float* G_conv_v;
  float* G_conv_v_bias;
  float* G_conv_h[kLen];
  float* G_conv_h_bias[kLen];
  int64_t nW, off_fcb, off_kv, off_bv, off_kh, off_bh;
  int B, L, d, nv, nh, chunks, rpc;
};

// grid (elements / 256, chunks): element e of the variables laid end to end (fc kernel, fc bias, conv_v kernel and bias,
// the conv_h kernels by height, their biases by height), over the rows of chunk blockIdx.y in row order
__global__ __launch_bounds__(256) void caser_wgrad_kernel(WArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.nW) return;
  const int chunk = blockIdx.y, L = a.L, d = a.d, nv = a.nv, nh = a.nh;
  const int nvd = nv * d, F = nvd + nh * L;
  const int b0 = chunk * a.rpc, b1 = b0 + a.rpc < a.B ? b0 + a.rpc : a.B;
  float acc = 0.0f;
  if (e < a.off_fcb) {
    const int f = (int)(e / d), k = (int)(e - (int64_t)f * d);
    for (int b = b0; b < b1; ++b) acc = __builtin_fmaf(a.X[(int64_t)b * F + f], a.DZ[(int64_t)b * d + k], acc);
  } else if (e < a.off_kv) {
    const int k = (int)(e - a.off_fcb);
    for (int b = b0; b < b1; ++b) acc += a.DZ[(int64_t)b * d + k];
  } else if (e < a.off_bv) {
    const int r = (int)(e - a.off_kv);                       // the rows' shares, summed over d in the row kernel
    for (int b = b0; b < b1; ++b) acc += a.KV[(int64_t)b * (L * nv + nv) + r];
  } else if (e < a.off_kh) {
    const int r = L * nv + (int)(e - a.off_bv);
    for (int b = b0; b < b1; ++b) acc += a.KV[(int64_t)b * (L * nv + nv) + r];
  } else if (e < a.off_bh) {
    int64_t r = e - a.off_kh;
    int i = 1;
    while (r >= (int64_t)i * d * nh) {
      r -= (int64_t)i * d * nh;
      ++i;
    }
    const int t = (int)(r / ((int64_t)d * nh)), j = (int)(r / nh) % d, c = (int)(r % nh);
    const int q = (i - 1) * nh + c;
    for (int b = b0; b < b1; ++b) {
      const float g = a.DF[(int64_t)b * F + nvd + q];
      if (g != 0.0f) {
        const int p = (int)a.ARG[(int64_t)b * L * nh + q];
        acc = __builtin_fmaf(g, a.E[((int64_t)b * L + p + t) * d + j], acc);
      }
    }
  } else {
    const int q = (int)(e - a.off_bh);
    for (int b = b0; b < b1; ++b) acc += a.DF[(int64_t)b * F + nvd + q];
  }
  a.part[(int64_t)chunk * a.nW + e] = acc;
}

__global__ __launch_bounds__(256) void caser_reduce_kernel(WArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.nW) return;
  float acc = 0.0f;
  for (int c = 0; c < a.chunks; ++c) acc += a.part[(int64_t)c * a.nW + e];
  if (e < a.off_fcb) {
    a.G_fc[e] = acc;
  } else if (e < a.off_kv) {
    a.G_fc_bias[e - a.off_fcb] = acc;
  } else if (e < a.off_bv) {
    a.G_conv_v[e - a.off_kv] = acc;
  } else if (e < a.off_kh) {
    a.G_conv_v_bias[e - a.off_bv] = acc;
  } else if (e < a.off_bh) {
    int64_t r = e - a.off_kh;
    int i = 1;
    while (r >= (int64_t)i * a.d * a.nh) {
      r -= (int64_t)i * a.d * a.nh;
      ++i;
    }
    a.G_conv_h[i - 1][r] = acc;
  } else {
    const int q = (int)(e - a.off_bh);
    a.G_conv_h_bias[q / a.nh][q % a.nh] = acc;
  }
}

struct RowsArgs {
  const uint64_t* keys;
  const float *DU, *DE, *P, *GT;
  float *G_user, *G_seq_item, *G_item, *G_item_bias;
  int64_t n_keys;
  int B, L, d, TN, U, I;
};

// one wavefront per sorted key, lanes over the columns (2 d <= 256: four per lane)
__global__ __launch_bounds__(256) void caser_rows_kernel(RowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = nr::rowkey::head_row(a.keys, a.n_keys, w);
  if (row < 0) return;
  const int d = a.d, table = row < a.U ? 0 : row < a.U + a.I ? 1 : 2;
  const int width = table == 2 ? 2 * d : d;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float ab = 0.0f;
  nr::rowkey::for_run(a.keys, a.n_keys, w, row, [&](uint32_t slot) {
    if (table == 2) {
      const int s = (int)slot - a.B - a.B * a.L;
      const float g = a.GT[s];
      const float* p = a.P + (int64_t)(s / a.TN) * 2 * d;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (lane + 64 * m < width) acc[m] = __builtin_fmaf(g, p[lane + 64 * m], acc[m]);
      ab += g;
    } else {
      const float* src = table == 0 ? a.DU + (int64_t)slot * d : a.DE + (int64_t)((int)slot - a.B) * d;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (lane + 64 * m < width) acc[m] += src[lane + 64 * m];
    }
  });
  float* dst = table == 0 ? a.G_user + (int64_t)row * d
               : table == 1 ? a.G_seq_item + (int64_t)(row - a.U) * d
                            : a.G_item + (int64_t)(row - a.U - a.I) * 2 * d;
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (lane + 64 * m < width) dst[lane + 64 * m] = acc[m];
  if (table == 2 && lane == 0) a.G_item_bias[row - a.U - a.I] = ab;
}

struct L2Args {
  const float* W[4];
  float* G[4];
  int64_t end[4];                 // running ends of the four tables laid end to end
  double* part;
  float l2;
};

__global__ __launch_bounds__(256) void caser_l2_kernel(L2Args a) {
  double v[1] = {0.0};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.end[3]; e += (int64_t)gridDim.x * 256) {
    const int k = e < a.end[0] ? 0 : e < a.end[1] ? 1 : e < a.end[2] ? 2 : 3;
    const int64_t at = e - (k ? a.end[k - 1] : 0);
    const float x = a.W[k][at];
    a.G[k][at] = __builtin_fmaf(a.l2, x, a.G[k][at]);
    v[0] += (double)x * (double)x;
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) a.part[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void caser_loss_kernel(const float* __restrict__ term, int B, int T, int N,
                                                         const double* __restrict__ l2part, float l2,
                                                         float* __restrict__ loss2) {
  double v[3] = {0.0, 0.0, 0.0};
  const int TN = T + N;
  for (int64_t e = threadIdx.x; e < (int64_t)B * TN; e += 256) v[(int)(e % TN) < T ? 0 : 1] += (double)term[e];
  if (l2 != 0.0f)
    for (int i = threadIdx.x; i < kL2Blocks; i += 256) v[2] += l2part[i];
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) {
    loss2[0] = (float)(v[0] / ((double)B * T) + v[1] / ((double)B * N));
    loss2[1] = l2 != 0.0f ? (float)(0.5 * (double)l2 * v[2]) : 0.0f;
  }
}

// rows wider than nrhip_gru4rec_scores takes (2 d > 128): one thread per score, items along the lanes, one ascending
// fmaf chain
__global__ __launch_bounds__(256) void caser_scores_kernel(const float* __restrict__ H, int64_t ldh,
                                                           const float* __restrict__ Q, int n, int n_items, int width,
                                                           float* __restrict__ out, int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n_items) return;
  const int r = (int)(e / n_items), i = (int)(e - (int64_t)r * n_items);
  const float* h = H + (int64_t)r * ldh;
  const float* q = Q + (int64_t)i * width;
  float acc = 0.0f;
  for (int c = 0; c < width; ++c) acc = __builtin_fmaf(h[c], q[c], acc);
  out[(int64_t)r * ld + i] = acc;
}

int check_shape(const char* who, int B, int L, int d, int nv, int nh, int T, int N) {
  NR_REQUIRE(d >= 1 && d <= kD, NR_ERR_UNSUPPORTED, "%s: factors_num %d outside 1..%d", who, d, kD);
  NR_REQUIRE(L >= 1 && L <= kLen, NR_ERR_UNSUPPORTED, "%s: seq_L %d outside 1..%d", who, L, kLen);
  NR_REQUIRE(nv >= 1 && nv <= kNV, NR_ERR_UNSUPPORTED, "%s: nv %d outside 1..%d", who, nv, kNV);
  NR_REQUIRE(nh >= 1 && nh <= kNH, NR_ERR_UNSUPPORTED, "%s: nh %d outside 1..%d", who, nh, kNH);
  NR_REQUIRE(T >= 1 && T <= kTN, NR_ERR_UNSUPPORTED, "%s: seq_T %d outside 1..%d", who, T, kTN);
  NR_REQUIRE(N >= 1 && N <= kTN, NR_ERR_UNSUPPORTED, "%s: neg_samples %d outside 1..%d", who, N, kTN);
  NR_REQUIRE(B >= 0 && B <= kB, NR_ERR_UNSUPPORTED, "%s: batch %d outside 0..%d", who, B, kB);
  return NR_OK;
}

int check_weights(const nrhip_caser_weights& w, const char* who) {
  NR_REQUIRE(w.d_user && w.d_seq_item && w.d_item && w.d_item_bias && w.d_conv_v && w.d_conv_v_bias && w.d_fc &&
                 w.d_fc_bias, NR_ERR_ARG, "%s: null weight pointer", who);
  for (int i = 0; i < w.L; ++i)
    NR_REQUIRE(w.d_conv_h[i] && w.d_conv_h_bias[i], NR_ERR_ARG, "%s: null weight pointer (conv_h of height %d)", who,
               i + 1);
  NR_REQUIRE(w.n_users >= 0 && w.n_items >= 0 && (int64_t)w.n_users + 2 * (int64_t)w.n_items < (1ll << 31),
             NR_ERR_UNSUPPORTED, "%s: n_users + 2 n_items = %lld does not fit the 31-bit row of a sort key", who,
             (long long)((int64_t)w.n_users + 2 * (int64_t)w.n_items));
  return NR_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int nrhip_caser_workspace_floats(int max_batch, int seq_L, int factors_num, int nv, int nh, int seq_T, int neg_samples,
                                 size_t* floats) {
  NR_REQUIRE(floats, NR_ERR_ARG, "caser_workspace_floats: null argument");
  NR_TRY(check_shape("caser_workspace_floats", max_batch, seq_L, factors_num, nv, nh, seq_T, neg_samples));
  *floats = layout_of(max_batch, seq_L, factors_num, nv, nh, seq_T, neg_samples).total;
  return NR_OK;
}

int nrhip_caser_step(const nrhip_caser_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "caser_step: null argument block");
  const nrhip_caser_step_args a = *args;
  const nrhip_caser_weights& w = a.w;
  NR_TRY(check_shape("caser_step", a.batch, w.L, w.d, w.nv, w.nh, a.T, a.N));
  NR_TRY(check_weights(w, "caser_step"));
  NR_REQUIRE(a.rate >= 0.0f && a.rate < 1.0f, NR_ERR_ARG, "caser_step: dropout rate %g outside [0, 1)", (double)a.rate);
  const int B = a.batch, L = w.L, d = w.d, nv = w.nv, nh = w.nh, TN = a.T + a.N;
  if (B == 0) return NR_OK;
  NR_REQUIRE(a.d_G_user && a.d_G_seq_item && a.d_G_item && a.d_G_item_bias && a.d_G_conv_v && a.d_G_conv_v_bias &&
                 a.d_G_fc && a.d_G_fc_bias && a.d_users && a.d_seq && a.d_pos && a.d_neg && a.d_keys && a.d_ws &&
                 a.d_loss2, NR_ERR_ARG, "caser_step: null pointer argument");
  for (int i = 0; i < L; ++i)
    NR_REQUIRE(a.d_G_conv_h[i] && a.d_G_conv_h_bias[i], NR_ERR_ARG,
               "caser_step: null gradient pointer (conv_h of height %d)", i + 1);
  hipStream_t st = (hipStream_t)stream;
  const Layout y = layout_of(B, L, d, nv, nh, a.T, a.N);
  float* ws = a.d_ws;
  const dim3 blk(256);

  RowArgs r = {};
  r.w = w;
  r.users = a.d_users, r.seq = a.d_seq, r.pos = a.d_pos, r.neg = a.d_neg;
  r.mask = a.d_mask;
  r.keys = a.d_keys;
  r.E = ws + y.E, r.X = ws + y.X, r.DF = ws + y.DF, r.ARG = ws + y.ARG, r.P = ws + y.P, r.DZ = ws + y.DZ;
  r.DU = ws + y.DU, r.DE = ws + y.DE, r.GT = ws + y.GT, r.TERM = ws + y.TERM, r.KV = ws + y.KV;
  r.seed = a.seed, r.step = a.step, r.B = B, r.T = a.T, r.N = a.N;
  r.drop_on = a.rate > 0.0f ? 1 : 0;
  r.keep = 1.0f - a.rate;
  r.inv_keep = 1.0f / r.keep;
  hipLaunchKernelGGL(caser_row_kernel<true>, dim3(B), blk, 0, st, r);
  NR_LAUNCH_CHECK();

  WArgs g = {};
  g.E = r.E, g.X = r.X, g.DF = r.DF, g.ARG = r.ARG, g.DZ = r.DZ, g.KV = r.KV;
  g.part = ws + y.part;
  g.G_fc = a.d_G_fc, g.G_fc_bias = a.d_G_fc_bias, g.G_conv_v = a.d_G_conv_v, g.G_conv_v_bias = a.d_G_conv_v_bias;
  for (int i = 0; i < L; ++i) g.G_conv_h[i] = a.d_G_conv_h[i], g.G_conv_h_bias[i] = a.d_G_conv_h_bias[i];
  g.nW = y.nW, g.off_fcb = y.off_fcb, g.off_kv = y.off_kv, g.off_bv = y.off_bv, g.off_kh = y.off_kh, g.off_bh = y.off_bh;
  g.B = B, g.L = L, g.d = d, g.nv = nv, g.nh = nh, g.chunks = y.chunks, g.rpc = y.rpc;
  hipLaunchKernelGGL(caser_wgrad_kernel, dim3(blocks_of(y.nW), y.chunks), blk, 0, st, g);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(caser_reduce_kernel, dim3(blocks_of(y.nW)), blk, 0, st, g);
  NR_LAUNCH_CHECK();

  const int64_t n_keys = (int64_t)B * (1 + L + TN);
  NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
  RowsArgs q = {};
  q.keys = a.d_keys;
  q.DU = r.DU, q.DE = r.DE, q.P = r.P, q.GT = r.GT;
  q.G_user = a.d_G_user, q.G_seq_item = a.d_G_seq_item, q.G_item = a.d_G_item, q.G_item_bias = a.d_G_item_bias;
  q.n_keys = n_keys;
  q.B = B, q.L = L, q.d = d, q.TN = TN, q.U = w.n_users, q.I = w.n_items;
  hipLaunchKernelGGL(caser_rows_kernel, dim3((unsigned)((n_keys + 3) / 4)), blk, 0, st, q);
  NR_LAUNCH_CHECK();

  double* l2part = (double*)(ws + y.l2part);
  if (a.l2_reg != 0.0f) {
    L2Args l = {};
    l.W[0] = w.d_user, l.W[1] = w.d_seq_item, l.W[2] = w.d_item, l.W[3] = w.d_item_bias;
    l.G[0] = a.d_G_user, l.G[1] = a.d_G_seq_item, l.G[2] = a.d_G_item, l.G[3] = a.d_G_item_bias;
    l.end[0] = (int64_t)w.n_users * d;
    l.end[1] = l.end[0] + (int64_t)w.n_items * d;
    l.end[2] = l.end[1] + (int64_t)w.n_items * 2 * d;
    l.end[3] = l.end[2] + w.n_items;
    l.part = l2part;
    l.l2 = a.l2_reg;
    hipLaunchKernelGGL(caser_l2_kernel, dim3(kL2Blocks), blk, 0, st, l);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(caser_loss_kernel, dim3(1), blk, 0, st, (const float*)r.TERM, B, a.T, a.N, (const double*)l2part,
                     a.l2_reg, a.d_loss2);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_caser_forward(const nrhip_caser_weights* weights, const int32_t* d_users, const int32_t* d_seq, int n,
                        float* d_ws, float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "caser_forward: null argument block");
  const nrhip_caser_weights w = *weights;
  NR_TRY(check_shape("caser_forward", n, w.L, w.d, w.nv, w.nh, 1, 1));
  NR_TRY(check_weights(w, "caser_forward"));
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_users && d_seq && d_out && ld >= 2 * w.d, NR_ERR_ARG,
             "caser_forward: null pointer argument or ld < 2 factors_num");
  (void)d_ws;                                        // the evaluation pass keeps the whole row in LDS
  RowArgs r = {};
  r.w = w;
  r.users = d_users, r.seq = d_seq;
  r.out = d_out, r.ld = ld;
  r.B = n;
  r.keep = r.inv_keep = 1.0f;
  hipLaunchKernelGGL(caser_row_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, r);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_caser_scores(const float* d_H, int64_t ldh, const float* d_Q, int n, int n_items, int width, float* d_out,
                       int64_t ld, void* stream) {
  NR_REQUIRE(width >= 1 && width <= 2 * kD, NR_ERR_UNSUPPORTED, "caser_scores: width %d outside 1..%d", width, 2 * kD);
  NR_REQUIRE(n >= 0 && n_items >= 0 && ldh >= width && ld >= n_items, NR_ERR_ARG, "caser_scores: bad sizes");
  if (n == 0 || n_items == 0) return NR_OK;
  NR_REQUIRE(d_H && d_Q && d_out, NR_ERR_ARG, "caser_scores: null pointer argument");
  hipLaunchKernelGGL(caser_scores_kernel, dim3(blocks_of((int64_t)n * n_items)), dim3(256), 0, (hipStream_t)stream, d_H,
                     ldh, d_Q, n, n_items, width, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
