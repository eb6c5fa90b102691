// jca.hip — JCA (Zhu et al., WWW 2019; model/general_recommender/JCA.py) on gfx950: the pair builder of one block of
// the rating matrix, the block step, the optimiser sweep and the scorer.  The model and the layouts are stated in
// include/neurec_hip.h; nothing here forms a dense [B, I] or [U, B] slab: both encoders pool table rows over the CSR
// row or the CSC column.
//
// Pairs (JCA.py:179-200)
//   jca_slots_kernel     colslot[c_b] = stamp << 32 | b
//   jca_bits_kernel      a wavefront per block row: the row's train items looked up in colslot set bits of the row's 16
//                        LDS words (integer atomics: order-free); the words and the row's number of positives go out
//   jca_draw_kernel      a wavefront per block row: its offset (the rows before it), a lane per positive, num_neg draws
// Step (JCA.py:80-112)
//   jca_encode_kernel    a workgroup per batch row / column: the history's table rows pooled in fp64 by four wavefronts
//                        in a fixed order, bias, factor, g; the slot maps
//   jca_decode_kernel    32 x 32 cells per workgroup (64 x 64 in the scorer), both products from LDS tiles over 32 hidden units at a time:
//                        Yu = f(xu), Yi = f(xi); the cell's pair count is zeroed on the way
//   jca_hinge_kernel     a thread per pair: the active pairs add +1 / -1 to the integer count of their cells; the losses
//                        summed in double by a fixed tree per workgroup;  jca_sum_kernel: the partials in a fixed order
//   jca_back_cells_kernel  a wavefront per block column, then per block row: the cells with a count (ballot over 64 at a
//                        time, ascending) give dxu = count / 2 * f'(Yu) and dxi: the decoder gradients G_UWt[c_b],
//                        G_Ub2[c_b], G_IWt[r_a], G_Ib2[r_a], G_IF[c_b], and dpu [n_rows][H], dpi [n_cols][H]
//   jca_back_rows_kernel a wavefront per item: its CSC column against rowslot, the batch's users ascending, G_UV[i] =
//                        the sum of their dpu; a wavefront per user: its CSR row against colslot, G_IV[u]; two wavefronts
//                        for the bias gradients.  A row without a hit is neither written nor flagged
// Apply                  jca_apply_kernel: a wavefront per table row, a thread per scalar; jca_sum_kernel for sum(w^2)
// Both activations' derivatives are taken from the outputs (sigmoid y (1 - y), tanh 1 - y^2, relu y > 0, elu y > 0 ? 1 :
// y + 1), so no pre-activation is kept but the item encoder's, which I_factor_vector's gradient needs.
#include "history_common.h"
#include "neurec_hip.h"

namespace {

constexpr int kWords = NRHIP_JCA_MAX_BATCH / 32;          // the words of one block row's bit set
constexpr int kHingeBlocks = 1024;                        // the most workgroups (and partial sums) of the hinge kernel
constexpr int kApplyRowBlocks = 2048, kApplyScalBlocks = 256;

struct Layout {                                           // offsets into d_W / d_M / d_V / d_G, and into d_flag
  int64_t UV, UWt, IV, IWt, Ub2, IF, Ib2, Ub1, Ib1, total;
  int64_t fUV, fUWt, fIV, fIWt, fUb2, fIF, fIb2;
};
__host__ __device__ inline Layout layout_of(int U, int I, int H) {
  Layout l;
  l.UV = 0;
  l.UWt = (int64_t)I * H;
  l.IV = 2 * (int64_t)I * H;
  l.IWt = l.IV + (int64_t)U * H;
  l.Ub2 = l.IWt + (int64_t)U * H;
  l.IF = l.Ub2 + I;
  l.Ib2 = l.IF + I;
  l.Ub1 = l.Ib2 + U;
  l.Ib1 = l.Ub1 + H;
  l.total = l.Ib1 + H;
  l.fUV = 0;
  l.fUWt = I;
  l.fIV = 2 * (int64_t)I;
  l.fIWt = l.fIV + U;
  l.fUb2 = l.fIWt + U;
  l.fIF = l.fUb2 + I;
  l.fIb2 = l.fIF + I;
  return l;
}

struct Work {                                             // the pieces of d_wsf / d_wsi / d_wsd
  float *hu, *hi, *pi, *dpu, *dpi, *Yu, *Yi;
  int32_t *cnt, *rowcnt;
  uint32_t* bits;
  double *hinge_part, *apply_part;
};
__host__ __device__ inline Work work_of(const nrhip_jca_args& a) {
  const int64_t B = a.batch_size, BH = B * a.H;
  Work w;
  w.hu = a.d_wsf;
  w.hi = w.hu + BH;
  w.pi = w.hi + BH;
  w.dpu = w.pi + BH;
  w.dpi = w.dpu + BH;
  w.Yu = w.dpi + BH;
  w.Yi = w.Yu + B * B;
  w.cnt = a.d_wsi;
  w.bits = (uint32_t*)(w.cnt + B * B);
  w.rowcnt = (int32_t*)(w.bits + B * kWords);
  w.hinge_part = a.d_wsd;
  w.apply_part = a.d_wsd + kHingeBlocks;
  return w;
}

__device__ __forceinline__ float act(int kind, float x) {
  switch (kind) {
    case NRHIP_JCA_ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    case NRHIP_JCA_ACT_TANH: return tanhf(x);
    case NRHIP_JCA_ACT_RELU: return x > 0.f ? x : 0.f;
    case NRHIP_JCA_ACT_ELU: return x > 0.f ? x : expm1f(x);
    default: return x;
  }
}
// the derivative from the OUTPUT y
__device__ __forceinline__ float dact(int kind, float y) {
  switch (kind) {
    case NRHIP_JCA_ACT_SIGMOID: return y * (1.0f - y);
    case NRHIP_JCA_ACT_TANH: return 1.0f - y * y;
    case NRHIP_JCA_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case NRHIP_JCA_ACT_ELU: return y > 0.f ? 1.f : y + 1.0f;
    default: return 1.f;
  }
}

__device__ __forceinline__ int64_t slot_of(int64_t stamp, int pos) { return (stamp << 32) | (uint32_t)pos; }

// ------------------------------------------------------------------------------------------------------ pairs
__global__ __launch_bounds__(256) void jca_slots_kernel(const int32_t* __restrict__ ids, int n, int64_t stamp,
                                                        int64_t* __restrict__ slot) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < n) slot[ids[x]] = slot_of(stamp, x);
}

__global__ __launch_bounds__(256) void jca_bits_kernel(nrhip_jca_args a) {
  __shared__ uint32_t s_bits[4][kWords];
  const Work w = work_of(a);
  const int wv = threadIdx.x >> 6, lane = nr_lane();
  const int row = blockIdx.x * 4 + wv;
  if (lane < kWords) s_bits[wv][lane] = 0u;
  __syncthreads();
  if (row < a.n_rows) {
    const int u = a.d_rows[row];
    const int64_t e0 = a.d_indptr[u + 1];
    for (int64_t k = a.d_indptr[u] + lane; k < e0; k += NR_WAVE) {
      const int64_t sl = a.d_colslot[a.d_indices[k]];
      if ((sl >> 32) == a.stamp) {
        const int b = (int)(uint32_t)sl;
        if (b < a.n_cols) atomicOr(&s_bits[wv][b >> 5], 1u << (b & 31));
      }
    }
  }
  __syncthreads();
  if (row >= a.n_rows) return;
  int n = 0;
  if (lane < kWords) {
    const uint32_t word = s_bits[wv][lane];
    w.bits[(int64_t)row * kWords + lane] = word;
    n = __popc(word);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, NR_WAVE);
  // a row short of num_neg unobserved columns gives no pair
  if (lane == 0) w.rowcnt[row] = a.n_cols - n >= a.num_neg ? n : 0;
}

__device__ __forceinline__ bool bit_at(const uint32_t* bits, int x) { return (bits[x >> 5] >> (x & 31)) & 1u; }

__global__ __launch_bounds__(256) void jca_draw_kernel(nrhip_jca_args a) {
  const Work w = work_of(a);
  const int wv = threadIdx.x >> 6, lane = nr_lane();
  const int row = blockIdx.x * 4 + wv;
  if (row >= a.n_rows) return;                             // no workgroup barrier below
  int before = 0;
  for (int r = lane; r < row; r += NR_WAVE) before += w.rowcnt[r];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, NR_WAVE);
  const int n_pos = w.rowcnt[row];
  if (row == a.n_rows - 1 && lane == 0) *a.d_total = (before + n_pos) * a.num_neg;
  if (n_pos == 0) return;
  const uint32_t* bits = w.bits + (int64_t)row * kWords;
  const int Bi = a.n_cols, K = a.num_neg;
  const uint64_t key = a.seed ^ nr::splitmix64(((uint64_t)(uint32_t)a.block_i << 32) | (uint32_t)a.block_j);
  for (int q = lane; q < n_pos; q += NR_WAVE) {
    int bp = -1, left = q;                                // the q-th set bit
    for (int x = 0; x < kWords && bp < 0; ++x) {
      uint32_t word = bits[x];
      const int c = __popc(word);
      if (left >= c) { left -= c; continue; }
      while (left--) word &= word - 1;
      bp = x * 32 + __builtin_ctz(word);
    }
    int taken[NRHIP_JCA_MAX_NEG];
    for (int k = 0; k < K; ++k) {
      nr::XorShift64s g;
      g.seed(key, a.epoch, ((uint64_t)(row * 512 + bp)) * 8 + (uint64_t)k);
      int neg = -1;
      for (int tries = 0; tries < nr::kMaxRejects && neg < 0; ++tries) {
        const int cand = (int)__umul64hi(g.next(), (uint64_t)Bi);
        bool bad = bit_at(bits, cand);
        for (int e = 0; e < k; ++e) bad = bad || taken[e] == cand;
        if (!bad) neg = cand;
      }
      if (neg < 0) {                                       // the rank-th free column, ascending
        int rank = (int)__umul64hi(g.next(), (uint64_t)(Bi - n_pos - k));
        for (int x = 0; x < Bi && neg < 0; ++x) {
          bool bad = bit_at(bits, x);
          for (int e = 0; e < k; ++e) bad = bad || taken[e] == x;
          if (!bad && rank-- == 0) neg = x;
        }
      }
      taken[k] = neg;
      a.d_pairs[((int64_t)before + q) * K + k] = ((uint32_t)row << 18) | ((uint32_t)bp << 9) | (uint32_t)neg;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ encoders
struct EncArgs {
  const int64_t* indptr;
  const int32_t* indices;
  const float* table;
  const float* bias;
  const float* factor;                                    // the item encoder's I_factor_vector, or nullptr
  const int32_t* ids;                                     // nullptr: 0..n-1
  int64_t* slot;                                          // nullptr: no slot map
  float* out;
  float* pre_out;                                         // the pooled row plus bias, before the factor; or nullptr
  int64_t stamp;
  int n, H, kind;
};

// a workgroup per row or column: wavefront v takes the entries [64 (v + 4 t), +64) of the history, their ids loaded 64
// at a time and handed round by lane, so that the table rows' loads do not wait on one another; fp64 partial sums, the
// four wavefronts' combined in the order 0, 1, 2, 3
template <int CPL>
__global__ __launch_bounds__(256) void jca_encode_kernel(EncArgs e) {
  __shared__ double s_part[3][NRHIP_JCA_MAX_H];
  const int lane = nr_lane(), wv = threadIdx.x >> 6;
  const int w = blockIdx.x;
  const int id = e.ids ? e.ids[w] : w;
  const int64_t e0 = e.indptr[id + 1];
  double acc[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0.0;
  for (int64_t base = e.indptr[id] + wv * NR_WAVE; base < e0; base += 4 * NR_WAVE) {
    const int64_t k = base + lane;
    const int mine = k < e0 ? e.indices[k] : 0;
    const int n = (int)(e0 - base < NR_WAVE ? e0 - base : NR_WAVE);
    for (int x0 = 0; x0 < n; x0 += 8) {                    // eight rows' loads in flight; a lane past the end holds row 0
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int h = __shfl(mine, x0 + u, NR_WAVE);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const int col = lane + j * NR_WAVE;
          const float v = col < e.H ? e.table[(int64_t)h * e.H + col] : 0.f;
          if (x0 + u < n) acc[j] += (double)v;
        }
      }
    }
  }
  if (wv > 0) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < e.H) s_part[wv - 1][col] = acc[j];
    }
  }
  __syncthreads();
  if (wv != 0) return;
  if (lane == 0 && e.slot) e.slot[id] = slot_of(e.stamp, w);
  const float fac = e.factor ? e.factor[id] : 1.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col >= e.H) continue;
    const double sum = ((acc[j] + s_part[0][col]) + s_part[1][col]) + s_part[2][col];
    float pre = (float)sum + e.bias[col];
    if (e.pre_out) e.pre_out[(int64_t)w * e.H + col] = pre;
    if (e.factor) pre = pre * fac;
    e.out[(int64_t)w * e.H + col] = act(e.kind, pre);
  }
}

// ------------------------------------------------------------------------------------------------------ decode
struct DecArgs {
  const float *hu, *hi, *UWt, *IWt, *Ub2, *Ib2;
  const int32_t *rows, *cols;                             // cols nullptr: column b is item b
  float *Yu, *Yi;
  int32_t* cnt;
  float* D;
  int64_t ld;
  int n_rows, n_cols, H, f_act;
};

// T x T cells per workgroup of 16 x 16 threads, T / 16 squared cells per thread
template <bool TRAIN, int T>
__global__ __launch_bounds__(256) void jca_decode_kernel(DecArgs a) {
  constexpr int KC = 32, M = T / 16;
  __shared__ float s_hu[T][KC + 1], s_uw[T][KC + 1], s_iw[T][KC + 1], s_hi[T][KC + 1];
  const int row0 = blockIdx.y * T, col0 = blockIdx.x * T;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int H = a.H;
  float au[M][M] = {}, ai[M][M] = {};
  for (int k0 = 0; k0 < H; k0 += KC) {
    for (int e = threadIdx.x; e < T * KC; e += 256) {
      const int r = e / KC, k = e % KC;
      const bool kin = k0 + k < H;
      const int ap = row0 + r, bp = col0 + r;
      float vhu = 0.f, viw = 0.f, vuw = 0.f, vhi = 0.f;
      if (kin && ap < a.n_rows) {
        vhu = a.hu[(int64_t)ap * H + k0 + k];
        viw = a.IWt[(int64_t)a.rows[ap] * H + k0 + k];
      }
      if (kin && bp < a.n_cols) {
        const int cid = a.cols ? a.cols[bp] : bp;
        vuw = a.UWt[(int64_t)cid * H + k0 + k];
        vhi = a.hi[(int64_t)bp * H + k0 + k];
      }
      s_hu[r][k] = vhu;
      s_iw[r][k] = viw;
      s_uw[r][k] = vuw;
      s_hi[r][k] = vhi;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < KC; ++k) {
      float h4[M], w4[M], u4[M], i4[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        h4[i] = s_hu[ty + 16 * i][k];
        w4[i] = s_iw[ty + 16 * i][k];
        u4[i] = s_uw[tx + 16 * i][k];
        i4[i] = s_hi[tx + 16 * i][k];
      }
#pragma unroll
      for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          au[i][j] = fmaf(h4[i], u4[j], au[i][j]);
          ai[i][j] = fmaf(i4[j], w4[i], ai[i][j]);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int ap = row0 + ty + 16 * i;
    if (ap >= a.n_rows) continue;
    const float ib2 = a.Ib2[a.rows[ap]];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const int bp = col0 + tx + 16 * j;
      if (bp >= a.n_cols) continue;
      const int cid = a.cols ? a.cols[bp] : bp;
      const float yu = act(a.f_act, au[i][j] + a.Ub2[cid]), yi = act(a.f_act, ai[i][j] + ib2);
      if (TRAIN) {
        const int64_t o = (int64_t)ap * a.n_cols + bp;
        a.Yu[o] = yu;
        a.Yi[o] = yi;
        a.cnt[o] = 0;
      } else {
        a.D[(int64_t)ap * a.ld + bp] = (yu + yi) * 0.5f;
      }
    }
  }
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void jca_score_pairs_kernel(const float* __restrict__ W, Layout l,
                                                              const int32_t* __restrict__ users,
                                                              const int32_t* __restrict__ items,
                                                              const int32_t* __restrict__ slot, int64_t n,
                                                              const float* __restrict__ hu,
                                                              const float* __restrict__ hi, int H, int f_act,
                                                              float* __restrict__ out) {
  using namespace nr::rowkey;
  const int c = group_lane<DP>();
  const int64_t p = group_index<DP, int64_t>();
  const bool in = p < n;
  float xu = 0.f, xi = 0.f;
  int u = 0, i = 0;
  if (in) {
    u = users[p];
    i = items[p];
    const int s = slot[p];
#pragma unroll
    for (int m = 0; m < CPL; ++m) {
      const int col = c + m * DP;
      if (col < H) {
        xu = fmaf(hu[(int64_t)s * H + col], W[l.UWt + (int64_t)i * H + col], xu);
        xi = fmaf(hi[(int64_t)i * H + col], W[l.IWt + (int64_t)u * H + col], xi);
      }
    }
  }
  group_sum<DP>(xu, xi);
  if (in && c == 0) out[p] = (act(f_act, xu + W[l.Ub2 + i]) + act(f_act, xi + W[l.Ib2 + u])) * 0.5f;
}

// ------------------------------------------------------------------------------------------------------ hinge
__global__ __launch_bounds__(256) void jca_hinge_kernel(nrhip_jca_args a) {
  const Work w = work_of(a);
  const int Bi = a.n_cols;
  double v[1] = {0.0};
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.n_pairs; p += (int64_t)gridDim.x * 256) {
    const uint32_t pr = a.d_pairs[p];
    const int row = (int)(pr >> 18), bp = (int)((pr >> 9) & 511u), bn = (int)(pr & 511u);
    if (row >= a.n_rows || bp >= Bi || bn >= Bi) continue;
    const int64_t op = (int64_t)row * Bi + bp, on = (int64_t)row * Bi + bn;
    const float dp = (w.Yu[op] + w.Yi[op]) * 0.5f, dn = (w.Yu[on] + w.Yi[on]) * 0.5f;
    const float x = (dn - dp) + a.margin;
    if (x > 0.f) {
      v[0] += (double)x;
      atomicAdd(&w.cnt[on], 1);
      atomicSub(&w.cnt[op], 1);
    }
  }
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) w.hinge_part[blockIdx.x] = v[0];
}

// out = (float)(scale * the sum of part[0..n)) by one workgroup, in a fixed order
__global__ __launch_bounds__(256) void jca_sum_kernel(const double* __restrict__ part, int n, double scale,
                                                      float* __restrict__ out) {
  double v[1] = {0.0};
  for (int x = threadIdx.x; x < n; x += 256) v[0] += part[x];
  nr::rowkey::block_sum(v);
  if (threadIdx.x == 0) *out = (float)(scale * v[0]);
}

// ------------------------------------------------------------------------------------------------------ backward
template <int CPL>
__global__ __launch_bounds__(256) void jca_back_cells_kernel(nrhip_jca_args a) {
  const Work w = work_of(a);
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  const int lane = nr_lane(), H = a.H, Bu = a.n_rows, Bi = a.n_cols;
  const int wi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= Bu + Bi) return;
  const bool by_col = wi < Bi;                            // a block column: sums over the rows; else the other way
  const int self = by_col ? wi : wi - Bi, n_other = by_col ? Bu : Bi;
  const int self_id = by_col ? a.d_cols[self] : a.d_rows[self];
  float gW[CPL] = {}, dh[CPL] = {}, gb = 0.f;
  for (int o0 = 0; o0 < n_other; o0 += NR_WAVE) {
    const int o = o0 + lane;
    const int64_t cell = by_col ? (int64_t)o * Bi + self : (int64_t)self * Bi + o;
    const int c = o < n_other ? w.cnt[cell] : 0;
    uint64_t mask = __ballot(c != 0);
    while (mask) {
      const int j0 = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int ox = o0 + j0;
      const float half = 0.5f * (float)__shfl(c, j0, NR_WAVE);
      const int64_t cx = by_col ? (int64_t)ox * Bi + self : (int64_t)self * Bi + ox;
      const float dxu = half * dact(a.f_act, w.Yu[cx]), dxi = half * dact(a.f_act, w.Yi[cx]);
      // the own table's gradient takes the other side's code; the other side's code gradient takes the other table
      const float own = by_col ? dxu : dxi, cross = by_col ? dxi : dxu;
      const float* code = by_col ? w.hu + (int64_t)ox * H : w.hi + (int64_t)ox * H;
      const float* tab = by_col ? a.d_W + l.IWt + (int64_t)a.d_rows[ox] * H : a.d_W + l.UWt + (int64_t)a.d_cols[ox] * H;
      gb += own;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int col = lane + j * NR_WAVE;
        if (col < H) {
          gW[j] = fmaf(own, code[col], gW[j]);
          dh[j] = fmaf(cross, tab[col], dh[j]);
        }
      }
    }
  }
  float* G_tab = a.d_G + (by_col ? l.UWt : l.IWt) + (int64_t)self_id * H;
  const float* my_code = (by_col ? w.hi : w.hu) + (int64_t)self * H;
  const float fac = by_col ? a.d_W[l.IF + self_id] : 1.f;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col >= H) continue;
    G_tab[col] = gW[j];
    const float dz = dh[j] * dact(a.g_act, my_code[col]);
    if (by_col) {
      s += dz * w.pi[(int64_t)self * H + col];
      w.dpi[(int64_t)self * H + col] = dz * fac;
    } else {
      w.dpu[(int64_t)self * H + col] = dz;
    }
  }
  if (by_col) s = nr_wave_sum_f32(s);
  if (lane == 0) {
    if (by_col) {
      a.d_G[l.Ub2 + self_id] = gb;
      a.d_G[l.IF + self_id] = s;
      a.d_flag[l.fUWt + self_id] = 1;
      a.d_flag[l.fUb2 + self_id] = 1;
      a.d_flag[l.fIF + self_id] = 1;
    } else {
      a.d_G[l.Ib2 + self_id] = gb;
      a.d_flag[l.fIWt + self_id] = 1;
      a.d_flag[l.fIb2 + self_id] = 1;
    }
  }
}

template <int CPL>
__global__ __launch_bounds__(256) void jca_back_rows_kernel(nrhip_jca_args a) {
  const Work w = work_of(a);
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  const int lane = nr_lane(), H = a.H, U = a.n_users, I = a.n_items;
  const int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= (int64_t)U + I + 2) return;
  float acc[CPL] = {};
  if (wi >= (int64_t)U + I) {                             // the first-layer biases: the codes' gradients in order
    const bool user_side = wi == (int64_t)U + I;
    const float* src = user_side ? w.dpu : w.dpi;
    const int n = user_side ? a.n_rows : a.n_cols;
    for (int x = 0; x < n; ++x) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int col = lane + j * NR_WAVE;
        if (col < H) acc[j] += src[(int64_t)x * H + col];
      }
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < H) a.d_G[(user_side ? l.Ub1 : l.Ib1) + col] = acc[j];
    }
    return;
  }
  const bool item_row = wi < I;                           // UV row of an item: its users; else IV row of a user
  const int r = item_row ? (int)wi : (int)(wi - I);
  const int64_t* ptr = item_row ? a.d_t_indptr : a.d_indptr;
  const int32_t* idx = item_row ? a.d_t_users : a.d_indices;
  const int64_t* slot = item_row ? a.d_rowslot : a.d_colslot;
  const float* src = item_row ? w.dpu : w.dpi;
  const int n_src = item_row ? a.n_rows : a.n_cols;
  const int64_t kb = ptr[r], ke = ptr[r + 1];
  bool any = false;
  for (int64_t base = kb; base < ke; base += NR_WAVE) {
    const int64_t k = base + lane;
    const int64_t sl = k < ke ? slot[idx[k]] : 0;
    const bool hit = (sl >> 32) == a.stamp && (int)(uint32_t)sl < n_src;
    uint64_t mask = __ballot(hit);
    while (mask) {
      const int j0 = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int pos = __shfl((int)(uint32_t)sl, j0, NR_WAVE);
      any = true;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int col = lane + j * NR_WAVE;
        if (col < H) acc[j] += src[(int64_t)pos * H + col];
      }
    }
  }
  if (!any) return;
  float* G = a.d_G + (item_row ? l.UV : l.IV) + (int64_t)r * H;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < H) G[col] = acc[j];
  }
  if (lane == 0) a.d_flag[(item_row ? l.fUV : l.fIV) + r] = 1;
}

// ------------------------------------------------------------------------------------------------------ apply
struct Opt {
  int adam;
  float step, omb1, omb2, eps, half_reg;
};

__device__ __forceinline__ void move(const Opt& o, float g, float& wv, float& m, float& v) {
  if (o.adam) nr::adam_dense_tf(g, wv, m, v, o.step, o.omb1, o.omb2, o.eps);
  else wv = __fsub_rn(wv, __fmul_rn(o.step, g));
}

__global__ __launch_bounds__(256) void jca_apply_kernel(nrhip_jca_args a, Opt o, int n_row_blocks) {
  const Work w = work_of(a);
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  const int lane = nr_lane(), H = a.H;
  const bool sweep = o.adam || o.half_reg != 0.f;         // every row moves
  double v[1] = {0.0};
  if ((int)blockIdx.x < n_row_blocks) {
    const int64_t n_rows = 2 * ((int64_t)a.n_users + a.n_items);    // the flags and the rows are in the same order
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += (int64_t)n_row_blocks * 4) {
      const bool has = a.d_flag[r] != 0;
      if (!has && !sweep) continue;
      for (int k = lane; k < H; k += NR_WAVE) {
        const int64_t x = r * H + k;
        float wv = a.d_W[x], m = 0.f, vv = 0.f, g = 0.f;
        if (has) {
          g = a.d_G[x];
          a.d_G[x] = 0.f;
        }
        if (o.adam) {
          m = a.d_M[x];
          vv = a.d_V[x];
        }
        v[0] += (double)wv * (double)wv;
        move(o, __fadd_rn(g, __fmul_rn(o.half_reg, wv)), wv, m, vv);
        a.d_W[x] = wv;
        if (o.adam) {
          a.d_M[x] = m;
          a.d_V[x] = vv;
        }
      }
      if (has && lane == 0) a.d_flag[r] = 0;
    }
  } else {
    const int64_t n_scal = l.total - l.Ub2, n_flagged = l.Ub1 - l.Ub2;
    const int64_t stride = (int64_t)(gridDim.x - n_row_blocks) * 256;
    for (int64_t s = (int64_t)(blockIdx.x - n_row_blocks) * 256 + threadIdx.x; s < n_scal; s += stride) {
      const int64_t x = l.Ub2 + s;
      const bool flagged = s < n_flagged;                 // Ub2, IF, Ib2 under flags; Ub1 and Ib1 always have one
      const bool has = flagged ? a.d_flag[l.fUb2 + s] != 0 : true;
      const bool is_factor = x >= l.IF && x < l.Ib2;      // I_factor_vector is not regularised
      if (!has && !(o.adam || (o.half_reg != 0.f && !is_factor))) continue;
      float wv = a.d_W[x], m = 0.f, vv = 0.f, g = 0.f;
      if (has) {
        g = a.d_G[x];
        a.d_G[x] = 0.f;
        if (flagged) a.d_flag[l.fUb2 + s] = 0;
      }
      if (o.adam) {
        m = a.d_M[x];
        vv = a.d_V[x];
      }
      if (!is_factor) {
        v[0] += (double)wv * (double)wv;
        g = __fadd_rn(g, __fmul_rn(o.half_reg, wv));
      }
      move(o, g, wv, m, vv);
      a.d_W[x] = wv;
      if (o.adam) {
        a.d_M[x] = m;
        a.d_V[x] = vv;
      }
    }
  }
  if (o.half_reg != 0.f) {                                // uniform over the grid
    nr::rowkey::block_sum(v);
    if (threadIdx.x == 0) w.apply_part[blockIdx.x] = v[0];
  }
}

// ------------------------------------------------------------------------------------------------------ host
int check_model(const char* entry, const nrhip_jca_args& a) {
  NR_REQUIRE(a.H >= 1 && a.H <= NRHIP_JCA_MAX_H, NR_ERR_UNSUPPORTED, "%s: hidden_neuron %d outside 1..%d", entry, a.H,
             NRHIP_JCA_MAX_H);
  NR_REQUIRE(a.batch_size >= 1 && a.batch_size <= NRHIP_JCA_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "%s: batch_size %d outside 1..%d", entry, a.batch_size, NRHIP_JCA_MAX_BATCH);
  NR_REQUIRE(a.num_neg >= 1 && a.num_neg <= NRHIP_JCA_MAX_NEG, NR_ERR_UNSUPPORTED, "%s: num_neg %d outside 1..%d", entry,
             a.num_neg, NRHIP_JCA_MAX_NEG);
  NR_REQUIRE(a.f_act >= 0 && a.f_act <= NRHIP_JCA_ACT_IDENTITY && a.g_act >= 0 && a.g_act <= NRHIP_JCA_ACT_IDENTITY,
             NR_ERR_UNSUPPORTED, "%s: unknown activation (f_act %d, g_act %d; 0 sigmoid, 1 tanh, 2 relu, 3 elu, "
             "4 identity)", entry, a.f_act, a.g_act);
  NR_REQUIRE(a.n_users >= 1 && a.n_items >= 1, NR_ERR_ARG, "%s: bad sizes", entry);
  NR_REQUIRE(a.d_W && a.d_indptr && a.d_indices && a.d_t_indptr && a.d_t_users, NR_ERR_ARG,
             "%s: null pointer argument", entry);
  return NR_OK;
}

int check_block(const char* entry, const nrhip_jca_args& a) {
  NR_TRY(check_model(entry, a));
  NR_REQUIRE(a.n_rows >= 0 && a.n_rows <= a.batch_size && a.n_cols >= 0 && a.n_cols <= a.batch_size &&
                 a.n_rows <= a.n_users && a.n_cols <= a.n_items, NR_ERR_ARG,
             "%s: a block of %d x %d outside batch_size %d", entry, a.n_rows, a.n_cols, a.batch_size);
  NR_REQUIRE(a.stamp >= 1 && a.stamp < ((int64_t)1 << 31), NR_ERR_ARG, "%s: stamp outside 1..2^31-1", entry);
  NR_REQUIRE(a.d_rows && a.d_cols && a.d_rowslot && a.d_colslot && a.d_wsf && a.d_wsi && a.d_wsd && a.d_pairs,
             NR_ERR_ARG, "%s: null pointer argument", entry);
  return NR_OK;
}

EncArgs encoder(const nrhip_jca_args& a, int which) {
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  EncArgs e = {};
  e.indptr = which ? a.d_t_indptr : a.d_indptr;
  e.indices = which ? a.d_t_users : a.d_indices;
  e.table = a.d_W + (which ? l.IV : l.UV);
  e.bias = a.d_W + (which ? l.Ib1 : l.Ub1);
  e.factor = which ? a.d_W + l.IF : nullptr;
  e.H = a.H;
  e.kind = a.g_act;
  return e;
}

int launch_encoder(const EncArgs& e, hipStream_t st) {
  if (e.n == 0) return NR_OK;
  const dim3 grid((unsigned)e.n);
  NR_HIST_BY_CPL(jca_encode_kernel, e.H, grid, st, e);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_jca_workspace(int n_users, int n_items, int H, int batch_size, int num_neg, int64_t* out) {
  NR_REQUIRE(out, NR_ERR_ARG, "jca_workspace: null pointer argument");
  NR_REQUIRE(n_users >= 1 && n_items >= 1, NR_ERR_ARG, "jca_workspace: bad sizes");
  NR_REQUIRE(H >= 1 && H <= NRHIP_JCA_MAX_H, NR_ERR_UNSUPPORTED, "jca_workspace: hidden_neuron %d outside 1..%d", H,
             NRHIP_JCA_MAX_H);
  NR_REQUIRE(batch_size >= 1 && batch_size <= NRHIP_JCA_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "jca_workspace: batch_size %d outside 1..%d", batch_size, NRHIP_JCA_MAX_BATCH);
  NR_REQUIRE(num_neg >= 1 && num_neg <= NRHIP_JCA_MAX_NEG, NR_ERR_UNSUPPORTED, "jca_workspace: num_neg %d outside 1..%d",
             num_neg, NRHIP_JCA_MAX_NEG);
  const int64_t B = batch_size;
  out[0] = 5 * B * H + 2 * B * B;
  out[1] = B * B + B * kWords + B;
  out[2] = kHingeBlocks + kApplyRowBlocks + kApplyScalBlocks;
  out[3] = B * B * num_neg;
  return NR_OK;
}

int nrhip_jca_pairs(const nrhip_jca_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_pairs: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_block("jca_pairs", a));
  NR_REQUIRE(a.d_total, NR_ERR_ARG, "jca_pairs: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  if (a.n_rows == 0 || a.n_cols == 0) {
    NR_CHECK_HIP(hipMemsetAsync(a.d_total, 0, sizeof(int32_t), st));
    return NR_OK;
  }
  hipLaunchKernelGGL(jca_slots_kernel, dim3((unsigned)((a.n_cols + 255) / 256)), dim3(256), 0, st, a.d_cols, a.n_cols,
                     a.stamp, a.d_colslot);
  NR_LAUNCH_CHECK();
  const dim3 grid((unsigned)((a.n_rows + 3) / 4));
  hipLaunchKernelGGL(jca_bits_kernel, grid, dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(jca_draw_kernel, grid, dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_jca_step(const nrhip_jca_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_step: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_block("jca_step", a));
  int64_t cap[4];
  NR_TRY(nrhip_jca_workspace(a.n_users, a.n_items, a.H, a.batch_size, a.num_neg, cap));
  NR_REQUIRE(a.n_pairs >= 0 && a.n_pairs <= cap[3], NR_ERR_ARG, "jca_step: %lld pairs outside 0..%lld",
             (long long)a.n_pairs, (long long)cap[3]);
  if (a.n_pairs == 0 || a.n_rows == 0 || a.n_cols == 0) return NR_OK;   // no work: nothing is launched or written
  NR_REQUIRE(a.d_G && a.d_flag && a.d_loss2, NR_ERR_ARG, "jca_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const Work w = work_of(a);
  const Layout l = layout_of(a.n_users, a.n_items, a.H);

  EncArgs eu = encoder(a, 0), ei = encoder(a, 1);
  eu.ids = a.d_rows; eu.n = a.n_rows; eu.slot = a.d_rowslot; eu.stamp = a.stamp; eu.out = w.hu;
  ei.ids = a.d_cols; ei.n = a.n_cols; ei.slot = a.d_colslot; ei.stamp = a.stamp; ei.out = w.hi; ei.pre_out = w.pi;
  NR_TRY(launch_encoder(eu, st));
  NR_TRY(launch_encoder(ei, st));

  DecArgs d = {};
  d.hu = w.hu; d.hi = w.hi;
  d.UWt = a.d_W + l.UWt; d.IWt = a.d_W + l.IWt; d.Ub2 = a.d_W + l.Ub2; d.Ib2 = a.d_W + l.Ib2;
  d.rows = a.d_rows; d.cols = a.d_cols;
  d.Yu = w.Yu; d.Yi = w.Yi; d.cnt = w.cnt;
  d.n_rows = a.n_rows; d.n_cols = a.n_cols; d.H = a.H; d.f_act = a.f_act;
  // a block is at most 512 x 512 cells: tiles of 32 x 32 give it up to 256 workgroups
  hipLaunchKernelGGL((jca_decode_kernel<true, 32>), dim3((unsigned)((a.n_cols + 31) / 32), (unsigned)((a.n_rows + 31) / 32)),
                     dim3(256), 0, st, d);
  NR_LAUNCH_CHECK();

  const int hinge_blocks = (int)((a.n_pairs + 255) / 256 < kHingeBlocks ? (a.n_pairs + 255) / 256 : kHingeBlocks);
  hipLaunchKernelGGL(jca_hinge_kernel, dim3((unsigned)hinge_blocks), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(jca_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)w.hinge_part, hinge_blocks, 1.0,
                     a.d_loss2);
  NR_LAUNCH_CHECK();

  const dim3 cells((unsigned)((a.n_rows + a.n_cols + 3) / 4));
  NR_HIST_BY_CPL(jca_back_cells_kernel, a.H, cells, st, a);
  NR_LAUNCH_CHECK();
  const dim3 rows((unsigned)(((int64_t)a.n_users + a.n_items + 2 + 3) / 4));
  NR_HIST_BY_CPL(jca_back_rows_kernel, a.H, rows, st, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_jca_apply(const nrhip_jca_args* args, int adam, float step, float beta1, float beta2, float eps,
                    void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_apply: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_model("jca_apply", a));
  NR_REQUIRE(a.d_G && a.d_flag && a.d_wsd && a.d_loss2 && (!adam || (a.d_M && a.d_V)), NR_ERR_ARG,
             "jca_apply: null pointer argument");
  NR_REQUIRE(a.reg >= 0.f, NR_ERR_ARG, "jca_apply: reg must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  Opt o;
  o.adam = adam ? 1 : 0;
  o.step = step;
  o.omb1 = 1.0f - beta1;
  o.omb2 = 1.0f - beta2;
  o.eps = eps;
  o.half_reg = 0.5f * a.reg;
  const int64_t n_rows = 2 * ((int64_t)a.n_users + a.n_items), n_scal = l.total - l.Ub2;
  const int row_blocks = (int)((n_rows + 3) / 4 < kApplyRowBlocks ? (n_rows + 3) / 4 : kApplyRowBlocks);
  const int scal_blocks = (int)((n_scal + 255) / 256 < kApplyScalBlocks ? (n_scal + 255) / 256 : kApplyScalBlocks);
  hipLaunchKernelGGL(jca_apply_kernel, dim3((unsigned)(row_blocks + scal_blocks)), dim3(256), 0, st, a, o, row_blocks);
  NR_LAUNCH_CHECK();
  if (o.half_reg != 0.f) {
    const Work w = work_of(a);
    hipLaunchKernelGGL(jca_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)w.apply_part, row_blocks + scal_blocks,
                       (double)a.reg * 0.25, a.d_loss2 + 1);
    NR_LAUNCH_CHECK();
  } else {
    NR_CHECK_HIP(hipMemsetAsync(a.d_loss2 + 1, 0, sizeof(float), st));
  }
  return NR_OK;
}

int nrhip_jca_encode(const nrhip_jca_args* args, int which, const int32_t* d_ids, int n, float* d_out, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_encode: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_model("jca_encode", a));
  NR_REQUIRE(which == 0 || which == 1, NR_ERR_ARG, "jca_encode: which must be 0 (users) or 1 (items)");
  NR_REQUIRE(n >= 0 && (d_ids || n <= (which ? a.n_items : a.n_users)), NR_ERR_ARG, "jca_encode: bad count %d", n);
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_out, NR_ERR_ARG, "jca_encode: null pointer argument");
  EncArgs e = encoder(a, which);
  e.ids = d_ids;
  e.n = n;
  e.out = d_out;
  return launch_encoder(e, (hipStream_t)stream);
}

int nrhip_jca_score(const nrhip_jca_args* args, const int32_t* d_users, int n, const float* d_hu, const float* d_hi,
                    float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_score: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_model("jca_score", a));
  NR_REQUIRE(n >= 0 && ld >= a.n_items, NR_ERR_ARG, "jca_score: bad sizes");
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_users && d_hu && d_hi && d_out, NR_ERR_ARG, "jca_score: null pointer argument");
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  DecArgs d = {};
  d.hu = d_hu; d.hi = d_hi;
  d.UWt = a.d_W + l.UWt; d.IWt = a.d_W + l.IWt; d.Ub2 = a.d_W + l.Ub2; d.Ib2 = a.d_W + l.Ib2;
  d.rows = d_users; d.cols = nullptr;
  d.D = d_out; d.ld = ld;
  d.n_rows = n; d.n_cols = a.n_items; d.H = a.H; d.f_act = a.f_act;
  const unsigned gy = (unsigned)((n + 63) / 64);
  NR_REQUIRE(gy <= 65535u, NR_ERR_ARG, "jca_score: at most %d users per call", 65535 * 64);
  hipLaunchKernelGGL((jca_decode_kernel<false, 64>), dim3((unsigned)((a.n_items + 63) / 64), gy), dim3(256), 0,
                     (hipStream_t)stream, d);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_jca_score_pairs(const nrhip_jca_args* args, const int32_t* d_users, const int32_t* d_items,
                          const int32_t* d_slot, int64_t n, const float* d_hu, const float* d_hi, float* d_out,
                          void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "jca_score_pairs: null argument block");
  const nrhip_jca_args a = *args;
  NR_TRY(check_model("jca_score_pairs", a));
  NR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), NR_ERR_ARG, "jca_score_pairs: bad count");
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_users && d_items && d_slot && d_hu && d_hi && d_out, NR_ERR_ARG,
             "jca_score_pairs: null pointer argument");
  const Layout l = layout_of(a.n_users, a.n_items, a.H);
  hipStream_t st = (hipStream_t)stream;
  NR_BY_WIDTH(jca_score_pairs_kernel, a.H, n, st, (const float*)a.d_W, l, d_users, d_items, d_slot, n, d_hu, d_hi, a.H,
              a.f_act, d_out);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
