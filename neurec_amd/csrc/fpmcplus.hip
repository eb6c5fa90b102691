// fpmcplus.hip — FPMCplus: the step and predict() of model/sequential_recommender/FPMCplus.py on gfx950.
//
// An instance is (user u, recents r_0..r_{L-1}, item i[, negative j]).  FPMC's four row tables UI [U][d], IU / IL / LI
// [I][d] and a small attention MLP W [3d][w] = [W_u; W_i; W_l], b [w], h [w] that weights the recents PER TARGET ITEM:
//     a_l[k] = tanh(UI[u] . W_u[:,k] + IL[i] . W_i[:,k] + LI[r_l] . W_l[:,k] + b[k])               FPMCplus.py:75-82
//     A_l    = sum_k a_l[k] h[k],   alpha_l = exp(A_l) / sum_m exp(A_m)   (no max is subtracted)    FPMCplus.py:85-91
//     s      = sum_l alpha_l LI[r_l]                                                               FPMCplus.py:93
//     x(u,i) = <UI[u], IU[i]> + <IL[i], s>                                                         FPMCplus.py:103-105
// A slot whose recent is outside [0, n_items) takes no part in the softmax or in any gradient.
//
//   fpmcplus_instance_kernel  one wavefront per batch slot, forward and backward in one pass with the instance's rows
//                             and activations in LDS: the projections UI[u] W_u and LI[r_l] W_l once (shared by the
//                             positive and the negative side), per side a, A, alpha, s, x; then g, and per side
//                                 dA_l = g alpha_l (<IL[i], LI[r_l]> - <IL[i], s>),  delta_l[k] = dA_l h[k] (1 - a_l[k]^2)
//                             It leaves ONE gradient row per looked-up row ("contribution", regulariser included), its
//                             sort key (table row | contribution index), and the instance's delta sums for the dense
//                             gradients.  Contribution kinds, index = kind * B + t:
//                                 0 UI[u]   1 IU[i]   2 IL[i]   (pairwise: 3 IU[j]   4 IL[j])   then LI[r_l], l = 0..L-1
//   nrhip_sort_u64            the keys, ascending: one key space of U + 3 I rows (UI, IU, IL, LI)
//   fpmcplus_rows_kernel      one lane group per sorted key: the head of a run adds the run's contributions in key
//                             order and STORES the row's gradient
//   fpmcplus_dense_kernel     G_W, G_b, G_h: per chunk of the batch, one thread per element, instances in batch order
//   fpmcplus_reduce_kernel    the chunks' partials in chunk order (+ reg_w W, reg_w h in pairwise mode), stored
//   fpmcplus_loss_kernel      one workgroup: the loss and regulariser sums in a fixed order
//
//   fpmcplus_item_proj / user_proj / pairs    predict(): the pre-activation is additive,
//                                 c_{u,l}[k] = UI[u] . W_u[:,k] + LI[r_{u,l}] . W_l[:,k] + b[k]     n L w values
//                                 p_i[k]     = IL[i] . W_i[:,k]                                     I w values
//                             so a (u, i) pair costs L w tanh and (1 + L) d multiply-adds and nothing of size n I L is
//                             stored: a tile of items keeps its IU / IL rows and p_i in LDS (one lane per item), a
//                             wavefront walks the block's users with the pair's L logits and L + 1 products in registers
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

constexpr int kChunks = NRHIP_FPMCPLUS_MAX_CHUNKS;

__host__ __device__ inline int chunks_of(int B) { return B <= 0 ? 0 : (B + 31) / 32 < kChunks ? (B + 31) / 32 : kChunks; }

// 0 in a vector register, opaque to the compiler: what is derived from it is kept per lane, not in scalar registers
__device__ __forceinline__ int vector_zero() {
  int z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}

// The kernel's argument block read again from the kernarg segment (the first parameter lies at its start), behind a
// point the compiler cannot move loads across: a pointer that only a kernel's last section uses is loaded there
// instead of being held in scalar registers from the entry on — held from the entry, the blocks' pointers spilled
template <typename Args>
__device__ __forceinline__ const Args __attribute__((address_space(4)))* kernel_args_again() {
  auto p = (const Args __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// out[k] = sum over c of vec[c] Wb[c w + k], k < w: lane (q, k) of a wavefront takes the columns c = q, q + Q, ..;
// WP = the power of two >= w, Q = 64 / WP.  Every lane of the wavefront calls it.
__device__ __forceinline__ void project(const float* vec, const float* __restrict__ Wb, int d, int w, int WP,
                                        float* out) {
  const int lane = threadIdx.x & 63, k = lane & (WP - 1), q = lane / WP, Q = NR_WAVE / WP;
  float acc = 0.f;
  if (k < w)
    for (int c = q; c < d; c += Q) acc += vec[c] * Wb[(int64_t)c * w + k];
  for (int m = WP; m < NR_WAVE; m <<= 1) acc += __shfl_xor(acc, m, NR_WAVE);
  if (q == 0 && k < w) out[k] = acc;
}

__global__ __launch_bounds__(64) void fpmcplus_instance_kernel(nrhip_fpmcplus_step_args a, int WP) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x, t = blockIdx.x;
  const int B = a.batch, d = a.d, w = a.w, L = a.L, U = a.n_users, I = a.n_items;
  const int S = a.pairwise ? 2 : 1, ds = d + 1;
  // the instance's LDS: rows, projections, activations (delta in place), per-slot scalars.  The twelve offsets are
  // held in vector registers (vector_zero): the scalar file is taken by the argument block's pointers, and uniform
  // offsets on top of them spilled scalar registers
  float* zu = lds + vector_zero();       // [d]         UI[u]
  float* zi = zu + d;                    // [2][d]      IL[i], IL[j]
  float* zl = zi + 2 * d;                // [L][d + 1]  LI[r_l]
  float* ss = zl + L * ds;               // [2][d]      s per side
  float* pre = ss + 2 * d;               // [L][w]      LI[r_l] W_l
  float* pu = pre + L * w;               // [w]         UI[u] W_u + b
  float* pi = pu + w;                    // [2][w]      IL[item] W_i
  float* act = pi + 2 * w;               // [2][L][w]   a, then delta
  float* Dl = act + 2 * L * w;           // [2][w]      Delta per side
  float* al = Dl + 2 * w;                // [2][L]      alpha
  float* ee = al + 2 * L;                // [2][L]      <IL[item], LI[r_l]>
  float* dA = ee + 2 * L;                // [2][L]
  const int n_kinds = 1 + 2 * S + L;
  const int u = a.d_users[t];
  int item[2];
  item[0] = a.d_items[t];
  item[1] = a.pairwise ? ((const int32_t*)a.d_third)[t] : 0;
  const bool ok = u >= 0 && u < U && item[0] >= 0 && item[0] < I && item[1] >= 0 && item[1] < I;
  if (!ok) {                             // the slot takes no part (uniform over the wavefront)
    float* sc = a.d_scal + (int64_t)t * kScal;
    float* dl_out = a.d_delta + (int64_t)t * (L + 4) * w;
    if (lane < n_kinds) a.d_keys[(int64_t)lane * B + t] = kSentinel;
    if (lane < kScal) sc[lane] = 0.f;
    for (int k = lane; k < (L + 4) * w; k += NR_WAVE) dl_out[k] = 0.f;
    return;
  }
  const int my_r = lane < L ? a.d_recents[(int64_t)t * L + lane] : -1;      // lane l holds recent l
  const bool my_valid = my_r >= 0 && my_r < I;
  for (int c = lane; c < d; c += NR_WAVE) {
    zu[c] = a.d_UI[(int64_t)u * d + c];
    zi[c] = a.d_IL[(int64_t)item[0] * d + c];
    zi[d + c] = a.d_IL[(int64_t)item[1] * d + c];
  }
  for (int l = 0; l < L; ++l) {
    const int r = __shfl(my_r, l, NR_WAVE);
    const bool v = r >= 0 && r < I;
    for (int c = lane; c < d; c += NR_WAVE) zl[l * ds + c] = v ? a.d_LI[(int64_t)r * d + c] : 0.f;
  }
  __syncthreads();
  // the projections that do not depend on the side
  project(zu, a.d_W, d, w, WP, pu);
  for (int l = 0; l < L; ++l) project(zl + l * ds, a.d_W + (int64_t)2 * d * w, d, w, WP, pre + l * w);
  for (int s = 0; s < S; ++s) project(zi + s * d, a.d_W + (int64_t)d * w, d, w, WP, pi + s * w);
  __syncthreads();
  if (lane < w) pu[lane] += a.d_b[lane];
  __syncthreads();
  float x[2] = {0.f, 0.f}, is[2] = {0.f, 0.f}, sq = 0.f;
  for (int s = 0; s < S; ++s) {
    for (int e = lane; e < L * w; e += NR_WAVE) {
      const int k = e % w;
      act[s * L * w + e] = tanhf(pu[k] + pi[s * w + k] + pre[e]);
    }
    __syncthreads();
    float ex = 0.f;
    if (lane < L) {
      float A = 0.f, dot = 0.f;
      for (int k = 0; k < w; ++k) A += act[(s * L + lane) * w + k] * a.d_h[k];
      for (int c = 0; c < d; ++c) dot += zi[s * d + c] * zl[lane * ds + c];
      ex = my_valid ? expf(A) : 0.f;
      ee[s * L + lane] = dot;
    }
    float sum = 0.f;                                       // in l order, the same in every lane
    for (int l = 0; l < L; ++l) sum += __shfl(ex, l, NR_WAVE);
    if (lane < L) al[s * L + lane] = my_valid ? ex / sum : 0.f;
    __syncthreads();
    // <IL[item], s> as sum_l alpha_l <IL[item], LI[r_l]>, in l order: with one slot present alpha is exactly 1 and
    // dA exactly 0 — at L = 1 the model IS FPMC and the attention's gradients are the regulariser's alone
    float isum = 0.f;
    for (int l = 0; l < L; ++l) isum += al[s * L + l] * ee[s * L + l];
    is[s] = isum;
    float px = 0.f, psq = 0.f;
    for (int c = lane; c < d; c += NR_WAVE) {
      float sv = 0.f;
      for (int l = 0; l < L; ++l) sv += al[s * L + l] * zl[l * ds + c];
      ss[s * d + c] = sv;
      const float iu = a.d_IU[(int64_t)item[s] * d + c], il = zi[s * d + c];
      px += zu[c] * iu;
      psq += iu * iu + il * il;
      if (s == 0) {
        psq += zu[c] * zu[c];
        for (int l = 0; l < L; ++l) psq += zl[l * ds + c] * zl[l * ds + c];      // absent slots hold zeros
      }
    }
    px = nr_wave_sum_f32(px);
    sq += nr_wave_sum_f32(psq);
    x[s] = px + is[s];
  }
  // what only this half of the kernel touches is read from here on
  const auto* late = kernel_args_again<nrhip_fpmcplus_step_args>();
  float* sc = late->d_scal + (int64_t)t * kScal;
  float* dl_out = late->d_delta + (int64_t)t * (L + 4) * w;
  const float* h = late->d_h;
  const int loss_kind = late->loss_kind;
  float g, loss;
  if (S == 2) {
    const float y = x[0] - x[1];
    loss = nr::pairwise_loss(loss_kind, y);
    g = nr::pairwise_dloss(loss_kind, y);
  } else {
    // tf.losses.sigmoid_cross_entropy is a MEAN over the batch, every other loss of util/learner.py a sum
    const float scale = loss_kind == nr::NR_POINT_CROSS_ENTROPY ? 1.0f / (float)B : 1.0f;
    const float z = ((const float*)late->d_third)[t];
    loss = scale * nr::pointwise_loss(loss_kind, z, x[0]);
    g = scale * nr::pointwise_dloss(loss_kind, z, x[0]);
  }
  // backward through the attention, per side
  float hh = 0.f;                                          // lane k: sum over sides and l of dA_l a_l[k]
  for (int s = 0; s < S; ++s) {
    const float gs = s == 0 ? g : -g;
    if (lane < L) dA[s * L + lane] = gs * al[s * L + lane] * (ee[s * L + lane] - is[s]);
    __syncthreads();
    if (lane < w) {
      const float hk = h[lane];
      float D = 0.f;
      for (int l = 0; l < L; ++l) {
        const float av = act[(s * L + l) * w + lane], dAl = dA[s * L + l];
        const float del = dAl * hk * (1.0f - av * av);
        hh += dAl * av;
        D += del;
        act[(s * L + l) * w + lane] = del;
      }
      Dl[s * w + lane] = D;
    }
  }
  __syncthreads();
  // what the dense gradients need of this instance: Delta summed over the sides, per side, G_h's share, delta_l summed
  if (lane < w) {
    const float D0 = Dl[lane], D1 = S == 2 ? Dl[w + lane] : 0.f;
    const float Dsum = S == 2 ? D0 + D1 : D0;
    pu[lane] = Dsum;                                       // the projection is spent: Delta over the sides for W_u
    dl_out[lane] = Dsum;
    dl_out[w + lane] = D0;
    dl_out[2 * w + lane] = D1;
    dl_out[3 * w + lane] = hh;
  }
  for (int e = lane; e < L * w; e += NR_WAVE) {
    const float v = S == 2 ? act[e] + act[L * w + e] : act[e];
    act[e] = v;
    dl_out[4 * w + e] = v;
  }
  __syncthreads();
  // the contributions: one gradient row per looked-up row, the regulariser's share of this occurrence included
  const float reg = late->reg_mf;
  const float* Wu = late->d_W;
  const float* Wi = Wu + (int64_t)d * w;
  const float* Wl = Wu + (int64_t)2 * d * w;
  const float* IU = late->d_IU;
  float* contrib = late->d_contrib;
  for (int c = lane; c < d; c += NR_WAVE) {
    float mu = 0.f;
    for (int k = 0; k < w; ++k) mu += Wu[(int64_t)c * w + k] * pu[k];
    float gu = 0.f;
    for (int s = 0; s < S; ++s) {
      const float gs = s == 0 ? g : -g;
      const float iu = IU[(int64_t)item[s] * d + c];
      gu += gs * iu;
      float mi = 0.f;
      for (int k = 0; k < w; ++k) mi += Wi[(int64_t)c * w + k] * Dl[s * w + k];
      contrib[((int64_t)(1 + 2 * s) * B + t) * d + c] = gs * zu[c] + reg * iu;
      contrib[((int64_t)(2 + 2 * s) * B + t) * d + c] = gs * ss[s * d + c] + mi + reg * zi[s * d + c];
    }
    contrib[(int64_t)t * d + c] = gu + mu + reg * zu[c];
    for (int l = 0; l < L; ++l) {
      float ml = 0.f, gl = 0.f;
      for (int k = 0; k < w; ++k) ml += Wl[(int64_t)c * w + k] * act[l * w + k];
      for (int s = 0; s < S; ++s) gl += (s == 0 ? g : -g) * al[s * L + l] * zi[s * d + c];
      contrib[((int64_t)(1 + 2 * S + l) * B + t) * d + c] = gl + ml + reg * zl[l * ds + c];
    }
  }
  // keys and row flags
  uint64_t* keys = late->d_keys;
  uint8_t *flag_UI = late->d_flag_UI, *flag_IU = late->d_flag_IU, *flag_IL = late->d_flag_IL, *flag_LI = late->d_flag_LI;
  if (lane == 0) {
    keys[t] = row_key(u, (uint32_t)t);
    if (flag_UI) flag_UI[u] = 1;
    for (int s = 0; s < S; ++s) {
      keys[(int64_t)(1 + 2 * s) * B + t] = row_key(U + item[s], (uint32_t)((1 + 2 * s) * B + t));
      keys[(int64_t)(2 + 2 * s) * B + t] = row_key(U + I + item[s], (uint32_t)((2 + 2 * s) * B + t));
      if (flag_IU) flag_IU[item[s]] = 1;
      if (flag_IL) flag_IL[item[s]] = 1;
    }
    sc[S_G] = g;
    sc[S_LOSS] = loss;
    sc[S_L2] = 0.5f * sq;
    sc[S_OK] = 1.f;
  }
  if (lane < L) {
    const uint32_t idx = (uint32_t)((1 + 2 * S + lane) * B + t);
    keys[(int64_t)idx] = my_valid ? row_key(U + 2 * I + my_r, idx) : kSentinel;
    if (my_valid && flag_LI) flag_LI[my_r] = 1;
  }
}

__global__ __launch_bounds__(256) void fpmcplus_loss_kernel(nrhip_fpmcplus_step_args a) {
  double v[3] = {0.0, 0.0, 0.0};                           // the loss, the rows' l2 sum, |W|^2 + |h|^2
  slot_sums(a.d_scal, a.batch, v[0], v[1]);
  if (a.pairwise) {                                        // reg_w l2_loss(W, h): the pairwise loss alone has it
    for (int e = threadIdx.x; e < 3 * a.d * a.w; e += 256) v[2] += (double)a.d_W[e] * (double)a.d_W[e];
    for (int e = threadIdx.x; e < a.w; e += 256) v[2] += (double)a.d_h[e] * (double)a.d_h[e];
  }
  block_sum(v);
  if (threadIdx.x == 0) {
    a.d_loss2[0] = (float)v[0];
    a.d_loss2[1] = (float)((double)a.reg_mf * v[1] + (double)a.reg_w * 0.5 * v[2]);
  }
}

// the sum of one run of the sorted keys: the contributions of the row's occurrences, added in key order and stored.
// The column loop strides by DP: the columns per lane of the launch ladder are not used
template <int DP, int>
__global__ __launch_bounds__(256) void fpmcplus_rows_kernel(nrhip_fpmcplus_step_args a, int n_keys) {
  const int c0 = group_lane<DP>();
  const int64_t q0 = group_index<DP, int64_t>();
  const int head = head_row(a.d_keys, n_keys, q0);
  if (head < 0) return;
  const int d = a.d, U = a.n_users, I = a.n_items;
  float* dst;
  if (head < U) dst = a.d_G_UI + (int64_t)head * d;
  else if (head < U + I) dst = a.d_G_IU + (int64_t)(head - U) * d;
  else if (head < U + 2 * I) dst = a.d_G_IL + (int64_t)(head - U - I) * d;
  else dst = a.d_G_LI + (int64_t)(head - U - 2 * I) * d;
  for (int c = c0; c < d; c += DP) {
    float acc = 0.f;
    for_run(a.d_keys, n_keys, q0, head, [&](uint32_t idx) { acc += a.d_contrib[(int64_t)idx * d + c]; });
    dst[c] = acc;
  }
}

// G_W [3d][w], G_b [w], G_h [w] of one chunk of the batch: element e of the partial, the chunk's instances in order
__global__ __launch_bounds__(256) void fpmcplus_dense_kernel(nrhip_fpmcplus_step_args a, int chunks) {
  const int d = a.d, w = a.w, L = a.L, B = a.batch, I = a.n_items, n_el = 3 * d * w + 2 * w;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_el) return;
  const int per = (B + chunks - 1) / chunks;
  const int t0 = blockIdx.y * per, t1 = min(B, t0 + per);
  const int stride = (L + 4) * w;
  float acc = 0.f;
  if (e < 3 * d * w) {
    const int c = e / w, k = e % w, blk = c / d, cc = c - blk * d;
    for (int t = t0; t < t1; ++t) {
      if (a.d_scal[(int64_t)t * kScal + S_OK] == 0.f) continue;
      const float* dl = a.d_delta + (int64_t)t * stride;
      if (blk == 0) {
        acc += a.d_UI[(int64_t)a.d_users[t] * d + cc] * dl[k];
      } else if (blk == 1) {
        acc += a.d_IL[(int64_t)a.d_items[t] * d + cc] * dl[w + k];
        if (a.pairwise) acc += a.d_IL[(int64_t)((const int32_t*)a.d_third)[t] * d + cc] * dl[2 * w + k];
      } else {
        for (int l = 0; l < L; ++l) {
          const int r = a.d_recents[(int64_t)t * L + l];
          if (r >= 0 && r < I) acc += a.d_LI[(int64_t)r * d + cc] * dl[(4 + l) * w + k];
        }
      }
    }
  } else {
    const int k = (e - 3 * d * w) % w, off = e < 3 * d * w + w ? 0 : 3 * w;     // G_b: Delta; G_h: its own share
    for (int t = t0; t < t1; ++t)
      if (a.d_scal[(int64_t)t * kScal + S_OK] != 0.f) acc += a.d_delta[(int64_t)t * stride + off + k];
  }
  a.d_partial[(int64_t)blockIdx.y * n_el + e] = acc;
}

__global__ __launch_bounds__(256) void fpmcplus_reduce_kernel(nrhip_fpmcplus_step_args a, int chunks) {
  const int n_w = 3 * a.d * a.w, w = a.w, n_el = n_w + 2 * w;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_el) return;
  float acc = 0.f;
  for (int y = 0; y < chunks; ++y) acc += a.d_partial[(int64_t)y * n_el + e];
  // reg_w l2_loss(W, h): pairwise alone (FPMCplus.py:114-119); b is never regularised
  if (e < n_w) a.d_G_W[e] = a.pairwise ? acc + a.reg_w * a.d_W[e] : acc;
  else if (e < n_w + w) a.d_G_b[e - n_w] = acc;
  else a.d_G_h[e - n_w - w] = a.pairwise ? acc + a.reg_w * a.d_h[e - n_w - w] : acc;
}

// ------------------------------------------------------------------ predict()
// tanh on the scoring path: 1 - 2 / (exp(2 z) + 1) on the hardware's exp2 and reciprocal (1 ulp each): absolute error
// of a few 1e-7 on a value in [-1, 1], against the 1e-5 of a score the evaluation's bound allows
__device__ __forceinline__ float tanh_score(float z) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * z) + 1.0f);
}

__global__ __launch_bounds__(256) void fpmcplus_item_proj_kernel(nrhip_fpmcplus_scores_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d = a.d, w = a.w;
  if (e >= (int64_t)a.n_items * w) return;
  const int i = (int)(e / w), k = (int)(e % w);
  const float* Wi = a.d_W + (int64_t)d * w;
  float acc = 0.f;
  for (int c = 0; c < d; ++c) acc += a.d_IL[(int64_t)i * d + c] * Wi[(int64_t)c * w + k];
  a.d_p[e] = acc;
}

__global__ __launch_bounds__(256) void fpmcplus_user_proj_kernel(nrhip_fpmcplus_scores_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d = a.d, w = a.w, L = a.L;
  if (e >= (int64_t)a.batch * L * w) return;
  const int k = (int)(e % w), l = (int)((e / w) % L), n = (int)(e / ((int64_t)L * w));
  const int u = a.d_users[n];
  float acc = 0.f;
  if (u >= 0 && u < a.n_users) {
    const int r = a.d_last[(int64_t)u * L + l];
    if (r >= 0 && r < a.n_items) {
      const float* Wl = a.d_W + (int64_t)2 * d * w;
      for (int c = 0; c < d; ++c) acc += a.d_UI[(int64_t)u * d + c] * a.d_W[(int64_t)c * w + k];
      float lw = 0.f;
      for (int c = 0; c < d; ++c) lw += a.d_LI[(int64_t)r * d + c] * Wl[(int64_t)c * w + k];
      acc = acc + lw + a.d_b[k];
    }
  }
  a.d_c[e] = acc;
}

// One workgroup: a tile of TI items (lane % TI is the item) against a block of users_per_block users.  The tile's IU
// and IL rows and p_i sit in LDS column-major ([c][TI]: a wavefront's lanes read consecutive banks); a wavefront takes
// 64 / TI users at a time and reads their rows and c_{u,l} from global memory, every lane of a user the same address.
// LP is high_order rounded up to a power of two: the pair's logits and products are LP registers each, and only LP
// slot tests are live (sixteen uniform tests, hoisted out of the loops, spilled scalar registers).
template <int TI, int LP>
__global__ __launch_bounds__(256) void fpmcplus_pairs_kernel(nrhip_fpmcplus_scores_args a, int users_per_block) {
  extern __shared__ float lds[];
  constexpr int UPW = NR_WAVE / TI;                        // users a wavefront holds at a time
  const int d = a.d, w = a.w, L = a.L, I = a.n_items;
  float* s_iu = lds;                                       // [d][TI]
  float* s_il = s_iu + d * TI;                             // [d][TI]
  float* s_p = s_il + d * TI;                              // [w][TI]
  const int i0 = blockIdx.x * TI;
  for (int e = threadIdx.x; e < d * TI; e += 256) {
    const int it = e / d, c = e - it * d, i = i0 + it;
    s_iu[c * TI + it] = i < I ? a.d_IU[(int64_t)i * d + c] : 0.f;
    s_il[c * TI + it] = i < I ? a.d_IL[(int64_t)i * d + c] : 0.f;
  }
  for (int e = threadIdx.x; e < w * TI; e += 256) {
    const int it = e / w, k = e - it * w, i = i0 + it;
    s_p[k * TI + it] = i < I ? a.d_p[(int64_t)i * w + k] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int it = lane % TI, i = i0 + it;
  const int n0 = blockIdx.y * users_per_block, n1 = min(a.batch, n0 + users_per_block);
  for (int n = n0 + wave * UPW + lane / TI; n < n1; n += 4 * UPW) {
    const int u = a.d_users[n];
    float x = 0.f;
    if (u >= 0 && u < a.n_users) {
      const float* ui = a.d_UI + (int64_t)u * d;
      for (int c = 0; c < d; ++c) x += ui[c] * s_iu[c * TI + it];
      float A[LP], E[LP];
      int present = 0;
#pragma unroll
      for (int l = 0; l < LP; ++l) {
        A[l] = 0.f;
        E[l] = 0.f;
        if (l < LP / 2 || l < L) {
          const int r = a.d_last[(int64_t)u * L + l];
          if (r >= 0 && r < I) {
            present |= 1 << l;
            const float* li = a.d_LI + (int64_t)r * d;
            float dot = 0.f;
            for (int c = 0; c < d; ++c) dot += li[c] * s_il[c * TI + it];
            E[l] = dot;
          }
        }
      }
      const float* cu = a.d_c + (int64_t)n * L * w;
      for (int k = 0; k < w; ++k) {
        const float pk = s_p[k * TI + it], hk = a.d_h[k];
        const float* q = cu + k;                           // walks the L rows of c: one running address, no L offsets
#pragma unroll
        for (int l = 0; l < LP; ++l)
          if (l < LP / 2 || l < L) {
            A[l] += hk * tanh_score(*q + pk);
            q += w;
          }
      }
      float sum = 0.f, num = 0.f;
#pragma unroll
      for (int l = 0; l < LP; ++l)
        if (present >> l & 1) {
          const float ex = expf(A[l]);
          sum += ex;
          num += ex * E[l];
        }
      if (present) x += num / sum;
    }
    if (i < I) a.d_out[(int64_t)n * a.ld + i] = x;
  }
}

}  // namespace

extern "C" {

int nrhip_fpmcplus_step(const nrhip_fpmcplus_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "fpmcplus_step: null argument block");
  const nrhip_fpmcplus_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_FPMCPLUS_MAX_D, NR_ERR_UNSUPPORTED,
             "fpmcplus_step: embedding_size %d outside 1..%d", a.d, NRHIP_FPMCPLUS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_FPMCPLUS_MAX_W, NR_ERR_UNSUPPORTED,
             "fpmcplus_step: weight_size %d outside 1..%d", a.w, NRHIP_FPMCPLUS_MAX_W);
  NR_REQUIRE(a.L >= 1 && a.L <= NRHIP_FPMCPLUS_MAX_L, NR_ERR_UNSUPPORTED,
             "fpmcplus_step: high_order %d outside 1..%d", a.L, NRHIP_FPMCPLUS_MAX_L);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_FPMCPLUS_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + 3 * (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG,
             "fpmcplus_step: bad sizes");
  NR_TRY(check_loss_kind("fpmcplus_step", a.pairwise, a.loss_kind));
  const int B = a.batch;
  if (B == 0) return NR_OK;                                // no work: nothing is launched, nothing is written
  NR_REQUIRE(a.d_UI && a.d_IU && a.d_IL && a.d_LI && a.d_W && a.d_b && a.d_h && a.d_G_UI && a.d_G_IU && a.d_G_IL &&
                 a.d_G_LI && a.d_G_W && a.d_G_b && a.d_G_h && a.d_users && a.d_recents && a.d_items && a.d_third &&
                 a.d_keys && a.d_contrib && a.d_scal && a.d_delta && a.d_partial && a.d_loss2, NR_ERR_ARG,
             "fpmcplus_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int d = a.d, w = a.w, L = a.L, S = a.pairwise ? 2 : 1;
  const int n_keys = (1 + 2 * S + L) * B, chunks = chunks_of(B), n_el = 3 * d * w + 2 * w;
  int WP = 1;
  while (WP < w) WP <<= 1;
  const size_t lds = sizeof(float) * ((size_t)5 * d + (size_t)L * (d + 1) + (size_t)3 * L * w + 5 * w + 6 * L);
  hipLaunchKernelGGL(fpmcplus_instance_kernel, dim3(B), dim3(64), lds, st, a, WP);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(a.d_keys, n_keys, stream));
  hipLaunchKernelGGL(fpmcplus_loss_kernel, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  NR_BY_WIDTH(fpmcplus_rows_kernel, d, n_keys, st, a, n_keys);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fpmcplus_dense_kernel, dim3((n_el + 255) / 256, chunks), dim3(256), 0, st, a, chunks);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fpmcplus_reduce_kernel, dim3((n_el + 255) / 256), dim3(256), 0, st, a, chunks);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_fpmcplus_scores(const nrhip_fpmcplus_scores_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "fpmcplus_scores: null argument block");
  const nrhip_fpmcplus_scores_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_FPMCPLUS_MAX_D, NR_ERR_UNSUPPORTED,
             "fpmcplus_scores: embedding_size %d outside 1..%d", a.d, NRHIP_FPMCPLUS_MAX_D);
  NR_REQUIRE(a.w >= 1 && a.w <= NRHIP_FPMCPLUS_MAX_W, NR_ERR_UNSUPPORTED,
             "fpmcplus_scores: weight_size %d outside 1..%d", a.w, NRHIP_FPMCPLUS_MAX_W);
  NR_REQUIRE(a.L >= 1 && a.L <= NRHIP_FPMCPLUS_MAX_L, NR_ERR_UNSUPPORTED,
             "fpmcplus_scores: high_order %d outside 1..%d", a.L, NRHIP_FPMCPLUS_MAX_L);
  NR_REQUIRE(a.batch >= 0 && a.n_users >= 0 && a.n_items >= 0 && a.ld >= a.n_items, NR_ERR_ARG,
             "fpmcplus_scores: bad sizes");
  if (a.batch == 0 || a.n_items == 0) return NR_OK;
  NR_REQUIRE(a.d_UI && a.d_IU && a.d_IL && a.d_LI && a.d_W && a.d_b && a.d_h && a.d_last && a.d_users && a.d_c &&
                 a.d_p && a.d_out, NR_ERR_ARG, "fpmcplus_scores: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int d = a.d, w = a.w;
  const int64_t n_p = (int64_t)a.n_items * w, n_c = (int64_t)a.batch * a.L * w;
  hipLaunchKernelGGL(fpmcplus_item_proj_kernel, dim3((unsigned)((n_p + 255) / 256)), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fpmcplus_user_proj_kernel, dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  // a block of users per workgroup: the item tile is staged once for all of them; at most 65,535 blocks in y
  int upb = NRHIP_FPMCPLUS_SCORE_USERS;
  while ((a.batch + upb - 1) / upb > 65535) upb *= 2;
  const unsigned gy = (unsigned)((a.batch + upb - 1) / upb);
  const int TI = d <= 64 ? 64 : 32;                      // the tile's rows and p_i: (2 d + w) TI floats, at most 48 KB
  const size_t lds = sizeof(float) * (size_t)(2 * d + w) * TI;
  const dim3 grid((a.n_items + TI - 1) / TI, gy);
#define NR_FPMCPLUS_PAIRS(LP)                                                                                       \
  do {                                                                                                              \
    if (TI == 64) hipLaunchKernelGGL((fpmcplus_pairs_kernel<64, LP>), grid, dim3(256), lds, st, a, upb);            \
    else hipLaunchKernelGGL((fpmcplus_pairs_kernel<32, LP>), grid, dim3(256), lds, st, a, upb);                     \
  } while (0)
  if (a.L <= 1) NR_FPMCPLUS_PAIRS(1);
  else if (a.L <= 2) NR_FPMCPLUS_PAIRS(2);
  else if (a.L <= 4) NR_FPMCPLUS_PAIRS(4);
  else if (a.L <= 8) NR_FPMCPLUS_PAIRS(8);
  else NR_FPMCPLUS_PAIRS(16);
#undef NR_FPMCPLUS_PAIRS
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
