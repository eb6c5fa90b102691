// cfgan.hip — CFGAN (model/general_recommender/CFGAN.py): the per-epoch masks, one sess.run(trainer_d) and one
// sess.run(trainer_g) up to the optimiser, the optimiser pass that carries the regularisers, and the scorer's factors.
//
// R is the train CSR (rows = users, or items in itemBased mode), c a row of it as a 0/1 vector, n = n_cols.
//   G: c -> sigmoid layers -> out [B][n];  D: [c | y] -> sigmoid layers -> one logit.
// Neither a dense c, the [B][2 n] concatenation nor a dense mask exists.  The masks are bit rows (column 32 w + k at bit
// k of word w).  The products with an n-long dimension are nrhip_gemm_f32 (split over K where n is the contraction);
// what it cannot do is here:
//   cfgan_mask_kernel     one workgroup per (batch row, plane): the row's train columns, then a radix select over
//                         256-bin LDS histograms of the 64-bit pairs (key << 32 | column) of every other column — the
//                         n smallest are set.  The key of a column is regenerated in every pass and never stored; the
//                         pairs are distinct, so a tie of two keys falls to the lower column inside the same passes.
//                         The histogram counts are integers (LDS adds, any order gives the same counts).
//   cfgan_pool_kernel     a first layer from the CSR row: sum of the kernel's rows (+ those of its lower half for D's
//                         real branch), bias, sigmoid; for D's fake branch the pre-activation the GEMM continues from
//   cfgan_mask_apply_kernel   one pass over out and the bit planes: forward y_fake = out . pm and the row's chunk sums
//                         of out^2 . zr; backward dout = dy . pm + (2 zr_coef / B) out . zr in place of dy (dy exists
//                         only after D's backward pass, so the triple takes two launches of this kernel)
//   cfgan_head_kernel     a wavefront per row of the last hidden layer, real and fake rows in one launch: logit, loss
//                         term, its derivative, and the derivative at the layer's pre-activation
//   cfgan_head_sums_kernel    one workgroup: the loss terms in row order, the output layer's gradient
//   cfgan_dsig_kernel     d *= h (1 - h)
//   cfgan_prep_kernel     the (column << 32 | slot) keys of the batch's CSR entries, and the ones vector of the bias sums
//   cfgan_rows_kernel     a wavefront per sorted key: the head of a column's run sums its slots' derivative rows in key
//                         order into the pooled half of the first kernel's gradient (rowkey_common.h's head rule)
//   cfgan_apply_kernel    every variable of a network in one pass: g + reg v, ApplyAdam or gradient descent, the
//                         gradient cleared, sum v^2 per workgroup (cfgan_reg_kernel adds the partials in order)
// Every float sum is taken in a fixed order: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

constexpr int kChunk = 2048;                               // columns of one workgroup of cfgan_mask_apply_kernel
enum { POOL_GEN = 0, POOL_DIS_REAL = 1, POOL_DIS_FAKE = 2 };

// ---------------------------------------------------------------------------------------------------- masks
__host__ __device__ __forceinline__ uint64_t mask_base(uint64_t seed, uint64_t epoch, int plane, int row) {
  const uint64_t z = nr::splitmix64(seed ^ nr::splitmix64(epoch * 0xd1342543de82ef95ull + 0x632be59bd9b4e019ull));
  return nr::splitmix64(z ^ (((uint64_t)(uint32_t)row << 1) | (uint64_t)(plane & 1)));
}
__host__ __device__ __forceinline__ uint64_t mask_pair(uint64_t base, int col) {
  return (nr::splitmix64(base + (uint64_t)(uint32_t)col) & 0xffffffff00000000ull) | (uint64_t)(uint32_t)col;
}

__device__ __forceinline__ int lower_bound(const int32_t* a, int n, int32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the train columns of word w of a row
__device__ __forceinline__ uint32_t pos_word(const int32_t* idx, int deg, int w) {
  uint32_t bits = 0;
  for (int j = lower_bound(idx, deg, 32 * w); j < deg && idx[j] < 32 * w + 32; ++j) bits |= 1u << (idx[j] - 32 * w);
  return bits;
}
// the columns of word w that exist
__device__ __forceinline__ uint32_t valid_word(int n_cols, int w) {
  const int left = n_cols - 32 * w;
  return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : ((1u << left) - 1u));
}

__global__ __launch_bounds__(256) void cfgan_mask_kernel(const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ n_sample, int n_cols, int words,
                                                         uint64_t seed, uint64_t epoch, uint32_t* zr, uint32_t* pm) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[3];
  const int b = blockIdx.x, plane = blockIdx.y, tid = threadIdx.x;
  const int row = rows[b];
  const int64_t p0 = indptr[row];
  const int deg = (int)(indptr[row + 1] - p0);
  const int32_t* idx = indices + p0;
  uint32_t* out = (plane ? pm : zr) + (int64_t)b * words;
  for (int w = tid; w < words; w += 256) out[w] = pos_word(idx, deg, w);   // re-read below by the thread that wrote it
  int want = n_sample[2 * b + plane];
  const int free_cols = n_cols - deg;
  want = want < 0 ? 0 : (want > free_cols ? free_cols : want);
  if (want == 0) return;
  if (want == free_cols) {
    for (int w = tid; w < words; w += 256) out[w] = valid_word(n_cols, w);
    return;
  }
  const uint64_t base = mask_base(seed, epoch, plane, row);
  uint64_t prefix = 0;                                    // the leading bytes of the threshold pair found so far
  uint32_t remaining = (uint32_t)want;                    // pairs still to take among those with these leading bytes
  int shift = 56;
  for (int pass = 0; pass < 8; ++pass, shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int w = tid; w < words; w += 256) {
      uint32_t open = ~out[w] & valid_word(n_cols, w);
      while (open) {
        const int k = __ffs(open) - 1;
        open &= open - 1;
        const uint64_t pair = mask_pair(base, 32 * w + k);
        if (pass == 0 || (pair >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(pair >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t below = 0;
      int bin = 0;
      for (; bin < 255; ++bin) {
        if (below + hist[bin] >= remaining) break;
        below += hist[bin];
      }
      s_sel[0] = (uint32_t)bin;
      s_sel[1] = remaining - below;
      s_sel[2] = hist[bin];
    }
    __syncthreads();
    prefix = (prefix << 8) | s_sel[0];
    remaining = s_sel[1];
    const bool whole_bin = remaining == s_sel[2];           // the whole bin is taken: the threshold is known
    __syncthreads();
    if (whole_bin) break;
  }
  if (shift < 0) shift = 0;                                 // (all eight passes ran: the pairs are distinct, so the
                                                            // last bin held one pair and the loop left through break)
  for (int w = tid; w < words; w += 256) {
    const uint32_t have = out[w];
    uint32_t open = ~have & valid_word(n_cols, w), take = 0;
    while (open) {
      const int k = __ffs(open) - 1;
      open &= open - 1;
      if ((mask_pair(base, 32 * w + k) >> shift) <= prefix) take |= 1u << k;
    }
    out[w] = have | take;
  }
}

// ---------------------------------------------------------------------------------------------------- first layers
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void cfgan_pool_kernel(const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const int32_t* __restrict__ rows, int batch,
                                                         const float* __restrict__ W, int n_cols, int width,
                                                         const float* __restrict__ bias, int mode_base, float* out,
                                                         int64_t ld) {
  const int b = blockIdx.x, mode = mode_base + (int)blockIdx.y;
  const int row = rows ? rows[b] : b;
  const int64_t p0 = indptr[row], p1 = indptr[row + 1];
  const float* W2 = W + (int64_t)n_cols * width;
  float* dst = out + (int64_t)(mode == POOL_DIS_FAKE ? batch + b : b) * ld;
  for (int c = threadIdx.x; c < width; c += 256) {
    float top = 0.f, bot = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t i = indices[p];
      top += W[i * width + c];
      if (mode == POOL_DIS_REAL) bot += W2[i * width + c];
    }
    const float pre = (top + bot) + bias[c];
    dst[c] = mode == POOL_DIS_FAKE ? pre : sigmoidf(pre);
  }
}

// ---------------------------------------------------------------------------------------------------- the wide side
__global__ __launch_bounds__(256) void cfgan_mask_apply_kernel(const float* __restrict__ out, float* y,
                                                               const uint32_t* __restrict__ zr,
                                                               const uint32_t* __restrict__ pm, int n_cols, int words,
                                                               int chunks, int backward, float coef, float* zr_part) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const uint32_t* zrow = zr + (int64_t)b * words;
  const uint32_t* prow = pm + (int64_t)b * words;
  const float* o = out + (int64_t)b * n_cols;
  float* yy = y + (int64_t)b * n_cols;
  double v[1] = {0.0};
  float s = 0.f;
  for (int k = 0; k < kChunk / 256; ++k) {
    const int col = chunk * kChunk + k * 256 + (int)threadIdx.x;
    if (col >= n_cols) break;
    const bool z = (zrow[col >> 5] >> (col & 31)) & 1u, p = (prow[col >> 5] >> (col & 31)) & 1u;
    const float x = o[col];
    if (!backward) {
      yy[col] = p ? x : 0.f;
      if (z) s += x * x;
    } else {
      float r = p ? yy[col] : 0.f;
      if (z) r += coef * x;
      yy[col] = r;
    }
  }
  if (backward) return;
  v[0] = (double)s;
  block_sum(v);
  if (threadIdx.x == 0) zr_part[(int64_t)b * chunks + chunk] = (float)v[0];
}

// rows r0..n_rows of the last hidden layer h [n_rows][w]; rows below `batch` are D's real branch (label 1), the others
// the fake branch (label 0 in D's step, 1 in G's)
__global__ __launch_bounds__(256) void cfgan_head_kernel(const float* __restrict__ h, int w,
                                                         const float* __restrict__ w_out,
                                                         const float* __restrict__ b_out, int r0, int n_rows, int batch,
                                                         int g_step, float* loss_r, float* dl_r, float* dpre) {
  const int r = r0 + (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = nr_lane();
  if (r >= n_rows) return;
  const float* hr = h + (int64_t)r * w;
  float dot = 0.f;
  for (int k = lane; k < w; k += NR_WAVE) dot += hr[k] * w_out[k];
  const float logit = nr_wave_sum_f32(dot) + b_out[0];
  const float label = (g_step || r < batch) ? 1.0f : 0.0f, inv = 1.0f / (float)batch;
  const float dl = inv * nr::pointwise_dloss(nr::NR_POINT_CROSS_ENTROPY, label, logit);
  if (lane == 0) {
    loss_r[r] = inv * nr::pointwise_loss(nr::NR_POINT_CROSS_ENTROPY, label, logit);
    dl_r[r] = dl;
  }
  for (int k = lane; k < w; k += NR_WAVE) {
    const float a = hr[k];
    dpre[(int64_t)r * w + k] = (dl * w_out[k]) * (a * (1.0f - a));
  }
}

__global__ __launch_bounds__(256) void cfgan_head_sums_kernel(const float* __restrict__ h, int w,
                                                              const float* __restrict__ loss_r,
                                                              const float* __restrict__ dl_r,
                                                              const float* __restrict__ zr_part, int n_part, int batch,
                                                              int g_step, float zr_coef, float* loss3, float* G_w,
                                                              float* G_b) {
  double v[3] = {0.0, 0.0, 0.0};
  const int tid = threadIdx.x;
  for (int r = tid; r < batch; r += 256) {
    if (!g_step) v[0] += (double)loss_r[r];
    v[1] += (double)loss_r[batch + r];
  }
  if (g_step)
    for (int q = tid; q < n_part; q += 256) v[2] += (double)zr_part[q];
  if (!g_step) {
    for (int k = tid; k < w; k += 256) {
      float acc = 0.f;
      for (int r = 0; r < 2 * batch; ++r) acc += dl_r[r] * h[(int64_t)r * w + k];
      G_w[k] = acc;
    }
    if (tid == 0) {
      float acc = 0.f;
      for (int r = 0; r < 2 * batch; ++r) acc += dl_r[r];
      G_b[0] = acc;
    }
  }
  block_sum(v);
  if (tid == 0) {
    if (g_step) {
      loss3[0] = (float)v[1];
      loss3[2] = (float)((double)zr_coef * v[2] / (double)batch);
    } else {
      loss3[0] = (float)v[0];
      loss3[1] = (float)v[1];
    }
  }
}

__global__ __launch_bounds__(256) void cfgan_dsig_kernel(float* d, const float* __restrict__ h, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float a = h[i];
    d[i] = d[i] * (a * (1.0f - a));
  }
}

// ---------------------------------------------------------------------------------------------------- the row sums
__global__ __launch_bounds__(256) void cfgan_prep_kernel(const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const int32_t* __restrict__ rows,
                                                         const int64_t* __restrict__ ent_ptr, int batch, uint64_t* keys,
                                                         float* ones) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int row = rows[b];
  const int64_t p0 = indptr[row], e0 = ent_ptr[b];
  const int deg = (int)(ent_ptr[b + 1] - e0);
  for (int j = tid; j < deg; j += 256) keys[e0 + j] = row_key(indices[p0 + j], (uint32_t)b);
  const int g = b * 256 + tid;
  if (g < 2 * batch) ones[g] = 1.0f;
}

// top[col] = sum over the column's slots, in key order, of src_a[slot] (+ src_b[slot]); bot[col] += the sum of src_a
// alone (bot already holds the dense product's row; NULL: no such half)
__global__ __launch_bounds__(256) void cfgan_rows_kernel(const uint64_t* __restrict__ keys, int64_t n_keys, int width,
                                                         const float* __restrict__ src_a,
                                                         const float* __restrict__ src_b, float* top, float* bot) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = head_row(keys, n_keys, w), lane = nr_lane();
  if (row < 0) return;
  for (int c = lane; c < width; c += NR_WAVE) {
    float t = 0.f, u = bot ? bot[(int64_t)row * width + c] : 0.f;
    for_run(keys, n_keys, w, row, [&](uint32_t slot) {
      const float a = src_a[(int64_t)slot * width + c];
      t += src_b ? a + src_b[(int64_t)slot * width + c] : a;
      u += a;
    });
    top[(int64_t)row * width + c] = t;
    if (bot) bot[(int64_t)row * width + c] = u;
  }
}

// ---------------------------------------------------------------------------------------------------- the optimiser
struct ApplyTab {
  float* var[2 * (NRHIP_CFGAN_MAX_HIDDEN + 1)];
  float* grad[2 * (NRHIP_CFGAN_MAX_HIDDEN + 1)];
  float* m[2 * (NRHIP_CFGAN_MAX_HIDDEN + 1)];
  float* v[2 * (NRHIP_CFGAN_MAX_HIDDEN + 1)];
  int64_t off[2 * (NRHIP_CFGAN_MAX_HIDDEN + 1) + 1];
  int n;
};

__global__ __launch_bounds__(256) void cfgan_apply_kernel(ApplyTab tab, int64_t per, int sgd, float step, float omb1,
                                                          float omb2, float eps, float reg, double* partials) {
  const int64_t total = tab.off[tab.n];
  const int64_t start = (int64_t)blockIdx.x * per, end = start + per < total ? start + per : total;
  double v[1] = {0.0};
  int t = 0;
  for (int64_t i = start + threadIdx.x; i < end; i += 256) {
    while (i >= tab.off[t + 1]) ++t;
    const int64_t j = i - tab.off[t];
    float x = tab.var[t][j];
    v[0] += (double)x * (double)x;
    const float g = NR_ADD(tab.grad[t][j], NR_MUL(reg, x));
    if (sgd) {
      x = NR_SUB(x, NR_MUL(step, g));
    } else {
      float mm = tab.m[t][j], vv = tab.v[t][j];
      nr::adam_dense_tf(g, x, mm, vv, step, omb1, omb2, eps);
      tab.m[t][j] = mm;
      tab.v[t][j] = vv;
    }
    tab.var[t][j] = x;
    tab.grad[t][j] = 0.f;
  }
  block_sum(v);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void cfgan_reg_kernel(const double* __restrict__ partials, int n, float reg,
                                                        float* out) {
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += 256) v[0] += partials[i];
  block_sum(v);
  if (threadIdx.x == 0) out[0] = (float)((double)reg * 0.5 * v[0]);
}

__global__ __launch_bounds__(256) void cfgan_pairs_kernel(const float* __restrict__ F, int64_t ldf,
                                                          const float* __restrict__ Q, int64_t ldq, int width,
                                                          const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ items, int64_t n, float* out) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n) return;
  const float* f = F + (int64_t)rows[e] * ldf;
  const float* q = Q + (int64_t)items[e] * ldq;
  float dot = 0.f;
  for (int k = nr_lane(); k < width; k += NR_WAVE) dot += f[k] * q[k];
  dot = nr_wave_sum_f32(dot);
  if (nr_lane() == 0) out[e] = dot;
}

// ---------------------------------------------------------------------------------------------------- host side
int check_net(const char* entry, const nrhip_cfgan_net& n, bool pointers) {
  NR_REQUIRE(n.n_hidden >= 1 && n.n_hidden <= NRHIP_CFGAN_MAX_HIDDEN, NR_ERR_UNSUPPORTED,
             "%s: %d hidden layers are not supported (1 to %d)", entry, n.n_hidden, NRHIP_CFGAN_MAX_HIDDEN);
  for (int k = 0; k < n.n_hidden; ++k)
    NR_REQUIRE(n.width[k] >= 1 && n.width[k] <= NRHIP_CFGAN_MAX_WIDTH, NR_ERR_UNSUPPORTED,
               "%s: a hidden layer of %d units is not supported (1 to %d)", entry, n.width[k], NRHIP_CFGAN_MAX_WIDTH);
  if (pointers)
    for (int k = 0; k <= n.n_hidden; ++k)
      NR_REQUIRE(n.d_W[k] && n.d_b[k], NR_ERR_ARG, "%s: layer %d has a null kernel or bias", entry, k);
  return NR_OK;
}

int splits_for(int K) { return K <= 1024 ? 1 : (K / 512 > 32 ? 32 : K / 512); }

// the layout of d_ws for one batch size (floats)
struct Layout {
  size_t hG[NRHIP_CFGAN_MAX_HIDDEN], dG[NRHIP_CFGAN_MAX_HIDDEN], hD[NRHIP_CFGAN_MAX_HIDDEN], dD[NRHIP_CFGAN_MAX_HIDDEN];
  size_t out, y, loss_r, dl_r, ones, zr_part, total;
  int chunks;
};
Layout layout_of(const nrhip_cfgan_step_args& a, int B) {
  Layout L;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
  for (int k = 0; k < a.gen.n_hidden; ++k) { L.hG[k] = take((size_t)B * a.gen.width[k]); L.dG[k] = take((size_t)B * a.gen.width[k]); }
  for (int k = 0; k < a.dis.n_hidden; ++k) { L.hD[k] = take((size_t)2 * B * a.dis.width[k]); L.dD[k] = take((size_t)2 * B * a.dis.width[k]); }
  L.out = take((size_t)B * a.n_cols);
  L.y = take((size_t)B * a.n_cols);
  L.loss_r = take((size_t)2 * B);
  L.dl_r = take((size_t)2 * B);
  L.ones = take((size_t)2 * B);
  L.chunks = (a.n_cols + kChunk - 1) / kChunk;
  L.zr_part = take((size_t)B * L.chunks);
  L.total = at;
  return L;
}

int gemm_bytes_for(const nrhip_cfgan_step_args& a, int B, size_t* bytes) {
  size_t need = 0, n = 0;
  const int s = splits_for(a.n_cols);
  NR_TRY(nrhip_gemm_workspace_bytes(B, a.dis.width[0], s, &n));
  need = n > need ? n : need;
  NR_TRY(nrhip_gemm_workspace_bytes(B, a.gen.width[a.gen.n_hidden - 1], s, &n));
  need = n > need ? n : need;
  *bytes = need;
  return NR_OK;
}

int check_step(const char* entry, const nrhip_cfgan_step_args& a) {
  NR_TRY(check_net(entry, a.gen, true));
  NR_TRY(check_net(entry, a.dis, true));
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_CFGAN_MAX_BATCH && a.max_batch >= a.batch, NR_ERR_UNSUPPORTED,
             "%s: a batch of %d rows is not supported (up to %d, and the workspace's %d)", entry, a.batch,
             NRHIP_CFGAN_MAX_BATCH, a.max_batch);
  NR_REQUIRE(a.n_cols >= 1 && a.n_cols < (1 << 24), NR_ERR_UNSUPPORTED, "%s: n_cols=%d is not supported (1 to 2^24 - 1)",
             entry, a.n_cols);
  NR_REQUIRE(a.n_ent >= 0 && a.n_ent <= (1 << 30), NR_ERR_UNSUPPORTED, "%s: %d batch entries are not supported", entry,
             a.n_ent);
  NR_REQUIRE(a.batch == 0 || (a.d_indptr && a.d_indices && a.d_rows && a.d_ent_ptr && a.d_zr && a.d_pm && a.d_ws &&
                              a.d_loss3 && (a.n_ent == 0 || a.d_keys)),
             NR_ERR_ARG, "%s: null argument", entry);
  size_t need = 0;
  if (a.batch > 0) NR_TRY(gemm_bytes_for(a, a.batch, &need));
  NR_REQUIRE(need == 0 || (a.d_gemm_ws && a.gemm_ws_bytes >= need), NR_ERR_WORKSPACE,
             "%s: the GEMM workspace holds %zu bytes, %zu needed", entry, a.gemm_ws_bytes, need);
  return NR_OK;
}

// C [M][N] = act(A [M][K] B [K][N] + bias): a dense layer on row-major activations
int dense_fwd(const float* x, int M, int K, const float* W, const float* bias, int N, float* y, int64_t ldy, int act,
              void* stream) {
  return nrhip_gemm_f32(x, K, 1, W, N, 0, M, N, K, y, ldy, 0, bias, act, 1, nullptr, 0, stream);
}

// G's hidden layers on the batch rows: h[k] [B][width[k]]
int gen_hidden(const nrhip_cfgan_net& g, const int64_t* indptr, const int32_t* indices, const int32_t* rows, int B,
               int n_cols, float* const* h, const int64_t* ld, hipStream_t st) {
  hipLaunchKernelGGL(cfgan_pool_kernel, dim3((unsigned)B, 1), dim3(256), 0, st, indptr, indices, rows, B,
                     (const float*)g.d_W[0], n_cols, g.width[0], (const float*)g.d_b[0], (int)POOL_GEN, h[0], ld[0]);
  NR_LAUNCH_CHECK();
  for (int k = 1; k < g.n_hidden; ++k)
    NR_TRY(nrhip_gemm_f32(h[k - 1], ld[k - 1], 1, g.d_W[k], g.width[k], 0, B, g.width[k], g.width[k - 1], h[k], ld[k], 0,
                          g.d_b[k], 1, 1, nullptr, 0, st));
  return NR_OK;
}

// the hidden layers' backward pass from d[last] (at the pre-activation) down to d[0]; rows r0.. of n_rows; with
// `grads` the kernels' and biases' gradients of layers 1..last over ALL n_rows rows (r0 must be 0 then)
int hidden_bwd(const nrhip_cfgan_net& net, float* const* h, float* const* d, int r0, int n_rows, bool grads,
               const float* ones, hipStream_t st) {
  for (int k = net.n_hidden - 1; k >= 1; --k) {
    const int wi = net.width[k - 1], wo = net.width[k], M = n_rows - r0;
    if (grads) {
      NR_TRY(nrhip_gemm_f32(h[k - 1], wi, 0, d[k], wo, 0, wi, wo, n_rows, net.d_G_W[k], wo, 0, nullptr, -1, 1, nullptr, 0,
                            st));
      NR_TRY(nrhip_gemm_f32(ones, 1, 0, d[k], wo, 0, 1, wo, n_rows, net.d_G_b[k], wo, 0, nullptr, -1, 1, nullptr, 0, st));
    }
    float* dk = d[k - 1] + (int64_t)r0 * wi;
    NR_TRY(nrhip_gemm_f32(d[k] + (int64_t)r0 * wo, wo, 1, net.d_W[k], wo, 1, M, wi, wo, dk, wi, 0, nullptr, -1, 1, nullptr,
                          0, st));
    const int64_t n = (int64_t)M * wi;
    hipLaunchKernelGGL(cfgan_dsig_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dk,
                       (const float*)(h[k - 1] + (int64_t)r0 * wi), n);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int step(const nrhip_cfgan_step_args& a, int g_step, void* stream) {
  const char* entry = g_step ? "cfgan_g_step" : "cfgan_d_step";
  NR_TRY(check_step(entry, a));
  if (a.batch == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int B = a.batch, n = a.n_cols, words = (n + 31) / 32;
  const nrhip_cfgan_net& G = a.gen;
  const nrhip_cfgan_net& D = a.dis;
  const int LG = G.n_hidden, LD = D.n_hidden, gl = G.width[LG - 1], e1 = D.width[0], el = D.width[LD - 1];
  const Layout L = layout_of(a, B);
  float *hG[NRHIP_CFGAN_MAX_HIDDEN], *dG[NRHIP_CFGAN_MAX_HIDDEN], *hD[NRHIP_CFGAN_MAX_HIDDEN], *dD[NRHIP_CFGAN_MAX_HIDDEN];
  int64_t ldG[NRHIP_CFGAN_MAX_HIDDEN];
  for (int k = 0; k < LG; ++k) { hG[k] = a.d_ws + L.hG[k]; dG[k] = a.d_ws + L.dG[k]; ldG[k] = G.width[k]; }
  for (int k = 0; k < LD; ++k) { hD[k] = a.d_ws + L.hD[k]; dD[k] = a.d_ws + L.dD[k]; }
  float *out = a.d_ws + L.out, *y = a.d_ws + L.y, *loss_r = a.d_ws + L.loss_r, *dl_r = a.d_ws + L.dl_r;
  float *ones = a.d_ws + L.ones, *zr_part = a.d_ws + L.zr_part;
  const int ksplit = splits_for(n);
  const float* Wd_bot = D.d_W[0] + (int64_t)n * e1;         // the kernel rows that meet y
  const int r0 = g_step ? B : 0;                             // G's step needs the fake branch alone

  hipLaunchKernelGGL(cfgan_prep_kernel, dim3((unsigned)B), dim3(256), 0, st, a.d_indptr, a.d_indices, a.d_rows,
                     a.d_ent_ptr, B, a.d_keys, ones);
  NR_LAUNCH_CHECK();
  if (a.n_ent > 0) NR_TRY(nrhip_sort_u64(a.d_keys, a.n_ent, stream));

  // G forward, y_fake = out . pm and the zero-reconstruction sums
  NR_TRY(gen_hidden(G, a.d_indptr, a.d_indices, a.d_rows, B, n, hG, ldG, st));
  NR_TRY(dense_fwd(hG[LG - 1], B, gl, G.d_W[LG], G.d_b[LG], n, out, n, -1, stream));
  hipLaunchKernelGGL(cfgan_mask_apply_kernel, dim3((unsigned)L.chunks, (unsigned)B), dim3(256), 0, st, (const float*)out,
                     y, a.d_zr, a.d_pm, n, words, L.chunks, 0, 0.f, zr_part);
  NR_LAUNCH_CHECK();

  // D forward: rows [0, B) see [c | c], rows [B, 2 B) see [c | y_fake]
  hipLaunchKernelGGL(cfgan_pool_kernel, dim3((unsigned)B, g_step ? 1u : 2u), dim3(256), 0, st, a.d_indptr, a.d_indices,
                     a.d_rows, B, (const float*)D.d_W[0], n, e1, (const float*)D.d_b[0],
                     (int)(g_step ? POOL_DIS_FAKE : POOL_DIS_REAL), hD[0], (int64_t)e1);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_gemm_f32(y, n, 1, Wd_bot, e1, 0, B, e1, n, hD[0] + (int64_t)B * e1, e1, 1, nullptr, 1, ksplit, a.d_gemm_ws,
                        a.gemm_ws_bytes, stream));
  for (int k = 1; k < LD; ++k)
    NR_TRY(dense_fwd(hD[k - 1] + (int64_t)r0 * D.width[k - 1], 2 * B - r0, D.width[k - 1], D.d_W[k], D.d_b[k], D.width[k],
                     hD[k] + (int64_t)r0 * D.width[k], D.width[k], 1, stream));
  hipLaunchKernelGGL(cfgan_head_kernel, dim3((unsigned)((2 * B - r0 + 3) / 4)), dim3(256), 0, st,
                     (const float*)hD[LD - 1], el, (const float*)D.d_W[LD], (const float*)D.d_b[LD], r0, 2 * B, B, g_step,
                     loss_r, dl_r, dD[LD - 1]);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cfgan_head_sums_kernel, dim3(1), dim3(256), 0, st, (const float*)hD[LD - 1], el,
                     (const float*)loss_r, (const float*)dl_r, (const float*)zr_part, B * L.chunks, B, g_step, a.zr_coef,
                     a.d_loss3, D.d_G_W[LD], D.d_G_b[LD]);
  NR_LAUNCH_CHECK();
  NR_TRY(hidden_bwd(D, hD, dD, r0, 2 * B, !g_step, ones, st));

  if (!g_step) {
    // D's first layer: the bias, the dense half y_fake^T dpre_fake, then the pooled rows along the sorted keys
    NR_TRY(nrhip_gemm_f32(ones, 1, 0, dD[0], e1, 0, 1, e1, 2 * B, D.d_G_b[0], e1, 0, nullptr, -1, 1, nullptr, 0, stream));
    float* G_bot = D.d_G_W[0] + (int64_t)n * e1;
    NR_TRY(nrhip_gemm_f32(y, n, 0, dD[0] + (int64_t)B * e1, e1, 0, n, e1, B, G_bot, e1, 0, nullptr, -1, 1, nullptr, 0,
                          stream));
    if (a.n_ent > 0) {
      hipLaunchKernelGGL(cfgan_rows_kernel, dim3((unsigned)((a.n_ent + 3) / 4)), dim3(256), 0, st,
                         (const uint64_t*)a.d_keys, (int64_t)a.n_ent, e1, (const float*)dD[0],
                         (const float*)(dD[0] + (int64_t)B * e1), D.d_G_W[0], G_bot);
      NR_LAUNCH_CHECK();
    }
    return NR_OK;
  }

  // G's step: dy = dpre_fake Wd1[n:]^T (in place of y_fake), dout = dy . pm + (2 zr_coef / B) out . zr
  NR_TRY(nrhip_gemm_f32(dD[0] + (int64_t)B * e1, e1, 1, Wd_bot, e1, 1, B, n, e1, y, n, 0, nullptr, -1, 1, nullptr, 0,
                        stream));
  hipLaunchKernelGGL(cfgan_mask_apply_kernel, dim3((unsigned)L.chunks, (unsigned)B), dim3(256), 0, st, (const float*)out,
                     y, a.d_zr, a.d_pm, n, words, L.chunks, 1, 2.0f * a.zr_coef / (float)B, zr_part);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_gemm_f32(hG[LG - 1], gl, 0, y, n, 0, gl, n, B, G.d_G_W[LG], n, 0, nullptr, -1, 1, nullptr, 0, stream));
  NR_TRY(nrhip_gemm_f32(ones, 1, 0, y, n, 0, 1, n, B, G.d_G_b[LG], n, 0, nullptr, -1, 1, nullptr, 0, stream));
  NR_TRY(nrhip_gemm_f32(y, n, 1, G.d_W[LG], n, 1, B, gl, n, dG[LG - 1], gl, 0, nullptr, -1, ksplit, a.d_gemm_ws,
                        a.gemm_ws_bytes, stream));
  {
    const int64_t cnt = (int64_t)B * gl;
    hipLaunchKernelGGL(cfgan_dsig_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, dG[LG - 1],
                       (const float*)hG[LG - 1], cnt);
    NR_LAUNCH_CHECK();
  }
  NR_TRY(hidden_bwd(G, hG, dG, 0, B, true, ones, st));
  NR_TRY(nrhip_gemm_f32(ones, 1, 0, dG[0], G.width[0], 0, 1, G.width[0], B, G.d_G_b[0], G.width[0], 0, nullptr, -1, 1,
                        nullptr, 0, stream));
  if (a.n_ent > 0) {
    hipLaunchKernelGGL(cfgan_rows_kernel, dim3((unsigned)((a.n_ent + 3) / 4)), dim3(256), 0, st,
                       (const uint64_t*)a.d_keys, (int64_t)a.n_ent, G.width[0], (const float*)dG[0],
                       (const float*)nullptr, G.d_G_W[0], (float*)nullptr);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_cfgan_workspace(const nrhip_cfgan_step_args* shape, size_t* floats, size_t* gemm_bytes) {
  NR_REQUIRE(shape && floats && gemm_bytes, NR_ERR_ARG, "cfgan_workspace: null argument");
  const nrhip_cfgan_step_args& a = *shape;
  NR_TRY(check_net("cfgan_workspace", a.gen, false));
  NR_TRY(check_net("cfgan_workspace", a.dis, false));
  NR_REQUIRE(a.max_batch >= 0 && a.max_batch <= NRHIP_CFGAN_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "cfgan_workspace: a batch of %d rows is not supported (up to %d)", a.max_batch, NRHIP_CFGAN_MAX_BATCH);
  NR_REQUIRE(a.n_cols >= 1 && a.n_cols < (1 << 24), NR_ERR_UNSUPPORTED,
             "cfgan_workspace: n_cols=%d is not supported (1 to 2^24 - 1)", a.n_cols);
  const int B = a.max_batch > 0 ? a.max_batch : 1;
  *floats = layout_of(a, B).total;
  return gemm_bytes_for(a, B, gemm_bytes);
}

int nrhip_cfgan_masks(const int64_t* d_indptr, const int32_t* d_indices, const int32_t* d_rows,
                      const int32_t* d_n_sample, int batch, int n_rows, int n_cols, uint64_t seed, uint64_t epoch,
                      uint32_t* d_zr, uint32_t* d_pm, void* stream) {
  NR_REQUIRE(batch >= 0 && batch <= 65535 && n_rows >= 0 && n_cols >= 1 && n_cols < (1 << 24), NR_ERR_UNSUPPORTED,
             "cfgan_masks: batch=%d (up to 65535) or n_cols=%d (1 to 2^24 - 1) is not supported", batch, n_cols);
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_indptr && d_indices && d_rows && d_n_sample && d_zr && d_pm, NR_ERR_ARG, "cfgan_masks: null argument");
  hipLaunchKernelGGL(cfgan_mask_kernel, dim3((unsigned)batch, 2), dim3(256), 0, (hipStream_t)stream, d_indptr, d_indices,
                     d_rows, d_n_sample, n_cols, (n_cols + 31) / 32, seed, epoch, d_zr, d_pm);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_cfgan_d_step(const nrhip_cfgan_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "cfgan_d_step: null argument block");
  return step(*args, 0, stream);
}

int nrhip_cfgan_g_step(const nrhip_cfgan_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "cfgan_g_step: null argument block");
  return step(*args, 1, stream);
}

int nrhip_cfgan_apply(const nrhip_cfgan_net* net, int n_in, int n_out, int sgd, float step, float beta1, float beta2,
                      float eps, float reg, double* d_partials, float* d_reg_loss, void* stream) {
  NR_REQUIRE(net && d_partials && d_reg_loss && n_in >= 1 && n_out >= 1, NR_ERR_ARG, "cfgan_apply: bad arguments");
  NR_TRY(check_net("cfgan_apply", *net, true));
  ApplyTab tab;
  tab.n = 0;
  tab.off[0] = 0;
  int in = n_in;
  for (int k = 0; k <= net->n_hidden; ++k) {
    const int outw = k < net->n_hidden ? net->width[k] : n_out;
    const int64_t sizes[2] = {(int64_t)in * outw, (int64_t)outw};
    float* const vars[2] = {net->d_W[k], net->d_b[k]};
    float* const grads[2] = {net->d_G_W[k], net->d_G_b[k]};
    float* const ms[2] = {net->d_m_W[k], net->d_m_b[k]};
    float* const vs[2] = {net->d_v_W[k], net->d_v_b[k]};
    for (int j = 0; j < 2; ++j) {
      NR_REQUIRE(grads[j] && (sgd || (ms[j] && vs[j])), NR_ERR_ARG, "cfgan_apply: layer %d lacks a gradient or a moment",
                 k);
      tab.var[tab.n] = vars[j];
      tab.grad[tab.n] = grads[j];
      tab.m[tab.n] = ms[j];
      tab.v[tab.n] = vs[j];
      tab.off[tab.n + 1] = tab.off[tab.n] + sizes[j];
      ++tab.n;
    }
    in = outw;
  }
  const int64_t total = tab.off[tab.n];
  int64_t per = (total + NRHIP_CFGAN_APPLY_BLOCKS - 1) / NRHIP_CFGAN_APPLY_BLOCKS;
  per = (per + 1023) / 1024 * 1024;
  const int blocks = (int)((total + per - 1) / per);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cfgan_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, tab, per, sgd, step, 1.0f - beta1,
                     1.0f - beta2, eps, reg, d_partials);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cfgan_reg_kernel, dim3(1), dim3(256), 0, st, (const double*)d_partials, blocks, reg, d_reg_loss);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_cfgan_hidden(const nrhip_cfgan_net* net, const int64_t* d_indptr, const int32_t* d_indices,
                       const int32_t* d_rows, int batch, int n_cols, float* d_tmp, float* d_out, int64_t ld,
                       void* stream) {
  NR_REQUIRE(net, NR_ERR_ARG, "cfgan_hidden: null argument");
  NR_TRY(check_net("cfgan_hidden", *net, true));
  const int L = net->n_hidden;
  NR_REQUIRE(batch >= 0 && n_cols >= 1 && ld >= net->width[L - 1], NR_ERR_ARG, "cfgan_hidden: bad arguments");
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_indptr && d_indices && d_out && (L == 1 || d_tmp), NR_ERR_ARG, "cfgan_hidden: null argument");
  float* h[NRHIP_CFGAN_MAX_HIDDEN];
  int64_t lds[NRHIP_CFGAN_MAX_HIDDEN];
  for (int k = 0; k < L; ++k) {
    h[k] = k == L - 1 ? d_out : d_tmp + (size_t)(k & 1) * batch * NRHIP_CFGAN_MAX_WIDTH;
    lds[k] = k == L - 1 ? ld : net->width[k];
  }
  return gen_hidden(*net, d_indptr, d_indices, d_rows, batch, n_cols, h, lds, (hipStream_t)stream);
}

int nrhip_cfgan_pairs(const float* d_F, int64_t ldf, const float* d_Q, int64_t ldq, int width, const int32_t* d_rows,
                      const int32_t* d_items, int64_t n, float* d_out, void* stream) {
  NR_REQUIRE(n >= 0 && width >= 0 && ldf >= width && ldq >= width, NR_ERR_ARG, "cfgan_pairs: bad arguments");
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_F && d_Q && d_rows && d_items && d_out, NR_ERR_ARG, "cfgan_pairs: null argument");
  hipLaunchKernelGGL(cfgan_pairs_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_F, ldf, d_Q,
                     ldq, width, d_rows, d_items, n, d_out);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
