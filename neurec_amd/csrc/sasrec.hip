// sasrec.hip — the SASRec step (model/sequential_recommender/SASRec.py:311-383 up to the optimiser) and its
// evaluation-mode forward pass, fp32, as a chain of plain-FMA kernels over the batch's R = B L rows.
//
// The graph is computed in the reference's FULL form: padded positions are rows like any other (x = 0, so K = bk,
// V = bv, q = ln1's beta), every mask is evaluated as the reference writes it (key mask from sum(keys) == 0, the lower
// triangle, the query mask from sum(q) == 0, the row mask at each block's end, is_target), and a query none of whose
// keys is visible gets the uniform softmax over all L keys that -2**32 + 1 in every logit gives.  Nothing is special-cased
// on "real suffix" grounds, so whatever the reference computes for odd inputs (a real row that dropout zeroed, a target
// at a padded position) is computed here too.  Masked logits are not formed: their softmax weight is exactly 0 whenever
// one key is visible (exp(-2**32 + 1 - max) underflows for any |max| < 2**31).
//
//   sas_prep_kernel      1 / sum(is_target) of the batch (0 when there is none: every gradient is then exactly 0)
//   sas_embed_kernel     x = (item_emb[seq] sqrt(d) + pos_emb[t]) drop * rowmask; the (item << 32 | slot) keys
//   sas_ln_kernel        one wavefront per row: biased variance, (x - mean) / sqrt(var + 1e-8), gamma . + beta;
//                        optional flags sum(in) != 0, sum(out) != 0
//   sas_linear_kernel    out = in W + b with the three epilogues of the graph (plain; ReLU, dropout; dropout, + residual,
//                        * rowmask)
//   sas_softmax_kernel   one thread per (head, query): the masked softmax row P[L]
//   sas_attnout_kernel   Y = (P qm drop) V per head + q
//   sas_loss_kernel      one wavefront per row: the two logits, the loss term, dz, and the item rows' gradient slots
//   ... and the mirror of each for the backward pass; weight, bias and layer-norm gradients as per-chunk partial sums
//   over rows (sas_wgrad_kernel, sas_lnparam_kernel) added in chunk order by sas_reduce_kernel; the item table's
//   gradient from its 3 R slots (sequence, positive, negative occurrences) by sorted keys and gru_rows_kernel
//   (gru4rec_cell.h).  One thread per output, one ascending fmaf chain per output, no atomics: two calls on the same
//   inputs are bit-identical.
#include "gru4rec_cell.h"

namespace {

constexpr int kNB = NRHIP_SASREC_MAX_BLOCKS;
constexpr int kD = NRHIP_SASREC_MAX_WIDTH;
constexpr int kLen = NRHIP_SASREC_MAX_LEN;
constexpr int kB = NRHIP_SASREC_MAX_BATCH;
constexpr int kChunks = 128;                     // row chunks of the weight-gradient partials
enum { P_LN1B = 0, P_LN1G, P_WQ, P_BQ, P_WK, P_BK, P_WV, P_BV, P_LN2B, P_LN2G, P_W1, P_B1, P_W2, P_B2 };
enum { EPI_PLAIN = 0, EPI_RELU_DROP = 1, EPI_DROP_RES = 2 };
enum { BWD_STORE = 0, BWD_ADD = 1, BWD_RELU_DROP = 2, BWD_ADD_MASKED = 3 };

struct Drop {                                    // the dropout of a step: given masks, or the counter-based generator
  const uint8_t* mask[1 + 3 * kNB];
  uint64_t seed;
  int step;
  int on;                                        // 0: evaluation, or rate 0 without masks
  float keep;                                    // 1 - rate
  float inv_keep;
};

// splitmix64 over (seed, step, site, element): a uniform in [0, 1) from the top 24 bits
__device__ __forceinline__ float drop_uniform(uint64_t seed, int step, int site, int64_t idx) {
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * ((uint64_t)(uint32_t)step * 64u + (uint64_t)site + 1u);
  z ^= (uint64_t)idx * 0xd1342543de82ef95ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}
// mask / (1 - rate) of one element of a site
__device__ __forceinline__ float drop_factor(const Drop& dr, int site, int64_t idx) {
  if (!dr.on) return 1.0f;
  const uint8_t* m = dr.mask[site];
  const bool kept = m ? m[idx] != 0 : drop_uniform(dr.seed, dr.step, site, idx) < dr.keep;
  return kept ? dr.inv_keep : 0.0f;
}

__global__ __launch_bounds__(256) void sas_prep_kernel(const int32_t* __restrict__ pos, int64_t R, int n_items,
                                                       float* __restrict__ hdr) {
  __shared__ int part[256];
  int c = 0;
  for (int64_t r = threadIdx.x; r < R; r += 256) c += pos[r] != n_items;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hdr[0] = (float)part[0];
    hdr[1] = part[0] > 0 ? 1.0f / (float)part[0] : 0.0f;
  }
}

__device__ __forceinline__ bool real_item(int id, int n_items) { return id >= 0 && id < n_items; }

__global__ __launch_bounds__(256) void sas_embed_kernel(const float* __restrict__ item, const float* __restrict__ pe,
                                                        const int32_t* __restrict__ seq, const int32_t* __restrict__ pos,
                                                        const int32_t* __restrict__ neg, int n_items, int64_t R, int L,
                                                        int d, float sd, Drop dr, float* __restrict__ x,
                                                        uint64_t* __restrict__ keys) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int c = (int)(idx - r * d), t = (int)(r % L);
  const int id = seq[r];
  const bool real = real_item(id, n_items);
  float v = 0.0f;
  if (real) v = __builtin_fmaf(item[(int64_t)id * d + c], sd, pe[(int64_t)t * d + c]) * drop_factor(dr, 0, idx);
  x[idx] = v;
  if (c == 0 && keys) {
    keys[r] = real ? ((uint64_t)(uint32_t)id << 32) | (uint64_t)r : kSentinel;
    const int ip = pos[r], in = neg[r];
    keys[R + r] = real_item(ip, n_items) ? ((uint64_t)(uint32_t)ip << 32) | (uint64_t)(R + r) : kSentinel;
    keys[2 * R + r] = real_item(in, n_items) ? ((uint64_t)(uint32_t)in << 32) | (uint64_t)(2 * R + r) : kSentinel;
  }
}

// one wavefront per row (d <= 128: lanes hold columns lane and lane + 64)
__global__ __launch_bounds__(256) void sas_ln_kernel(const float* __restrict__ in, const float* __restrict__ beta,
                                                     const float* __restrict__ gamma, int64_t R, int d,
                                                     float* __restrict__ xh, float* __restrict__ rstd,
                                                     float* __restrict__ out, float* __restrict__ in_nonzero,
                                                     float* __restrict__ out_nonzero) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const bool h0 = lane < d, h1 = lane + 64 < d;
  const float a0 = h0 ? in[r * d + lane] : 0.0f, a1 = h1 ? in[r * d + lane + 64] : 0.0f;
  const float sum = nr_wave_sum_f32(a0 + a1);
  const float mean = sum / (float)d;
  const float c0 = h0 ? a0 - mean : 0.0f, c1 = h1 ? a1 - mean : 0.0f;
  const float var = nr_wave_sum_f32(c0 * c0 + c1 * c1) / (float)d;
  const float rs = 1.0f / sqrtf(var + 1e-8f);
  float o0 = 0.0f, o1 = 0.0f;
  if (h0) {
    const float n = c0 * rs;
    o0 = __builtin_fmaf(gamma[lane], n, beta[lane]);
    xh[r * d + lane] = n;
    out[r * d + lane] = o0;
  }
  if (h1) {
    const float n = c1 * rs;
    o1 = __builtin_fmaf(gamma[lane + 64], n, beta[lane + 64]);
    xh[r * d + lane + 64] = n;
    out[r * d + lane + 64] = o1;
  }
  const float osum = nr_wave_sum_f32(o0 + o1);
  if (lane == 0) {
    rstd[r] = rs;
    if (in_nonzero) in_nonzero[r] = sum != 0.0f ? 1.0f : 0.0f;
    if (out_nonzero) out_nonzero[r] = osum != 0.0f ? 1.0f : 0.0f;
  }
}

// out[r][j] = epilogue(sum_k in[r][k] W[k][j] + b[j])
__global__ __launch_bounds__(256) void sas_linear_kernel(const float* __restrict__ in, const float* __restrict__ W,
                                                         const float* __restrict__ b, int64_t R, int d, int epi, Drop dr,
                                                         int site, float* __restrict__ pre, const float* __restrict__ res,
                                                         const int32_t* __restrict__ seq, int n_items,
                                                         float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int j = (int)(idx - r * d);
  const float* row = in + r * d;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < d; ++k) acc = __builtin_fmaf(row[k], W[(int64_t)k * d + j], acc);
  acc += b[j];
  if (epi == EPI_RELU_DROP) {
    pre[idx] = acc;
    acc = fmaxf(acc, 0.0f) * drop_factor(dr, site, idx);
  } else if (epi == EPI_DROP_RES) {
    acc = acc * drop_factor(dr, site, idx) + res[idx];
    if (!real_item(seq[r], n_items)) acc = 0.0f;
  }
  out[idx] = acc;
}

// one thread per (head-major row hb = hd B + b, query i): P[hb][i][0..L)
__global__ __launch_bounds__(256) void sas_softmax_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                          const float* __restrict__ kvis, int B, int L, int d, int h,
                                                          float* __restrict__ P) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)h * B * L) return;
  const int i = (int)(idx % L);
  const int64_t hb = idx / L;
  const int b = (int)(hb % B), hd = (int)(hb / B);
  const int dh = d / h;
  const float scale = 1.0f / sqrtf((float)dh);
  const float* q = Q + ((int64_t)b * L + i) * d + hd * dh;
  float* p = P + idx * L;
  float mx = -__builtin_huge_valf();
  int seen = 0;
  for (int j = 0; j <= i; ++j) {
    if (kvis[(int64_t)b * L + j] == 0.0f) continue;
    const float* k = K + ((int64_t)b * L + j) * d + hd * dh;
    float s = 0.0f;
    for (int c = 0; c < dh; ++c) s = __builtin_fmaf(q[c], k[c], s);
    s *= scale;
    p[j] = s;
    mx = fmaxf(mx, s);
    ++seen;
  }
  if (!seen) {                                   // every logit is the padding value: uniform over all L keys
    const float u = 1.0f / (float)L;
    for (int j = 0; j < L; ++j) p[j] = u;
    return;
  }
  float den = 0.0f;
  for (int j = 0; j <= i; ++j) {
    if (kvis[(int64_t)b * L + j] == 0.0f) continue;
    const float e = expf(p[j] - mx);
    p[j] = e;
    den += e;
  }
  for (int j = 0; j < L; ++j) p[j] = (j <= i && kvis[(int64_t)b * L + j] != 0.0f) ? p[j] / den : 0.0f;
}

// the dropped, query-masked weight the graph multiplies V with
__device__ __forceinline__ float attn_weight(const float* __restrict__ P, const Drop& dr, int site, int64_t hb, int i,
                                             int j, int L, float qm) {
  const int64_t e = (hb * L + i) * L + j;
  return P[e] * qm * drop_factor(dr, site, e);
}

// Y[r][c] = sum_j W[hb][i][j] V[b][j][c] + q[r][c]
__global__ __launch_bounds__(256) void sas_attnout_kernel(const float* __restrict__ P, const float* __restrict__ V,
                                                          const float* __restrict__ qn, const float* __restrict__ qm,
                                                          int B, int L, int d, int h, Drop dr, int site,
                                                          float* __restrict__ Y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t R = (int64_t)B * L;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int c = (int)(idx - r * d), b = (int)(r / L), i = (int)(r % L);
  const int hd = c / (d / h);
  const int64_t hb = (int64_t)hd * B + b;
  const float m = qm[r];
  float acc = 0.0f;
  for (int j = 0; j < L; ++j) {
    const float w = attn_weight(P, dr, site, hb, i, j, L, m);
    if (w != 0.0f) acc = __builtin_fmaf(w, V[((int64_t)b * L + j) * d + c], acc);
  }
  Y[idx] = acc + qn[idx];
}

// one wavefront per row: logits, loss term, dz, and the positive / negative slots of the item gradient
__global__ __launch_bounds__(256) void sas_loss_kernel(const float* __restrict__ item, const float* __restrict__ z,
                                                       const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                       int n_items, int64_t R, int d, float sd,
                                                       const float* __restrict__ hdr, float* __restrict__ term,
                                                       float* __restrict__ dz, float* __restrict__ src) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int ip = pos[r], in = neg[r];
  const bool rp = real_item(ip, n_items), rn = real_item(in, n_items);
  const bool h0 = lane < d, h1 = lane + 64 < d;
  const float z0 = h0 ? z[r * d + lane] : 0.0f, z1 = h1 ? z[r * d + lane + 64] : 0.0f;
  const float p0 = (rp && h0) ? item[(int64_t)ip * d + lane] * sd : 0.0f;
  const float p1 = (rp && h1) ? item[(int64_t)ip * d + lane + 64] * sd : 0.0f;
  const float n0 = (rn && h0) ? item[(int64_t)in * d + lane] * sd : 0.0f;
  const float n1 = (rn && h1) ? item[(int64_t)in * d + lane + 64] * sd : 0.0f;
  const float lp = nr_wave_sum_f32(__builtin_fmaf(p0, z0, p1 * z1));
  const float ln = nr_wave_sum_f32(__builtin_fmaf(n0, z0, n1 * z1));
  const float it = ip != n_items ? 1.0f : 0.0f;
  const float sp = sigmoidf_(lp), sn = sigmoidf_(ln);
  // -log(sigmoid(p) + 1e-24) - log(1 - sigmoid(n) + 1e-24), as written (SASRec.py:373-374)
  const float a = sp + 1e-24f, c = (1.0f - sn) + 1e-24f;
  const float inv_T = hdr[1];
  const float dp = -(sp * (1.0f - sp)) / a * it * inv_T;
  const float dn = (sn * (1.0f - sn)) / c * it * inv_T;
  if (lane == 0) term[r] = (-logf(a) - logf(c)) * it;
  if (h0) {
    dz[r * d + lane] = __builtin_fmaf(dp, p0, dn * n0);
    src[(R + r) * d + lane] = dp * z0 * sd;
    src[(2 * R + r) * d + lane] = dn * z0 * sd;
  }
  if (h1) {
    dz[r * d + lane + 64] = __builtin_fmaf(dp, p1, dn * n1);
    src[(R + r) * d + lane + 64] = dp * z1 * sd;
    src[(2 * R + r) * d + lane + 64] = dn * z1 * sd;
  }
}

// loss2[0] = sum(term) / T in double, rounded once; loss2[1] = l2 / 2 (sum item^2 + sum pos^2) (0 when l2 == 0)
__global__ __launch_bounds__(256) void sas_losssum_kernel(const float* __restrict__ term, int64_t R,
                                                          const float* __restrict__ hdr, const float* __restrict__ item,
                                                          int64_t n_item, const float* __restrict__ pe, int64_t n_pe,
                                                          float l2, float* __restrict__ loss2) {
  __shared__ double part[256];
  for (int pass = 0; pass < 2; ++pass) {
    double acc = 0.0;
    if (pass == 0) {
      for (int64_t r = threadIdx.x; r < R; r += 256) acc += (double)term[r];
    } else if (l2 != 0.0f) {
      for (int64_t k = threadIdx.x; k < n_item; k += 256) acc += (double)item[k] * (double)item[k];
      for (int64_t k = threadIdx.x; k < n_pe; k += 256) acc += (double)pe[k] * (double)pe[k];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) loss2[pass] = pass == 0 ? (float)(part[0] * (double)hdr[1]) : (float)(0.5 * (double)l2 * part[0]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- backward
// dx (+)= rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dy gamma; one wavefront per row
__global__ __launch_bounds__(256) void sas_lnbwd_kernel(const float* __restrict__ dy, const float* __restrict__ xh,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        int64_t R, int d, int add, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const bool h0 = lane < d, h1 = lane + 64 < d;
  const float g0 = h0 ? dy[r * d + lane] * gamma[lane] : 0.0f, g1 = h1 ? dy[r * d + lane + 64] * gamma[lane + 64] : 0.0f;
  const float x0 = h0 ? xh[r * d + lane] : 0.0f, x1 = h1 ? xh[r * d + lane + 64] : 0.0f;
  const float m1 = nr_wave_sum_f32(g0 + g1) / (float)d;
  const float m2 = nr_wave_sum_f32(__builtin_fmaf(g0, x0, g1 * x1)) / (float)d;
  const float rs = rstd[r];
  if (h0) {
    const float v = rs * (g0 - m1 - x0 * m2);
    dx[r * d + lane] = add ? dx[r * d + lane] + v : v;
  }
  if (h1) {
    const float v = rs * (g1 - m1 - x1 * m2);
    dx[r * d + lane + 64] = add ? dx[r * d + lane + 64] + v : v;
  }
}

// din[r][k] = sum_j dout[r][j] W[k][j], stored / added / through the ReLU and its dropout / added to the masked gx
__global__ __launch_bounds__(256) void sas_backlinear_kernel(const float* __restrict__ dout, const float* __restrict__ W,
                                                             int64_t R, int d, int mode, Drop dr, int site,
                                                             const float* __restrict__ pre, const float* __restrict__ gx,
                                                             const int32_t* __restrict__ seq, int n_items,
                                                             float* __restrict__ din) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int k = (int)(idx - r * d);
  const float* g = dout + r * d;
  const float* w = W + (int64_t)k * d;
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(g[j], w[j], acc);
  if (mode == BWD_ADD) acc += din[idx];
  else if (mode == BWD_RELU_DROP) acc = pre[idx] > 0.0f ? acc * drop_factor(dr, site, idx) : 0.0f;
  else if (mode == BWD_ADD_MASKED) acc += real_item(seq[r], n_items) ? gx[idx] : 0.0f;
  din[idx] = acc;
}

// out = gx rowmask drop(site)
__global__ __launch_bounds__(256) void sas_maskdrop_kernel(const float* __restrict__ gx, const int32_t* __restrict__ seq,
                                                           int n_items, int64_t R, int d, Drop dr, int site,
                                                           float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * d) return;
  out[idx] = real_item(seq[idx / d], n_items) ? gx[idx] * drop_factor(dr, site, idx) : 0.0f;
}

// partial[chunk][a d + c] = sum over the chunk's rows of X[r][a] dY[r][c]  (a == d: the bias row, X = 1)
__global__ __launch_bounds__(256) void sas_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ dY,
                                                        int64_t R, int d, int64_t rows_per_chunk,
                                                        float* __restrict__ partial) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = (d + 1) * d;
  if (idx >= n) return;
  const int a = idx / d, c = idx - a * d;
  const int64_t lo = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t hi = lo + rows_per_chunk < R ? lo + rows_per_chunk : R;
  float acc = 0.0f;
  if (a < d) {
    for (int64_t r = lo; r < hi; ++r) acc = __builtin_fmaf(X[r * d + a], dY[r * d + c], acc);
  } else {
    for (int64_t r = lo; r < hi; ++r) acc += dY[r * d + c];
  }
  partial[(int64_t)blockIdx.y * n + idx] = acc;
}

// partial[chunk][c] = sum dy[r][c] (beta), partial[chunk][d + c] = sum dy[r][c] xh[r][c] (gamma)
__global__ __launch_bounds__(256) void sas_lnparam_kernel(const float* __restrict__ dy, const float* __restrict__ xh,
                                                          int64_t R, int d, int64_t rows_per_chunk,
                                                          float* __restrict__ partial) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * d) return;
  const int c = idx < d ? idx : idx - d;
  const int64_t lo = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t hi = lo + rows_per_chunk < R ? lo + rows_per_chunk : R;
  float acc = 0.0f;
  if (idx < d) {
    for (int64_t r = lo; r < hi; ++r) acc += dy[r * d + c];
  } else {
    for (int64_t r = lo; r < hi; ++r) acc = __builtin_fmaf(dy[r * d + c], xh[r * d + c], acc);
  }
  partial[(int64_t)blockIdx.y * 2 * d + idx] = acc;
}

// the chunks in ascending order; the first n0 sums go to dst0, the rest to dst1
__global__ __launch_bounds__(256) void sas_reduce_kernel(const float* __restrict__ partial, int n, int chunks, int n0,
                                                         float* __restrict__ dst0, float* __restrict__ dst1) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < chunks; ++k) acc += partial[(int64_t)k * n + idx];
  if (idx < n0) dst0[idx] = acc;
  else dst1[idx - n0] = acc;
}

// one thread per (hb, i): dW_ij = dO_i . V_j, dP = dW qm drop, dS = P (dP - sum_j dP P) / sqrt(dh); a uniform row has no
// gradient into its logits
__global__ __launch_bounds__(256) void sas_attn_ds_kernel(const float* __restrict__ P, const float* __restrict__ dO,
                                                          const float* __restrict__ V, const float* __restrict__ qm,
                                                          const float* __restrict__ kvis, int B, int L, int d, int h,
                                                          Drop dr, int site, float* __restrict__ dS) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)h * B * L) return;
  const int i = (int)(idx % L);
  const int64_t hb = idx / L;
  const int b = (int)(hb % B), hd = (int)(hb / B);
  const int dh = d / h;
  const float scale = 1.0f / sqrtf((float)dh);
  const float* p = P + idx * L;
  float* ds = dS + idx * L;
  int seen = 0;
  for (int j = 0; j <= i; ++j) seen += kvis[(int64_t)b * L + j] != 0.0f;
  const float m = qm[(int64_t)b * L + i];
  if (!seen || m == 0.0f) {
    for (int j = 0; j < L; ++j) ds[j] = 0.0f;
    return;
  }
  const float* g = dO + ((int64_t)b * L + i) * d + hd * dh;
  float D = 0.0f;
  for (int j = 0; j < L; ++j) {
    float dp = 0.0f;
    if (p[j] != 0.0f) {
      const float* v = V + ((int64_t)b * L + j) * d + hd * dh;
      for (int c = 0; c < dh; ++c) dp = __builtin_fmaf(g[c], v[c], dp);
      dp *= m * drop_factor(dr, site, idx * L + j);
      D = __builtin_fmaf(dp, p[j], D);
    }
    ds[j] = dp;
  }
  for (int j = 0; j < L; ++j) ds[j] = p[j] != 0.0f ? p[j] * (ds[j] - D) * scale : 0.0f;
}

// dQ[r][c] = sum_j dS[hb][i][j] K[b][j][c]
__global__ __launch_bounds__(256) void sas_attn_dq_kernel(const float* __restrict__ dS, const float* __restrict__ K, int B,
                                                          int L, int d, int h, float* __restrict__ dQ) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t R = (int64_t)B * L;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int c = (int)(idx - r * d), b = (int)(r / L), i = (int)(r % L);
  const int64_t hb = (int64_t)(c / (d / h)) * B + b;
  const float* ds = dS + (hb * L + i) * L;
  float acc = 0.0f;
  for (int j = 0; j <= i; ++j) acc = __builtin_fmaf(ds[j], K[((int64_t)b * L + j) * d + c], acc);
  dQ[idx] = acc;
}

// dK[b][j][c] = sum_i dS[hb][i][j] Q[b][i][c];  dV[b][j][c] = sum_i W[hb][i][j] dO[b][i][c]
__global__ __launch_bounds__(256) void sas_attn_dkv_kernel(const float* __restrict__ dS, const float* __restrict__ P,
                                                           const float* __restrict__ Q, const float* __restrict__ dO,
                                                           const float* __restrict__ qm, int B, int L, int d, int h,
                                                           Drop dr, int site, float* __restrict__ dK,
                                                           float* __restrict__ dV) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t R = (int64_t)B * L;
  if (idx >= R * d) return;
  const int64_t r = idx / d;
  const int c = (int)(idx - r * d), b = (int)(r / L), j = (int)(r % L);
  const int64_t hb = (int64_t)(c / (d / h)) * B + b;
  float ak = 0.0f, av = 0.0f;
  for (int i = 0; i < L; ++i) {                   // a uniform row weighs every key, the later ones too
    const int64_t ri = (int64_t)b * L + i;
    const float s = dS[(hb * L + i) * L + j];
    if (s != 0.0f) ak = __builtin_fmaf(s, Q[ri * d + c], ak);
    const float w = attn_weight(P, dr, site, hb, i, j, L, qm[ri]);
    if (w != 0.0f) av = __builtin_fmaf(w, dO[ri * d + c], av);
  }
  dK[idx] = ak;
  dV[idx] = av;
}

// de = gx rowmask drop0: the sequence slots of the item gradient (times sqrt(d)) and G_pos[t][c] = sum_b de, b ascending
__global__ __launch_bounds__(256) void sas_embedbwd_kernel(const float* __restrict__ gx, const int32_t* __restrict__ seq,
                                                           int n_items, int B, int L, int d, float sd, Drop dr,
                                                           float* __restrict__ src, float* __restrict__ Gpos) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= L * d) return;
  const int t = idx / d, c = idx - t * d;
  float acc = 0.0f;
  for (int b = 0; b < B; ++b) {
    const int64_t r = (int64_t)b * L + t;
    const int64_t e = r * d + c;
    const float de = real_item(seq[r], n_items) ? gx[e] * drop_factor(dr, 0, e) : 0.0f;
    src[e] = de * sd;
    acc += de;
  }
  Gpos[idx] = acc;
}

// G += l2 w
__global__ __launch_bounds__(256) void sas_l2_kernel(const float* __restrict__ w, int64_t n, float l2,
                                                     float* __restrict__ G) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) G[idx] = __builtin_fmaf(l2, w[idx], G[idx]);
}

// out[b][c] = z[b][L - 1][c] * scale
__global__ __launch_bounds__(256) void sas_last_kernel(const float* __restrict__ z, int B, int L, int d, float scale,
                                                       float* __restrict__ out, int64_t ld) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * d) return;
  const int b = idx / d, c = idx - b * d;
  out[(int64_t)b * ld + c] = z[((int64_t)b * L + (L - 1)) * d + c] * scale;
}

struct Layout {
  // per block: the saved activations [R][d] and per-row scalars; P [h B L L]
  size_t X[kNB + 1], XH1[kNB], QN[kNB], Q[kNB], K[kNB], V[kNB], Y[kNB], YH[kNB], U[kNB], H1[kNB], A[kNB], P[kNB];
  size_t rstd1[kNB], rstd2[kNB], kvis[kNB], qm[kNB];
  size_t ZH, Z, rstdf, t[4], src, term, dS, partial, hdr, total;
};

Layout layout_of(int B, int L, int d, int nb, int h, bool step) {
  Layout y;
  size_t off = 0;
  const size_t R = (size_t)B * L, Rd = R * d, PP = (size_t)h * B * L * L;
  auto take = [&](size_t n) { const size_t o = off; off += nr_align_up(n, 64); return o; };
  y.hdr = take(64);
  for (int i = 0; i < nb; ++i) {
    y.X[i] = take(Rd); y.XH1[i] = take(Rd); y.QN[i] = take(Rd); y.Q[i] = take(Rd); y.K[i] = take(Rd); y.V[i] = take(Rd);
    y.Y[i] = take(Rd); y.YH[i] = take(Rd); y.U[i] = take(Rd); y.H1[i] = take(Rd); y.A[i] = take(Rd);
    y.rstd1[i] = take(R); y.rstd2[i] = take(R); y.kvis[i] = take(R); y.qm[i] = take(R);
    y.P[i] = (step || i == 0) ? take(PP) : y.P[0];           // the forward pass alone reuses one buffer
  }
  y.X[nb] = take(Rd);
  y.ZH = take(Rd); y.Z = take(Rd); y.rstdf = take(R);
  if (step) {
    for (int k = 0; k < 4; ++k) y.t[k] = take(Rd);
    y.src = take(3 * Rd); y.term = take(R); y.dS = take(PP);
    y.partial = take((size_t)kChunks * (d + 1) * d);
  }
  y.total = off;
  return y;
}

int check_shape(const char* who, int B, int L, int d, int nb, int h) {
  NR_REQUIRE(d >= 1 && d <= kD, NR_ERR_UNSUPPORTED, "%s: hidden_units %d outside 1..%d", who, d, kD);
  NR_REQUIRE(L >= 1 && L <= kLen, NR_ERR_UNSUPPORTED, "%s: max_len %d outside 1..%d", who, L, kLen);
  NR_REQUIRE(nb >= 1 && nb <= kNB, NR_ERR_UNSUPPORTED, "%s: num_blocks %d outside 1..%d", who, nb, kNB);
  NR_REQUIRE(h >= 1 && d % h == 0, NR_ERR_ARG, "%s: num_heads %d does not divide hidden_units %d", who, h, d);
  NR_REQUIRE(B >= 0 && B <= kB, NR_ERR_UNSUPPORTED, "%s: batch %d outside 0..%d", who, B, kB);
  NR_REQUIRE((int64_t)h * B * L * L <= NRHIP_SASREC_MAX_WEIGHTS, NR_ERR_UNSUPPORTED,
             "%s: num_heads * batch * max_len^2 = %lld attention weights are more than %lld", who,
             (long long)((int64_t)h * B * L * L), (long long)NRHIP_SASREC_MAX_WEIGHTS);
  return NR_OK;
}

int check_weights(const nrhip_sasrec_weights& w, const char* who) {
  NR_REQUIRE(w.d_item && w.d_pos && w.d_lnf_beta && w.d_lnf_gamma && w.n_items >= 0, NR_ERR_ARG, "%s: null weight pointer",
             who);
  for (int i = 0; i < w.n_blocks; ++i)
    for (int k = 0; k < NRHIP_SASREC_BLOCK_VARS; ++k)
      NR_REQUIRE(w.d_blk[i][k], NR_ERR_ARG, "%s: null weight pointer (block %d, variable %d)", who, i, k);
  return NR_OK;
}

inline unsigned waves_of(int64_t rows) { return (unsigned)((rows + 3) / 4); }

// the forward pass of the graph over B rows; training decides the dropout
int forward(const nrhip_sasrec_weights& w, const int32_t* seq, const int32_t* pos, const int32_t* neg, int B,
            const Drop& dr, const Layout& y, float* ws, uint64_t* keys, hipStream_t st) {
  const int L = w.L, d = w.d, h = w.n_heads;
  const int64_t R = (int64_t)B * L;
  const dim3 blk(256);
  const unsigned ge = blocks_of(R * d);
  const float sd = sqrtf((float)d);
  hipLaunchKernelGGL(sas_embed_kernel, dim3(ge), blk, 0, st, w.d_item, w.d_pos, seq, pos, neg, w.n_items, R, L, d, sd, dr,
                     ws + y.X[0], keys);
  NR_LAUNCH_CHECK();
  for (int i = 0; i < w.n_blocks; ++i) {
    const float* const* p = w.d_blk[i];
    hipLaunchKernelGGL(sas_ln_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)(ws + y.X[i]), p[P_LN1B], p[P_LN1G], R,
                       d, ws + y.XH1[i], ws + y.rstd1[i], ws + y.QN[i], ws + y.kvis[i], ws + y.qm[i]);
    NR_LAUNCH_CHECK();
    const struct { const float* in; int W, b; size_t out; } lin[3] = {
        {ws + y.QN[i], P_WQ, P_BQ, y.Q[i]}, {ws + y.X[i], P_WK, P_BK, y.K[i]}, {ws + y.X[i], P_WV, P_BV, y.V[i]}};
    for (const auto& l : lin) {
      hipLaunchKernelGGL(sas_linear_kernel, dim3(ge), blk, 0, st, l.in, p[l.W], p[l.b], R, d, (int)EPI_PLAIN, dr, 0,
                         (float*)nullptr, (const float*)nullptr, seq, w.n_items, ws + l.out);
      NR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sas_softmax_kernel, dim3(blocks_of((int64_t)h * R)), blk, 0, st, (const float*)(ws + y.Q[i]),
                       (const float*)(ws + y.K[i]), (const float*)(ws + y.kvis[i]), B, L, d, h, ws + y.P[i]);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_attnout_kernel, dim3(ge), blk, 0, st, (const float*)(ws + y.P[i]), (const float*)(ws + y.V[i]),
                       (const float*)(ws + y.QN[i]), (const float*)(ws + y.qm[i]), B, L, d, h, dr, 1 + 3 * i, ws + y.Y[i]);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_ln_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)(ws + y.Y[i]), p[P_LN2B], p[P_LN2G], R,
                       d, ws + y.YH[i], ws + y.rstd2[i], ws + y.U[i], (float*)nullptr, (float*)nullptr);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_linear_kernel, dim3(ge), blk, 0, st, (const float*)(ws + y.U[i]), p[P_W1], p[P_B1], R, d,
                       (int)EPI_RELU_DROP, dr, 2 + 3 * i, ws + y.H1[i], (const float*)nullptr, seq, w.n_items,
                       ws + y.A[i]);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_linear_kernel, dim3(ge), blk, 0, st, (const float*)(ws + y.A[i]), p[P_W2], p[P_B2], R, d,
                       (int)EPI_DROP_RES, dr, 3 + 3 * i, (float*)nullptr, (const float*)(ws + y.U[i]), seq, w.n_items,
                       ws + y.X[i + 1]);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sas_ln_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)(ws + y.X[w.n_blocks]), w.d_lnf_beta,
                     w.d_lnf_gamma, R, d, ws + y.ZH, ws + y.rstdf, ws + y.Z, (float*)nullptr, (float*)nullptr);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // namespace

extern "C" {

int nrhip_sasrec_workspace_floats(int max_batch, int max_len, int hidden_units, int num_blocks, int num_heads,
                                  size_t* floats) {
  NR_REQUIRE(floats, NR_ERR_ARG, "sasrec_workspace_floats: null argument");
  NR_TRY(check_shape("sasrec_workspace_floats", max_batch, max_len, hidden_units, num_blocks, num_heads));
  *floats = layout_of(max_batch, max_len, hidden_units, num_blocks, num_heads, true).total;
  return NR_OK;
}

int nrhip_sasrec_step(const nrhip_sasrec_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "sasrec_step: null argument block");
  const nrhip_sasrec_step_args a = *args;
  const nrhip_sasrec_weights& w = a.w;
  NR_TRY(check_shape("sasrec_step", a.batch, w.L, w.d, w.n_blocks, w.n_heads));
  NR_TRY(check_weights(w, "sasrec_step"));
  NR_REQUIRE(a.rate >= 0.0f && a.rate < 1.0f, NR_ERR_ARG, "sasrec_step: dropout rate %g outside [0, 1)", (double)a.rate);
  const int B = a.batch, L = w.L, d = w.d, h = w.n_heads, nb = w.n_blocks;
  if (B == 0) return NR_OK;
  NR_REQUIRE(a.d_G_item && a.d_G_pos && a.d_G_lnf_beta && a.d_G_lnf_gamma && a.d_seq && a.d_pos_ids && a.d_neg_ids &&
                 a.d_keys && a.d_ws && a.d_loss2, NR_ERR_ARG, "sasrec_step: null pointer argument");
  for (int i = 0; i < nb; ++i)
    for (int k = 0; k < NRHIP_SASREC_BLOCK_VARS; ++k)
      NR_REQUIRE(a.d_G_blk[i][k], NR_ERR_ARG, "sasrec_step: null gradient pointer (block %d, variable %d)", i, k);
  hipStream_t st = (hipStream_t)stream;
  const Layout y = layout_of(B, L, d, nb, h, true);
  float* ws = a.d_ws;
  const int64_t R = (int64_t)B * L;
  const dim3 blk(256);
  const unsigned ge = blocks_of(R * d);
  const float sd = sqrtf((float)d);
  Drop dr;
  for (int k = 0; k < 1 + 3 * kNB; ++k) dr.mask[k] = k < 1 + 3 * nb ? a.d_mask[k] : nullptr;
  dr.seed = a.seed;
  dr.step = a.step;
  dr.keep = 1.0f - a.rate;
  dr.inv_keep = 1.0f / dr.keep;
  dr.on = a.rate > 0.0f ? 1 : 0;
  if (dr.on && a.d_mask[0])
    for (int k = 0; k < 1 + 3 * nb; ++k)
      NR_REQUIRE(a.d_mask[k], NR_ERR_ARG, "sasrec_step: dropout masks are given for all %d sites or for none", 1 + 3 * nb);

  hipLaunchKernelGGL(sas_prep_kernel, dim3(1), blk, 0, st, a.d_pos_ids, R, w.n_items, ws + y.hdr);
  NR_LAUNCH_CHECK();
  NR_TRY(forward(w, a.d_seq, a.d_pos_ids, a.d_neg_ids, B, dr, y, ws, a.d_keys, st));
  float* t0 = ws + y.t[0];
  float* t1 = ws + y.t[1];
  float* t2 = ws + y.t[2];
  float* t3 = ws + y.t[3];
  float* src = ws + y.src;
  float* part = ws + y.partial;
  const int chunks = (int)((R + 31) / 32 < kChunks ? (R + 31) / 32 : kChunks);
  const int64_t rpc = (R + chunks - 1) / chunks;
  const int nW = (d + 1) * d;
  auto wgrad = [&](const float* X, const float* dY, float* GW, float* Gb) -> int {
    hipLaunchKernelGGL(sas_wgrad_kernel, dim3(blocks_of(nW), chunks), blk, 0, st, X, dY, R, d, rpc, part);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_reduce_kernel, dim3(blocks_of(nW)), blk, 0, st, (const float*)part, nW, chunks, d * d, GW, Gb);
    NR_LAUNCH_CHECK();
    return NR_OK;
  };
  auto lnparam = [&](const float* dy, const float* xh, float* Gbeta, float* Ggamma) -> int {
    hipLaunchKernelGGL(sas_lnparam_kernel, dim3(blocks_of(2 * d), chunks), blk, 0, st, dy, xh, R, d, rpc, part);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_reduce_kernel, dim3(blocks_of(2 * d)), blk, 0, st, (const float*)part, 2 * d, chunks, d, Gbeta,
                       Ggamma);
    NR_LAUNCH_CHECK();
    return NR_OK;
  };
  auto backlin = [&](const float* dout, const float* W, int mode, int site, const float* pre, const float* gx,
                     float* din) -> int {
    hipLaunchKernelGGL(sas_backlinear_kernel, dim3(ge), blk, 0, st, dout, W, R, d, mode, dr, site, pre, gx, a.d_seq,
                       w.n_items, din);
    NR_LAUNCH_CHECK();
    return NR_OK;
  };

  // loss, dz (t0) and the positive / negative slots
  hipLaunchKernelGGL(sas_loss_kernel, dim3(waves_of(R)), blk, 0, st, w.d_item, (const float*)(ws + y.Z), a.d_pos_ids,
                     a.d_neg_ids, w.n_items, R, d, sd, (const float*)(ws + y.hdr), ws + y.term, t0, src);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sas_losssum_kernel, dim3(1), blk, 0, st, (const float*)(ws + y.term), R, (const float*)(ws + y.hdr),
                     w.d_item, (int64_t)w.n_items * d, w.d_pos, (int64_t)L * d, a.l2_emb, a.d_loss2);
  NR_LAUNCH_CHECK();
  NR_TRY(lnparam(t0, ws + y.ZH, a.d_G_lnf_beta, a.d_G_lnf_gamma));
  float* gx = t1;
  hipLaunchKernelGGL(sas_lnbwd_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)t0, (const float*)(ws + y.ZH),
                     (const float*)(ws + y.rstdf), w.d_lnf_gamma, R, d, 0, gx);
  NR_LAUNCH_CHECK();
  float* fa = t0;
  float* fb = t2;
  float* fc = t3;
  for (int i = nb - 1; i >= 0; --i) {
    const float* const* p = w.d_blk[i];
    float* const* G = a.d_G_blk[i];
    // feed-forward: dF = gx rowmask drop2 (fa)
    hipLaunchKernelGGL(sas_maskdrop_kernel, dim3(ge), blk, 0, st, (const float*)gx, a.d_seq, w.n_items, R, d, dr,
                       3 + 3 * i, fa);
    NR_LAUNCH_CHECK();
    NR_TRY(wgrad(ws + y.A[i], fa, G[P_W2], G[P_B2]));
    NR_TRY(backlin(fa, p[P_W2], BWD_RELU_DROP, 2 + 3 * i, ws + y.H1[i], nullptr, fb));          // dH1 (fb)
    NR_TRY(wgrad(ws + y.U[i], fb, G[P_W1], G[P_B1]));
    NR_TRY(backlin(fb, p[P_W1], BWD_ADD_MASKED, 0, nullptr, gx, fc));                            // dU (fc)
    NR_TRY(lnparam(fc, ws + y.YH[i], G[P_LN2B], G[P_LN2G]));
    hipLaunchKernelGGL(sas_lnbwd_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)fc, (const float*)(ws + y.YH[i]),
                       (const float*)(ws + y.rstd2[i]), p[P_LN2G], R, d, 0, fa);                 // dY (fa)
    NR_LAUNCH_CHECK();
    // attention: dS, then dQ (fb), dK (fc), dV (gx: the incoming gradient is spent)
    hipLaunchKernelGGL(sas_attn_ds_kernel, dim3(blocks_of((int64_t)h * R)), blk, 0, st, (const float*)(ws + y.P[i]),
                       (const float*)fa, (const float*)(ws + y.V[i]), (const float*)(ws + y.qm[i]),
                       (const float*)(ws + y.kvis[i]), B, L, d, h, dr, 1 + 3 * i, ws + y.dS);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_attn_dq_kernel, dim3(ge), blk, 0, st, (const float*)(ws + y.dS), (const float*)(ws + y.K[i]), B,
                       L, d, h, fb);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_attn_dkv_kernel, dim3(ge), blk, 0, st, (const float*)(ws + y.dS), (const float*)(ws + y.P[i]),
                       (const float*)(ws + y.Q[i]), (const float*)fa, (const float*)(ws + y.qm[i]), B, L, d, h, dr,
                       1 + 3 * i, fc, gx);
    NR_LAUNCH_CHECK();
    NR_TRY(wgrad(ws + y.QN[i], fb, G[P_WQ], G[P_BQ]));
    NR_TRY(wgrad(ws + y.X[i], fc, G[P_WK], G[P_BK]));
    NR_TRY(wgrad(ws + y.X[i], gx, G[P_WV], G[P_BV]));
    NR_TRY(backlin(fb, p[P_WQ], BWD_ADD, 0, nullptr, nullptr, fa));                              // dq = dY + dQ Wq^T (fa)
    NR_TRY(lnparam(fa, ws + y.XH1[i], G[P_LN1B], G[P_LN1G]));
    NR_TRY(backlin(fc, p[P_WK], BWD_STORE, 0, nullptr, nullptr, fb));                            // dx (fb)
    NR_TRY(backlin(gx, p[P_WV], BWD_ADD, 0, nullptr, nullptr, fb));
    hipLaunchKernelGGL(sas_lnbwd_kernel, dim3(waves_of(R)), blk, 0, st, (const float*)fa, (const float*)(ws + y.XH1[i]),
                       (const float*)(ws + y.rstd1[i]), p[P_LN1G], R, d, 1, fb);
    NR_LAUNCH_CHECK();
    float* spent = gx;
    gx = fb;
    fb = spent;
  }
  hipLaunchKernelGGL(sas_embedbwd_kernel, dim3(blocks_of((int64_t)L * d)), blk, 0, st, (const float*)gx, a.d_seq,
                     w.n_items, B, L, d, sd, dr, src, a.d_G_pos);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(a.d_keys, (int)(3 * R), stream));
  hipLaunchKernelGGL(gru_rows_kernel, dim3((unsigned)((3 * R + 3) / 4)), blk, 0, st, a.d_keys, (int)(3 * R), d,
                     (const float*)src, a.d_G_item, (const float*)nullptr, (float*)nullptr);
  NR_LAUNCH_CHECK();
  if (a.l2_emb != 0.0f) {
    hipLaunchKernelGGL(sas_l2_kernel, dim3(blocks_of((int64_t)w.n_items * d)), blk, 0, st, w.d_item,
                       (int64_t)w.n_items * d, a.l2_emb, a.d_G_item);
    NR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sas_l2_kernel, dim3(blocks_of((int64_t)L * d)), blk, 0, st, w.d_pos, (int64_t)L * d, a.l2_emb,
                       a.d_G_pos);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_sasrec_forward(const nrhip_sasrec_weights* weights, const int32_t* d_seq, int batch, float* d_ws, float scale,
                         float* d_out, int64_t ld, void* stream) {
  NR_REQUIRE(weights, NR_ERR_ARG, "sasrec_forward: null argument block");
  const nrhip_sasrec_weights w = *weights;
  NR_TRY(check_shape("sasrec_forward", batch, w.L, w.d, w.n_blocks, w.n_heads));
  NR_TRY(check_weights(w, "sasrec_forward"));
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_seq && d_ws && d_out && ld >= w.d, NR_ERR_ARG, "sasrec_forward: null pointer argument or ld < hidden_units");
  hipStream_t st = (hipStream_t)stream;
  const Layout y = layout_of(batch, w.L, w.d, w.n_blocks, w.n_heads, false);
  Drop dr = {};
  dr.keep = dr.inv_keep = 1.0f;
  NR_TRY(forward(w, d_seq, d_seq, d_seq, batch, dr, y, d_ws, nullptr, st));
  hipLaunchKernelGGL(sas_last_kernel, dim3(blocks_of((int64_t)batch * w.d)), dim3(256), 0, st, (const float*)(d_ws + y.Z),
                     batch, w.L, w.d, scale, d_out, ld);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
