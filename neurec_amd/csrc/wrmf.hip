// WRMF (Hu, Koren & Volinsky, ICDM 2008) as the reference trains it: model/general_recommender/WRMF.py:47-59 solves,
// for every row u of one side against the other side's table Y (n x d),
//
//     A_u = Y^T Y + alpha * sum_{j in N(u)} y_j y_j^T + lambda I,    b_u = (1 + alpha) * sum_{j in N(u)} y_j,
//     x_u = A_u^{-1} b_u
//
// one tf.linalg.solve per row.  Every row of a half-sweep reads only the OTHER table, so the half-sweep is one batched
// solve here:
//   wrmf_gram_partial_kernel / wrmf_gram_reduce_kernel   G = Y^T Y: row ranges per workgroup, the partial d x d sums
//                                                         added in workgroup order by the second kernel (no atomics)
//   wrmf_chunk_kernel                                    rows with more than NRHIP_WRMF_CHUNK neighbours: the partial
//                                                         (sum y y^T, sum y) of each CHUNK-long piece of the list
//   wrmf_solve_kernel                                    one workgroup per row: its own sums (or its chunks' partials,
//                                                         added in chunk order), + G, + lambda I, factored in registers
//                                                         (square-root-free Cholesky, A = L D L^T), b eliminated along,
//                                                         back substitution by one wave, row written
// Every sum is taken in a fixed order: the tables are bit-identical from run to run.
//
// Layout.  The padded width DP = TG * R (8, 16, 32, 64, 128) is spread over a TG x TG thread grid; thread (ti, tj)
// owns the R x R elements (ti + TG a, tj + TG b), cyclically, and keeps only the blocks a >= b — they cover the lower
// triangle, which is all the factorisation reads.  A staged neighbour row sits in LDS permuted so that a thread's R
// values of it are contiguous (column c at (c % TG) * R + c / TG).  Padding rows / columns (>= d) are the identity and
// stay out of the elimination.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "neurec_hip.h"
#include "nr_common.h"

namespace {

constexpr int kTile = 32;            // neighbour rows staged per LDS tile
constexpr int kGramBlocksMax = 256;  // workgroups of the Gram's first pass (the fixed order of its partial sums)
constexpr int64_t kChunk = NRHIP_WRMF_CHUNK;

template <int R>
__device__ __forceinline__ void lds_read_r(const float* p, float (&v)[R]) {
  if constexpr (R % 4 == 0) {
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
      const float4 x = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
  } else if constexpr (R == 2) {
    const float2 x = *reinterpret_cast<const float2*>(p);
    v[0] = x.x, v[1] = x.y;
  } else {
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = p[q];
  }
}

// one thread's share of the staged tile at positions [p0, p0 + nt): element e = tid + s NT is row t = e / DP, column
// c = e % DP.  Every load is issued unconditionally on a clamped position and masked afterwards (a load behind a
// branch is waited for before the next one is issued).  Callers guarantee nt >= 1 and n_other >= 1.
template <int TG, int R, bool kCsr>
__device__ __forceinline__ void gather_tile(const int32_t* __restrict__ idx, int64_t p0, int nt,
                                            const float* __restrict__ Y, int n_other, int d,
                                            float (&v)[kTile * TG * R / (TG * TG)]) {
  constexpr int DP = TG * R, NT = TG * TG, S = kTile * DP / NT;
  const int tid = threadIdx.x;
  int64_t rows[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int t = (tid + s * NT) / DP;
    rows[s] = kCsr ? (int64_t)idx[p0 + (t < nt ? t : nt - 1)] : p0 + (t < nt ? t : nt - 1);
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int e = tid + s * NT, t = e / DP, c = e % DP;
    const bool ok = t < nt && c < d && (uint64_t)rows[s] < (uint64_t)n_other;
    const float x = Y[(ok ? rows[s] : 0) * d + (c < d ? c : d - 1)];
    v[s] = ok ? x : 0.f;
  }
}

// acc (+)= sum over positions [begin, end) of y y^T (owned lower blocks), sb (+)= sum of y (columns tj + TG b);
// y = Y[idx[p]] (CSR) or Y[p] (Gram).  Positions in ascending order.  kPrefetch: the next tile's loads are in flight
// while the current one is summed (long lists).  Ends with a barrier: ys is free afterwards.
template <int TG, int R, bool kCsr, bool kPrefetch>
__device__ __forceinline__ void accumulate(const int32_t* __restrict__ idx, int64_t begin, int64_t end,
                                           const float* __restrict__ Y, int n_other, int d, float* ys,
                                           float (&acc)[R][R], float (&sb)[R]) {
  constexpr int DP = TG * R, NT = TG * TG, S = kTile * DP / NT;
  const int tid = threadIdx.x, ti = tid / TG, tj = tid % TG;
  if (end <= begin || n_other <= 0) return;
  float v[S];
  if (kPrefetch) gather_tile<TG, R, kCsr>(idx, begin, (int)(end - begin < kTile ? end - begin : kTile), Y, n_other, d, v);
  for (int64_t p0 = begin; p0 < end; p0 += kTile) {
    const int nt = (int)(end - p0 < kTile ? end - p0 : kTile);
    if (!kPrefetch) gather_tile<TG, R, kCsr>(idx, p0, nt, Y, n_other, d, v);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int e = tid + s * NT, t = e / DP, c = e % DP;
      ys[t * DP + (c % TG) * R + c / TG] = v[s];
    }
    __syncthreads();
    if (kPrefetch && p0 + kTile < end) {
      const int64_t p1 = p0 + kTile;
      gather_tile<TG, R, kCsr>(idx, p1, (int)(end - p1 < kTile ? end - p1 : kTile), Y, n_other, d, v);
    }
    for (int t = 0; t < nt; ++t) {
      float yi[R], yj[R];
      lds_read_r<R>(ys + t * DP + ti * R, yi);
      lds_read_r<R>(ys + t * DP + tj * R, yj);
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) acc[a][b] = fmaf(yi[a], yj[b], acc[a][b]);
#pragma unroll
      for (int b = 0; b < R; ++b) sb[b] += yj[b];
    }
    __syncthreads();
  }
}

template <int TG, int R>
__device__ __forceinline__ void zero(float (&acc)[R][R], float (&sb)[R]) {
#pragma unroll
  for (int a = 0; a < R; ++a) {
    sb[a] = 0.f;
#pragma unroll
    for (int b = 0; b < R; ++b) acc[a][b] = 0.f;
  }
}

template <int TG, int R>
__global__ __launch_bounds__(TG* TG) void wrmf_gram_partial_kernel(const float* __restrict__ Y, int n, int d, int per,
                                                                   float* __restrict__ part) {
  constexpr int DP = TG * R;
  __shared__ float ys[kTile * DP];
  const int ti = threadIdx.x / TG, tj = threadIdx.x % TG;
  float acc[R][R], sb[R];
  zero<TG, R>(acc, sb);
  const int64_t begin = (int64_t)blockIdx.x * per, end = begin + per < n ? begin + per : n;
  accumulate<TG, R, false, true>(nullptr, begin, end, Y, n, d, ys, acc, sb);
  float* out = part + (size_t)blockIdx.x * DP * DP;
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) out[(ti + TG * a) * DP + tj + TG * b] = acc[a][b];
}

// G[i][j] = sum over the partials in workgroup order; element (i, j) was kept by the partial as (i, j) when
// i / TG >= j / TG, else as (j, i)
__global__ __launch_bounds__(256) void wrmf_gram_reduce_kernel(const float* __restrict__ part, int nb, int d, int DP,
                                                               int TG, float* __restrict__ G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d * d) return;
  int i = e / d, j = e % d;
  if (i / TG < j / TG) {
    const int t = i;
    i = j, j = t;
  }
  const float* p = part + i * DP + j;
  const size_t stride = (size_t)DP * DP;
  float s = 0.f;
  int g = 0;
  for (; g + 8 <= nb; g += 8) {        // eight loads in flight, added in order
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = p[(g + q) * stride];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += x[q];
  }
  for (; g < nb; ++g) s += p[g * stride];
  G[e] = s;
}

// chunk c of a long neighbour list: its partial (sum y y^T, sum y) into part[c] (DP*DP + DP floats)
template <int TG, int R>
__global__ __launch_bounds__(TG* TG) void wrmf_chunk_kernel(const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices, int n_rows,
                                                            const float* __restrict__ Y, int n_other, int d,
                                                            const int32_t* __restrict__ row_chunk,
                                                            const int32_t* __restrict__ chunk_row,
                                                            float* __restrict__ part) {
  constexpr int DP = TG * R;
  __shared__ float ys[kTile * DP];
  const int ti = threadIdx.x / TG, tj = threadIdx.x % TG;
  const int c = blockIdx.x, row = chunk_row[c];
  if (row < 0 || row >= n_rows) return;
  const int64_t k = (int64_t)c - row_chunk[row];
  const int64_t lo = indptr[row], hi = indptr[row + 1];
  int64_t begin = lo + k * kChunk, end = begin + kChunk < hi ? begin + kChunk : hi;
  if (k < 0 || begin > hi) begin = end = hi;
  float acc[R][R], sb[R];
  zero<TG, R>(acc, sb);
  accumulate<TG, R, true, true>(indices, begin, end, Y, n_other, d, ys, acc, sb);
  float* out = part + (size_t)c * (DP * DP + DP);
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) out[(ti + TG * a) * DP + tj + TG * b] = acc[a][b];
  if (ti == 0) {
#pragma unroll
    for (int b = 0; b < R; ++b) out[DP * DP + tj + TG * b] = sb[b];
  }
}

template <int TG, int R>
__global__ __launch_bounds__(TG* TG) void wrmf_solve_kernel(const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices,
                                                            const float* __restrict__ Y, int n_other,
                                                            const float* __restrict__ G, int d, float alpha,
                                                            float lambda, const int32_t* __restrict__ row_chunk,
                                                            int n_chunks, const float* __restrict__ part,
                                                            float* __restrict__ X) {
  constexpr int DP = TG * R, NT = TG * TG, LD = DP + 1;
  constexpr int kSmem = kTile * DP > DP * LD ? kTile * DP : DP * LD;
  __shared__ float smem[kSmem];        // the neighbour tile, then the factored matrix
  __shared__ float colbuf[2][DP];      // column k of step k (two buffers: one barrier per step)
  __shared__ float bvec[DP];
  const int tid = threadIdx.x, ti = tid / TG, tj = tid % TG;
  const int row = blockIdx.x;
  const int64_t begin = indptr[row], end = indptr[row + 1];
  float* xrow = X + (size_t)row * d;
  if (end <= begin || n_other <= 0) {  // no neighbours: b = 0, x = 0
    for (int c = tid; c < d; c += NT) xrow[c] = 0.f;
    return;
  }
  float acc[R][R], sb[R];
  zero<TG, R>(acc, sb);
  if (end - begin > kChunk) {          // the chunks' partials, in chunk order
    const int first = row_chunk ? row_chunk[row] : -1;
    const int nc = (int)((end - begin + kChunk - 1) / kChunk);
    for (int c = first < 0 ? n_chunks : first; c < first + nc && c < n_chunks; ++c) {
      const float* p = part + (size_t)c * (DP * DP + DP);
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) acc[a][b] += p[(ti + TG * a) * DP + tj + TG * b];
#pragma unroll
      for (int b = 0; b < R; ++b) sb[b] += p[DP * DP + tj + TG * b];
    }
  } else {
    accumulate<TG, R, true, false>(indices, begin, end, Y, n_other, d, smem, acc, sb);
  }
  // A = (G + alpha S) + lambda I on the d x d part, identity on the padding; b = (1 + alpha) sum y
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const int i = ti + TG * a, j = tj + TG * b;
      acc[a][b] = (i < d && j < d) ? (G[i * d + j] + alpha * acc[a][b]) + (i == j ? lambda : 0.f)
                                   : (i == j ? 1.f : 0.f);
    }
  if (ti == 0) {
#pragma unroll
    for (int b = 0; b < R; ++b) {
      const int j = tj + TG * b;
      bvec[j] = j < d ? (1.f + alpha) * sb[b] : 0.f;
    }
  }
  // elimination, step k: A[i][j] -= (A[i][k] / A[k][k]) A[j][k] and b[i] -= (A[i][k] / A[k][k]) b[k], i, j > k.
  // Column k is final after step k - 1; its owners publish it, one barrier, everyone updates their trailing blocks
  // (blocks before k / TG are finished: skipped by a uniform branch).
  for (int k = 0; k < d; ++k) {
    const int kb = k / TG, kt = k % TG;
    float* cb = colbuf[k & 1];
    if (tj == kt) {
#pragma unroll
      for (int b = 0; b < R; ++b)
        if (b == kb) {
#pragma unroll
          for (int a = b; a < R; ++a) cb[ti + TG * a] = acc[a][b];
        }
    }
    __syncthreads();
    const float inv = 1.f / cb[k];
    const float bk = bvec[k];
    float l[R], cj[R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const int i = ti + TG * a, j = tj + TG * a;
      l[a] = 0.f, cj[a] = 0.f;
      if (a >= kb) {
        const float ci = cb[i], cjj = cb[j];
        l[a] = i > k ? ci * inv : 0.f;
        cj[a] = j > k ? cjj : 0.f;
      }
    }
#pragma unroll
    for (int a = 0; a < R; ++a)
      if (a >= kb) {
#pragma unroll
        for (int b = 0; b <= a; ++b)
          if (b >= kb) acc[a][b] = fmaf(-l[a], cj[b], acc[a][b]);
      }
    if (tj == 0) {
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const int i = ti + TG * a;
        if (a >= kb && i > k) bvec[i] = fmaf(-l[a], bk, bvec[i]);
      }
    }
  }
  // the factored matrix to LDS (the tile is free: accumulate ended with a barrier)
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) smem[(ti + TG * a) * LD + tj + TG * b] = acc[a][b];
  __syncthreads();
  // back substitution L^T x = D^{-1} z by wave 0: x_k = (z_k - sum_{i>k} A[i][k] x_i) / A[k][k], as a column sweep
  // over the rows k of the lower triangle (lane i keeps w_i, which becomes x_i)
  if (tid < NR_WAVE) {
    constexpr int M = (DP + NR_WAVE - 1) / NR_WAVE;
    float w[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int i = tid + NR_WAVE * m;
      w[m] = i < DP ? bvec[i] : 0.f;
    }
    for (int k = d - 1; k >= 0; --k) {
      float wk = w[0];
#pragma unroll
      for (int m = 1; m < M; ++m)
        if (k / NR_WAVE == m) wk = w[m];
      wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wk), k % NR_WAVE));
      const float xk = wk / smem[k * LD + k];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int i = tid + NR_WAVE * m;
        if (i < k)
          w[m] = fmaf(-smem[k * LD + i], xk, w[m]);
        else if (i == k)
          w[m] = xk;
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int i = tid + NR_WAVE * m;
      if (i < d) xrow[i] = w[m];
    }
  }
}

// thread grid and register block for a width: DP = TG * R >= d
struct Shape {
  int TG, R;
  int dp() const { return TG * R; }
};
Shape shape_of(int d) {
  if (d <= 8) return {8, 1};
  if (d <= 16) return {8, 2};
  if (d <= 32) return {8, 4};
  if (d <= 64) return {8, 8};
  return {16, 8};
}

int check_width(int d) {
  NR_REQUIRE(d >= 1, NR_ERR_ARG, "wrmf: embedding_size must be >= 1, got %d", d);
  NR_REQUIRE(d <= 128, NR_ERR_UNSUPPORTED, "wrmf: embedding_size %d is not supported (at most 128)", d);
  return NR_OK;
}

size_t chunk_slot_floats(int d) {
  const size_t dp = (size_t)shape_of(d).dp();
  return dp * dp + dp;
}

void gram_split(int n, int& per, int& nb) {
  per = (n + kGramBlocksMax - 1) / kGramBlocksMax;
  if (per < 64) per = 64;
  nb = (n + per - 1) / per;
}

#define NR_WRMF_DISPATCH(d, CALL)                 \
  do {                                            \
    const Shape s_ = shape_of(d);                 \
    if (s_.TG == 8 && s_.R == 1) CALL(8, 1);      \
    else if (s_.TG == 8 && s_.R == 2) CALL(8, 2); \
    else if (s_.TG == 8 && s_.R == 4) CALL(8, 4); \
    else if (s_.TG == 8 && s_.R == 8) CALL(8, 8); \
    else CALL(16, 8);                             \
  } while (0)

}  // namespace

extern "C" {

int nrhip_wrmf_chunk_plan(const int64_t* h_indptr, int n_rows, int32_t* h_row_chunk, int32_t* h_chunk_row,
                          int* n_chunks) {
  NR_REQUIRE(h_indptr && n_chunks && n_rows >= 0, NR_ERR_ARG, "wrmf_chunk_plan: bad arguments");
  int64_t total = 0;
  for (int r = 0; r < n_rows; ++r) {
    const int64_t deg = h_indptr[r + 1] - h_indptr[r];
    NR_REQUIRE(deg >= 0, NR_ERR_ARG, "wrmf_chunk_plan: indptr decreases at row %d", r);
    const int64_t nc = deg > kChunk ? (deg + kChunk - 1) / kChunk : 0;
    if (h_row_chunk) h_row_chunk[r] = nc ? (int32_t)total : -1;
    if (h_chunk_row)
      for (int64_t c = 0; c < nc; ++c) h_chunk_row[total + c] = r;
    total += nc;
    NR_REQUIRE(total < INT32_MAX, NR_ERR_UNSUPPORTED, "wrmf_chunk_plan: more than 2^31 chunks");
  }
  *n_chunks = (int)total;
  return NR_OK;
}

int nrhip_wrmf_workspace_bytes(int d, int n_chunks, size_t* bytes) {
  NR_REQUIRE(bytes && n_chunks >= 0, NR_ERR_ARG, "wrmf_workspace_bytes: bad arguments");
  NR_TRY(check_width(d));
  const size_t dp = (size_t)shape_of(d).dp();
  const size_t gram = (size_t)kGramBlocksMax * dp * dp, chunks = (size_t)n_chunks * chunk_slot_floats(d);
  *bytes = (gram > chunks ? gram : chunks) * sizeof(float);
  return NR_OK;
}

int nrhip_wrmf_gram(const float* d_Y, int n, int d, float* d_G, void* d_ws, size_t ws_bytes, void* stream) {
  NR_REQUIRE(d_G && n >= 0 && (n == 0 || d_Y), NR_ERR_ARG, "wrmf_gram: bad arguments");
  NR_TRY(check_width(d));
  int per, nb;
  gram_split(n, per, nb);
  const Shape s = shape_of(d);
  const size_t need = (size_t)nb * s.dp() * s.dp() * sizeof(float);
  NR_REQUIRE(ws_bytes >= need && (need == 0 || d_ws), NR_ERR_WORKSPACE,
             "wrmf_gram: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)d_ws;
#define NR_WRMF_GRAM(TG, R)                                                                                   \
  do {                                                                                                        \
    if (nb)                                                                                                   \
      hipLaunchKernelGGL((wrmf_gram_partial_kernel<TG, R>), dim3(nb), dim3(TG * TG), 0, st, d_Y, n, d, per, part); \
  } while (0)
  NR_WRMF_DISPATCH(d, NR_WRMF_GRAM);
#undef NR_WRMF_GRAM
  hipLaunchKernelGGL(wrmf_gram_reduce_kernel, dim3((d * d + 255) / 256), dim3(256), 0, st, part, nb, d, s.dp(), s.TG,
                     d_G);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_wrmf_solve(const int64_t* d_indptr, const int32_t* d_indices, int n_rows, const float* d_Y, int n_other,
                     const float* d_G, int d, float alpha, float lambda, const int32_t* d_row_chunk,
                     const int32_t* d_chunk_row, int n_chunks, float* d_X, void* d_ws, size_t ws_bytes,
                     void* stream) {
  NR_REQUIRE(d_indptr && d_indices && d_G && d_X && n_rows >= 0 && n_other >= 0 && n_chunks >= 0 &&
                 (n_other == 0 || d_Y),
             NR_ERR_ARG, "wrmf_solve: bad arguments");
  NR_TRY(check_width(d));
  NR_REQUIRE(std::isfinite(lambda) && lambda > 0.f, NR_ERR_ARG,
             "wrmf_solve: reg_mf (lambda) must be > 0, got %g", (double)lambda);
  NR_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, NR_ERR_ARG, "wrmf_solve: alpha must be >= 0, got %g",
             (double)alpha);
  const size_t need = (size_t)n_chunks * chunk_slot_floats(d) * sizeof(float);
  NR_REQUIRE(n_chunks == 0 || (d_row_chunk && d_chunk_row), NR_ERR_ARG, "wrmf_solve: chunk plan missing");
  NR_REQUIRE(ws_bytes >= need && (need == 0 || d_ws), NR_ERR_WORKSPACE,
             "wrmf_solve: workspace of %zu bytes, %zu needed", ws_bytes, need);
  if (n_rows == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)d_ws;
#define NR_WRMF_SOLVE(TG, R)                                                                                        \
  do {                                                                                                             \
    if (n_chunks)                                                                                                  \
      hipLaunchKernelGGL((wrmf_chunk_kernel<TG, R>), dim3(n_chunks), dim3(TG * TG), 0, st, d_indptr, d_indices,    \
                         n_rows, d_Y, n_other, d, d_row_chunk, d_chunk_row, part);                                 \
    hipLaunchKernelGGL((wrmf_solve_kernel<TG, R>), dim3(n_rows), dim3(TG * TG), 0, st, d_indptr, d_indices, d_Y,   \
                       n_other, d_G, d, alpha, lambda, d_row_chunk, n_chunks, part, d_X);                          \
  } while (0)
  NR_WRMF_DISPATCH(d, NR_WRMF_SOLVE);
#undef NR_WRMF_SOLVE
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
