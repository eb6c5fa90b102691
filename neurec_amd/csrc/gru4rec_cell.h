// gru4rec_cell.h — what the steps of the GRU models share (gru4rec.hip, gru4recplus.hip): the activations, the GRU
// cell's forward and backward kernels, the sorted-key run kernel for the table rows' gradients and the weight checks.
//
// The cell [EXT: tensorflow r1.12 rnn_cell_impl.GRUCell]:
//     [r, u] = sigmoid([x, s] Wg + bg)      r the first n columns, u the last n
//     c      = act([x, r * s] Wc + bc)      the reset gate multiplies the state BEFORE the product
//     h      = u s + (1 - u) c
// The states are constants of a step (placeholders in the reference): nothing flows back through them.
//
//   gru_gates_kernel      per layer: the gates [B][2 n]
//   gru_cand_kernel       per layer: c and h (= the new state, = the next layer's input)
//   gru_cellbwd_kernel    per layer, top down: dc -> d(pre-candidate); du -> d(pre-update gate)
//   gru_dr_kernel         d(r * s) = d(pre-candidate) Wc[in:]^T -> dr -> d(pre-reset gate)
//   gru_dx_kernel         dx = d(pre-candidate) Wc[:in]^T + d(pre-gates) Wg[:in]^T (layer 0: + reg x0, per slot)
//   gru_dw_kernel         G_Wg, G_bg, G_Wc, G_bc whole: per element the slots' sum in slot order
//   gru_rows_kernel       one wavefront per sorted key: the head of a run adds the run's slot rows in key order and
//                         STORES the table row's gradient once
// Every kernel one thread per output and one k-ascending fmaf chain per output; no atomics.
//
// Everything here has internal linkage (an unnamed namespace): each of the two files gets its own copy of the kernels,
// and their names stay unqualified there.
#pragma once
#include "nr_common.h"
#include "neurec_hip.h"

namespace {

constexpr uint64_t kSentinel = 0x7fffffffffffffffull;     // a slot whose id is no table row sorts behind every key
constexpr int kL = NRHIP_GRU4REC_MAX_LAYERS;
constexpr int kW = NRHIP_GRU4REC_MAX_WIDTH;
enum { ACT_TANH = 0, ACT_RELU = 1 };
enum { FIN_LINEAR = 0, FIN_RELU = 1, FIN_LEAKY = 2 };
constexpr float kLeaky = 0.2f;                            // tf.nn.leaky_relu's default alpha

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float hidden_act(int act, float x) { return act == ACT_RELU ? fmaxf(x, 0.0f) : tanhf(x); }
// the derivative from the OUTPUT c = act(pre)
__device__ __forceinline__ float hidden_dact(int act, float c) {
  return act == ACT_RELU ? (c > 0.0f ? 1.0f : 0.0f) : 1.0f - c * c;
}
__device__ __forceinline__ float final_act(int act, float z) {
  if (act == FIN_RELU) return fmaxf(z, 0.0f);
  if (act == FIN_LEAKY) return fmaxf(kLeaky * z, z);
  return z;
}
__device__ __forceinline__ float final_dact(int act, float z) {
  if (act == FIN_RELU) return z > 0.0f ? 1.0f : 0.0f;
  if (act == FIN_LEAKY) return z > 0.0f ? 1.0f : kLeaky;
  return 1.0f;
}

// gate[t][j] = sigmoid(sum_k [x, s][t][k] Wg[k][j] + bg[j]), j < 2 n
__global__ __launch_bounds__(256) void gru_gates_kernel(const float* __restrict__ x, int in, const float* __restrict__ s,
                                                        int n, const float* __restrict__ Wg,
                                                        const float* __restrict__ bg, int B, float* __restrict__ gate) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n2 = 2 * n;
  if (idx >= (int64_t)B * n2) return;
  const int t = (int)(idx / n2), j = (int)(idx - (int64_t)t * n2);
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < in; ++k) acc = __builtin_fmaf(x[(int64_t)t * in + k], Wg[(int64_t)k * n2 + j], acc);
#pragma unroll 8
  for (int k = 0; k < n; ++k) acc = __builtin_fmaf(s[(int64_t)t * n + k], Wg[(int64_t)(in + k) * n2 + j], acc);
  gate[idx] = sigmoidf_(acc + bg[j]);
}

// c = act([x, r * s] Wc + bc), h = u s + (1 - u) c
__global__ __launch_bounds__(256) void gru_cand_kernel(const float* __restrict__ x, int in, const float* __restrict__ s,
                                                       int n, const float* __restrict__ Wc,
                                                       const float* __restrict__ bc, const float* __restrict__ gate,
                                                       int act, int B, float* __restrict__ c, float* __restrict__ h) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n) return;
  const int t = (int)(idx / n), j = (int)(idx - (int64_t)t * n);
  const float* g = gate + (int64_t)t * 2 * n;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < in; ++k) acc = __builtin_fmaf(x[(int64_t)t * in + k], Wc[(int64_t)k * n + j], acc);
#pragma unroll 8
  for (int k = 0; k < n; ++k) acc = __builtin_fmaf(g[k] * s[(int64_t)t * n + k], Wc[(int64_t)(in + k) * n + j], acc);
  const float cv = hidden_act(act, acc + bc[j]);
  const float u = g[n + j], sv = s[idx];
  c[idx] = cv;
  h[idx] = u * sv + (1.0f - u) * cv;
}

// h = u s + (1 - u) c:  dc = dh (1 - u) -> dpc = dc act'(c);  du = dh (s - c) -> dpg[:, n + j] = du u (1 - u)
__global__ __launch_bounds__(256) void gru_cellbwd_kernel(const float* __restrict__ dh, const float* __restrict__ s,
                                                          const float* __restrict__ gate, const float* __restrict__ c,
                                                          int act, int B, int n, float* __restrict__ dpc,
                                                          float* __restrict__ dpg) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n) return;
  const int t = (int)(idx / n), j = (int)(idx - (int64_t)t * n);
  const float d = dh[idx], u = gate[(int64_t)t * 2 * n + n + j], cv = c[idx], sv = s[idx];
  dpc[idx] = d * (1.0f - u) * hidden_dact(act, cv);
  dpg[(int64_t)t * 2 * n + n + j] = d * (sv - cv) * (u * (1.0f - u));
}

// d(r s)[t][k] = sum_j dpc[t][j] Wc[in + k][j];  dr = d(r s) s;  dpg[:, k] = dr r (1 - r)
__global__ __launch_bounds__(256) void gru_dr_kernel(const float* __restrict__ dpc, const float* __restrict__ Wc,
                                                     const float* __restrict__ s, const float* __restrict__ gate, int in,
                                                     int B, int n, float* __restrict__ dpg) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n) return;
  const int t = (int)(idx / n), k = (int)(idx - (int64_t)t * n);
  const float* w = Wc + (int64_t)(in + k) * n;
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < n; ++j) acc = __builtin_fmaf(dpc[(int64_t)t * n + j], w[j], acc);
  const float r = gate[(int64_t)t * 2 * n + k];
  dpg[(int64_t)t * 2 * n + k] = acc * s[idx] * (r * (1.0f - r));
}

// dx[t][k] = sum_j dpc[t][j] Wc[k][j] + sum_j dpg[t][j] Wg[k][j] (+ reg x0[t][k] in layer 0: per slot)
__global__ __launch_bounds__(256) void gru_dx_kernel(const float* __restrict__ dpc, const float* __restrict__ dpg,
                                                     const float* __restrict__ Wc, const float* __restrict__ Wg, int in,
                                                     int B, int n, const float* __restrict__ x0, float reg,
                                                     float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * in) return;
  const int t = (int)(idx / in), k = (int)(idx - (int64_t)t * in);
  float acc = 0.0f;
#pragma unroll 8
  for (int j = 0; j < n; ++j) acc = __builtin_fmaf(dpc[(int64_t)t * n + j], Wc[(int64_t)k * n + j], acc);
#pragma unroll 8
  for (int j = 0; j < 2 * n; ++j) acc = __builtin_fmaf(dpg[(int64_t)t * 2 * n + j], Wg[(int64_t)k * 2 * n + j], acc);
  dx[idx] = x0 ? acc + reg * x0[idx] : acc;
}

// rows k < in + n: G_Wg[k][j] = sum_t [x, s][t][k] dpg[t][j] (j < 2 n), G_Wc[k][j - 2 n] = sum_t [x, r s][t][k] dpc[t][.]
// row k = in + n: the bias gradients, sum_t of the column.  Slot order, one chain per element.
__global__ __launch_bounds__(256) void gru_dw_kernel(const float* __restrict__ x, int in, const float* __restrict__ s,
                                                     const float* __restrict__ gate, const float* __restrict__ dpg,
                                                     const float* __restrict__ dpc, int B, int n, float* __restrict__ GWg,
                                                     float* __restrict__ Gbg, float* __restrict__ GWc,
                                                     float* __restrict__ Gbc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n3 = 3 * n, K = in + n;
  if (idx >= (int64_t)(K + 1) * n3) return;
  const int k = (int)(idx / n3), j = (int)(idx - (int64_t)k * n3);
  const bool gates = j < 2 * n;
  const float* g = gates ? dpg + j : dpc + (j - 2 * n);
  const int ldg = gates ? 2 * n : n;
  float acc = 0.0f;
  if (k == K) {
#pragma unroll 8
    for (int t = 0; t < B; ++t) acc += g[(int64_t)t * ldg];
    if (gates) Gbg[j] = acc;
    else Gbc[j - 2 * n] = acc;
    return;
  }
  if (k < in) {
#pragma unroll 8
    for (int t = 0; t < B; ++t) acc = __builtin_fmaf(x[(int64_t)t * in + k], g[(int64_t)t * ldg], acc);
  } else if (gates) {
#pragma unroll 8
    for (int t = 0; t < B; ++t) acc = __builtin_fmaf(s[(int64_t)t * n + (k - in)], g[(int64_t)t * ldg], acc);
  } else {
#pragma unroll 8
    for (int t = 0; t < B; ++t)
      acc = __builtin_fmaf(gate[(int64_t)t * 2 * n + (k - in)] * s[(int64_t)t * n + (k - in)], g[(int64_t)t * ldg], acc);
  }
  if (gates) GWg[(int64_t)k * 2 * n + j] = acc;
  else GWc[(int64_t)k * n + (j - 2 * n)] = acc;
}

// one wavefront per sorted key; the head of a run adds the run's slot rows in key (= slot) order and stores the row
__global__ __launch_bounds__(256) void gru_rows_kernel(const uint64_t* __restrict__ keys, int n_keys, int d,
                                                       const float* __restrict__ src, float* __restrict__ dst,
                                                       const float* __restrict__ src1, float* __restrict__ dst1) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_keys) return;
  const uint64_t key = keys[w];
  if (key == kSentinel) return;
  const uint32_t row = (uint32_t)(key >> 32);
  if (w > 0 && (uint32_t)(keys[w - 1] >> 32) == row) return;
  float a0 = 0.0f, a1 = 0.0f, ab = 0.0f;
  for (int q = w; q < n_keys; ++q) {
    const uint64_t kk = keys[q];
    if ((uint32_t)(kk >> 32) != row) break;
    const int t = (int)(uint32_t)kk;
    if (lane < d) a0 += src[(int64_t)t * d + lane];
    if (lane + 64 < d) a1 += src[(int64_t)t * d + lane + 64];
    if (src1) ab += src1[t];
  }
  if (lane < d) dst[(int64_t)row * d + lane] = a0;
  if (lane + 64 < d) dst[(int64_t)row * d + lane + 64] = a1;
  if (src1 && lane == 0) dst1[row] = ab;
}

int check_weights(const nrhip_gru4rec_weights& w, const char* who) {
  NR_REQUIRE(w.n_layers >= 1 && w.n_layers <= kL, NR_ERR_UNSUPPORTED, "%s: %d layers outside 1..%d", who, w.n_layers, kL);
  for (int l = 0; l < w.n_layers; ++l) {
    NR_REQUIRE(w.width[l] >= 1 && w.width[l] <= kW, NR_ERR_UNSUPPORTED, "%s: layer width %d outside 1..%d", who,
               w.width[l], kW);
    NR_REQUIRE(w.d_Wg[l] && w.d_bg[l] && w.d_Wc[l] && w.d_bc[l], NR_ERR_ARG, "%s: null weight pointer", who);
  }
  NR_REQUIRE(w.hidden_act == ACT_TANH || w.hidden_act == ACT_RELU, NR_ERR_ARG,
             "%s: unknown hidden_act %d (0 tanh, 1 relu)", who, w.hidden_act);
  return NR_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace
