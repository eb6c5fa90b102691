// rowkey_common.h — what the steps of the time-order models share (fpmc.hip, hrm.hip, npe.hip, transrec.hip,
// fpmcplus.hip): every table is read through embedding_lookup, so a row's gradient is the sum over its occurrences in
// the batch, taken in the order of sort keys (row << 32 | the model's low word), and STORED by the head of the row's run.
//
//   kSentinel / kScal / S_* / row_key   the key of a slot that takes no part, the four floats per slot in d_scal
//   group_lane / group_index / group_sum / group_any   a 256-thread workgroup as lane groups of DP lanes, one per batch
//                    slot or sorted key: this lane's first column, the group's index over the grid, the xor tree
//   pointwise_loss_g / instance_loss_g / store_slot   the forward kernels' tail: the loss and its derivative g of one
//                    instance, and its d_scal slot
//   slot_sums / block_sum / loss_kernel   the one-workgroup loss kernel: S_LOSS and S_L2 over the batch in double, the
//                    256-thread tree, and the kernel of a model whose regulariser is reg * (the slots' l2 sum)
//   head_row / load_row / for_run / store_row   the rows kernels' opening, walk and close
//   check_loss_kind  the host entries' refusal of a loss the mode does not have
//   NR_BY_WIDTH      the launch ladder over the width: KERNEL<lanes per row, columns per lane>
//
// A model writes its forward arithmetic, its key layout, its per-occurrence body and its extra loss term.  Every float
// sum is taken in a fixed order.  history_common.h takes the sentinel, the head test, the tree and the ladder from here.
#pragma once
#include "nr_common.h"

namespace nr {
namespace rowkey {

constexpr uint64_t kSentinel = 0x7fffffffffffffffull;     // a slot that takes no part sorts behind every key
constexpr int kScal = 4;                                  // floats per batch slot in d_scal
enum { S_G = 0, S_LOSS = 1, S_L2 = 2, S_OK = 3 };         // S_OK: the models with a dense gradient over the batch

__device__ __forceinline__ uint64_t row_key(int row, uint32_t low) { return ((uint64_t)(uint32_t)row << 32) | low; }

// ---- lane groups: DP lanes per row, 64 / DP groups per wavefront, 4 wavefronts per workgroup
template <int DP>
__device__ __forceinline__ int group_lane() { return (threadIdx.x & 63) % DP; }

// Index: int over the batch, int64_t over the sorted keys
template <int DP, class Index = int>
__device__ __forceinline__ Index group_index() {
  return (Index)(blockIdx.x * 4 + (threadIdx.x >> 6)) * (NR_WAVE / DP) + (threadIdx.x & 63) / DP;
}

// every x summed over its lane group, in all its lanes.  Groups are DP-aligned: the xor partners of a lane are lanes
// of its own group
template <int DP, class... T>
__device__ __forceinline__ void group_sum(T&... x) {
#pragma unroll
  for (int m = DP / 2; m >= 1; m >>= 1) ((x += __shfl_xor(x, m, NR_WAVE)), ...);
}

template <int DP>
__device__ __forceinline__ int group_any(int x) {
#pragma unroll
  for (int m = DP / 2; m >= 1; m >>= 1) x |= __shfl_xor(x, m, NR_WAVE);
  return x;
}

// ---- the forward kernels' tail
__device__ __forceinline__ void pointwise_loss_g(int kind, int B, float z, float x, float& loss, float& g) {
  // tf.losses.sigmoid_cross_entropy is a MEAN over the batch, every other loss of util/learner.py a sum
  const float scale = kind == nr::NR_POINT_CROSS_ENTROPY ? 1.0f / (float)B : 1.0f;
  loss = scale * nr::pointwise_loss(kind, z, x);
  g = scale * nr::pointwise_dloss(kind, z, x);
}

// slot t of a model with both modes: the pair's scores xi and xj, or xi against the label third[t]
__device__ __forceinline__ void instance_loss_g(int pairwise, int kind, int B, const void* third, int t, float xi,
                                                float xj, float& loss, float& g) {
  if (pairwise) {
    const float y = xi - xj;
    loss = nr::pairwise_loss(kind, y);
    g = nr::pairwise_dloss(kind, y);
  } else {
    pointwise_loss_g(kind, B, ((const float*)third)[t], xi, loss, g);
  }
}

// sq: the squares of the slot's looked-up rows
__device__ __forceinline__ void store_slot(float* sc, float g, float loss, float sq, bool ok) {
  sc[S_G] = g;
  sc[S_LOSS] = loss;
  sc[S_L2] = ok ? 0.5f * sq : 0.f;
}

// ---- the loss kernel: one workgroup of 256 threads
__device__ __forceinline__ void slot_sums(const float* d_scal, int batch, double& loss, double& l2) {
  for (int t = threadIdx.x; t < batch; t += 256) {
    const float* sc = d_scal + (int64_t)t * kScal;
    loss += (double)sc[S_LOSS];
    l2 += (double)sc[S_L2];
  }
}

// v[0..N) summed over the 256 threads by a fixed tree; thread 0 returns with the sums
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N]) {
  __shared__ double s[N][256];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n][threadIdx.x] = v[n];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int n = 0; n < N; ++n) s[n][threadIdx.x] += s[n][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = s[n][0];
  }
}

template <class Args>
__global__ __launch_bounds__(256) void loss_kernel(Args a) {
  double v[2] = {0.0, 0.0};
  slot_sums(a.d_scal, a.batch, v[0], v[1]);
  block_sum(v);
  if (threadIdx.x == 0) {
    a.d_loss2[0] = (float)v[0];
    a.d_loss2[1] = (float)((double)a.reg * v[1]);
  }
}

// ---- the rows kernels: lane group w of the sorted keys
// -1 unless key w is the head of a run, then the run's row (the upper half of its keys)
__device__ __forceinline__ int head_row(const uint64_t* keys, int64_t w) {
  const uint64_t key = keys[w];
  if (key == kSentinel) return -1;
  const uint32_t row = (uint32_t)(key >> 32);
  if (w > 0 && (uint32_t)(keys[w - 1] >> 32) == row) return -1;             // not the head of its run
  return (int)row;
}
__device__ __forceinline__ int head_row(const uint64_t* keys, int64_t n_keys, int64_t w) {
  return w < n_keys ? head_row(keys, w) : -1;
}

// row r of a [rows][d] table, columns c + k DP of this lane (zeros beyond d), and back
template <int DP, int CPL>
__device__ __forceinline__ void load_row(const float* table, int r, int d, int c, float (&own)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    own[k] = col < d ? table[(int64_t)r * d + col] : 0.f;
  }
}
template <int DP, int CPL>
__device__ __forceinline__ void store_row(float* table, int r, int d, int c, const float (&acc)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) table[(int64_t)r * d + col] = acc[k];
  }
}

// body(the low word) per key of the run of `row` that starts at w, in key order
template <class Body>
__device__ __forceinline__ void for_run(const uint64_t* keys, int64_t n_keys, int64_t w, int row, Body body) {
  for (int64_t q = w; q < n_keys; ++q) {
    const uint64_t kk = keys[q];
    if ((uint32_t)(kk >> 32) != (uint32_t)row) break;
    body((uint32_t)kk);
  }
}

// ---- host side
// NR_OK, or NR_ERR_ARG and the message of `entry`, for the losses of util/learner.py in the entry's mode
inline int check_loss_kind(const char* entry, int pairwise, int loss_kind) {
  if (pairwise)
    NR_REQUIRE(loss_kind >= nr::NR_PAIR_BPR && loss_kind <= nr::NR_PAIR_SQUARE, NR_ERR_ARG,
               "%s: unknown pairwise loss %d (0 bpr, 1 hinge, 2 square)", entry, loss_kind);
  else
    NR_REQUIRE(loss_kind == nr::NR_POINT_CROSS_ENTROPY || loss_kind == nr::NR_POINT_SQUARE, NR_ERR_ARG,
               "%s: unknown pointwise loss %d (0 cross_entropy, 1 square)", entry, loss_kind);
  return NR_OK;
}

// the grid of NR_BY_WIDTH: one lane group of dp lanes per each of `groups`, or a grid that is given as it is
inline dim3 width_grid(int64_t groups, int dp) {
  const int per = 4 * NR_WAVE / dp;
  return dim3((unsigned)((groups + per - 1) / per));
}
inline dim3 width_grid(dim3 grid, int) { return grid; }

}  // namespace rowkey
}  // namespace nr

// lane groups sized to d: KERNEL<lanes per row, columns per lane>.  `grid`: the number of lane groups (an integer) for
// the kernels with one group per slot or key, or the dim3 itself for the kernels that run a wavefront per instance
#define NR_BY_WIDTH(KERNEL, d, grid, st, ...)                                                                          \
  do {                                                                                                                 \
    using nr::rowkey::width_grid;                                                                                      \
    if ((d) <= 16) hipLaunchKernelGGL((KERNEL<16, 1>), width_grid(grid, 16), dim3(256), 0, st, __VA_ARGS__);           \
    else if ((d) <= 32) hipLaunchKernelGGL((KERNEL<32, 1>), width_grid(grid, 32), dim3(256), 0, st, __VA_ARGS__);      \
    else if ((d) <= 64) hipLaunchKernelGGL((KERNEL<64, 1>), width_grid(grid, 64), dim3(256), 0, st, __VA_ARGS__);      \
    else hipLaunchKernelGGL((KERNEL<64, 2>), width_grid(grid, 64), dim3(256), 0, st, __VA_ARGS__);                     \
  } while (0)
