// apr.hip — APR (He et al., SIGIR 2018): the step of model/general_recommender/APR.py on gfx950, the adversarial graph
// the class builds (APR.py:73-118) run the way the paper runs it: Delta from the plain gradient of THIS batch at the
// current tables, then one optimiser step on loss + reg l2 + reg_adv loss_adv with Delta constant.
//
// A row's perturbation is the normalised sum of the plain gradient over ALL of the row's occurrences in the batch, so
// the perturbed forward pass cannot start before every run of the first pass is complete: two dependent passes over
// the batch, each a forward kernel (a lane group per triplet) and a rows kernel (the head of each run of the sorted
// keys walks the run), with the kernel boundary as the dependency.
//
//   apr_l2_kernel          with_reg && reg != 0 only: NRHIP_APR_L2_BLOCKS workgroups over the whole tables, sum(x^2)/2
//                          in double (fixed grid, fixed order) and G = reg W everywhere — the dense part of the
//                          gradient; the rows kernels then overwrite the batch's rows
//   apr_forward_kernel     x_t, s_t = -sigmoid(-x_t), softplus(-x_t); three keys per triplet, row << 32 | slot * 4 + role
//                          (role 0 user, 1 positive, 2 negative; item rows at n_users + item); a triplet with an id
//                          outside its table writes the sentinel
//   nrhip_sort_u64         the 3 B keys, ascending
//   apr_rows_a_kernel      the head of a run at position w: Gamma over the run in key order, d_where[3 slot + role] = w
//                          for every occurrence; plain step: G[row] = Gamma (+ reg row) and done; adversarial step:
//                          |Gamma|^2 over the lane group, Delta (or the draw, or the given row), both stored at w
//   apr_adv_forward_kernel the perturbed scores through d_where: sa_t = -reg_adv sigmoid(-xa_t), softplus(-xa_t)
//   apr_rows_b_kernel      the head of a run: Gamma[w] + the adversarial terms of its occurrences in key order, the
//                          partners' perturbed rows rebuilt from d_where (+ reg row): the row of G
//   apr_loss_kernel        one workgroup: {loss, reg l2 + reg_adv loss_adv} in double by the fixed tree
//
// fp32, every float sum in a fixed order, no atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

enum { S_G_ADV = 2, S_LOSS_ADV = 3 };                     // the slot's second pair of d_scal floats

__device__ __forceinline__ float uniform01(uint64_t h) { return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f); }

// column `col` of the draw of key-space row `row` at (seed, step): N(0, 0.01^2) truncated at two standard deviations by
// redrawing (tf.truncated_normal), Box-Muller over a splitmix64 chain
__device__ __forceinline__ float truncated_draw(uint64_t seed, uint64_t step, int row, int col) {
  const uint64_t rk = nr::splitmix64(nr::splitmix64(seed ^ (step * 0x9e3779b97f4a7c15ull)) ^ (uint64_t)(uint32_t)row);
  uint64_t h = nr::splitmix64(rk ^ ((uint64_t)(uint32_t)col * 0xd1342543de82ef95ull));
  float z = 0.f;
  for (int tries = 0; tries < 64; ++tries) {              // P(|z| > 2) = 0.0455 a draw
    const float u1 = uniform01(h);
    h = nr::splitmix64(h);
    const float u2 = uniform01(h);
    h = nr::splitmix64(h);
    z = sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);
    if (fabsf(z) <= 2.0f) break;
  }
  return 0.01f * fminf(fmaxf(z, -2.0f), 2.0f);
}

__global__ __launch_bounds__(256) void apr_l2_kernel(nrhip_apr_step_args a) {
  const int64_t nP = (int64_t)a.n_users * a.d, n = nP + (int64_t)a.n_items * a.d;
  double v[1] = {0.0};
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)NRHIP_APR_L2_BLOCKS * 256) {
    const bool user = idx < nP;
    const float x = user ? a.d_P[idx] : a.d_Q[idx - nP];
    (user ? a.d_G_P[idx] : a.d_G_Q[idx - nP]) = a.reg * x;
    v[0] += 0.5 * (double)x * (double)x;
  }
  block_sum(v);
  if (threadIdx.x == 0) a.d_part[blockIdx.x] = v[0];
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void apr_forward_kernel(nrhip_apr_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items;
  const bool in = t < B;
  int u = -1, i = -1, j = -1;
  if (in) {
    u = a.d_users[t];
    i = a.d_pos[t];
    j = a.d_neg[t];
  }
  const bool ok = in && u >= 0 && u < U && i >= 0 && i < I && j >= 0 && j < I;
  float xi = 0.f, xj = 0.f;
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col];
        xi += p * a.d_Q[(int64_t)i * d + col];
        xj += p * a.d_Q[(int64_t)j * d + col];
      }
    }
  }
  group_sum<DP>(xi, xj);
  if (!in || c != 0) return;
  float* sc = a.d_scal + (int64_t)t * kScal;
  float s = 0.f, loss = 0.f;
  if (ok) {
    const float x = xi - xj;                               // output - output_neg, APR.py:78
    s = nr::bpr_dloss(x);
    loss = nr::bpr_loss(x);
    if (a.d_flag_P) a.d_flag_P[u] = 1;
    if (a.d_flag_Q) {
      a.d_flag_Q[i] = 1;
      a.d_flag_Q[j] = 1;
    }
  }
  sc[S_G] = s;
  sc[S_LOSS] = loss;
  sc[S_G_ADV] = 0.f;
  sc[S_LOSS_ADV] = 0.f;
  const uint32_t low = (uint32_t)t * 4u;
  a.d_keys[t] = ok ? row_key(u, low) : kSentinel;
  a.d_keys[(int64_t)B + t] = ok ? row_key(U + i, low + 1) : kSentinel;
  a.d_keys[2 * (int64_t)B + t] = ok ? row_key(U + j, low + 2) : kSentinel;
}

// the occurrence `low` of a run, with coefficient slot S: acc += g (Q[i] - Q[j]) for a user's row, +- g P[u] for an
// item's; with Delta != nullptr the partners are the perturbed rows
template <int DP, int CPL, int S>
__device__ __forceinline__ void add_occurrence(const nrhip_apr_step_args& a, uint32_t low, int c, const float* delta,
                                               float (&acc)[CPL]) {
  const int t = (int)(low >> 2), role = (int)(low & 3u), d = a.d;
  const float g = a.d_scal[(int64_t)t * kScal + S];
  if (role == 0) {
    const int i = a.d_pos[t], j = a.d_neg[t];
    const int64_t wi = delta ? a.d_where[3 * (int64_t)t + 1] : 0, wj = delta ? a.d_where[3 * (int64_t)t + 2] : 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        float qi = a.d_Q[(int64_t)i * d + col], qj = a.d_Q[(int64_t)j * d + col];
        if (delta) {
          qi += delta[wi * d + col];
          qj += delta[wj * d + col];
        }
        acc[k] += g * (qi - qj);
      }
    }
  } else {
    const int u = a.d_users[t];
    const int64_t wu = delta ? a.d_where[3 * (int64_t)t] : 0;
    const float gs = role == 1 ? g : -g;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        float p = a.d_P[(int64_t)u * d + col];
        if (delta) p += delta[wu * d + col];
        acc[k] += gs * p;
      }
    }
  }
}

// the row of G: acc (+ reg own row)
template <int DP, int CPL>
__device__ __forceinline__ void store_gradient(const nrhip_apr_step_args& a, int row, int c, float (&acc)[CPL]) {
  const bool user = row < a.n_users;
  const int r = user ? row : row - a.n_users;
  if (a.with_reg && a.reg != 0.f) {
    float own[CPL];
    load_row<DP, CPL>(user ? a.d_P : a.d_Q, r, a.d, c, own);
#pragma unroll
    for (int k = 0; k < CPL; ++k) acc[k] += a.reg * own[k];
  }
  store_row<DP, CPL>(user ? a.d_G_P : a.d_G_Q, r, a.d, c, acc);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void apr_rows_a_kernel(nrhip_apr_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int64_t n_keys = 3 * (int64_t)a.batch;
  const int d = a.d;
  const int row = head_row(a.d_keys, n_keys, w);
  // every lane group of a wavefront reaches the tree below: a group without a head carries zeros through it
  float acc[CPL] = {};
  if (row >= 0) {
    for_run(a.d_keys, n_keys, w, row, [&](uint32_t low) {
      add_occurrence<DP, CPL, S_G>(a, low, c, nullptr, acc);
      if (c == 0) a.d_where[3 * (int64_t)(low >> 2) + (low & 3u)] = (int32_t)w;
    });
  }
  if (!a.adversarial) {
    if (row >= 0) store_gradient<DP, CPL>(a, row, c, acc);
    return;
  }
  float dir[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    dir[k] = acc[k];
    if (a.adv_random && row >= 0 && col < d) dir[k] = truncated_draw(a.seed, a.step, row, col);
  }
  float n2 = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) n2 += dir[k] * dir[k];      // columns beyond d hold zeros
  group_sum<DP>(n2);
  if (row < 0) return;
  const float inv = 1.0f / sqrtf(fmaxf(n2, 1e-12f));        // tf.nn.l2_normalize(g, 1): g * rsqrt(max(sum g^2, 1e-12))
  float delta[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    delta[k] = (dir[k] * inv) * a.eps;
    if (a.d_delta_given && col < d) delta[k] = a.d_delta_given[(int64_t)row * d + col];
  }
  store_row<DP, CPL>(a.d_gamma + w * d, 0, d, c, acc);
  store_row<DP, CPL>(a.d_delta + w * d, 0, d, c, delta);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void apr_adv_forward_kernel(nrhip_apr_step_args a) {
  const int c = group_lane<DP>(), t = group_index<DP>();
  const int B = a.batch, d = a.d, U = a.n_users, I = a.n_items;
  int u = -1, i = -1, j = -1;
  if (t < B) {
    u = a.d_users[t];
    i = a.d_pos[t];
    j = a.d_neg[t];
  }
  // the test of the plain pass: d_where holds a position for the triplets that took part, and for no other
  const bool ok = u >= 0 && u < U && i >= 0 && i < I && j >= 0 && j < I;
  float xi = 0.f, xj = 0.f;
  if (ok) {
    const int64_t wu = a.d_where[3 * (int64_t)t], wi = a.d_where[3 * (int64_t)t + 1], wj = a.d_where[3 * (int64_t)t + 2];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float p = a.d_P[(int64_t)u * d + col] + a.d_delta[wu * d + col];
        const float qi = a.d_Q[(int64_t)i * d + col] + a.d_delta[wi * d + col];
        const float qj = a.d_Q[(int64_t)j * d + col] + a.d_delta[wj * d + col];
        xi += p * qi;
        xj += p * qj;
      }
    }
  }
  group_sum<DP>(xi, xj);
  if (!ok || c != 0) return;
  const float x = xi - xj;
  float* sc = a.d_scal + (int64_t)t * kScal;
  sc[S_G_ADV] = a.reg_adv * nr::bpr_dloss(x);
  sc[S_LOSS_ADV] = nr::bpr_loss(x);
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void apr_rows_b_kernel(nrhip_apr_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int64_t n_keys = 3 * (int64_t)a.batch;
  const int row = head_row(a.d_keys, n_keys, w);
  if (row < 0) return;
  float acc[CPL];
  load_row<DP, CPL>(a.d_gamma + w * a.d, 0, a.d, c, acc);
  for_run(a.d_keys, n_keys, w, row,
          [&](uint32_t low) { add_occurrence<DP, CPL, S_G_ADV>(a, low, c, a.d_delta, acc); });
  store_gradient<DP, CPL>(a, row, c, acc);
}

__global__ __launch_bounds__(256) void apr_loss_kernel(nrhip_apr_step_args a) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < a.batch; t += 256) {
    const float* sc = a.d_scal + (int64_t)t * kScal;
    v[0] += (double)sc[S_LOSS];
    v[1] += (double)sc[S_LOSS_ADV];
  }
  if (a.with_reg && a.reg != 0.f) v[2] = a.d_part[threadIdx.x];   // NRHIP_APR_L2_BLOCKS == 256 partial sums
  block_sum(v);
  if (threadIdx.x == 0) {
    a.d_loss2[0] = (float)v[0];
    a.d_loss2[1] = (float)((a.with_reg ? (double)a.reg * v[2] : 0.0) + (a.adversarial ? (double)a.reg_adv * v[1] : 0.0));
  }
}

}  // namespace

static_assert(NRHIP_APR_L2_BLOCKS == 256, "apr_loss_kernel reads one partial sum per thread");

extern "C" {

int nrhip_apr_step(const nrhip_apr_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "apr_step: null argument block");
  const nrhip_apr_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_APR_MAX_D, NR_ERR_UNSUPPORTED, "apr_step: embedding_size %d outside 1..%d", a.d,
             NRHIP_APR_MAX_D);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_APR_MAX_BATCH && a.n_users >= 0 && a.n_items >= 0 &&
                 (int64_t)a.n_users + (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG, "apr_step: bad sizes");
  const bool dense = a.with_reg && a.reg != 0.f;
  NR_REQUIRE(a.d_loss2 && (a.batch == 0 || (a.d_scal && a.d_keys)), NR_ERR_ARG, "apr_step: null pointer argument");
  NR_REQUIRE((a.batch == 0 && !dense) || (a.d_P && a.d_Q && a.d_G_P && a.d_G_Q), NR_ERR_ARG,
             "apr_step: null table pointer");
  NR_REQUIRE(a.batch == 0 || (a.d_users && a.d_pos && a.d_neg && a.d_where), NR_ERR_ARG,
             "apr_step: null pointer argument");
  NR_REQUIRE(a.batch == 0 || !a.adversarial || (a.d_gamma && a.d_delta), NR_ERR_ARG,
             "apr_step: an adversarial step needs d_gamma and d_delta");
  NR_REQUIRE(!dense || a.d_part, NR_ERR_ARG, "apr_step: reg != 0 needs d_part");
  hipStream_t st = (hipStream_t)stream;
  const int B = a.batch;
  const int64_t n_keys = 3 * (int64_t)B;
  if (dense) {
    hipLaunchKernelGGL(apr_l2_kernel, dim3(NRHIP_APR_L2_BLOCKS), dim3(256), 0, st, a);
    NR_LAUNCH_CHECK();
  }
  if (B > 0) {
    NR_BY_WIDTH(apr_forward_kernel, a.d, B, st, a);
    NR_LAUNCH_CHECK();
    NR_TRY(nrhip_sort_u64(a.d_keys, (int)n_keys, stream));
    NR_BY_WIDTH(apr_rows_a_kernel, a.d, n_keys, st, a);
    NR_LAUNCH_CHECK();
    if (a.adversarial) {
      NR_BY_WIDTH(apr_adv_forward_kernel, a.d, B, st, a);
      NR_LAUNCH_CHECK();
      NR_BY_WIDTH(apr_rows_b_kernel, a.d, n_keys, st, a);
      NR_LAUNCH_CHECK();
    }
  }
  if (B > 0 || dense) {
    hipLaunchKernelGGL(apr_loss_kernel, dim3(1), dim3(256), 0, st, a);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

}  // extern "C"
