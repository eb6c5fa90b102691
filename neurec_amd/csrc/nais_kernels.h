// nais_kernels.h — the kernels of nais.hip, in a header since deepicf.hip runs the same attention pooling: the scan,
// the forward walk, the backward walk (VEC: the gradient that reaches p is a vector per instance, not dout q), the
// rows / walk / reduce kernels of the step, and predict()'s mark / compact / project / pairs / gather kernels.
// nais.hip has the description of each; every TU that includes this file gets its own copy (anonymous namespace).
#pragma once
#include "history_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::hist;

enum { S_SUM = 5, S_SB = 6, S_PDQ = 7 };                  // d_scal beyond the shared slots
enum { F_PAD = 4 };
constexpr int kMaxD = NRHIP_NAIS_MAX_D, kMaxW = NRHIP_NAIS_MAX_W;
constexpr int kWS = kMaxW + 1;                            // odd row stride of W in LDS at the bounds

__device__ __forceinline__ float nais_act(int act, float z) {
  if (act == 0) return fmaxf(z, 0.f);
  if (act == 1) return 1.0f / (1.0f + expf(-z));
  if (act == 2) return tanhf(z);
  return z;
}
// d act / d z from z and a = act(z)
__device__ __forceinline__ float nais_dact(int act, float z, float a) {
  if (act == 0) return z > 0.f ? 1.f : 0.f;
  if (act == 1) return a * (1.f - a);
  if (act == 2) return 1.f - a * a;
  return 1.f;
}
__device__ __forceinline__ float nais_pow(float x, float e) { return e == 0.f ? 1.f : (e == 1.f ? x : powf(x, e)); }
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// d_off[b] = rows of the ragged buffer in front of instance b (its CSR row length each, the excluded slot included);
// F_PAD for the instances shorter than the longest history (n - 1 items) of their side
__global__ __launch_bounds__(256) void nais_scan_kernel(nrhip_nais_step_args a, int N) {
  __shared__ int64_t s_scan[256];
  __shared__ int s_max[256];
  __shared__ int s_lmax[2];
  const int tid = threadIdx.x;
  for (int side = 0; side < (a.pairwise ? 2 : 1); ++side) {
    int mx = 0;
    for (int t = tid; t < a.batch; t += 256) {
      const int b = side * a.batch + t;
      if (a.d_inst[4 * b + 3] & F_VALID) mx = max(mx, (int)a.d_n[b] - 1);
    }
    s_max[tid] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (tid < s) s_max[tid] = max(s_max[tid], s_max[tid + s]);
      __syncthreads();
    }
    if (tid == 0) s_lmax[side] = s_max[0];
    __syncthreads();
  }
  int64_t carry = 0;
  for (int base = 0; base < N; base += 256) {
    const int b = base + tid;
    int64_t len = 0;
    if (b < N && (a.d_inst[4 * b + 3] & F_VALID)) {
      const int u = a.d_inst[4 * b];
      len = a.d_indptr[u + 1] - a.d_indptr[u];
      if (a.reference_mask && (int)a.d_n[b] - 1 < s_lmax[b / a.batch]) a.d_inst[4 * b + 3] |= F_PAD;
    }
    s_scan[tid] = len;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const int64_t v = tid >= s ? s_scan[tid - s] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    if (b < N) a.d_off[b] = carry + s_scan[tid] - len;
    carry += s_scan[255];
    __syncthreads();
  }
  // the batch's history positions, and the largest any batch has asked of this buffer: the caller compares it with
  // row_cap (a batch beyond it has lost gradient rows — an error on the host side)
  if (tid == 0) {
    a.d_need[0] = carry;
    if (carry > a.d_need[1]) a.d_need[1] = carry;
  }
}

// what a wave keeps resident: W[0:d] (row stride ws, odd), b, h (zero beyond w), and per wave q, dz and the
// history ids of the round
struct NaisLds {
  float W[kMaxD * kWS];
  float b[kMaxW], h[kMaxW];
  float q[4][kMaxD];
  float dz[4][NR_WAVE];
  int hid[4][16];
};

__device__ __forceinline__ void nais_stage(NaisLds& L, const nrhip_nais_step_args& a, int ws) {
  for (int e = threadIdx.x; e < a.d * a.w; e += 256) L.W[(e / a.w) * ws + (e % a.w)] = a.d_W[e];
  for (int m = threadIdx.x; m < kMaxW; m += 256) {
    L.b[m] = m < a.w ? a.d_b[m] : 0.f;
    L.h[m] = m < a.w ? a.d_h[m] : 0.f;
  }
}

// the q-side part of z, lane column m: b (algorithm 0) or q W[d:2d] + b (algorithm 1); also the padding row's z
__device__ __forceinline__ float nais_zq(const NaisLds& L, const nrhip_nais_step_args& a, int wv, int m) {
  if (m >= a.w) return 0.f;
  float z = 0.f;
  if (a.algorithm == 1)
    for (int k = 0; k < a.d; ++k) z += L.q[wv][k] * a.d_W[(int64_t)(a.d + k) * a.w + m];
  return z + L.b[m];
}

// z of lane column m for the history row c (a pointer to c1[h]), without zq
__device__ __forceinline__ float nais_z(const NaisLds& L, const nrhip_nais_step_args& a, int wv, int ws, int m,
                                        const float* __restrict__ c) {
  const int mm = m < a.w ? m : a.w - 1;
  float z = 0.f;
  if (a.algorithm == 0)
    for (int k = 0; k < a.d; ++k) z += (c[k] * L.q[wv][k]) * L.W[k * ws + mm];
  else
    for (int k = 0; k < a.d; ++k) z += c[k] * L.W[k * ws + mm];
  return z;
}

template <int WP>
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int s = WP / 2; s >= 1; s >>= 1) x += __shfl_xor(x, s, NR_WAVE);
  return x;
}

template <int WP, int CPL>
__global__ __launch_bounds__(256) void nais_forward_kernel(nrhip_nais_step_args a, int N) {
  __shared__ NaisLds L;
  constexpr int G = NR_WAVE / WP;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wv;
  const int d = a.d, ws = a.w | 1, g = lane / WP, m = lane % WP;
  nais_stage(L, a, ws);
  const bool live = b < N;
  const int flags = live ? a.d_inst[4 * b + 3] : 0;
  const int item = live ? a.d_inst[4 * b + 1] : 0;
  if (flags & F_VALID)
    for (int k = lane; k < d; k += NR_WAVE) L.q[wv][k] = a.d_Q[(int64_t)item * d + k];
  __syncthreads();
  if (!live) return;
  float* sc = a.d_scal + (int64_t)b * kScal;
  if (!(flags & F_VALID)) {
    if (lane < kScal) sc[lane] = 0.f;
    return;
  }
  const int u = a.d_inst[4 * b], excl = a.d_inst[4 * b + 2];
  const float zq = nais_zq(L, a, wv, m), hm = L.h[m < kMaxW ? m : 0] * (m < a.w ? 1.f : 0.f);
  double S = 0.0, csq = 0.0, pe[CPL];
#pragma unroll
  for (int t = 0; t < CPL; ++t) pe[t] = 0.0;
  const int64_t b0 = a.d_indptr[u], e0 = a.d_indptr[u + 1];
  for (int64_t k0 = b0; k0 < e0; k0 += G) {
    const int64_t k = k0 + g;
    const int hh = k < e0 ? a.d_indices[k] : -1;
    const bool on = hh >= 0 && hh != excl && hh < a.n_items;
    const float* c = a.d_c1 + (int64_t)(on ? hh : 0) * d;
    const float z = nais_z(L, a, wv, ws, m, c) + zq;
    const float s = group_sum<WP>(nais_act(a.activation, z) * hm);
    if (!on) continue;
    if (a.d_flag_c1 && m == 0) a.d_flag_c1[hh] = 1;
    const float e = expf(s);
    S += (double)e;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int col = m + t * WP;
      if (col < d) {
        const float cv = c[col];
        pe[t] += (double)(e * cv);
        csq += (double)(cv * cv);
      }
    }
  }
#pragma unroll
  for (int s = WP; s < NR_WAVE; s <<= 1) {
    S += shfl_xor_f64(S, s);
#pragma unroll
    for (int t = 0; t < CPL; ++t) pe[t] += shfl_xor_f64(pe[t], s);
  }
#pragma unroll
  for (int s = 1; s < NR_WAVE; s <<= 1) csq += shfl_xor_f64(csq, s);
  if (flags & F_PAD) S += (double)expf(group_sum<WP>(nais_act(a.activation, zq) * hm));
  const float Sf = (float)S, SB = nais_pow(Sf, a.beta);
  float dot = 0.f, qsq = 0.f;
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    const int col = m + t * WP;
    if (col < d) {
      const float pf = Sf > 0.f ? (float)pe[t] / SB : 0.f, q = L.q[wv][col];
      if (g == 0) a.d_p[(int64_t)b * d + col] = pf;
      dot += pf * q;
      qsq += q * q;
    }
  }
  dot = group_sum<WP>(dot);
  qsq = group_sum<WP>(qsq);
  if (lane == 0) {
    const float coeff = nais_pow(a.d_n[b], a.alpha);
    sc[S_OUT] = coeff * dot + a.d_bias[item];
    sc[S_COEFF] = coeff;
    sc[S_RSQ] = (float)csq;
    sc[S_QSQ] = qsq;
    sc[S_SUM] = Sf;
    sc[S_SB] = SB;
    sc[S_PDQ] = dot;
  }
}

// VEC (deepicf.hip): d loss / d p is the vector gp[b] (NAIS: dout n^alpha q), and what reaches Q[i] beside the
// attention's own part is the vector gq[b] (NAIS: dout n^alpha p + reg_q q).  !VEC is NAIS's arithmetic, unchanged.
template <int WP, int CPL, bool VEC>
__device__ __forceinline__ void nais_backward_body(NaisLds& L, const nrhip_nais_step_args& a, int N,
                                                   const float* __restrict__ gp, const float* __restrict__ gq) {
  constexpr int G = NR_WAVE / WP;
  static_assert(G <= 16, "hid holds 16 groups");
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wv;
  const int d = a.d, w = a.w, ws = a.w | 1, g = lane / WP, m = lane % WP, dw = d * w;
  nais_stage(L, a, ws);
  const bool live = b < N;
  const int flags = live ? a.d_inst[4 * b + 3] : 0;
  const int item = live ? a.d_inst[4 * b + 1] : 0;
  if (flags & F_VALID)
    for (int k = lane; k < d; k += NR_WAVE) L.q[wv][k] = a.d_Q[(int64_t)item * d + k];
  __syncthreads();
  if (!live || !(flags & F_VALID)) return;
  const int u = a.d_inst[4 * b], excl = a.d_inst[4 * b + 2], act = a.activation;
  const float* sc = a.d_scal + (int64_t)b * kScal;
  const float f = VEC ? 0.f : sc[S_DOUT] * sc[S_COEFF], Sf = sc[S_SUM], SB = sc[S_SB];
  float gv[CPL], dpp = f * sc[S_PDQ];
#pragma unroll
  for (int t = 0; t < CPL; ++t) gv[t] = 0.f;
  if constexpr (VEC) {
    float gpp = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int col = m + t * WP;
      if (col < d) {
        gv[t] = gp[(int64_t)b * d + col];
        gpp += gv[t] * a.d_p[(int64_t)b * d + col];
      }
    }
    dpp = group_sum<WP>(gpp);
  }
  const float regp = (flags & F_REGP) ? a.reg_p : 0.f;
  const float zq = nais_zq(L, a, wv, m), hm = m < w ? L.h[m] : 0.f;
  float* dWp = a.d_dWp + (int64_t)b * dw;
  // the instance's partial of dW[0:d]: entry e = lane + 64 t belongs to one lane; up to 512 entries stay in registers,
  // a larger W is accumulated in place
  constexpr int kRegE = 8;
  const bool inreg = dw <= kRegE * NR_WAVE;
  float wacc[kRegE];
  int wk[kRegE], wm[kRegE];
#pragma unroll
  for (int t = 0; t < kRegE; ++t) {
    const int e = lane + t * NR_WAVE;
    wacc[t] = 0.f;
    wk[t] = e < dw ? e / w : 0;
    wm[t] = e < dw ? e - wk[t] * w : 0;
  }
  if (!inreg)
    for (int e = lane; e < dw; e += NR_WAVE) dWp[e] = 0.f;
  float dh = 0.f, db = 0.f, dq[CPL];
#pragma unroll
  for (int t = 0; t < CPL; ++t) dq[t] = 0.f;
  const int64_t b0 = a.d_indptr[u], e0 = a.d_indptr[u + 1], off = a.d_off[b];
  for (int64_t k0 = b0; k0 < e0; k0 += G) {
    const int64_t k = k0 + g;
    const int hh = k < e0 ? a.d_indices[k] : -1;
    const bool on = hh >= 0 && hh != excl && hh < a.n_items;
    const float* c = a.d_c1 + (int64_t)(on ? hh : 0) * d;
    const float z = nais_z(L, a, wv, ws, m, c) + zq;
    const float av = nais_act(act, z);
    const float s = group_sum<WP>(av * hm);
    float cq = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int col = m + t * WP;
      if (col < d) cq += c[col] * (VEC ? gv[t] : L.q[wv][col]);
    }
    cq = group_sum<WP>(cq);
    float A = 0.f, dz = 0.f;
    if (on && Sf > 0.f) {
      const float e = expf(s);
      A = e / SB;
      const float ds = A * (VEC ? cq : f * cq) - a.beta * (e / Sf) * dpp;
      dz = ds * hm * nais_dact(act, z, av);
      dh += ds * av;
      db += dz;
    }
    if (a.c1_sort && m == 0 && k < e0) {                  // (item | position) of this row of the ragged buffer
      const int64_t r = off + (k - b0);
      if (r < a.row_cap) a.d_pkeys[r] = on ? (((uint64_t)(uint32_t)hh << 32) | (uint32_t)r) : kSentinel;
    }
    wave_sync_lds();                                      // the round before has read dz / hid
    L.dz[wv][lane] = dz;
    if (m == 0) L.hid[wv][g] = on ? hh : -1;
    wave_sync_lds();
    if (on) {
      const int64_t r = off + (k - b0);
#pragma unroll
      for (int t = 0; t < CPL; ++t) {
        const int col = m + t * WP;
        if (col < d) {
          float dx = 0.f;
          for (int m2 = 0; m2 < w; ++m2) dx += L.W[col * ws + m2] * L.dz[wv][g * WP + m2];
          const float cv = c[col], qv = L.q[wv][col];
          float dc = A * (VEC ? gv[t] : f * qv);
          if (a.algorithm == 0) {
            dc += dx * qv;
            dq[t] += dx * cv;
          } else {
            dc += dx;
          }
          dc += regp * cv;
          if (r < a.row_cap) a.d_rows[r * d + col] = dc;
        }
      }
    }
    // the round's rows in group order
    if (inreg) {
#pragma unroll
      for (int t = 0; t < kRegE; ++t) {
        if (lane + t * NR_WAVE < dw) {
          const float qv = a.algorithm == 0 ? L.q[wv][wk[t]] : 1.f;
#pragma unroll
          for (int gg = 0; gg < G; ++gg) {
            const int h2 = L.hid[wv][gg];
            if (h2 >= 0) wacc[t] += (a.d_c1[(int64_t)h2 * d + wk[t]] * qv) * L.dz[wv][gg * WP + wm[t]];
          }
        }
      }
    } else
    for (int e = lane; e < dw; e += NR_WAVE) {
      const int kk = e / w, mm = e - kk * w;
      float v = dWp[e];
      const float qv = a.algorithm == 0 ? L.q[wv][kk] : 1.f;
#pragma unroll
      for (int gg = 0; gg < G; ++gg) {
        const int h2 = L.hid[wv][gg];
        if (h2 >= 0) v += (a.d_c1[(int64_t)h2 * d + kk] * qv) * L.dz[wv][gg * WP + mm];
      }
      dWp[e] = v;
    }
  }
  if (inreg) {
#pragma unroll
    for (int t = 0; t < kRegE; ++t)
      if (lane + t * NR_WAVE < dw) dWp[lane + t * NR_WAVE] = wacc[t];
  }
#pragma unroll
  for (int s = WP; s < NR_WAVE; s <<= 1) {
    dh += __shfl_xor(dh, s, NR_WAVE);
    db += __shfl_xor(db, s, NR_WAVE);
#pragma unroll
    for (int t = 0; t < CPL; ++t) dq[t] += __shfl_xor(dq[t], s, NR_WAVE);
  }
  if ((flags & F_PAD) && Sf > 0.f) {
    const float ap = nais_act(act, zq);
    const float ep = expf(group_sum<WP>(ap * hm));
    const float ds = -a.beta * (ep / Sf) * dpp;
    const float dz = ds * hm * nais_dact(act, zq, ap);
    dh += ds * ap;
    db += dz;
  }
  wave_sync_lds();
  L.dz[wv][lane] = db;                                    // group 0's copy is read below
  wave_sync_lds();
  if (g == 0 && m < w) {
    a.d_dbp[(int64_t)b * w + m] = db;
    a.d_dhp[(int64_t)b * w + m] = dh;
  }
  if (g == 0) {
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int col = m + t * WP;
      if (col < d) {
        float v = dq[t];
        if (a.algorithm == 1)
          for (int m2 = 0; m2 < w; ++m2) v += a.d_W[(int64_t)(d + col) * w + m2] * L.dz[wv][m2];
        if constexpr (VEC) a.d_dqp[(int64_t)b * d + col] = gq[(int64_t)b * d + col] + v;
        else a.d_dqp[(int64_t)b * d + col] = f * a.d_p[(int64_t)b * d + col] + v + a.reg_q * L.q[wv][col];
      }
    }
  }
}

template <int WP, int CPL>
__global__ __launch_bounds__(256) void nais_backward_kernel(nrhip_nais_step_args a, int N) {
  __shared__ NaisLds L;
  nais_backward_body<WP, CPL, false>(L, a, N, nullptr, nullptr);
}

// waves [0, 2N): the sorted keys
template <int CPL>
__global__ __launch_bounds__(256) void nais_rows_kernel(nrhip_nais_step_args a, int N) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int d = a.d;
  if (w >= 2 * N) return;
  const int head = item_run_head(a, w, lane);
  if (head < 0) return;
  const uint32_t row = (uint32_t)head;
  const int item = head - a.n_users;
  float acc[CPL], gb = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
  for (int k = w; k < 2 * N; ++k) {
    const uint64_t kk = a.d_keys[k];
    if ((uint32_t)(kk >> 32) != row) break;
    const int b = (int)(uint32_t)kk;
    gb += a.d_scal[(int64_t)b * kScal + S_DOUT];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) acc[j] += a.d_dqp[(int64_t)b * d + col];
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < d) a.d_G_Q[(int64_t)item * d + col] = acc[j];
  }
  if (lane == 0) a.d_G_bias[item] = gb;
}

template <int CPL>
__global__ __launch_bounds__(256) void nais_walk_kernel(nrhip_nais_step_args a, int N) {
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= a.n_items) return;
  walk_column<CPL>(
      a, N, h, lane,
      // where h stands in the user's (ascending) row: the ragged buffer keeps the row's order
      [&](int uu) -> int64_t {
        int64_t lo = a.d_indptr[uu], hi = a.d_indptr[uu + 1];
        const int64_t r0 = lo;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (a.d_indices[mid] < h) lo = mid + 1; else hi = mid;
        }
        return (lo >= a.d_indptr[uu + 1] || a.d_indices[lo] != h) ? -1 : lo - r0;
      },
      [&](int b, int64_t rpos) -> const float* {
        const int64_t r = a.d_off[b] + rpos;
        return r >= a.row_cap ? nullptr : a.d_rows + r * a.d;
      });
}

__global__ __launch_bounds__(256) void nais_fill_keys_kernel(nrhip_nais_step_args a) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < a.row_cap) a.d_pkeys[r] = kSentinel;
}

// the other way to G_c1: the sorted (item | position) keys; the head of an item's run adds the ragged buffer's rows
// of that item in position order (= batch order, then the order of the train row).  G_c1 is zeroed before.
template <int CPL>
__global__ __launch_bounds__(256) void nais_segsum_kernel(nrhip_nais_step_args a) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, d = a.d;
  if (w >= a.row_cap) return;
  const uint64_t key = a.d_pkeys[w];
  if (key == kSentinel) return;
  const uint32_t item = (uint32_t)(key >> 32);
  if (w > 0 && (uint32_t)(a.d_pkeys[w - 1] >> 32) == item) return;
  float acc[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
  for (int64_t k = w; k < a.row_cap; ++k) {
    const uint64_t kk = a.d_pkeys[k];
    if (kk == kSentinel || (uint32_t)(kk >> 32) != item) break;
    const int64_t r = (int64_t)(uint32_t)kk;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int col = lane + j * NR_WAVE;
      if (col < d) acc[j] += a.d_rows[r * d + col];
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int col = lane + j * NR_WAVE;
    if (col < d) a.d_G_c1[(int64_t)item * d + col] = acc[j];
  }
}

__global__ __launch_bounds__(256) void nais_reduce_kernel(nrhip_nais_step_args a, int N) {
  const int d = a.d, w = a.w, rw = (a.algorithm == 1 ? 2 * d : d) * w;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rw + 2 * w) return;
  float acc = 0.f;
  if (e < d * w) {
    for (int b = 0; b < N; ++b)
      if (a.d_inst[4 * b + 3] & F_VALID) acc += a.d_dWp[(int64_t)b * d * w + e];
    a.d_G_W[e] = acc;
  } else if (e < rw) {
    const int k = e / w - d, m = e % w;
    for (int b = 0; b < N; ++b)
      if (a.d_inst[4 * b + 3] & F_VALID)
        acc += a.d_Q[(int64_t)a.d_inst[4 * b + 1] * d + k] * a.d_dbp[(int64_t)b * w + m];
    a.d_G_W[e] = acc;
  } else {
    const bool is_b = e < rw + w;
    const int m = e - rw - (is_b ? 0 : w);
    const float* src = is_b ? a.d_dbp : a.d_dhp;
    for (int b = 0; b < N; ++b)
      if (a.d_inst[4 * b + 3] & F_VALID) acc += src[(int64_t)b * w + m];
    (is_b ? a.d_G_b : a.d_G_h)[m] = acc;
  }
}

// ------------------------------------------------------------------ predict()
__global__ __launch_bounds__(256) void nais_mark_kernel(nrhip_nais_scores_args a) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= a.batch) return;
  const int u = a.d_users[b];
  if (u < 0 || u >= a.n_users) return;
  for (int64_t k = a.d_indptr[u] + lane; k < a.d_indptr[u + 1]; k += NR_WAVE) {
    const int h = a.d_indices[k];
    if (h >= 0 && h < a.n_items) a.d_map[h] = 0;          // every writer stores the same value
  }
}

// d_map[h]: -1 or the index of h among the block's distinct history items; d_hs: those items, ascending
__global__ __launch_bounds__(256) void nais_compact_kernel(nrhip_nais_scores_args a) {
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int base = 0; base < a.n_items; base += 256) {
    const int h = base + tid;
    const bool on = h < a.n_items && a.d_map[h] == 0;
    const uint64_t bal = __ballot(on);
    if (lane == 0) s_cnt[wv] = __builtin_popcountll(bal);
    __syncthreads();
    int before = carry;
    for (int v = 0; v < wv; ++v) before += s_cnt[v];
    const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (on) {
      const int idx = before + nr_mbcnt(bal);
      a.d_map[h] = idx < a.h_cap ? idx : -1;
      if (idx < a.h_cap) a.d_hs[idx] = h;
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) a.d_cnt[0] = carry < a.h_cap ? carry : a.h_cap;
}

// [I][w] projections of algorithm 1: cW = c1 W[0:d], qW = Q W[d:2d] + b
__global__ __launch_bounds__(256) void nais_project_kernel(nrhip_nais_scores_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)a.n_items * a.w) return;
  const int i = (int)(e / a.w), m = (int)(e % a.w);
  float x = 0.f, y = 0.f;
  for (int k = 0; k < a.d; ++k) {
    x += a.d_c1[(int64_t)i * a.d + k] * a.d_W[(int64_t)k * a.w + m];
    y += a.d_Q[(int64_t)i * a.d + k] * a.d_W[(int64_t)(a.d + k) * a.w + m];
  }
  a.d_cW[e] = x;
  a.d_qW[e] = y + a.d_b[m];
}

constexpr int kHC = 32;                                   // history items per workgroup of the pair kernel

// E[hidx][il] = e(i, h), F[hidx][il] = e(i, h) (c1[h] . Q[i]) for the tile's targets i = i0 + il (one per thread) and
// kHC history items of the block's list; c1 rows, W, b, h come from LDS at wave-uniform addresses
template <int DK, int WT, int ALG>
__global__ __launch_bounds__(256) void nais_pairs_kernel(nrhip_nais_scores_args a, int i0, int ti) {
  __shared__ float s_c[kHC * DK];
  __shared__ float s_W[ALG == 0 ? DK * WT : 1];
  __shared__ float s_cW[ALG == 1 ? kHC * WT : 1];
  __shared__ float s_b[WT], s_h[WT];
  const int cnt = a.d_cnt[0], h0 = blockIdx.y * kHC;
  if (h0 >= cnt) return;
  const int nh = min(kHC, cnt - h0), d = a.d, w = a.w, tid = threadIdx.x;
  for (int e = tid; e < kHC * DK; e += 256) {
    const int hh = e / DK, k = e % DK;
    s_c[e] = (hh < nh && k < d) ? a.d_c1[(int64_t)a.d_hs[h0 + hh] * d + k] : 0.f;
  }
  if (ALG == 0) {
    for (int e = tid; e < DK * WT; e += 256) {
      const int k = e / WT, m = e % WT;
      s_W[e] = (k < d && m < w) ? a.d_W[(int64_t)k * w + m] : 0.f;
    }
  } else {
    for (int e = tid; e < kHC * WT; e += 256) {
      const int hh = e / WT, m = e % WT;
      s_cW[e] = (hh < nh && m < w) ? a.d_cW[(int64_t)a.d_hs[h0 + hh] * w + m] : 0.f;
    }
  }
  for (int m = tid; m < WT; m += 256) {
    s_b[m] = (ALG == 0 && m < w) ? a.d_b[m] : 0.f;
    s_h[m] = m < w ? a.d_h[m] : 0.f;
  }
  __syncthreads();
  const int il = blockIdx.x * 256 + tid, i = i0 + il;
  if (il >= ti || i >= a.n_items) return;
  // Q[i] stays in registers up to 32 columns; wider rows are read again, 16 columns at a time (the unrolled
  // d x w body would not fit the instruction cache)
  constexpr bool QREG = DK <= 32;
  float q[QREG ? DK : 1], zq[ALG == 1 ? WT : 1];
  const float* qrow = a.d_Q + (int64_t)i * d;
  if (QREG) {
#pragma unroll
    for (int k = 0; k < (QREG ? DK : 1); ++k) q[k] = k < d ? qrow[k] : 0.f;
  }
  if (ALG == 1) {
#pragma unroll
    for (int m = 0; m < WT; ++m) zq[m] = m < w ? a.d_qW[(int64_t)i * w + m] : 0.f;
  }
  const int act = a.activation;
  for (int hh = 0; hh < nh; ++hh) {
    float z[WT], dot = 0.f;
#pragma unroll
    for (int m = 0; m < WT; ++m) z[m] = ALG == 0 ? s_b[m] : s_cW[hh * WT + m] + zq[m];
    if constexpr (QREG) {
#pragma unroll
      for (int k = 0; k < DK; ++k) {
        const float x = s_c[hh * DK + k] * q[k];
        dot += x;
        if (ALG == 0) {
#pragma unroll
          for (int m = 0; m < WT; ++m) z[m] = fmaf(x, s_W[k * WT + m], z[m]);
        }
      }
    } else {
#pragma unroll 1
      for (int k0 = 0; k0 < DK; k0 += 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int k = k0 + j;
          const float x = s_c[hh * DK + k] * (k < d ? qrow[k] : 0.f);
          dot += x;
          if (ALG == 0) {
#pragma unroll
            for (int m = 0; m < WT; ++m) z[m] = fmaf(x, s_W[k * WT + m], z[m]);
          }
        }
      }
    }
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < WT; ++m) s = fmaf(nais_act(act, z[m]), s_h[m], s);
    const float e = expf(s);
    const int64_t o = (int64_t)(h0 + hh) * ti + il;
    a.d_E[o] = e;
    a.d_F[o] = e * dot;
  }
}

// The same E / F on the fp32 matrix cores, for algorithm 0 with d <= 16 and w <= 16: v_mfma_f32_16x16x4f32 takes 16
// (target, history item) rows x 4 of the d columns (built in registers: c1[h][k] Q[i][k]) against 4 rows of W; four of
// them give z for 16 targets of one history item, accumulator = b.  Lane (t = lane % 16, kq = lane / 16) holds row t,
// column 4 kk + kq of the pair rows, W[4 kk + kq][t], and of the result the rows 4 kq + r, column t.  A wave takes 4
// groups of 16 targets, a workgroup 256 targets and kHC history items, as the VALU kernel.
typedef float nais_v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void nais_pairs_mfma_kernel(nrhip_nais_scores_args a, int i0, int ti) {
  __shared__ float s_c[kHC * 16];
  __shared__ float s_e[4][16];
  const int cnt = a.d_cnt[0], h0 = blockIdx.y * kHC;
  if (h0 >= cnt) return;
  const int nh = min(kHC, cnt - h0), d = a.d, w = a.w, tid = threadIdx.x;
  for (int e = tid; e < kHC * 16; e += 256) {
    const int hh = e / 16, k = e % 16;
    s_c[e] = (hh < nh && k < d) ? a.d_c1[(int64_t)a.d_hs[h0 + hh] * d + k] : 0.f;
  }
  const int wv = tid >> 6, lane = tid & 63, t = lane & 15, kq = lane >> 4, act = a.activation;
  float Wr[4], q[4][4];
  const float br = t < w ? a.d_b[t] : 0.f, hr = t < w ? a.d_h[t] : 0.f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int k = 4 * kk + kq;
    Wr[kk] = (k < d && t < w) ? a.d_W[(int64_t)k * w + t] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int il = blockIdx.x * 256 + wv * 64 + g * 16 + t, i = i0 + il;
      q[g][kk] = (il < ti && i < a.n_items && k < d) ? a.d_Q[(int64_t)i * d + k] : 0.f;
    }
  }
  __syncthreads();
  for (int hh = 0; hh < nh; ++hh) {
    float c[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) c[kk] = s_c[hh * 16 + 4 * kk + kq];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      nais_v4f acc = {br, br, br, br};
      float dot = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float x = c[kk] * q[g][kk];
        dot += x;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x, Wr[kk], acc, 0, 0, 0);
      }
      dot += __shfl_xor(dot, 16, NR_WAVE);                // c1[h] . Q[i_t] in every lane of column t
      dot += __shfl_xor(dot, 32, NR_WAVE);
      float s[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = nais_act(act, acc[r]) * hr;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += __shfl_xor(s[r], m, NR_WAVE);
      }
      if (t == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s_e[wv][4 * kq + r] = expf(s[r]);
      }
      wave_sync_lds();
      if (lane < 16) {
        const int il = blockIdx.x * 256 + wv * 64 + g * 16 + lane;
        if (il < ti && i0 + il < a.n_items) {
          const float e = s_e[wv][lane];
          const int64_t o = (int64_t)(h0 + hh) * ti + il;
          a.d_E[o] = e;
          a.d_F[o] = e * dot;
        }
      }
      wave_sync_lds();
    }
  }
}

// out[b][i] = |R_u|^alpha (sum_{h in R_u} F[h][i]) / (sum_{h in R_u} E[h][i])^beta + bias[i], the row in CSR order
__global__ __launch_bounds__(256) void nais_gather_kernel(nrhip_nais_scores_args a, int i0, int ti) {
  const int il = blockIdx.x * 256 + threadIdx.x, i = i0 + il, b = blockIdx.y;
  if (il >= ti || i >= a.n_items) return;
  const int u = a.d_users[b];
  float* out = a.d_out + (int64_t)b * a.ld;
  const float bias = a.d_bias[i];
  if (u < 0 || u >= a.n_users || a.d_indptr[u + 1] == a.d_indptr[u]) {      // no train row: the bias alone
    out[i] = bias;
    return;
  }
  double num = 0.0, den = 0.0;
  const int64_t b0 = a.d_indptr[u], e0 = a.d_indptr[u + 1];
  for (int64_t k = b0; k < e0; ++k) {
    const int h = a.d_indices[k];
    const int idx = (h >= 0 && h < a.n_items) ? a.d_map[h] : -1;
    if (idx < 0) continue;
    num += (double)a.d_F[(int64_t)idx * ti + il];
    den += (double)a.d_E[(int64_t)idx * ti + il];
  }
  const float denf = (float)den, coeff = nais_pow((float)(e0 - b0), a.alpha);
  const float pq = denf > 0.f ? (float)num / nais_pow(denf, a.beta) : 0.f;
  out[i] = coeff * pq + bias;
}

template <int DK, int WT>
void launch_pairs(const nrhip_nais_scores_args& a, int i0, int ti, dim3 grid, hipStream_t st) {
  if (a.algorithm == 0) hipLaunchKernelGGL((nais_pairs_kernel<DK, WT, 0>), grid, dim3(256), 0, st, a, i0, ti);
  else hipLaunchKernelGGL((nais_pairs_kernel<DK, WT, 1>), grid, dim3(256), 0, st, a, i0, ti);
}
template <int DK>
void launch_pairs_w(const nrhip_nais_scores_args& a, int i0, int ti, dim3 grid, hipStream_t st) {
  if (a.w <= 16) launch_pairs<DK, 16>(a, i0, ti, grid, st);
  else if (a.w <= 32) launch_pairs<DK, 32>(a, i0, ti, grid, st);
  else launch_pairs<DK, 64>(a, i0, ti, grid, st);
}

}  // namespace

#define NR_NAIS_BY_SHAPE(KERNEL, grid, st, ...)                                                       \
  do {                                                                                                \
    const int wp_ = a.w <= 16 ? 16 : (a.w <= 32 ? 32 : 64), cpl_ = (a.d + wp_ - 1) / wp_;             \
    if (wp_ == 16) {                                                                                  \
      if (cpl_ <= 1) hipLaunchKernelGGL((KERNEL<16, 1>), grid, dim3(256), 0, st, __VA_ARGS__);        \
      else if (cpl_ <= 2) hipLaunchKernelGGL((KERNEL<16, 2>), grid, dim3(256), 0, st, __VA_ARGS__);   \
      else if (cpl_ <= 4) hipLaunchKernelGGL((KERNEL<16, 4>), grid, dim3(256), 0, st, __VA_ARGS__);   \
      else hipLaunchKernelGGL((KERNEL<16, 8>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
    } else if (wp_ == 32) {                                                                           \
      if (cpl_ <= 1) hipLaunchKernelGGL((KERNEL<32, 1>), grid, dim3(256), 0, st, __VA_ARGS__);        \
      else if (cpl_ <= 2) hipLaunchKernelGGL((KERNEL<32, 2>), grid, dim3(256), 0, st, __VA_ARGS__);   \
      else hipLaunchKernelGGL((KERNEL<32, 4>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
    } else {                                                                                          \
      if (cpl_ <= 1) hipLaunchKernelGGL((KERNEL<64, 1>), grid, dim3(256), 0, st, __VA_ARGS__);        \
      else hipLaunchKernelGGL((KERNEL<64, 2>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
    }                                                                                                 \
  } while (0)
