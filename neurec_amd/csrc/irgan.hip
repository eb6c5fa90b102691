// irgan.hip — IRGAN (model/general_recommender/IRGAN.py): the discriminator's training data drawn from the generator's
// softmax (IRGAN.py:175-193), one sess.run(d_updates) (IRGAN.py:102-107, 211) and one generator user step — logits,
// draws, rewards and sess.run(gan_updates) (IRGAN.py:213-235).
//
// Two triples (P [U][d], Q [I][d], b [I]), G and D, plain gradient descent.  Plain launches in stream order; no
// cooperative launch, no float atomics, every float sum in a fixed order: two runs are bit-identical.
//   weights        w_i = floor(exp((z_i - max z) / tau) 2^31) as uint32, W = sum w_i in 64 bits (integer sums are
//                  order-free).  A draw with hash word h is the smallest i whose inclusive prefix sum exceeds
//                  mulhi64(h, W): the 1,024 threads of a workgroup each sum a contiguous range of items, the range sums
//                  are scanned in LDS, a draw bisects the ranges and walks one.
//   irgan_weights_kernel   a workgroup per row of a score slab: the row's maximum, then w over the row IN PLACE
//   irgan_draw_kernel      a workgroup per row: the range scan of w, then the row's draws.  Phase 0: deg(u) draws, the
//                  interleaved (u, pos_k, 1), (u, neg_k, 0) written at the user's offset.  Phase 1: the generator's
//                  mixture, 2 deg(u) draws (what irgan_sample_kernel does inside a G step; tests reach it here)
//   irgan_dstep_kernel     one workgroup, B <= 1,024 pairs: logits and e_b; the occurrences of a user row / an item row
//                  are linked in ascending batch position; the head of each chain sums its occurrences (regulariser per
//                  occurrence) from the values before the step into a scratch row; rows written after a barrier
//   irgan_logits_kernel    z = Q_g P_g[u] + b_g over chunks of 256 items, chunk maxima
//   irgan_sample_kernel    one workgroup: max, w, the float softmax sum E, the scan, the S draws (or the given ones),
//                  rewards from D's rows times p / pn, R, and the draws sorted by (item, draw index)
//   irgan_sweep_kernel     a workgroup per chunk of items: dz_i = (R p_i - sum of the item's r_s) / S, the chunk's part
//                  of Q^T dz from the rows before the step, then Q_i and b_i moved
//   irgan_tail_kernel      the parts added in chunk order, P_u moved
#include "nr_common.h"
#include "neurec_hip.h"

namespace {

constexpr int kScan = 1024;                                // threads of the scanning workgroups
constexpr int kLogitChunk = 256;                           // items of one workgroup of irgan_logits_kernel
constexpr int kSweepFloats = 8192;                         // floats of Q staged by one workgroup of irgan_sweep_kernel
constexpr float kSampleLambda = 0.2f;                      // IRGAN.py:215
constexpr int kRankLds = 2048;                             // draws whose rank sort compares out of LDS
constexpr int kTailTile = 4096;                            // floats of the parts one round of irgan_tail_kernel stages

__host__ __device__ inline int sweep_chunk(int d) {
  int c = kSweepFloats / d;
  return c > 1024 ? 1024 : c;                              // d <= 128: at least 64 items
}

__device__ __forceinline__ uint32_t weight_of(float z, float m, float tau) {
  return (uint32_t)floorf(expf((z - m) / tau) * 2147483648.0f);
}

// the three hash words of draw s of (seed, pass, phase, user)
__device__ __forceinline__ void draw_words(uint64_t seed, uint64_t pass, int phase, int user, int s, uint64_t (&h)[3]) {
  nr::XorShift64s g;
  g.seed(seed, (((pass << 2) | (uint64_t)(phase & 3)) << 32) | (uint64_t)(uint32_t)user, (uint64_t)(uint32_t)s);
  h[0] = g.next();
  h[1] = g.next();
  h[2] = g.next();
}

__device__ __forceinline__ float block_max(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (t < off) red[t] = fmaxf(red[t], red[t + off]);
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}
// a fixed tree: the same sum on every run
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (t < off) red[t] = red[t] + red[t + off];
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}

// incl[t] = the sum of w over the ranges of threads 0..t (range t = items [t per, t per + per)); returns W
__device__ __forceinline__ uint64_t scan_ranges(uint64_t own, uint64_t* incl) {
  const int t = threadIdx.x;
  incl[t] = own;
  __syncthreads();
  for (int off = 1; off < kScan; off <<= 1) {
    const uint64_t v = t >= off ? incl[t - off] : 0;
    __syncthreads();
    incl[t] += v;
    __syncthreads();
  }
  return incl[kScan - 1];
}
__device__ __forceinline__ uint64_t range_sum(const uint32_t* w, int n, int per) {
  const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
  uint64_t s = 0;
#pragma unroll 8
  for (int i = lo; i < hi; ++i) s += w[i];
  return s;
}
// the smallest i whose inclusive prefix sum exceeds x (x < W)
__device__ __forceinline__ int find_draw(uint64_t x, const uint32_t* w, int n, int per, const uint64_t* incl) {
  int lo = 0, hi = kScan - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (incl[mid] > x) hi = mid; else lo = mid + 1;
  }
  uint64_t acc = lo ? incl[lo - 1] : 0;
  const int start = min(lo * per, n), end = min(start + per, n);
  // eight loads in flight at a time: a walk is up to `per` reads of the last-level cache, one latency each otherwise
  for (int i = start; i < end; i += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = i + j < end ? w[i + j] : 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc += v[j];
      if (acc > x) return i + j;                           // a zero past the end cannot be the first to exceed x
    }
  }
  return max(min(end, n) - 1, 0);                          // only reached when W == 0
}
__device__ __forceinline__ int plain_draw(uint64_t h, uint64_t W, const uint32_t* w, int n, int per,
                                          const uint64_t* incl) {
  return find_draw(__umul64hi(h, W), w, n, per, incl);
}
// pn = 0.8 p + 0.2 / deg on the positives: one word in five picks a positive, else a weight draw
__device__ __forceinline__ int mixture_draw(const uint64_t (&h)[3], uint64_t W, const uint32_t* w, int n, int per,
                                            const uint64_t* incl, const int32_t* pos, int deg) {
  if (deg > 0 && __umul64hi(h[0], 5ull) == 0) return pos[(int)__umul64hi(h[1], (uint64_t)deg)];
  return find_draw(__umul64hi(h[2], W), w, n, per, incl);
}

// ---------------------------------------------------------------------------------------------------- D data
// the temperature division and the exponential in double: the weight is the floor of the exact value wherever a float
// exponential's last bits would decide it
__global__ __launch_bounds__(kScan) void irgan_weights_kernel(float* z, int64_t ld, int n, double tau) {
  __shared__ float red[kScan];
  float* zr = z + (int64_t)blockIdx.x * ld;
  const int t = threadIdx.x;
  float m = -__builtin_huge_valf();
  for (int i = t; i < n; i += kScan) m = fmaxf(m, zr[i]);
  m = block_max(m, red);
  for (int i = t; i < n; i += kScan) {
    const double e = exp(((double)zr[i] - (double)m) / tau);
    zr[i] = __uint_as_float((uint32_t)floor(e * 2147483648.0));
  }
}

__global__ __launch_bounds__(kScan) void irgan_draw_kernel(const uint32_t* __restrict__ w, int64_t ld, int n,
                                                           const int32_t* __restrict__ users,
                                                           const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const int64_t* __restrict__ out_off, int phase, uint64_t seed,
                                                           uint64_t pass, int32_t* out_users, int32_t* out_items,
                                                           float* out_labels) {
  __shared__ uint64_t incl[kScan];
  const int row = blockIdx.x, t = threadIdx.x, u = users[row];
  const uint32_t* wr = w + (int64_t)row * ld;
  const int per = (n + kScan - 1) / kScan;
  const uint64_t W = scan_ranges(range_sum(wr, n, per), incl);
  const int64_t p0 = indptr[u];
  const int deg = (int)(indptr[u + 1] - p0);
  const int32_t* pos = indices + p0;
  const int64_t o = out_off[row];
  uint64_t h[3];
  if (phase == 0) {
    for (int s = t; s < deg; s += kScan) {
      draw_words(seed, pass, 0, u, s, h);
      const int64_t at = o + 2 * (int64_t)s;
      out_users[at] = u;
      out_items[at] = pos[s];
      out_labels[at] = 1.0f;
      out_users[at + 1] = u;
      out_items[at + 1] = plain_draw(h[0], W, wr, n, per, incl);
      out_labels[at + 1] = 0.0f;
    }
  } else {
    for (int s = t; s < 2 * deg; s += kScan) {
      draw_words(seed, pass, 1, u, s, h);
      out_items[o + s] = mixture_draw(h, W, wr, n, per, incl, pos, deg);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- D step
struct DStep {
  float* P; float* Q; float* b;
  const int32_t* users; const int32_t* items; const float* labels; const int32_t* order;
  int64_t off;
  int B, d;
  float lr, breg;                                          // breg = B d_reg: the regulariser counts B times
  float* ws;                                               // [2 B d + B]
  float* loss3;                                            // or NULL
};

__global__ __launch_bounds__(kScan) void irgan_dstep_kernel(DStep a) {
  __shared__ int su[kScan], si[kScan], nxu[kScan], nxi[kScan];
  __shared__ float se[kScan], red[kScan];
  const int t = threadIdx.x, B = a.B, d = a.d;
  float ce = 0.f, sq_pq = 0.f, sq_b = 0.f;
  if (t < B) {
    const int64_t idx = a.order ? (int64_t)a.order[a.off + t] : a.off + t;
    const int u = a.users[idx], i = a.items[idx];
    const float y = a.labels[idx];
    const float* p = a.P + (int64_t)u * d;
    const float* q = a.Q + (int64_t)i * d;
    float dot = 0.f, np = 0.f, nq = 0.f;
    for (int k = 0; k < d; ++k) {
      dot += p[k] * q[k];
      np += p[k] * p[k];
      nq += q[k] * q[k];
    }
    const float bi = a.b[i], x = dot + bi;
    su[t] = u;
    si[t] = i;
    se[t] = 1.0f / (1.0f + expf(-x)) - y;
    ce = fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    sq_pq = np + nq;
    sq_b = bi * bi;
  }
  __syncthreads();
  // links to the next occurrence of the same row (-1: none); a head is a row's first occurrence
  bool head_u = false, head_i = false;
  if (t < B) {
    int nu = -1, ni = -1;
    for (int c = t + 1; c < B && (nu < 0 || ni < 0); ++c) {
      if (nu < 0 && su[c] == su[t]) nu = c;
      if (ni < 0 && si[c] == si[t]) ni = c;
    }
    nxu[t] = nu;
    nxi[t] = ni;
    head_u = head_i = true;
    for (int c = 0; c < t && (head_u || head_i); ++c) {
      if (su[c] == su[t]) head_u = false;
      if (si[c] == si[t]) head_i = false;
    }
  }
  if (a.loss3) {
    const float l0 = block_sum(ce, red), l1 = block_sum(sq_pq, red), l2 = block_sum(sq_b, red);
    if (t == 0) {
      a.loss3[0] = l0;
      a.loss3[1] = 0.5f * a.breg * l1;
      a.loss3[2] = 0.5f * a.breg * l2;
    }
  }
  __syncthreads();
  float* wsP = a.ws;
  float* wsQ = a.ws + (int64_t)B * d;
  float* wsB = a.ws + 2 * (int64_t)B * d;
  // which pairs head a user chain (bit 0) and an item chain (bit 1), for the (pair, column) loops below
  red[t] = (float)((head_u ? 1 : 0) | (head_i ? 2 : 0));
  __syncthreads();
  const int total = B * d;
  for (int e = t; e < total; e += kScan) {
    const int bb = e / d, k = e - bb * d;
    const int flags = (int)red[bb];
    if (flags & 1) {
      const float old = a.P[(int64_t)su[bb] * d + k];
      float acc = 0.f;
      for (int c = bb; c >= 0; c = nxu[c]) acc += se[c] * a.Q[(int64_t)si[c] * d + k] + a.breg * old;
      wsP[e] = old - a.lr * acc;
    }
    if (flags & 2) {
      const float old = a.Q[(int64_t)si[bb] * d + k];
      float acc = 0.f;
      for (int c = bb; c >= 0; c = nxi[c]) acc += se[c] * a.P[(int64_t)su[c] * d + k] + a.breg * old;
      wsQ[e] = old - a.lr * acc;
    }
  }
  if (t < B && head_i) {
    const float old = a.b[si[t]];
    float acc = 0.f;
    for (int c = t; c >= 0; c = nxi[c]) acc += se[c] + a.breg * old;
    wsB[t] = old - a.lr * acc;
  }
  __syncthreads();                                         // every read above saw the values from before the step
  for (int e = t; e < total; e += kScan) {
    const int bb = e / d, k = e - bb * d;
    const int flags = (int)red[bb];
    if (flags & 1) a.P[(int64_t)su[bb] * d + k] = wsP[e];
    if (flags & 2) a.Q[(int64_t)si[bb] * d + k] = wsQ[e];
  }
  if (t < B && head_i) a.b[si[t]] = wsB[t];
}

// ---------------------------------------------------------------------------------------------------- G step
__global__ __launch_bounds__(kLogitChunk) void irgan_logits_kernel(const float* __restrict__ P,
                                                                   const float* __restrict__ Q,
                                                                   const float* __restrict__ b, int user, int n, int d,
                                                                   float* __restrict__ z, float* __restrict__ zmax) {
  __shared__ float pu[128];
  __shared__ float red[kLogitChunk];
  const int t = threadIdx.x, i = blockIdx.x * kLogitChunk + t;
  if (t < d) pu[t] = P[(int64_t)user * d + t];
  __syncthreads();
  float v = -__builtin_huge_valf();
  if (i < n) {
    const float* q = Q + (int64_t)i * d;
    float acc = 0.f;
    for (int k = 0; k < d; ++k) acc += q[k] * pu[k];
    v = acc + b[i];
    z[i] = v;
  }
  v = block_max(v, red);
  if (t == 0) zmax[blockIdx.x] = v;
}

struct GStep {
  float* Pg; float* Qg; float* bg;
  const float* Pd; const float* Qd; const float* bd;
  const int64_t* indptr; const int32_t* indices;
  float* z; uint32_t* w; float* zmax;
  int32_t* draw_items; float* draw_r;                      // [2][cap]: as drawn, then sorted by (item, draw index)
  const int32_t* given;                                    // recorded draws or NULL
  float* hdr;                                              // max z, E, R, S (as int)
  float* part;                                             // [sweep chunks][d]
  int user, n, d, cap, n_chunks, sweep_c;
  float lr, reg;
  uint64_t seed, pass;
};

__global__ __launch_bounds__(kScan) void irgan_sample_kernel(GStep a) {
  __shared__ uint64_t incl[kScan];
  __shared__ float red[kScan];
  __shared__ int lds_items[kRankLds];
  const int t = threadIdx.x, n = a.n, d = a.d, u = a.user;
  float m = -__builtin_huge_valf();
  for (int c = t; c < a.n_chunks; c += kScan) m = fmaxf(m, a.zmax[c]);
  m = block_max(m, red);
  const int per = (n + kScan - 1) / kScan;
  float esum = 0.f;                                        // items t, t + 1,024, ...: coalesced, and a fixed order
  {
    const float* __restrict__ zs = a.z;
    uint32_t* __restrict__ ws = a.w;
#pragma unroll 4
    for (int i = t; i < n; i += kScan) {
      const float zi = zs[i];
      esum += expf(zi - m);
      ws[i] = weight_of(zi, m, 1.0f);
    }
  }
  const float E = block_sum(esum, red);                    // its barriers also publish w to the workgroup
  const uint64_t W = scan_ranges(range_sum(a.w, n, per), incl);
  const int64_t p0 = a.indptr[u];
  const int deg = (int)(a.indptr[u + 1] - p0);
  const int32_t* pos = a.indices + p0;
  const int S = min(2 * deg, a.cap);
  const float* pd = a.Pd + (int64_t)u * d;
  float rsum = 0.f;
  for (int s = t; s < S; s += kScan) {
    int item;
    if (a.given) {
      item = a.given[s];
    } else {
      uint64_t h[3];
      draw_words(a.seed, a.pass, 1, u, s, h);
      item = mixture_draw(h, W, a.w, n, per, incl, pos, deg);
    }
    const float p = expf(a.z[item] - m) / E;
    const float pn = (1.0f - kSampleLambda) * p + (nr::sorted_contains(pos, deg, item) ? kSampleLambda / (float)deg : 0.f);
    const float* qd = a.Qd + (int64_t)item * d;
    float x = 0.f;
    for (int k = 0; k < d; ++k) x += pd[k] * qd[k];
    x += a.bd[item];
    const float reward = 2.0f * (1.0f / (1.0f + expf(-x)) - 0.5f);
    const float r = pn > 0.f ? reward * p / pn : 0.f;
    a.draw_items[s] = item;
    a.draw_r[s] = r;
    rsum += r;
  }
  const float R = block_sum(rsum, red);                    // its barriers publish the draws
  // rank sort by (item, draw index); the items of up to kRankLds draws are compared out of LDS
  const bool staged = S <= kRankLds;
  if (staged) {
    for (int s = t; s < S; s += kScan) lds_items[s] = a.draw_items[s];
    __syncthreads();
  }
  for (int s = t; s < S; s += kScan) {
    const int item = a.draw_items[s];
    int rank = 0;
    for (int c = 0; c < S; ++c) {
      const int other = staged ? lds_items[c] : a.draw_items[c];
      rank += (other < item || (other == item && c < s)) ? 1 : 0;
    }
    a.draw_items[a.cap + rank] = item;
    a.draw_r[a.cap + rank] = a.draw_r[s];
  }
  if (t == 0) {
    a.hdr[0] = m;
    a.hdr[1] = E;
    a.hdr[2] = R;
    a.hdr[3] = __int_as_float(S);
  }
}

__global__ __launch_bounds__(256) void irgan_sweep_kernel(GStep a) {
  __shared__ float qs[kSweepFloats];
  __shared__ float dz[1024], cf[1024];
  __shared__ float sub[256], pu[128];
  const int t = threadIdx.x, n = a.n, d = a.d, C = a.sweep_c;
  const int i0 = blockIdx.x * C, cn = min(C, n - i0);
  const float m = a.hdr[0], E = a.hdr[1], R = a.hdr[2];
  const int S = __float_as_int(a.hdr[3]);
  const int32_t* s_items = a.draw_items + a.cap;
  const float* s_r = a.draw_r + a.cap;
  if (t < d) pu[t] = a.Pg[(int64_t)a.user * d + t];
  float* Qc = a.Qg + (int64_t)i0 * d;
  for (int e = t; e < cn * d; e += 256) qs[e] = Qc[e];
  for (int j = t; j < cn; j += 256) {
    const int i = i0 + j;
    const float p = expf(a.z[i] - m) / E;
    int lo = 0, hi = S;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_items[mid] < i) lo = mid + 1; else hi = mid;
    }
    float sum = 0.f;
    int c = 0;
    for (int q = lo; q < S && s_items[q] == i; ++q, ++c) sum += s_r[q];
    const float g = S > 0 ? (R * p - sum) / (float)S : 0.f;
    dz[j] = g;
    cf[j] = (float)c;
    const float bi = a.bg[i];
    a.bg[i] = bi - a.lr * (g + a.reg * (float)c * bi);
  }
  __syncthreads();
  const int G = 256 / d;                                   // d <= 128: at least two groups
  const int grp = t / d, k = t - grp * d;
  if (grp < G) {
    float acc = 0.f;
    for (int j = grp; j < cn; j += G) acc += dz[j] * qs[j * d + k];
    sub[grp * d + k] = acc;
  }
  __syncthreads();
  if (t < d) {
    float acc = 0.f;
    for (int g = 0; g < G; ++g) acc += sub[g * d + t];
    a.part[(int64_t)blockIdx.x * d + t] = acc;
  }
  for (int e = t; e < cn * d; e += 256) {
    const int j = e / d, kk = e - j * d;
    const float q = qs[e];
    Qc[e] = q - a.lr * (dz[j] * pu[kk] + a.reg * cf[j] * q);
  }
}

// the parts come through LDS in rounds, loaded by the whole workgroup: column k is then a chain of LDS reads in chunk
// order, not one cache latency per chunk
__global__ __launch_bounds__(256) void irgan_tail_kernel(GStep a, int sweep_chunks) {
  __shared__ float tile[kTailTile];
  const int k = threadIdx.x, d = a.d;
  const int per = kTailTile / d;                           // chunks of one round
  float acc = 0.f;
  for (int c0 = 0; c0 < sweep_chunks; c0 += per) {
    const int cn = min(per, sweep_chunks - c0);
    for (int e = k; e < cn * d; e += 256) tile[e] = a.part[(int64_t)c0 * d + e];
    __syncthreads();
    if (k < d)
      for (int c = 0; c < cn; ++c) acc += tile[c * d + k];
    __syncthreads();
  }
  if (k >= d) return;
  float* p = a.Pg + (int64_t)a.user * d + k;
  const float old = *p;
  *p = old - a.lr * (acc + a.reg * old);
}

int check_args(const char* who, const nrhip_irgan_args& a) {
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_IRGAN_MAX_D, NR_ERR_UNSUPPORTED, "%s: d=%d is not supported (1 to %d)", who, a.d,
             NRHIP_IRGAN_MAX_D);
  NR_REQUIRE(a.n_items >= 1 && a.n_items < (1 << 30) && a.n_users >= 0, NR_ERR_UNSUPPORTED,
             "%s: n_items=%d is not supported (1 to 2^30 - 1)", who, a.n_items);
  NR_REQUIRE(a.max_batch >= 0 && a.max_batch <= NRHIP_IRGAN_MAX_BATCH, NR_ERR_UNSUPPORTED,
             "%s: a batch of %d pairs is not supported (up to %d)", who, a.max_batch, NRHIP_IRGAN_MAX_BATCH);
  return NR_OK;
}

size_t g_floats(int n_items, int d) {
  const size_t lc = ((size_t)n_items + kLogitChunk - 1) / kLogitChunk;
  const int C = sweep_chunk(d);
  const size_t sc = ((size_t)n_items + C - 1) / C;
  return lc + sc * (size_t)d;
}
size_t d_floats(int max_batch, int d) { return 2 * (size_t)max_batch * d + (size_t)max_batch; }

}  // namespace

extern "C" {

int nrhip_irgan_workspace(int n_items, int d, int max_batch, size_t* floats) {
  NR_REQUIRE(floats, NR_ERR_ARG, "irgan_workspace: null argument");
  nrhip_irgan_args a = {};
  a.n_items = n_items;
  a.d = d;
  a.max_batch = max_batch;
  NR_TRY(check_args("irgan_workspace", a));
  *floats = g_floats(n_items, d) + d_floats(max_batch, d);
  return NR_OK;
}

int nrhip_irgan_weights(float* d_z, int64_t ld, int rows, int n, double tau, void* stream) {
  NR_REQUIRE(rows >= 0 && n >= 1 && ld >= n && tau > 0.0, NR_ERR_ARG,
             "irgan_weights: bad arguments (rows=%d, n=%d, tau=%g)", rows, n, tau);
  if (rows == 0) return NR_OK;
  NR_REQUIRE(d_z, NR_ERR_ARG, "irgan_weights: null argument");
  hipLaunchKernelGGL(irgan_weights_kernel, dim3((unsigned)rows), dim3(kScan), 0, (hipStream_t)stream, d_z, ld, n, tau);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_irgan_draws(const uint32_t* d_w, int64_t ld, int rows, int n, const int32_t* d_users, const int64_t* d_indptr,
                      const int32_t* d_indices, const int64_t* d_out_off, int phase, uint64_t seed, uint64_t pass,
                      int32_t* d_out_users, int32_t* d_out_items, float* d_out_labels, void* stream) {
  NR_REQUIRE(rows >= 0 && n >= 1 && ld >= n && (phase == 0 || phase == 1), NR_ERR_ARG,
             "irgan_draws: bad arguments (rows=%d, n=%d, phase=%d)", rows, n, phase);
  if (rows == 0) return NR_OK;
  NR_REQUIRE(d_w && d_users && d_indptr && d_indices && d_out_off && d_out_items &&
                 (phase == 1 || (d_out_users && d_out_labels)), NR_ERR_ARG, "irgan_draws: null argument");
  hipLaunchKernelGGL(irgan_draw_kernel, dim3((unsigned)rows), dim3(kScan), 0, (hipStream_t)stream, d_w, ld, n, d_users,
                     d_indptr, d_indices, d_out_off, phase, seed, pass, d_out_users, d_out_items, d_out_labels);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_irgan_d_pass(const nrhip_irgan_args* args, const int32_t* d_users, const int32_t* d_items,
                       const float* d_labels, const int32_t* d_order, int64_t n, int batch, float* d_loss, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "irgan_d_pass: null argument block");
  const nrhip_irgan_args& a = *args;
  NR_TRY(check_args("irgan_d_pass", a));
  NR_REQUIRE(n >= 0 && batch >= 1 && batch <= a.max_batch, NR_ERR_ARG,
             "irgan_d_pass: batch=%d, the workspace was made for %d", batch, a.max_batch);
  if (n == 0) return NR_OK;
  NR_REQUIRE(a.d_Pd && a.d_Qd && a.d_bd && a.d_ws && d_users && d_items && d_labels, NR_ERR_ARG,
             "irgan_d_pass: null argument");
  NR_REQUIRE(a.ws_floats >= g_floats(a.n_items, a.d) + d_floats(a.max_batch, a.d), NR_ERR_WORKSPACE,
             "irgan_d_pass: workspace too small");
  DStep s;
  s.P = a.d_Pd; s.Q = a.d_Qd; s.b = a.d_bd;
  s.users = d_users; s.items = d_items; s.labels = d_labels; s.order = d_order;
  s.d = a.d;
  s.lr = a.lr;
  s.ws = a.d_ws + g_floats(a.n_items, a.d);
  int64_t step = 0;
  for (int64_t off = 0; off < n; off += batch, ++step) {
    s.off = off;
    s.B = (int)(n - off < batch ? n - off : batch);
    s.breg = (float)s.B * a.d_reg;
    s.loss3 = d_loss ? d_loss + 3 * step : nullptr;
    hipLaunchKernelGGL(irgan_dstep_kernel, dim3(1), dim3(kScan), 0, (hipStream_t)stream, s);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_irgan_g_pass(const nrhip_irgan_args* args, const int32_t* h_users, int n_users, const int32_t* d_given,
                       uint64_t pass, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "irgan_g_pass: null argument block");
  const nrhip_irgan_args& a = *args;
  NR_TRY(check_args("irgan_g_pass", a));
  NR_REQUIRE(n_users >= 0 && (!d_given || n_users == 1), NR_ERR_ARG,
             "irgan_g_pass: recorded draws are fed to one user at a time");
  if (n_users == 0) return NR_OK;
  NR_REQUIRE(h_users && a.d_Pg && a.d_Qg && a.d_bg && a.d_Pd && a.d_Qd && a.d_bd && a.d_indptr && a.d_indices && a.d_z &&
                 a.d_w && a.d_draw_items && a.d_draw_r && a.d_hdr && a.d_ws && a.max_deg >= 1, NR_ERR_ARG,
             "irgan_g_pass: null argument");
  NR_REQUIRE(a.ws_floats >= g_floats(a.n_items, a.d) + d_floats(a.max_batch, a.d), NR_ERR_WORKSPACE,
             "irgan_g_pass: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  GStep g;
  g.Pg = a.d_Pg; g.Qg = a.d_Qg; g.bg = a.d_bg;
  g.Pd = a.d_Pd; g.Qd = a.d_Qd; g.bd = a.d_bd;
  g.indptr = a.d_indptr; g.indices = a.d_indices;
  g.z = a.d_z; g.w = a.d_w;
  g.n = a.n_items; g.d = a.d;
  g.n_chunks = (a.n_items + kLogitChunk - 1) / kLogitChunk;
  g.sweep_c = sweep_chunk(a.d);
  const int sweep_chunks = (a.n_items + g.sweep_c - 1) / g.sweep_c;
  g.zmax = a.d_ws;
  g.part = a.d_ws + g.n_chunks;
  g.draw_items = a.d_draw_items; g.draw_r = a.d_draw_r;
  g.cap = 2 * a.max_deg;
  g.given = d_given;
  g.hdr = a.d_hdr;
  g.lr = a.lr; g.reg = a.g_reg;
  g.seed = a.seed; g.pass = pass;
  for (int j = 0; j < n_users; ++j) {
    const int u = h_users[j];
    NR_REQUIRE(u >= 0 && u < a.n_users, NR_ERR_ARG, "irgan_g_pass: user %d outside [0, %d)", u, a.n_users);
    g.user = u;
    hipLaunchKernelGGL(irgan_logits_kernel, dim3((unsigned)g.n_chunks), dim3(kLogitChunk), 0, st, (const float*)g.Pg,
                       (const float*)g.Qg, (const float*)g.bg, u, g.n, g.d, g.z, g.zmax);
    hipLaunchKernelGGL(irgan_sample_kernel, dim3(1), dim3(kScan), 0, st, g);
    hipLaunchKernelGGL(irgan_sweep_kernel, dim3((unsigned)sweep_chunks), dim3(256), 0, st, g);
    hipLaunchKernelGGL(irgan_tail_kernel, dim3(1), dim3(256), 0, st, g, sweep_chunks);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

}  // extern "C"
