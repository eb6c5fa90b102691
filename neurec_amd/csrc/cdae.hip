// cdae.hip — CDAE (Wu et al., WSDM 2016): the batch loops, the step and the encoder of
// model/general_recommender/CDAE.py on gfx950.  include/neurec_hip.h has the graph and the layouts.
//
// nrhip_cdae_batch
//   cdae_draw_kernel      one thread per draw: key (slot << 32 | item) of draw q of the slot's user, the sampler's
//                         counter-based stream keyed (seed, user, q); membership by binary search in the CSR row
//   nrhip_sort_u64_segments / nrhip_sort_u64   every slot's draws ascending: in LDS, a workgroup per slot, while the
//                         largest slot has at most NRHIP_CDAE_SEGMENT_DRAWS draws; one sort of all keys beyond (the slot
//                         is the upper word, so the segments keep their places)
//   cdae_count_kernel     one workgroup: the distinct draws per slot (a wavefront per slot, ballots), then the scan
//                         of |R_u| + |N_s| over the slots: d_entry_ptr
//   cdae_fill_kernel      a wavefront per slot: N_s compacted behind R_u, labels, slots, and the merge of the two
//                         ascending lists by rank (own index + the lower bound in the other list): the input list
//                         and every decoder entry's place in it
// nrhip_cdae_step
//   cdae_keys_kernel      the sort keys: (item << 32 | entry) per decoder entry, (n_items + user << 32 | slot) per
//                         slot, the sentinel beyond d_entry_ptr[batch]
//   cdae_forward_kernel   one workgroup per slot, its 4 to 16 lane groups on contiguous shares of the slot's entries,
//                         partial sums added in group order: pools the kept en rows in entry order, adds the user row and the
//                         offset, activates; hidden stays in registers for the slot's decoder dots, the per-entry
//                         g_e, the slot's loss and d hidden = sum g_e de[item_e]; stores hidden and dz for the rows.
//                         Entries are taken DP at a time (a lane reads one entry's index, the group shuffles) and their
//                         rows four at a time, so that a slot's walk is not one chain of dependent loads
//   nrhip_sort_u64        the keys, ascending
//   cdae_rows_kernel      one lane group per sorted key: the head of an item's run sums g_e hidden (de), g_e (bias)
//                         and keep_e / k dz (en) in key order and adds reg row ONCE; a user's run sums dz, then reg
//                         row per occurrence; the item heads' l2 terms go to d_l2
//   cdae_loss_kernel      one workgroup: d offset over the slots in slot order, the loss and regulariser sums
// nrhip_cdae_user_factors, nrhip_cdae_pairs   the encoder on train rows alone, and candidate scores from its rows
//
// Every float sum is taken in a fixed order and nothing is accumulated with atomics: two runs are bit-identical.
#include "rowkey_common.h"
#include "neurec_hip.h"

namespace {

using namespace nr::rowkey;

constexpr uint32_t kNoDraw = 0xffffffffu;                 // a draw of a user who holds every item: behind its slot's items
enum { ACT_IDENTITY = 0, ACT_SIGMOID = 1 };
constexpr int kUnroll = 4;                                // entries of a slot whose row loads are in flight together

// the last s < n with ptr[s] <= i (ptr ascending, ptr[0] <= i)
__device__ __forceinline__ int slot_of(const int64_t* __restrict__ ptr, int n, int64_t i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// the number of a[0..n) below x (a ascending)
__device__ __forceinline__ int lower_bound(const int32_t* a, int n, int32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the corruption mask of entry e, as nrhip_edge_dropout draws it
__device__ __forceinline__ uint64_t mask_key(uint64_t seed, uint64_t step) {
  return nr::splitmix64(seed ^ (step * 0x9e3779b97f4a7c15ull + 0x6e6f6465ull));
}
__device__ __forceinline__ bool mask_draw(uint64_t key, int64_t e, float keep) {
  return (float)(nr::splitmix64(key ^ (uint64_t)e) >> 40) * (1.0f / 16777216.0f) < keep;
}

// ------------------------------------------------------------------------------------------------ the batch builder
__global__ __launch_bounds__(256) void cdae_draw_kernel(nrhip_cdae_batch_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_draws) return;
  const int s = slot_of(a.d_seg_off, a.batch, i);
  const int64_t q = i - a.d_seg_off[s];
  const int u = a.d_users[s];
  uint32_t low = kNoDraw;
  if (u >= 0 && u < a.n_users) {
    const int64_t b = a.d_indptr[u];
    nr::XorShift64s g;
    g.seed(a.seed, (uint64_t)u, (uint64_t)q);
    const int32_t x = nr::draw_negative(g, a.n_items, a.d_indices + b, (int)(a.d_indptr[u + 1] - b));
    if (x >= 0) low = (uint32_t)x;
  }
  a.d_keys[i] = row_key(s, low);
}

// lane `lane` of a wavefront: is sorted key q of the segment at kb the first of its item?
__device__ __forceinline__ bool draw_head(const uint64_t* __restrict__ keys, int64_t kb, int n, int q, uint64_t& key) {
  if (q >= n) return false;
  key = keys[kb + q];
  return (uint32_t)key != kNoDraw && (q == 0 || keys[kb + q - 1] != key);
}

__global__ __launch_bounds__(1024) void cdae_count_kernel(nrhip_cdae_batch_args a) {
  __shared__ int64_t cnt[NRHIP_CDAE_MAX_BATCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < NRHIP_CDAE_MAX_BATCH; s += 16) {
    int64_t c = 0;
    if (s < a.batch) {
      const int64_t kb = a.d_seg_off[s];
      const int n = a.d_seg_len[s];
      for (int q0 = 0; q0 < n; q0 += NR_WAVE) {
        uint64_t key;
        c += __popcll(__ballot(draw_head(a.d_keys, kb, n, q0 + lane, key)));
      }
      c += a.d_pos_ptr[s + 1] - a.d_pos_ptr[s];
    }
    if (lane == 0) cnt[s] = c;
  }
  __syncthreads();
  for (int off = 1; off < NRHIP_CDAE_MAX_BATCH; off <<= 1) {
    const int64_t v = (int)threadIdx.x >= off ? cnt[threadIdx.x - off] : 0;
    __syncthreads();
    cnt[threadIdx.x] += v;
    __syncthreads();
  }
  if ((int)threadIdx.x < a.batch) a.d_entry_ptr[threadIdx.x + 1] = cnt[threadIdx.x];
  if (threadIdx.x == 0) a.d_entry_ptr[0] = 0;
}

__global__ __launch_bounds__(64) void cdae_fill_kernel(nrhip_cdae_batch_args a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int u = a.d_users[s];
  if (u < 0 || u >= a.n_users) return;
  const int64_t base = a.d_entry_ptr[s];
  const int deg = (int)(a.d_pos_ptr[s + 1] - a.d_pos_ptr[s]);
  const int n_neg = (int)(a.d_entry_ptr[s + 1] - base) - deg;
  const int32_t* row = a.d_indices + a.d_indptr[u];
  int32_t* negs = a.d_items + base + deg;
  const int64_t kb = a.d_seg_off[s];
  const int n = a.d_seg_len[s];
  int at = 0;
  for (int q0 = 0; q0 < n; q0 += NR_WAVE) {
    uint64_t key = 0;
    const bool head = draw_head(a.d_keys, kb, n, q0 + lane, key);
    const uint64_t heads = __ballot(head);
    if (head) negs[at + nr_mbcnt(heads)] = (int32_t)(uint32_t)key;
    at += __popcll(heads);
  }
  __syncthreads();                                         // the negatives, for every lane of this one wavefront
  for (int k = lane; k < deg; k += NR_WAVE) {
    const int32_t p = row[k];
    const int64_t pos = base + k + lower_bound(negs, n_neg, p);
    a.d_items[base + k] = p;
    a.d_labels[base + k] = 1.0f;
    a.d_slot[base + k] = s;
    a.d_in_items[pos] = p;
    a.d_in_pos[base + k] = (int32_t)pos;
  }
  for (int j = lane; j < n_neg; j += NR_WAVE) {
    const int32_t x = negs[j];
    const int64_t e = base + deg + j, pos = base + j + lower_bound(row, deg, x);
    a.d_labels[e] = 0.0f;
    a.d_slot[e] = s;
    a.d_in_items[pos] = x;
    a.d_in_pos[e] = (int32_t)pos;
  }
}

// ------------------------------------------------------------------------------------------------ the step
__global__ __launch_bounds__(256) void cdae_keys_kernel(nrhip_cdae_step_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.entry_cap + a.batch) return;
  uint64_t key = kSentinel;
  if (i < a.entry_cap) {
    if (i < a.d_entry_ptr[a.batch]) {
      const int item = a.d_items[i];
      if (item >= 0 && item < a.n_items) key = row_key(item, (uint32_t)i);
    }
  } else {
    const int s = (int)(i - a.entry_cap), u = a.d_users[s];
    if (u >= 0 && u < a.n_users) key = row_key(a.n_items + u, (uint32_t)s);
  }
  a.d_keys[i] = key;
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void cdae_forward_kernel(nrhip_cdae_step_args a) {
  // one workgroup per slot: its G lane groups take contiguous shares of the slot's entries and their partial sums are
  // added in group order, so the slot's time is a G-th of the walk and the sums keep a fixed order
  constexpr int G = 256 / DP;
  __shared__ float part[G][NRHIP_CDAE_MAX_D];
  __shared__ float lpart[G];
  const int c = group_lane<DP>(), gi = threadIdx.x / DP, s = blockIdx.x;
  const int d = a.d;
  const int u = a.d_users[s];
  const bool ok = u >= 0 && u < a.n_users;
  const int64_t sb = a.d_entry_ptr[s], se = ok ? a.d_entry_ptr[s + 1] : sb;
  const int64_t share = (se - sb + G - 1) / G;
  const int64_t eb = sb + gi * share < se ? sb + gi * share : se, ee = eb + share < se ? eb + share : se;
  const float inv = __fdiv_rn(1.0f, a.keep_prob);
  const uint64_t mkey = mask_key(a.seed, a.step);
  float h[CPL] = {}, dh[CPL] = {};
  // A chunk of DP entries at a time: lane j of the group reads entry e0 + j's flag and item, the group then takes
  // them by shuffle, so the row loads of a chunk do not wait for one another's index.  A dropped entry loads
  // nothing and adds a selected 0.f in its place: the sum keeps the entry order.
  const int first = (threadIdx.x & 63) - c;                // this group's first lane in the wavefront
  for (int64_t e0 = eb; e0 < ee; e0 += DP) {
    const int64_t mine = e0 + c;
    int it = -1;
    if (mine < ee) {
      bool kp;
      if (a.keep_given) {
        kp = a.d_keep[mine] != 0;
      } else {
        kp = mask_draw(mkey, mine, a.keep_prob);
        a.d_keep[mine] = kp ? 1 : 0;
      }
      const int x = a.d_in_items[mine];
      if (kp && x >= 0 && x < a.n_items) it = x;
    }
    const int n = ee - e0 < DP ? (int)(ee - e0) : DP;
    for (int j0 = 0; j0 < n; j0 += kUnroll) {
      float row[kUnroll][CPL];
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) {
        const int item = __shfl(it, first + min(j0 + q, DP - 1), NR_WAVE);
        const bool on = j0 + q < n && item >= 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int col = c + k * DP;
          row[q][k] = on && col < d ? inv * a.d_en[(int64_t)item * d + col] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) h[k] += row[q][k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) part[gi][col] = h[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    h[k] = 0.f;
    if (col < d)
      for (int g = 0; g < G; ++g) h[k] += part[g][col];
  }
  __syncthreads();                                         // the partials are read: `part` is free for d hidden
  float sq = 0.f;
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        const float ur = a.d_user[(int64_t)u * d + col];
        float z = (h[k] + ur) + a.d_offset[col];
        if (a.act == ACT_SIGMOID) z = 1.0f / (1.0f + expf(-z));
        h[k] = z;
        sq += ur * ur;
      }
    }
  }
  // the decoder, hidden in registers: every entry's rating, g_e, and d hidden
  // in the same chunks: lane j holds entry e0 + j's item, bias and label, computes its g_e once the group's dot
  // products are in, and stores it; the loss and d hidden are summed in entry order
  float loss = 0.f;
  for (int64_t e0 = eb; e0 < ee; e0 += DP) {
    const int64_t mine = e0 + c;
    int it = -1;
    float bias = 0.f, label = 0.f;
    if (mine < ee) {
      const int x = a.d_items[mine];
      if (x >= 0 && x < a.n_items) {
        it = x;
        bias = a.d_bias[x];
        label = a.d_labels[mine];
      }
    }
    const int n = ee - e0 < DP ? (int)(ee - e0) : DP;
    for (int j0 = 0; j0 < n; j0 += kUnroll) {
      float row[kUnroll][CPL], dot[kUnroll];
      bool on[kUnroll];
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) {
        const int item = __shfl(it, first + min(j0 + q, DP - 1), NR_WAVE);
        on[q] = j0 + q < n && item >= 0;
        dot[q] = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int col = c + k * DP;
          row[q][k] = on[q] && col < d ? a.d_de[(int64_t)item * d + col] : 0.f;
          dot[q] += h[k] * row[q][k];
        }
      }
      static_assert(kUnroll == 4, "the xor trees below are written out for four entries");
      group_sum<DP>(dot[0], dot[1], dot[2], dot[3]);
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) {
        const int src = first + min(j0 + q, DP - 1);
        const float b = __shfl(bias, src, NR_WAVE), z = __shfl(label, src, NR_WAVE);
        float g = 0.f;
        if (on[q]) {
          const float x = dot[q] + b;
          g = nr::pointwise_dloss(a.loss_kind, z, x);
          loss += nr::pointwise_loss(a.loss_kind, z, x);
        }
        if (c == 0 && j0 + q < n) a.d_g[e0 + j0 + q] = g;
#pragma unroll
        for (int k = 0; k < CPL; ++k) dh[k] += g * row[q][k];
      }
    }
  }
  group_sum<DP>(sq);
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) part[gi][col] = dh[k];
  }
  if (c == 0) lpart[gi] = loss;
  __syncthreads();
  if (gi != 0) return;
  loss = 0.f;
  for (int g = 0; g < G; ++g) loss += lpart[g];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    dh[k] = 0.f;
    if (col < d) {
      for (int g = 0; g < G; ++g) dh[k] += part[g][col];
      a.d_hidden[(int64_t)s * d + col] = h[k];
      a.d_dz[(int64_t)s * d + col] = a.act == ACT_SIGMOID ? dh[k] * (h[k] * (1.0f - h[k])) : dh[k];
    }
  }
  if (c != 0) return;
  float* sc = a.d_scal + (int64_t)s * kScal;
  sc[S_G] = 0.f;
  sc[S_LOSS] = loss;
  sc[S_L2] = ok ? 0.5f * sq : 0.f;
  sc[S_OK] = ok ? 1.f : 0.f;
  if (ok && a.d_flag_user) a.d_flag_user[u] = 1;
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void cdae_rows_kernel(nrhip_cdae_step_args a) {
  const int c = group_lane<DP>();
  const int64_t w = group_index<DP, int64_t>();
  const int d = a.d, I = a.n_items;
  const int64_t n_keys = (int64_t)a.entry_cap + a.batch;
  if (w >= n_keys) return;
  const int row = head_row(a.d_keys, w);
  if (row < 0) {
    if (c == 0) a.d_l2[w] = 0.f;
    return;
  }
  const float reg = a.reg;
  if (row >= I) {
    // a user: dz of its slots in slot order, then the regulariser's lookup once per occurrence
    const int r = row - I;
    float own[CPL], acc[CPL] = {};
    load_row<DP, CPL>(a.d_user, r, d, c, own);
    int n_occ = 0;
    for_run(a.d_keys, n_keys, w, row, [&](uint32_t s) {
      ++n_occ;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) acc[k] += a.d_dz[(int64_t)s * d + col];
      }
    });
    for (int n = 0; n < n_occ; ++n) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] += reg * own[k];
    }
    store_row<DP, CPL>(a.d_G_user, r, d, c, acc);
    if (c == 0) a.d_l2[w] = 0.f;                            // the user rows' l2 is the slots' (S_L2)
    return;
  }
  const float inv = __fdiv_rn(1.0f, a.keep_prob);
  float own_de[CPL], own_en[CPL], acc_de[CPL] = {}, acc_en[CPL] = {}, acc_b = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    own_de[k] = col < d ? a.d_de[(int64_t)row * d + col] : 0.f;
    own_en[k] = col < d ? a.d_en[(int64_t)row * d + col] : 0.f;
  }
  const float b = a.d_bias[row];
  for_run(a.d_keys, n_keys, w, row, [&](uint32_t e) {
    const int s = a.d_slot[e];
    const float g = a.d_g[e];
    const bool kp = a.d_keep[a.d_in_pos[e]] != 0;
    acc_b += g;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) {
        acc_de[k] += g * a.d_hidden[(int64_t)s * d + col];
        if (kp) acc_en[k] += inv * a.d_dz[(int64_t)s * d + col];
      }
    }
  });
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    acc_de[k] += reg * own_de[k];
    acc_en[k] += reg * own_en[k];
    sq += own_de[k] * own_de[k] + own_en[k] * own_en[k];
  }
  group_sum<DP>(sq);
  store_row<DP, CPL>(a.d_G_de, row, d, c, acc_de);
  store_row<DP, CPL>(a.d_G_en, row, d, c, acc_en);
  if (c != 0) return;
  a.d_G_bias[row] = acc_b + reg * b;
  a.d_l2[w] = 0.5f * (sq + b * b);
  if (a.d_flag_de) a.d_flag_de[row] = 1;
  if (a.d_flag_en) a.d_flag_en[row] = 1;
  if (a.d_flag_bias) a.d_flag_bias[row] = 1;
}

__global__ __launch_bounds__(256) void cdae_loss_kernel(nrhip_cdae_step_args a) {
  const int d = a.d;
  double v[2] = {0.0, 0.0};
  for (int col = threadIdx.x; col < d; col += 256) {
    float acc = 0.f;
    for (int s = 0; s < a.batch; ++s) acc += a.d_dz[(int64_t)s * d + col];
    const float o = a.d_offset[col];
    a.d_G_offset[col] = acc + a.reg * o;
    v[1] += 0.5 * (double)(o * o);
  }
  slot_sums(a.d_scal, a.batch, v[0], v[1]);
  const int64_t n_keys = (int64_t)a.entry_cap + a.batch;
  for (int64_t w = threadIdx.x; w < n_keys; w += 256) v[1] += (double)a.d_l2[w];
  block_sum(v);
  if (threadIdx.x == 0) {
    a.d_loss2[0] = (float)v[0];
    a.d_loss2[1] = (float)((double)a.reg * v[1]);
  }
}

// ------------------------------------------------------------------------------------------------ scoring
struct FactorsArgs {
  const int64_t* indptr; const int32_t* indices;
  const float* user; const float* en; const float* offset;
  const int32_t* users; const int64_t* mask_ptr; uint8_t* keep_io;
  float* out; int64_t ld;
  uint64_t seed, step;
  int n_users, n_items, d, act, batch, keep_given;
  float keep_prob;
};

template <int DP, int CPL>
__global__ __launch_bounds__(256) void cdae_factors_kernel(FactorsArgs a) {
  const int c = group_lane<DP>(), b = group_index<DP>();
  const int d = a.d;
  if (b >= a.batch) return;
  const int u = a.users ? a.users[b] : b;
  const bool ok = u >= 0 && u < a.n_users;
  const bool all = a.keep_prob >= 1.0f;
  const float inv = all ? 1.0f : __fdiv_rn(1.0f, a.keep_prob);
  const uint64_t mkey = mask_key(a.seed, a.step);
  float h[CPL] = {};
  if (ok) {
    const int64_t rb = a.indptr[u], re = a.indptr[u + 1], mb = all ? 0 : a.mask_ptr[b];
    for (int64_t t = rb; t < re; ++t) {
      bool kp = true;
      if (!all) {
        const int64_t e = mb + (t - rb);
        if (a.keep_given) {
          kp = a.keep_io[e] != 0;
        } else {
          kp = mask_draw(mkey, e, a.keep_prob);
          if (c == 0) a.keep_io[e] = kp ? 1 : 0;
        }
      }
      if (!kp) continue;
      const int item = a.indices[t];
      if (item < 0 || item >= a.n_items) continue;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int col = c + k * DP;
        if (col < d) h[k] += inv * a.en[(int64_t)item * d + col];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int col = c + k * DP;
    if (col < d) {
      float z = 0.f;
      if (ok) {
        z = (h[k] + a.user[(int64_t)u * d + col]) + a.offset[col];
        if (a.act == ACT_SIGMOID) z = 1.0f / (1.0f + expf(-z));
      }
      a.out[(int64_t)b * a.ld + col] = z;
    }
  }
  if (c == 0) a.out[(int64_t)b * a.ld + d] = 1.0f;
}

template <int DP, int CPL>
__global__ __launch_bounds__(256) void cdae_pairs_kernel(const float* __restrict__ F, int64_t ld,
                                                         const float* __restrict__ de, const float* __restrict__ bias,
                                                         int n_items, int d, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ items, int64_t n,
                                                         float* __restrict__ out) {
  const int c = group_lane<DP>();
  const int64_t p = group_index<DP, int64_t>();
  const bool in = p < n;
  const int item = in ? items[p] : -1;
  const bool ok = item >= 0 && item < n_items;
  const int64_t r = in ? rows[p] : 0;
  float dot = 0.f;
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int col = c + k * DP;
      if (col < d) dot += F[r * ld + col] * de[(int64_t)item * d + col];
    }
  }
  group_sum<DP>(dot);
  if (in && c == 0) out[p] = ok ? dot + bias[item] : 0.f;
}

}  // namespace

extern "C" {

int nrhip_cdae_batch(const nrhip_cdae_batch_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "cdae_batch: null argument block");
  const nrhip_cdae_batch_args a = *args;
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_CDAE_MAX_BATCH, NR_ERR_UNSUPPORTED, "cdae_batch: batch %d outside 0..%d",
             a.batch, NRHIP_CDAE_MAX_BATCH);
  NR_REQUIRE(a.num_neg >= 1, NR_ERR_ARG, "cdae_batch: num_neg must be at least 1, got %d", a.num_neg);
  NR_REQUIRE(a.n_users >= 0 && a.n_items >= 1 && a.n_draws >= 0 && a.max_draws >= 0 && a.max_draws <= a.n_draws &&
                 a.n_draws / a.num_neg * ((int64_t)a.num_neg + 1) < ((int64_t)1 << 30),
             NR_ERR_ARG, "cdae_batch: bad sizes");
  if (a.batch == 0) return NR_OK;
  NR_REQUIRE(a.d_indptr && a.d_indices && a.d_users && a.d_pos_ptr && a.d_seg_off && a.d_seg_len && a.d_entry_ptr &&
                 (a.n_draws == 0 || (a.d_keys && a.d_items && a.d_labels && a.d_slot && a.d_in_items && a.d_in_pos)),
             NR_ERR_ARG, "cdae_batch: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  if (a.n_draws > 0) {
    hipLaunchKernelGGL(cdae_draw_kernel, dim3((unsigned)((a.n_draws + 255) / 256)), dim3(256), 0, st, a);
    NR_LAUNCH_CHECK();
    if (a.max_draws <= NRHIP_CDAE_SEGMENT_DRAWS)
      NR_TRY(nrhip_sort_u64_segments(a.d_keys, a.d_seg_off, a.d_seg_len, a.batch, a.max_draws, stream));
    else
      NR_TRY(nrhip_sort_u64(a.d_keys, (int)a.n_draws, stream));
  }
  hipLaunchKernelGGL(cdae_count_kernel, dim3(1), dim3(1024), 0, st, a);
  NR_LAUNCH_CHECK();
  if (a.n_draws > 0) {
    hipLaunchKernelGGL(cdae_fill_kernel, dim3((unsigned)a.batch), dim3(64), 0, st, a);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}

int nrhip_cdae_step(const nrhip_cdae_step_args* args, void* stream) {
  NR_REQUIRE(args, NR_ERR_ARG, "cdae_step: null argument block");
  const nrhip_cdae_step_args a = *args;
  NR_REQUIRE(a.d >= 1 && a.d <= NRHIP_CDAE_MAX_D, NR_ERR_UNSUPPORTED, "cdae_step: hidden_dim %d outside 1..%d", a.d,
             NRHIP_CDAE_MAX_D);
  NR_REQUIRE(a.batch >= 0 && a.batch <= NRHIP_CDAE_MAX_BATCH, NR_ERR_UNSUPPORTED, "cdae_step: batch %d outside 0..%d",
             a.batch, NRHIP_CDAE_MAX_BATCH);
  NR_REQUIRE(a.act == ACT_IDENTITY || a.act == ACT_SIGMOID, NR_ERR_ARG, "cdae_step: unknown activation %d", a.act);
  NR_TRY(check_loss_kind("cdae_step", 0, a.loss_kind));
  NR_REQUIRE(a.keep_prob > 0.f && a.keep_prob <= 1.f, NR_ERR_ARG, "cdae_step: keep_prob %g outside (0, 1]",
             (double)a.keep_prob);
  // nrhip_sort_u64 pads its count to a power of two in an int: entry_cap + batch keys stay at 2^30 or below
  NR_REQUIRE(a.entry_cap >= 0 && (int64_t)a.entry_cap + a.batch <= ((int64_t)1 << 30) && a.n_users >= 0 &&
                 a.n_items >= 0 &&
                 (a.batch == 0 || a.n_items >= 1) &&
                 (int64_t)a.n_users + (int64_t)a.n_items < ((int64_t)1 << 31) - 1, NR_ERR_ARG, "cdae_step: bad sizes");
  if (a.batch == 0) return NR_OK;
  NR_REQUIRE(a.d_user && a.d_en && a.d_offset && a.d_de && a.d_bias && a.d_G_user && a.d_G_en && a.d_G_offset &&
                 a.d_G_de && a.d_G_bias && a.d_users && a.d_entry_ptr && a.d_keys && a.d_hidden && a.d_dz &&
                 a.d_scal && a.d_l2 && a.d_loss2 &&
                 (a.entry_cap == 0 || (a.d_items && a.d_labels && a.d_slot && a.d_in_items && a.d_in_pos && a.d_keep &&
                                       a.d_g)),
             NR_ERR_ARG, "cdae_step: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int n_keys = a.entry_cap + a.batch;
  hipLaunchKernelGGL(cdae_keys_kernel, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  NR_BY_WIDTH(cdae_forward_kernel, a.d, dim3((unsigned)a.batch), st, a);
  NR_LAUNCH_CHECK();
  NR_TRY(nrhip_sort_u64(a.d_keys, n_keys, stream));
  NR_BY_WIDTH(cdae_rows_kernel, a.d, n_keys, st, a);
  NR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cdae_loss_kernel, dim3(1), dim3(256), 0, st, a);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_cdae_user_factors(const int64_t* d_indptr, const int32_t* d_indices, int n_users, int n_items,
                            const float* d_user, const float* d_en, const float* d_offset, int d, int act,
                            const int32_t* d_users, const int64_t* d_mask_ptr, int batch, uint8_t* d_keep_io,
                            int keep_given, float keep_prob, uint64_t seed, uint64_t step, float* d_out, int64_t ld,
                            void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_CDAE_MAX_D, NR_ERR_UNSUPPORTED, "cdae_user_factors: hidden_dim %d outside 1..%d", d,
             NRHIP_CDAE_MAX_D);
  NR_REQUIRE(act == ACT_IDENTITY || act == ACT_SIGMOID, NR_ERR_ARG, "cdae_user_factors: unknown activation %d", act);
  NR_REQUIRE(keep_prob > 0.f, NR_ERR_ARG, "cdae_user_factors: keep_prob %g must be positive", (double)keep_prob);
  NR_REQUIRE(n_users >= 0 && n_items >= 0 && batch >= 0 && ld >= d + 1 && (d_users || batch <= n_users), NR_ERR_ARG,
             "cdae_user_factors: bad sizes");
  if (batch == 0) return NR_OK;
  NR_REQUIRE(d_indptr && d_indices && d_user && d_en && d_offset && d_out &&
                 (keep_prob >= 1.f || (d_mask_ptr && d_keep_io)), NR_ERR_ARG,
             "cdae_user_factors: null pointer argument");
  FactorsArgs f{d_indptr, d_indices, d_user, d_en, d_offset, d_users, d_mask_ptr, d_keep_io, d_out, ld, seed, step,
                n_users, n_items, d, act, batch, keep_given ? 1 : 0, keep_prob};
  NR_BY_WIDTH(cdae_factors_kernel, d, batch, (hipStream_t)stream, f);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

int nrhip_cdae_pairs(const float* d_factors, int64_t ld, const float* d_de, const float* d_bias, int n_items, int d,
                     const int32_t* d_rows, const int32_t* d_items, int64_t n, float* d_out, void* stream) {
  NR_REQUIRE(d >= 1 && d <= NRHIP_CDAE_MAX_D, NR_ERR_UNSUPPORTED, "cdae_pairs: hidden_dim %d outside 1..%d", d,
             NRHIP_CDAE_MAX_D);
  NR_REQUIRE(n >= 0 && n_items >= 0 && ld >= d, NR_ERR_ARG, "cdae_pairs: bad sizes");
  if (n == 0) return NR_OK;
  NR_REQUIRE(d_factors && d_de && d_bias && d_rows && d_items && d_out, NR_ERR_ARG, "cdae_pairs: null pointer argument");
  NR_BY_WIDTH(cdae_pairs_kernel, d, n, (hipStream_t)stream, d_factors, ld, d_de, d_bias, n_items, d, d_rows, d_items, n,
              d_out);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // extern "C"
