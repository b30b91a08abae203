// embed_enc.hip — entity and item sets whose discrete columns are embedding lookups (SPEC.md §25;
// include/nmmo_heads.h, nmh_embed_features / nmh_embed_logits / nmh_embed_logits_backward). Part of
// libnmmo_heads.so.
//
// The takeru policy's ReducedPlayerEncoder.agent_fc and ReducedItemEncoder.fc are linear over
// cat(E[idx_0], .., E[idx_{D-1}], x_c / s_c), so with per-row score tables that torch folds,
//   pq[d][i] = (q W)[32 d, 32 d + 32) . E[i],   pq[cont c] = (q W)[32 D + c],   pq[bias] = q . b,
// a pointer logit is D table reads and C multiply-adds on the candidate's own columns, the mean pool
// needs the D x 256 bin counts and C column sums of a set, and no [N, R, H] tensor exists. The kernels
// hold no parameters. A kind (EntityKind, ItemKind) is a compile-time descriptor.
//
// features / counts / sums / own row: one 256-thread workgroup per set, thread t is column t % cols
// of slot t / cols, as in player_enc.hip: consecutive lanes on consecutive elements. The counts are
// LDS integer adds, a column's slot sums are added in ascending order by one thread, and the own row
// is an LDS integer min. With only the own row asked for, only column 0 is read.
//
// logits: one wave per obs row, four rows per workgroup, no workgroup barrier: player_enc.hip's
// list of the candidates that any head allows and its LDS staging of 64 listed candidates' columns
// (row stride cols | 1 words, so a lane per candidate reads without a bank conflict). The C + 1
// continuous weights and the bias of each head are in LDS; the D x 256 score bins stay in global
// memory and a lane reads only the D bins its candidate indexes, through L1 / L2.
//
// logits_backward: same list and staging, plus the listed candidates' indices (packed bytes) and
// g_out in LDS. Lane l owns bins l, l + 64, l + 128, l + 192 of every column in registers and walks
// the list in ascending order; lane c <= C owns continuous slot c (C: the bias). No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "heads_dev.h"   // wave_sync
#include "heads_host.h"  // heads_fail, heads_launched, check_set, check_ids, check_forward, check_backward, HEADS_SET_LAUNCH
#include "set_dev.h"     // legal_list_heads, stage_rows, scan_set, load_id
#include "../../include/nmmo_heads.h"

using namespace nmmo;
using set_dev::kHeadShift;
using set_dev::kJMask;
using set_dev::legal_list_heads;

namespace {

constexpr int kBins = NMH_EMBED_BINS, kMaxHeads = NMH_ITEM_MAX_HEADS;
constexpr int kThreads = set_dev::kScanThreads, kRowsPerBlock = 4, kChunk = 64;

// SPEC §25's two kinds. dslot / cslot: the discrete or continuous slot a column feeds, or -1.
struct EntityKind {
  static constexpr int kCols = 31, kD = 4, kC = 27, kMaxRows = NMH_PLAYER_MAX_ROWS, kQ = NMH_EMBED_ENTITY_QUERY;
  __host__ __device__ static constexpr int dcol(int d) { return d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 8 : 10; }
  __host__ __device__ static constexpr float doff(int d) { return 256.0f * (float)d; }
  __host__ __device__ static constexpr int ccol(int c) { return c < 6 ? c + 2 : c == 6 ? 9 : c + 4; }
  // row, col, damage, time_alive, freeze, item_level, latest_combat_tick, gold, health, food, water;
  // seven skills' (level / 10, exp / 100); alchemy_level / 100, alchemy_exp / 10 as the reference has them
  __host__ __device__ static constexpr float cdiv(int c) {
    return c < 2 ? 256.0f
           : c == 3 || c == 6 ? 1024.0f
           : c == 4 ? 3.0f
           : c == 5 ? 50.0f
           : c < 11 ? 100.0f
           : c < 25 ? ((c & 1) ? 10.0f : 100.0f)
           : c == 25 ? 100.0f : 10.0f;
  }
  __host__ __device__ static constexpr int dslot(int col) {
    return col == 0 ? 0 : col == 1 ? 1 : col == 8 ? 2 : col == 10 ? 3 : -1;
  }
  __host__ __device__ static constexpr int cslot(int col) {
    return col < 2 || col == 8 || col == 10 ? -1 : col < 8 ? col - 2 : col == 9 ? 6 : col - 4;
  }
};
struct ItemKind {
  static constexpr int kCols = 16, kD = 2, kC = 12, kMaxRows = NMH_ITEM_MAX_ROWS, kQ = NMH_EMBED_ITEM_QUERY;
  __host__ __device__ static constexpr int dcol(int d) { return d == 0 ? 1 : 14; }
  __host__ __device__ static constexpr float doff(int d) { return d == 0 ? 2.0f : 0.0f; }
  __host__ __device__ static constexpr int ccol(int c) { return c < 11 ? c + 3 : 15; }
  __host__ __device__ static constexpr float cdiv(int c) { return c < 3 ? 10.0f : c < 6 ? 100.0f : c < 9 ? 40.0f : 100.0f; }
  __host__ __device__ static constexpr int dslot(int col) { return col == 1 ? 0 : col == 14 ? 1 : -1; }
  __host__ __device__ static constexpr int cslot(int col) { return col >= 3 && col <= 13 ? col - 3 : col == 15 ? 11 : -1; }
};

template <typename K>
constexpr bool kind_is_sound() {
  for (int d = 0; d < K::kD; ++d)
    if (K::dslot(K::dcol(d)) != d || K::cslot(K::dcol(d)) != -1) return false;
  for (int c = 0; c < K::kC; ++c)
    if (K::cslot(K::ccol(c)) != c || K::dslot(K::ccol(c)) != -1 || K::ccol(c) >= K::kCols) return false;
  return K::kQ == ((K::kD * kBins + K::kC + 1 + 3) & ~3) && K::kD <= 4 && K::kMaxRows <= (1 << kHeadShift) &&
         K::kC + 1 <= 64 && K::kQ - K::kD * kBins <= 64;
}
static_assert(kind_is_sound<EntityKind>() && kind_is_sound<ItemKind>(), "SPEC §25's descriptors");
static_assert(EntityKind::cdiv(24) == 100.0f && EntityKind::cdiv(25) == 100.0f && EntityKind::cdiv(26) == 10.0f &&
                  EntityKind::cdiv(11) == 10.0f && EntityKind::cdiv(10) == 100.0f && EntityKind::cdiv(2) == 100.0f,
              "the reference's divisors");
static_assert(kBins == 256, "an index is a byte");

// SPEC §25's index rule: clip(trunc(x + off), 0, 255), NaN -> 0
__device__ inline int embed_idx(float x, float off) {
  const float v = x + off;
  return v >= 0.0f ? (v >= (float)(kBins - 1) ? kBins - 1 : (int)v) : 0;
}

// ---------------------------------------------------------------- features, counts, sums, own row
// column c's part of a candidate's idx [D] / cont [C]
template <typename K>
__device__ inline void put_feature(uint8_t* __restrict__ idx, float* __restrict__ cont, int c, float x) {
  const int d = K::dslot(c), cc = K::cslot(c);
  if (d >= 0 && idx) idx[d] = (uint8_t)embed_idx(x, K::doff(d));
  if (cc >= 0 && cont) cont[cc] = __fdiv_rn(x, K::cdiv(cc));
}

template <typename K, typename T>
__global__ __launch_bounds__(kThreads) void nmh_embed_features_kernel(
    const T* __restrict__ sets, int64_t set_stride, int R, const void* __restrict__ ids, int64_t id_stride, int id_kind,
    uint8_t* __restrict__ idx, float* __restrict__ cont, float* __restrict__ counts, float* __restrict__ sums,
    int32_t* __restrict__ mine_idx, uint8_t* __restrict__ mine_i, float* __restrict__ mine_c) {
  constexpr int kCols = K::kCols, kD = K::kD, kC = K::kC, kSlots = kThreads / kCols;
  __shared__ float s_part[kSlots][kCols];
  __shared__ int s_cnt[kD * kBins];
  __shared__ int s_first;
  const int tid = threadIdx.x, slot = tid / kCols, c = tid % kCols;
  const int64_t m = blockIdx.x;
  const bool own = mine_idx || mine_i || mine_c, all = idx || cont || counts || sums;
  for (int i = tid; i < kD * kBins; i += kThreads) s_cnt[i] = 0;
  if (tid == 0) s_first = R;
  __syncthreads();
  const T* __restrict__ set = sets + m * set_stride;
  const float id = own ? set_dev::load_id(ids, m * id_stride, id_kind) : 0.0f;
  const int d = K::dslot(c);
  if (slot < kSlots && (all || c == 0))
    s_part[slot][c] = set_dev::scan_set<kCols>(set, R, slot, c, own, id, &s_first, [&](int j, float x) {
      if (d >= 0 && counts) atomicAdd(&s_cnt[d * kBins + embed_idx(x, K::doff(d))], 1);
      const int64_t e = m * R + j;
      put_feature<K>(idx ? idx + e * kD : nullptr, cont ? cont + e * kC : nullptr, c, x);
    });
  __syncthreads();
  if (sums && tid < kC) {
    const int col = K::ccol(tid);
    float s = 0.0f;
    for (int q = 0; q < kSlots; ++q) s += s_part[q][col];
    sums[m * kC + tid] = s;
  }
  if (counts)
    for (int i = tid; i < kD * kBins; i += kThreads) counts[m * (kD * kBins) + i] = (float)s_cnt[i];
  if (own) {
    const int first = s_first < R ? s_first : 0;
    if (mine_idx && tid == 0) mine_idx[m] = first;
    if (tid < kCols)
      put_feature<K>(mine_i ? mine_i + m * kD : nullptr, mine_c ? mine_c + m * kC : nullptr, tid,
                     (float)set[(int64_t)first * kCols + tid]);
  }
}

// ---------------------------------------------------------------- pointer logits
template <typename K, typename T, int MK>
__device__ __forceinline__ void embed_logits_body(const NmhSetHeads& sh, int n_rows, const T* __restrict__ sets,
                                                  int64_t set_stride, int R, int share, const void* __restrict__ mask,
                                                  int64_t ms, const float* __restrict__ pq, float* __restrict__ out,
                                                  int64_t os) {
  constexpr int kD = K::kD, kC = K::kC, kQ = K::kQ, kS = K::kCols | 1, kW = kC + 1;
  __shared__ float s_w[kRowsPerBlock][kMaxHeads * kW];  // per head: the C continuous weights, the bias
  __shared__ float s_rows[kRowsPerBlock][kChunk * kS];
  __shared__ uint16_t s_list[kRowsPerBlock][K::kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const int H = sh.n_heads;
  float* sw = s_w[w];
  float* rows = s_rows[w];
  uint16_t* list = s_list[w];
  const float* __restrict__ pqr = pq + r * H * kQ;
  for (int i = lane; i < H * kW; i += 64) {
    const int h = i / kW;
    sw[i] = pqr[h * kQ + kD * kBins + (i - h * kW)];
  }
  const T* __restrict__ set = sets + (r / share) * set_stride;
  float* __restrict__ orow = out + r * os;
  const int cnt = legal_list_heads<MK, true>(sh, mask, r * ms, R, list, orow);
#pragma unroll
  for (int h = 0; h < kMaxHeads; ++h)
    if (h < H && lane == h) orow[sh.out_off[h] + R] = 0.0f;  // the no-op entries
  wave_sync();
  for (int i0 = 0; i0 < cnt; i0 += kChunk) {
    const int n = min(kChunk, cnt - i0);
    set_dev::stage_rows<K::kCols, kS>(set, list, i0, n, rows);
    wave_sync();
    if (lane < n) {
      const int entry = list[i0 + lane], j = entry & kJMask, hm = entry >> kHeadShift;
      const float* row = rows + lane * kS;
      int bin[kD];
      float x[kC];
#pragma unroll
      for (int d = 0; d < kD; ++d) bin[d] = d * kBins + embed_idx(row[K::dcol(d)], K::doff(d));
#pragma unroll
      for (int c = 0; c < kC; ++c) x[c] = __fdiv_rn(row[K::ccol(c)], K::cdiv(c));
#pragma unroll
      for (int h = 0; h < kMaxHeads; ++h) {
        if (h < H && (hm >> h & 1)) {
          float acc = sw[h * kW + kC];
#pragma unroll
          for (int d = 0; d < kD; ++d) acc += pqr[h * kQ + bin[d]];
#pragma unroll
          for (int c = 0; c < kC; ++c) acc = fmaf(x[c], sw[h * kW + c], acc);
          orow[sh.out_off[h] + j] = acc;
        }
      }
    }
    wave_sync();  // the next chunk overwrites the rows
  }
}

template <typename K, typename T, int MK>
__device__ __forceinline__ void embed_backward_body(const NmhSetHeads& sh, int n_rows, const T* __restrict__ sets,
                                                    int64_t set_stride, int R, int share,
                                                    const void* __restrict__ mask, int64_t ms,
                                                    const float* __restrict__ g_out, int64_t gs,
                                                    float* __restrict__ g_pq) {
  constexpr int kD = K::kD, kC = K::kC, kQ = K::kQ, kS = K::kCols | 1, kOwn = kBins / 64;
  __shared__ float s_rows[kRowsPerBlock][kChunk * kS];
  __shared__ float s_g[kRowsPerBlock][kMaxHeads][kChunk];
  __shared__ uint32_t s_idx[kRowsPerBlock][kChunk];  // a listed candidate's D indices, a byte each
  __shared__ uint16_t s_list[kRowsPerBlock][K::kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), f = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const int H = sh.n_heads;
  float* rows = s_rows[w];
  uint16_t* list = s_list[w];
  const T* __restrict__ set = sets + (r / share) * set_stride;
  const float* __restrict__ grow = g_out + r * gs;
  const int cnt = legal_list_heads<MK, false>(sh, mask, r * ms, R, list, nullptr);
  // the column continuous slot f reads and its divisor; the bias (f = C) and the lanes beyond read column 0
  const int col = f < kC ? K::ccol(f) : 0;
  const float div = f < kC ? K::cdiv(f) : 1.0f;
  float bins[kMaxHeads][kD][kOwn] = {};  // bin f + 64 q of column d
  float acc[kMaxHeads] = {};
  wave_sync();
  for (int i0 = 0; i0 < cnt; i0 += kChunk) {
    const int n = min(kChunk, cnt - i0);
    set_dev::stage_rows<K::kCols, kS>(set, list, i0, n, rows);
    if (f < n) {  // lane k: listed candidate k's g_out in the heads that allow it, no other entry
      const int entry = list[i0 + f], j = entry & kJMask, hm = entry >> kHeadShift;
#pragma unroll
      for (int h = 0; h < kMaxHeads; ++h)
        if (h < H && (hm >> h & 1)) s_g[w][h][f] = grow[sh.out_off[h] + j];
    }
    wave_sync();
    if (f < n) {
      uint32_t pk = 0;
#pragma unroll
      for (int d = 0; d < kD; ++d) pk |= (uint32_t)embed_idx(rows[f * kS + K::dcol(d)], K::doff(d)) << (8 * d);
      s_idx[w][f] = pk;
    }
    wave_sync();
    for (int k = 0; k < n; ++k) {
      const int hm = list[i0 + k] >> kHeadShift;  // (wave-uniform)
      const uint32_t pk = s_idx[w][k];            // (wave-uniform)
      const float x = f < kC ? __fdiv_rn(rows[k * kS + col], div) : 1.0f;
#pragma unroll
      for (int h = 0; h < kMaxHeads; ++h) {
        if (h < H && (hm >> h & 1)) {
          const float g = s_g[w][h][k];
#pragma unroll
          for (int d = 0; d < kD; ++d) {
            const int i = (int)(pk >> (8 * d) & 255u) - f;
#pragma unroll
            for (int q = 0; q < kOwn; ++q) bins[h][d][q] = i == 64 * q ? bins[h][d][q] + g : bins[h][d][q];
          }
          acc[h] = fmaf(g, x, acc[h]);
        }
      }
    }
    wave_sync();  // the next chunk overwrites the rows, s_g and s_idx
  }
#pragma unroll
  for (int h = 0; h < kMaxHeads; ++h) {
    if (h < H) {
      float* __restrict__ gq = g_pq + (r * H + h) * kQ;
#pragma unroll
      for (int d = 0; d < kD; ++d)
#pragma unroll
        for (int q = 0; q < kOwn; ++q) gq[d * kBins + 64 * q + f] = bins[h][d][q];
      if (f < kQ - kD * kBins) gq[kD * kBins + f] = f <= kC ? acc[h] : 0.0f;  // the pads: 0
    }
  }
}

#define EMBED_KERNELS(NAME, KIND)                                                                                       \
  template <typename T, int MK>                                                                                         \
  __global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_embed_##NAME##_logits_kernel(                                \
      NmhSetHeads sh, int n_rows, const T* __restrict__ sets, int64_t set_stride, int R, int share,                      \
      const void* __restrict__ mask, int64_t ms, const float* __restrict__ pq, float* __restrict__ out, int64_t os) {   \
    embed_logits_body<KIND, T, MK>(sh, n_rows, sets, set_stride, R, share, mask, ms, pq, out, os);                      \
  }                                                                                                                     \
  template <typename T, int MK>                                                                                         \
  __global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_embed_##NAME##_logits_backward_kernel(                       \
      NmhSetHeads sh, int n_rows, const T* __restrict__ sets, int64_t set_stride, int R, int share,                      \
      const void* __restrict__ mask, int64_t ms, const float* __restrict__ g_out, int64_t gs,                            \
      float* __restrict__ g_pq) {                                                                                       \
    embed_backward_body<KIND, T, MK>(sh, n_rows, sets, set_stride, R, share, mask, ms, g_out, gs, g_pq);                \
  }
EMBED_KERNELS(entity, EntityKind)
EMBED_KERNELS(item, ItemKind)
#undef EMBED_KERNELS

constexpr SetKind kEmbedSets[2] = {
    {EntityKind::kCols, EntityKind::kMaxRows, "set", "set_stride", "elem_kind", "sh"},
    {ItemKind::kCols, ItemKind::kMaxRows, "set", "set_stride", "elem_kind", "sh"},
};

int check_kind(const char* fn, int32_t kind) {
  if (kind != NMH_EMBED_ENTITY && kind != NMH_EMBED_ITEM) return heads_fail(NMH_E_INVALID, "%s: unknown kind %d", fn, kind);
  return NMH_OK;
}

template <typename K, typename T>
void launch_features(int32_t n_sets, const void* set, int64_t set_stride, int32_t set_rows, const void* ids,
                     int64_t id_stride, int32_t id_kind, uint8_t* idx, float* cont, float* counts, float* sums,
                     int32_t* mine_idx, uint8_t* mine_i, float* mine_c, hipStream_t st) {
  hipLaunchKernelGGL((nmh_embed_features_kernel<K, T>), dim3((unsigned)n_sets), dim3(kThreads), 0, st,
                     static_cast<const T*>(set), set_stride, set_rows, ids, id_stride, id_kind, idx, cont, counts, sums,
                     mine_idx, mine_i, mine_c);
}

}  // namespace

extern "C" {

int nmh_embed_features(int32_t kind, int32_t n_sets, const void* set, int64_t set_stride, int32_t elem_kind,
                       int32_t set_rows, const void* ids, int64_t id_stride, int32_t id_kind, uint8_t* idx, float* cont,
                       float* counts, float* sums, int32_t* mine_idx, uint8_t* mine_i, float* mine_c, void* stream) {
  const char* fn = "nmh_embed_features";
  int rc = check_kind(fn, kind);
  if (rc != NMH_OK) return rc;
  if (n_sets < 0) return heads_fail(NMH_E_INVALID, "%s: n_sets %d is negative", fn, n_sets);
  rc = check_set(fn, kEmbedSets[kind], set, set_stride, elem_kind, set_rows);
  if (rc != NMH_OK) return rc;
  const bool own = mine_idx || mine_i || mine_c;
  if (!idx && !cont && !counts && !sums && !own) return heads_fail(NMH_E_INVALID, "%s: every output is NULL", fn);
  if (own) {
    if (kind != NMH_EMBED_ENTITY)
      return heads_fail(NMH_E_INVALID, "%s: mine_idx, mine_i and mine_c are the entity kind's", fn);
    rc = check_ids(fn, ids, id_stride, id_kind, "a mine output is");
    if (rc != NMH_OK) return rc;
  }
  if (n_sets == 0) return NMH_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
#define EMBED_FEATURES(K, T) \
  launch_features<K, T>(n_sets, set, set_stride, set_rows, ids, id_stride, id_kind, idx, cont, counts, sums, mine_idx, mine_i, mine_c, st)
  const bool f32 = elem_kind == NMH_ELEM_F32;
  if (kind == NMH_EMBED_ENTITY) {
    if (f32) EMBED_FEATURES(EntityKind, float);
    else EMBED_FEATURES(EntityKind, int16_t);
  } else {
    if (f32) EMBED_FEATURES(ItemKind, float);
    else EMBED_FEATURES(ItemKind, int16_t);
  }
#undef EMBED_FEATURES
  return heads_launched(fn);
}

int nmh_embed_logits(int32_t kind, const NmhSetHeads* sh, int32_t n_rows, const void* set, int64_t set_stride,
                     int32_t elem_kind, int32_t set_rows, int32_t share, const void* mask, int64_t mask_stride,
                     int32_t mask_kind, const float* pq, float* out, int64_t out_stride, void* stream) {
  const char* fn = "nmh_embed_logits";
  int rc = check_kind(fn, kind);
  if (rc != NMH_OK) return rc;
  rc = check_forward(fn, kEmbedSets[kind], sh, n_rows, set, set_stride, elem_kind, set_rows, share, mask, mask_stride,
                     mask_kind, pq, out, out_stride);
  if (rc != NMH_OK || n_rows == 0) return rc;
  if (kind == NMH_EMBED_ENTITY)
    HEADS_SET_LAUNCH(nmh_embed_entity_logits_kernel, elem_kind, mask_kind, kRowsPerBlock, stream, sh, n_rows, set,
                     set_stride, set_rows, share, mask, mask_stride, pq, out, out_stride);
  else
    HEADS_SET_LAUNCH(nmh_embed_item_logits_kernel, elem_kind, mask_kind, kRowsPerBlock, stream, sh, n_rows, set,
                     set_stride, set_rows, share, mask, mask_stride, pq, out, out_stride);
  return heads_launched(fn);
}

int nmh_embed_logits_backward(int32_t kind, const NmhSetHeads* sh, int32_t n_rows, const void* set, int64_t set_stride,
                              int32_t elem_kind, int32_t set_rows, int32_t share, const void* mask,
                              int64_t mask_stride, int32_t mask_kind, const float* g_out, int64_t g_stride,
                              float* g_pq, void* stream) {
  const char* fn = "nmh_embed_logits_backward";
  int rc = check_kind(fn, kind);
  if (rc != NMH_OK) return rc;
  rc = check_backward(fn, kEmbedSets[kind], sh, n_rows, set, set_stride, elem_kind, set_rows, share, mask, mask_stride,
                      mask_kind, g_out, g_stride, g_pq);
  if (rc != NMH_OK || n_rows == 0) return rc;
  if (kind == NMH_EMBED_ENTITY)
    HEADS_SET_LAUNCH(nmh_embed_entity_logits_backward_kernel, elem_kind, mask_kind, kRowsPerBlock, stream, sh, n_rows,
                     set, set_stride, set_rows, share, mask, mask_stride, g_out, g_stride, g_pq);
  else
    HEADS_SET_LAUNCH(nmh_embed_item_logits_backward_kernel, elem_kind, mask_kind, kRowsPerBlock, stream, sh, n_rows,
                     set, set_stride, set_rows, share, mask, mask_stride, g_out, g_stride, g_pq);
  return heads_launched(fn);
}

}  // extern "C"
