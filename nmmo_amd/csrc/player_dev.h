// player_dev.h — the device functions of SPEC.md §21 that more than one translation unit of
// libnmmo_heads.so uses (player_enc.hip, decoder.hip): the npc_type class rule, the column a feature
// depends on, the listed candidates' columns as float32 rows in LDS and the pointer logit of one
// such row; and, for player_enc.hip and embed_enc.hip (SPEC.md §25), the list of the candidates
// that any head of a set allows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "heads_dev.h"  // legal_at
#include "../../include/nmmo_heads.h"

namespace nmmo {
namespace player_dev {

constexpr int kC = NMH_PLAYER_COLS, kF = NMH_PLAYER_FEATURES, kTypes = NMH_PLAYER_TYPES, kQ = NMH_PLAYER_QUERY;
constexpr int kTypeCol = 1;
constexpr int kRaw = kC - 2;  // features [6, 35) are columns [2, 31)
constexpr int kHeadShift = 12;  // a list entry is j | (the allowing heads' bits << 12)

// SPEC §21's class rule: clamp(trunc(v), 0, 4), NaN -> 0
__device__ inline int npc_class(float v) { return v >= 0.0f ? (v >= (float)(kTypes - 1) ? kTypes - 1 : (int)v) : 0; }

// the column feature f < 35 depends on
__device__ inline int feature_col(int f) { return f == 0 ? 0 : (f <= kTypes ? kTypeCol : f - kTypes + 1); }

// The j < R that any head of a set allows (player_enc.hip, embed_enc.hip), ascending, into list[0, cnt) as j | heads << 12; returns cnt
// (wave-uniform). ZERO: orow[out_off[h] + j] = 0 for every j < R head h forbids.
template <int MK, bool ZERO>
__device__ __forceinline__ int legal_list_heads(const NmhSetHeads& ph, const void* __restrict__ mask, int64_t mbase,
                                                 int R, uint16_t* list, float* __restrict__ orow) {
  const int H = ph.n_heads, lane = lane_id();
  int cnt = 0;
  for (int b0 = 0; b0 < R; b0 += 64) {  // (wave-uniform trip count: every lane ballots)
    const int j = b0 + lane;
    bool lg[NMH_ITEM_MAX_HEADS];
#pragma unroll
    for (int h = 0; h < NMH_ITEM_MAX_HEADS; ++h)  // unconditional loads, all in flight
      lg[h] = h < H && legal_at<MK>(mask, mbase + ph.mask_off[h] + min(j, R - 1));
    unsigned hm = 0;
#pragma unroll
    for (int h = 0; h < NMH_ITEM_MAX_HEADS; ++h) {
      if (h < H && j < R) {
        if (lg[h]) hm |= 1u << h;
        else if (ZERO) orow[ph.out_off[h] + j] = 0.0f;
      }
    }
    const uint64_t b = __ballot(hm != 0);
    if (hm) list[cnt + __popcll(b & lanes_below())] = (uint16_t)(j | (hm << kHeadShift));
    cnt += __popcll(b);
  }
  return cnt;
}

// The 31 columns of listed candidates [i0, i0 + n) into rows[n][31] as float32: lane e takes
// element e % 31 of candidate e / 31, so a candidate's 31 elements are consecutive lanes' loads.
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ set, const uint16_t* list, int i0, int n,
                                           float* rows) {
  constexpr int kU = 4;
  const int tot = n * kC;
  for (int e0 = lane_id(); e0 < tot; e0 += 64 * kU) {
    T v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int e = e0 + 64 * u;
      v[u] = (T)0;
      if (e < tot) {
        const int k = e / kC;
        v[u] = set[(int64_t)(list[i0 + k] & ((1 << kHeadShift) - 1)) * kC + (e - k * kC)];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int e = e0 + 64 * u;
      if (e < tot) rows[e] = (float)v[u];
    }
  }
}

// SPEC §21's sum of one candidate's LDS row with the head's projected query in LDS
__device__ __forceinline__ float player_logit(const float* pq, const float* row) {
  float v = pq[kF] + pq[1 + npc_class(row[kTypeCol])];
  v = fmaf(pq[0], row[0], v);
#pragma unroll
  for (int k = 0; k < kRaw; ++k) v = fmaf(pq[1 + kTypes + k], row[2 + k], v);
  return v;
}

}  // namespace player_dev
}  // namespace nmmo
