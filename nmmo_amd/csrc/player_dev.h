// player_dev.h — the device functions of SPEC.md §21 that more than one translation unit of
// libnmmo_heads.so uses (player_enc.hip, decoder.hip): the npc_type class rule, the column a feature
// depends on, the listed candidates' columns as float32 rows in LDS and the pointer logit of one
// such row.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
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
