// player_dev.h — the device functions of SPEC.md §21 that more than one translation unit of
// libnmmo_heads.so uses (player_enc.hip, decoder.hip): the npc_type class rule, the column a feature
// depends on and the pointer logit of one staged LDS row (set_dev.h's stage_rows).
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

static_assert(kC == 31 && kF == 35 && kTypes == 5 && kQ == 40 && kRaw == 29, "the start-kit entity row");

// SPEC §21's class rule: clamp(trunc(v), 0, 4), NaN -> 0
__device__ inline int npc_class(float v) { return v >= 0.0f ? (v >= (float)(kTypes - 1) ? kTypes - 1 : (int)v) : 0; }

// the column feature f < 35 depends on
__device__ inline int feature_col(int f) { return f == 0 ? 0 : (f <= kTypes ? kTypeCol : f - kTypes + 1); }

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
