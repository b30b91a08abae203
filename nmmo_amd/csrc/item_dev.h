// item_dev.h — the device functions of SPEC.md §20 that more than one translation unit of
// libnmmo_heads.so uses (item_enc.hip, decoder.hip): an item's class rules, its 16 columns loaded
// wherever it lies, the 15-term pointer logit and a feature from the one column it depends on.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmmo_heads.h"

namespace nmmo {
namespace item_dev {

constexpr int kC = NMH_ITEM_COLS, kF = NMH_ITEM_FEATURES, kTypes = NMH_ITEM_TYPES, kQ = NMH_ITEM_QUERY;
constexpr int kDiscrete = kTypes + 2;  // features [0, 20) are one-hots, [20, 32) scaled columns
constexpr int kCont = kF - kDiscrete;  // 12
constexpr int kTypeCol = 1, kEquipCol = 14;
constexpr float kScale = 0.01f;

// the item column behind scaled feature 20 + k: 3, 4, ..., 13, 15
__host__ __device__ constexpr int cont_col(int k) { return k < kCont - 1 ? 3 + k : 15; }

// SPEC §20's class rule: clamp(trunc(v), 0, hi), NaN -> 0
__device__ inline int item_class(float v, int hi) { return v >= 0.0f ? (v >= (float)hi ? hi : (int)v) : 0; }
__device__ inline int item_class(int16_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

struct Item {
  int type, equipped;
  float x[kCont];  // features 20..31
};

// The 16 columns of one item, wherever it lies: four (two) 16-byte loads when the item is 16-byte
// aligned, else element loads.
template <typename T>
__device__ __forceinline__ Item load_item(const T* __restrict__ p) {
  T c[kC];
  constexpr int kVec = (int)(sizeof(T) * kC / 16);
  if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    uint4 q[kVec];
#pragma unroll
    for (int i = 0; i < kVec; ++i) q[i] = reinterpret_cast<const uint4*>(p)[i];
    __builtin_memcpy(c, q, sizeof(c));
  } else {
#pragma unroll
    for (int i = 0; i < kC; ++i) c[i] = p[i];
  }
  Item it;
  it.type = item_class(c[kTypeCol], kTypes - 1);
  it.equipped = item_class(c[kEquipCol], 1);
#pragma unroll
  for (int k = 0; k < kCont; ++k) it.x[k] = (float)c[cont_col(k)] * kScale;
  return it;
}

// SPEC §20's 15-term sum with the head's projected query in LDS
__device__ __forceinline__ float item_logit(const float* pq, const Item& it) {
  float v = pq[kF] + pq[it.type];
  v += pq[kTypes + it.equipped];
#pragma unroll
  for (int k = 0; k < kCont; ++k) v = fmaf(pq[kDiscrete + k], it.x[k], v);
  return v;
}

// feature f < 32 of an item from the one column it depends on
template <typename T>
__device__ __forceinline__ float item_feature(int f, T c) {
  if (f < kTypes) return item_class(c, kTypes - 1) == f ? 1.0f : 0.0f;
  if (f < kDiscrete) return item_class(c, 1) == f - kTypes ? 1.0f : 0.0f;
  return (float)c * kScale;
}

// the column feature f < 32 depends on
__device__ inline int feature_col(int f) {
  return f < kTypes ? kTypeCol : (f < kDiscrete ? kEquipCol : cont_col(f - kDiscrete));
}

}  // namespace item_dev
}  // namespace nmmo
