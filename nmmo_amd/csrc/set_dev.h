// set_dev.h — the device code that the staged candidate-set kinds of libnmmo_heads.so share: entity
// rows (SPEC.md §21, player_enc.hip, decoder.hip) and both embedded kinds (§25, embed_enc.hip). The
// list of the candidates that any head of a set allows, the listed candidates' columns as float32
// rows in LDS, the rows' id and the column-by-slot scan of the features kernels. The forward and
// backward bodies over a list stay with their kinds (DESIGN.md §3.23 says why).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "heads_dev.h"  // legal_at
#include "../../include/nmmo_heads.h"

namespace nmmo {
namespace set_dev {

constexpr int kScanThreads = 256;  // scan_set's workgroup
constexpr int kHeadShift = 12;     // a list entry is j | (the allowing heads' bits << 12)
constexpr int kJMask = (1 << kHeadShift) - 1;

static_assert(NMH_ITEM_MAX_HEADS <= 16 - kHeadShift, "a list entry is 16 bits");

// The j < R that any head of a set allows, ascending, into list[0, cnt) as j | heads << 12; returns cnt
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

// The COLS columns of listed candidates [i0, i0 + n) into rows[n][STRIDE] as float32: lane e takes
// element e % COLS of candidate e / COLS, so a candidate's elements are consecutive lanes' loads.
template <int COLS, int STRIDE, typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ set, const uint16_t* list, int i0, int n,
                                           float* rows) {
  constexpr int kU = 4;
  const int tot = n * COLS;
  for (int e0 = lane_id(); e0 < tot; e0 += 64 * kU) {
    T v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int e = e0 + 64 * u;
      v[u] = (T)0;
      if (e < tot) {
        const int k = e / COLS;
        v[u] = set[(int64_t)(list[i0 + k] & kJMask) * COLS + (e - k * COLS)];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int e = e0 + 64 * u;
      if (e < tot) {
        if constexpr (STRIDE == COLS) {
          rows[e] = (float)v[u];
        } else {
          const int k = e / COLS;
          rows[k * STRIDE + (e - k * COLS)] = (float)v[u];
        }
      }
    }
  }
}

__device__ inline float load_id(const void* __restrict__ ids, int64_t i, int id_kind) {
  return id_kind == NMH_ELEM_F32 ? static_cast<const float*>(ids)[i] : (float)static_cast<const int16_t*>(ids)[i];
}

// ---------------------------------------------------------------- the features scan
// A 256-thread workgroup's pass over one set: this thread is column c of slot `slot` < 256 / COLS, so
// a pass reads 256 / COLS candidates' contiguous elements, four passes in flight. Returns the sum of
// the thread's column over its candidates in ascending order; sink(j, x) sees each of its elements;
// own: the least j whose column 0 equals id and is not 0 goes to *s_first by an LDS integer min.
template <int COLS, typename T, typename Sink>
__device__ __forceinline__ float scan_set(const T* __restrict__ set, int R, int slot, int c, bool own, float id,
                                          int* s_first, Sink sink) {
  constexpr int kSlots = kScanThreads / COLS, kU = 4;
  float acc = 0.0f;
  for (int j0 = 0; j0 < R; j0 += kSlots * kU) {
    T v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = j0 + u * kSlots + slot;
      v[u] = j < R ? set[(int64_t)j * COLS + c] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = j0 + u * kSlots + slot;
      if (j < R) {
        const float x = (float)v[u];
        acc += x;
        if (c == 0 && own && x == id && x != 0.0f) atomicMin(s_first, j);
        sink(j, x);
      }
    }
  }
  return acc;
}

}  // namespace set_dev
}  // namespace nmmo
