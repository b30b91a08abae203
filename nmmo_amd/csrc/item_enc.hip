// item_enc.hip — the item path of the reference's observation encoder without its embeddings
// (SPEC.md §20; include/nmmo_heads.h, nmh_item_features / nmh_item_logits /
// nmh_item_logits_backward). Part of libnmmo_heads.so.
//
// ItemEncoder.fc is linear and its input x is a fixed 32-feature function of an item's 16 columns
// (18 type one-hots, 2 equipped one-hots, 12 columns scaled by 0.01), so
//   mean_j fc(x_j) = fc(mean_j x_j)            -> the pool needs one 32-float sum per set,
//   q . fc(x_j)    = (W^T q) . x_j + q . b     -> a pointer logit needs the candidate's own 64 bytes.
// No [N, R, H] embedding exists in forward and no key gradient in backward.
//
// features / sums: 16 consecutive lanes take the 16 columns of one item, so a wave's load is 256
// contiguous bytes (128 for int16) whatever the section's alignment; a set is taken by a wave
// (R <= 64, four sets per workgroup) or by a 256-thread workgroup. A thread keeps the sum of its
// column over its items in ascending order, the 4 or 16 partial sums of a column are added in
// ascending order by one thread, and the sum is scaled once. The type and equipped counts are
// LDS integer adds. Every lane's loads of a pass are issued before the first is used.
//
// logits: one wave per obs row, four rows per workgroup. R <= 64: lane j is candidate j, loads its
// item once if any head allows it and evaluates every head. R > 64: per head, the legal j in
// ascending order in an LDS list (four mask loads in flight per lane, ballot + rank), one lane per
// listed candidate. Every entry of out is stored exactly once: 0 by the lane that read its mask
// entry as illegal, the logit by the lane that took the candidate. Illegal candidates' items are
// never addressed.
//
// logits_backward: same grid and list. Lane f < 33 owns feature f of the head and walks the list
// in ascending order, eight candidates' loads in flight: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "heads_dev.h"   // wave_sync, legal_at
#include "heads_host.h"  // heads_fail, heads_launched, check_set, check_forward, check_backward, HEADS_SET_LAUNCH
#include "item_dev.h"    // load_item, item_logit, item_feature, item_class: shared with decoder.hip
#include "../../include/nmmo_heads.h"

using namespace nmmo;
using namespace nmmo::item_dev;

namespace {

constexpr int kMaxRows = NMH_ITEM_MAX_ROWS, kMaxHeads = NMH_ITEM_MAX_HEADS;
constexpr int kThreads = 256, kRowsPerBlock = 4;

static_assert(kC == 16 && kF == 32 && kTypes == 18 && kQ == 36 && kCont == 12, "the start-kit item row");

// lane `src`'s value of v (every lane of the wave takes part)
__device__ inline float shfl_item(float v, int src) { return __shfl(v, src); }
__device__ inline int16_t shfl_item(int16_t v, int src) { return (int16_t)__shfl((int)v, src); }

// ---------------------------------------------------------------- features and sums
// G threads per set: 64 (a wave; R <= 64) or 256 (the workgroup).
template <typename T, int G>
__global__ __launch_bounds__(kThreads) void nmh_item_features_kernel(
    int n_sets, const T* __restrict__ items, int64_t item_stride, int R, float* __restrict__ features,
    float* __restrict__ sums) {
  constexpr int kSets = kThreads / G, kSlots = G / kC, kU = 4;
  __shared__ float s_part[kSets][kSlots][kC];
  __shared__ int s_cnt[kSets][kDiscrete];
  const int tid = threadIdx.x, sub = tid / G, t = tid % G, c = t & (kC - 1), slot = t / kC;
  const int64_t m = (int64_t)blockIdx.x * kSets + sub;
  const bool live = m < n_sets;  // uniform over a wave: G is a multiple of 64
  if (t < kDiscrete) s_cnt[sub][t] = 0;
  __syncthreads();
  float acc = 0.0f;
  if (live) {
    const T* __restrict__ set = items + m * item_stride;
    float* __restrict__ fset = features ? features + m * (int64_t)R * kF : nullptr;
    const int base = threadIdx.x & 63 & ~(kC - 1);  // first lane of this item's 16
    // feature c + 16 of an item: types 16 and 17, the two equipped classes, then the scaled columns
    const int src = c < 4 ? (c < 2 ? kTypeCol : kEquipCol) : cont_col(c - 4);
    for (int j0 = 0; j0 < R; j0 += kSlots * kU) {
      T v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int j = j0 + u * kSlots + slot;
        v[u] = j < R ? set[(int64_t)j * kC + c] : (T)0;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int j = j0 + u * kSlots + slot;  // the same in the 16 lanes of an item
        const bool in = j < R;
        if (in) {
          acc += (float)v[u];
          if (c == kTypeCol) atomicAdd(&s_cnt[sub][item_class(v[u], kTypes - 1)], 1);
          if (c == kEquipCol) atomicAdd(&s_cnt[sub][kTypes + item_class(v[u], 1)], 1);
        }
        if (fset) {  // (uniform) every lane takes part in the exchanges
          const T tv = shfl_item(v[u], base | kTypeCol), sv = shfl_item(v[u], base | src);
          const int type = item_class(tv, kTypes - 1);
          const float lo = c == type ? 1.0f : 0.0f;
          float hi;
          if (c < 2) hi = c + kC == type ? 1.0f : 0.0f;
          else if (c < 4) hi = item_class(sv, 1) == c - 2 ? 1.0f : 0.0f;
          else hi = (float)sv * kScale;
          if (in) {
            fset[(int64_t)j * kF + c] = lo;
            fset[(int64_t)j * kF + kC + c] = hi;
          }
        }
      }
    }
  }
  s_part[sub][slot][c] = acc;
  __syncthreads();
  if (live && sums && t < kF) {
    float s;
    if (t < kDiscrete) {
      s = (float)s_cnt[sub][t];
    } else {
      const int col = cont_col(t - kDiscrete);
      s = 0.0f;
      for (int q = 0; q < kSlots; ++q) s += s_part[sub][q][col];
      s *= kScale;
    }
    sums[m * kF + t] = s;
  }
}

// ---------------------------------------------------------------- pointer logits
// The legal j < m of mask entries mbase + [0, m), ascending, into list[0, cnt); returns cnt
// (wave-uniform). zero != NULL: zero[j] = 0 for every illegal j < m. (heads_dev.h's legal_list fills
// an LDS tile's every entry; this one stores to a global row, and only where the mask forbids.)
template <int MK>
__device__ __forceinline__ int item_legal_list(const void* __restrict__ mask, int64_t mbase, int m, uint16_t* list,
                                               float* __restrict__ zero) {
  constexpr int kU = 4;  // mask loads in flight per lane
  int cnt = 0;
  for (int b0 = 0; b0 < m; b0 += 64 * kU) {  // (wave-uniform trip count: every lane ballots)
    const int j0 = b0 + lane_id();
    bool l[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) l[u] = legal_at<MK>(mask, mbase + min(j0 + 64 * u, m - 1));  // unconditional loads
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const int j = j0 + 64 * u;
      const bool lg = l[u] && j < m;
      const uint64_t b = __ballot(lg);
      if (lg) list[cnt + __popcll(b & lanes_below())] = (uint16_t)j;
      if (zero && j < m && !lg) zero[j] = 0.0f;
      cnt += __popcll(b);
    }
  }
  return cnt;
}

template <typename T, int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_item_logits_kernel(
    NmhItemHeads ih, int n_rows, const T* __restrict__ items, int64_t item_stride, int R, int share,
    const void* __restrict__ mask, int64_t ms, const float* __restrict__ pq, float* __restrict__ out, int64_t os) {
  __shared__ float s_pq[kRowsPerBlock][kMaxHeads * kQ];
  __shared__ uint16_t s_list[kRowsPerBlock][kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const int H = ih.n_heads;
  float* spq = s_pq[w];
  uint16_t* list = s_list[w];
  for (int i = lane; i < H * kQ; i += 64) spq[i] = pq[r * H * kQ + i];
  const T* __restrict__ set = items + (r / share) * item_stride;
  float* __restrict__ orow = out + r * os;
  wave_sync();
  if (R <= 64) {  // lane j is candidate j: its item is loaded once for all heads
    bool lg[kMaxHeads];
    bool any = false;
#pragma unroll
    for (int h = 0; h < kMaxHeads; ++h) {
      lg[h] = h < H && lane < R && legal_at<MK>(mask, r * ms + ih.mask_off[h] + lane);
      any = any || lg[h];
    }
    Item it = {};
    if (any) it = load_item(set + (int64_t)lane * kC);
#pragma unroll
    for (int h = 0; h < kMaxHeads; ++h) {
      if (h < H) {
        if (lane < R) orow[ih.out_off[h] + lane] = lg[h] ? item_logit(spq + h * kQ, it) : 0.0f;
        if (lane == 0) orow[ih.out_off[h] + R] = 0.0f;  // the no-op entry
      }
    }
    return;
  }
  for (int h = 0; h < H; ++h) {
    float* __restrict__ oh = orow + ih.out_off[h];
    const int cnt = item_legal_list<MK>(mask, r * ms + ih.mask_off[h], R, list, oh);
    if (lane == 0) oh[R] = 0.0f;  // the no-op entry
    wave_sync();
    for (int i = lane; i < cnt; i += 64) {
      const int j = list[i];
      oh[j] = item_logit(spq + h * kQ, load_item(set + (int64_t)j * kC));
    }
    wave_sync();  // the next head rebuilds the list
  }
}

template <typename T, int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_item_logits_backward_kernel(
    NmhItemHeads ih, int n_rows, const T* __restrict__ items, int64_t item_stride, int R, int share,
    const void* __restrict__ mask, int64_t ms, const float* __restrict__ g_out, int64_t gs, float* __restrict__ g_pq) {
  constexpr int kU = 8;  // candidates in flight per lane
  __shared__ uint16_t s_list[kRowsPerBlock][kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), f = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  uint16_t* list = s_list[w];
  const int H = ih.n_heads;
  const T* __restrict__ set = items + (r / share) * item_stride;
  // the column feature f reads; the constant (f = 32) and the lanes beyond read none
  const int col = f < kTypes ? kTypeCol : (f < kDiscrete ? kEquipCol : cont_col(min(f, kF - 1) - kDiscrete));
  for (int h = 0; h < H; ++h) {
    const float* __restrict__ gh = g_out + r * gs + ih.out_off[h];
    const int cnt = item_legal_list<MK>(mask, r * ms + ih.mask_off[h], R, list, nullptr);
    wave_sync();
    float acc = 0.0f;
    if (f <= kF) {
      for (int i0 = 0; i0 < cnt; i0 += kU) {
        float g[kU];
        T c[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          g[u] = 0.0f;
          c[u] = (T)0;
          if (i0 + u < cnt) {
            const int j = list[i0 + u];
            g[u] = gh[j];
            if (f < kF) c[u] = set[(int64_t)j * kC + col];
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
          if (i0 + u < cnt) acc = fmaf(g[u], f < kF ? item_feature(f, c[u]) : 1.0f, acc);
      }
    }
    if (f < kQ) g_pq[(r * H + h) * kQ + f] = acc;  // the pads' lanes added nothing: 0
    wave_sync();  // the next head rebuilds the list
  }
}

}  // namespace

extern "C" {

int nmh_item_features(int32_t n_sets, const void* items, int64_t item_stride, int32_t item_kind, int32_t set_rows,
                      float* features, float* sums, void* stream) {
  const char* fn = "nmh_item_features";
  if (n_sets < 0) return heads_fail(NMH_E_INVALID, "%s: n_sets %d is negative", fn, n_sets);
  const int rc = check_set(fn, kItemSets, items, item_stride, item_kind, set_rows);
  if (rc != NMH_OK) return rc;
  if (!features && !sums) return heads_fail(NMH_E_INVALID, "%s: features and sums are both NULL", fn);
  if (n_sets == 0) return NMH_OK;
  const bool small = set_rows <= 64, f32 = item_kind == NMH_ITEM_F32;
  const int per_block = small ? kThreads / 64 : 1;
  const dim3 grid((unsigned)((n_sets + per_block - 1) / per_block)), block(kThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define ITEM_FEATURES(T, G)                                                                           \
  hipLaunchKernelGGL((nmh_item_features_kernel<T, G>), grid, block, 0, st, n_sets, static_cast<const T*>(items), \
                     item_stride, set_rows, features, sums)
  if (f32 && small) ITEM_FEATURES(float, 64);
  else if (f32) ITEM_FEATURES(float, 256);
  else if (small) ITEM_FEATURES(int16_t, 64);
  else ITEM_FEATURES(int16_t, 256);
#undef ITEM_FEATURES
  return heads_launched(fn);
}

int nmh_item_logits(const NmhItemHeads* ih, int32_t n_rows, const void* items, int64_t item_stride, int32_t item_kind,
                    int32_t set_rows, int32_t share, const void* mask, int64_t mask_stride, int32_t mask_kind,
                    const float* pq, float* out, int64_t out_stride, void* stream) {
  const char* fn = "nmh_item_logits";
  const int rc = check_forward(fn, kItemSets, ih, n_rows, items, item_stride, item_kind, set_rows, share, mask,
                               mask_stride, mask_kind, pq, out, out_stride);
  if (rc != NMH_OK || n_rows == 0) return rc;
  HEADS_SET_LAUNCH(nmh_item_logits_kernel, item_kind, mask_kind, kRowsPerBlock, stream, ih, n_rows, items, item_stride,
                   set_rows, share, mask, mask_stride, pq, out, out_stride);
  return heads_launched(fn);
}

int nmh_item_logits_backward(const NmhItemHeads* ih, int32_t n_rows, const void* items, int64_t item_stride,
                             int32_t item_kind, int32_t set_rows, int32_t share, const void* mask,
                             int64_t mask_stride, int32_t mask_kind, const float* g_out, int64_t g_stride,
                             float* g_pq, void* stream) {
  const char* fn = "nmh_item_logits_backward";
  const int rc = check_backward(fn, kItemSets, ih, n_rows, items, item_stride, item_kind, set_rows, share, mask,
                                mask_stride, mask_kind, g_out, g_stride, g_pq);
  if (rc != NMH_OK || n_rows == 0) return rc;
  HEADS_SET_LAUNCH(nmh_item_logits_backward_kernel, item_kind, mask_kind, kRowsPerBlock, stream, ih, n_rows, items,
                   item_stride, set_rows, share, mask, mask_stride, g_out, g_stride, g_pq);
  return heads_launched(fn);
}

}  // extern "C"
