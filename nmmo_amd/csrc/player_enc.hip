// player_enc.hip — the Entity path of the reference's observation encoder without its embeddings
// (SPEC.md §21; include/nmmo_heads.h, nmh_player_features / nmh_player_logits /
// nmh_player_logits_backward). Part of libnmmo_heads.so.
//
// PlayerEncoder.agent_fc is linear and its input x is a fixed 35-feature function of an entity's 31
// columns (column 0, five npc_type one-hots, columns 2..30 raw), so
//   mean_j agent_fc(x_j) = agent_fc(mean_j x_j)   -> the pool needs one 35-float sum per row,
//   q . agent_fc(x_j)    = (W^T q) . x_j + q . b  -> a pointer logit needs the candidate's own 124 bytes,
// and my_agent_fc needs the features of one entity row. No [N, R, H] embedding exists in forward and
// no key gradient in backward.
//
// An entity row is 31 elements: never 16-byte aligned, and a lane per entity would make 31 loads 124
// bytes apart. Every load of the Entity section here has consecutive lanes on consecutive elements.
//
// features / sums / own row: one 256-thread workgroup per set. Thread t < 248 is column t % 31 of slot
// t / 31, so a pass reads 8 entities = 248 contiguous elements, four passes in flight. A thread keeps
// the sum of its column over its entities in ascending order and one thread adds a column's 8
// partial sums in ascending order; the class counts are LDS integer adds and the own row is an LDS
// integer min over the matching j. With only the own row asked for, a wave per set reads column 0.
//
// logits: one wave per obs row, four rows per workgroup, no workgroup barrier. The wave reads the
// heads' mask entries (lane j is candidate j, 64 at a time), stores 0 where a head forbids j, and
// ballots the j that any head allows into an ascending LDS list with the allowing heads' bits. 64
// listed candidates at a time, their 31 columns are copied into LDS (lane e takes element e % 31 of
// listed candidate e / 31, four loads in flight) as float32 rows of 31 words: an odd stride, so the
// lanes that then take one candidate each read without a bank conflict. A lane evaluates SPEC §21's
// sum once per allowing head with the head's projected query in LDS. Entities no head allows are
// never addressed.
//
// logits_backward: same grid, list and LDS rows, plus the listed candidates' g_out per head. Lane
// f < 36 owns feature f and walks the list in ascending order: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "heads_dev.h"   // wave_sync
#include "heads_host.h"  // heads_fail, heads_launched, check_set, check_ids, check_forward, check_backward, HEADS_SET_LAUNCH
#include "player_dev.h"  // player_logit, feature_col, npc_class
#include "set_dev.h"     // legal_list_heads, stage_rows, scan_set, load_id
#include "../../include/nmmo_heads.h"

using namespace nmmo;
using namespace nmmo::player_dev;
using set_dev::kHeadShift;
using set_dev::kJMask;
using set_dev::legal_list_heads;
using set_dev::load_id;

namespace {

constexpr int kMaxRows = NMH_PLAYER_MAX_ROWS, kMaxHeads = NMH_PLAYER_MAX_HEADS;
constexpr int kThreads = set_dev::kScanThreads, kSlots = kThreads / kC, kRowsPerBlock = 4, kChunk = 64;

static_assert(kSlots == 8, "eight entities a pass");
static_assert(kMaxRows <= (1 << kHeadShift), "a list entry is 16 bits");

// column c's part of x [35]: feature 0, the five one-hots, or feature c + 4
__device__ inline void put_x(float* __restrict__ x, int c, float v) {
  if (c == kTypeCol) {
    const int t = npc_class(v);
#pragma unroll
    for (int i = 0; i < kTypes; ++i) x[1 + i] = i == t ? 1.0f : 0.0f;
  } else {
    x[c == 0 ? 0 : c + kTypes - 1] = v;
  }
}

// ---------------------------------------------------------------- features, sums and the own row
template <typename T>
__global__ __launch_bounds__(kThreads) void nmh_player_features_kernel(
    const T* __restrict__ ents, int64_t ent_stride, int R, const void* __restrict__ ids, int64_t id_stride,
    int id_kind, float* __restrict__ features, float* __restrict__ sums, float* __restrict__ mine,
    int32_t* __restrict__ mine_idx) {
  __shared__ float s_part[kSlots][kC];
  __shared__ int s_cnt[kTypes];
  __shared__ int s_first;
  const int tid = threadIdx.x, slot = tid / kC, c = tid % kC;
  const int64_t m = blockIdx.x;
  const bool own = mine || mine_idx;
  if (tid < kTypes) s_cnt[tid] = 0;
  if (tid == 0) s_first = R;
  __syncthreads();
  const T* __restrict__ set = ents + m * ent_stride;
  float* __restrict__ fset = features ? features + m * (int64_t)R * kF : nullptr;
  const float id = own ? load_id(ids, m * id_stride, id_kind) : 0.0f;
  if (slot < kSlots)
    s_part[slot][c] = set_dev::scan_set<kC>(set, R, slot, c, own, id, &s_first, [&](int j, float x) {
      if (c == kTypeCol) atomicAdd(&s_cnt[npc_class(x)], 1);
      if (fset) put_x(fset + (int64_t)j * kF, c, x);
    });
  __syncthreads();
  if (sums && tid < kF) {
    float s;
    if (tid >= 1 && tid <= kTypes) {
      s = (float)s_cnt[tid - 1];
    } else {
      const int col = feature_col(tid);
      s = 0.0f;
      for (int q = 0; q < kSlots; ++q) s += s_part[q][col];
    }
    sums[m * kF + tid] = s;
  }
  if (own) {
    const int idx = s_first < R ? s_first : 0;
    if (mine_idx && tid == 0) mine_idx[m] = idx;
    if (mine && tid < kC) put_x(mine + m * kF, tid, (float)set[(int64_t)idx * kC + tid]);
  }
}

// the own row alone: one wave per set reads column 0
template <typename T>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_player_own_kernel(
    int n_sets, const T* __restrict__ ents, int64_t ent_stride, int R, const void* __restrict__ ids,
    int64_t id_stride, int id_kind, float* __restrict__ mine, int32_t* __restrict__ mine_idx) {
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int64_t m = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (m >= n_sets) return;
  const T* __restrict__ set = ents + m * ent_stride;
  const float id = load_id(ids, m * id_stride, id_kind);
  int idx = 0;
  for (int b0 = 0; b0 < R; b0 += 64) {  // (wave-uniform: every lane ballots)
    const int j = b0 + lane;
    const float x = j < R ? (float)set[(int64_t)j * kC] : 0.0f;
    const uint64_t b = __ballot(j < R && x == id && x != 0.0f);
    if (b) {
      idx = b0 + __builtin_ctzll(b);
      break;
    }
  }
  if (mine_idx && lane == 0) mine_idx[m] = idx;
  if (mine && lane < kC) put_x(mine + m * kF, lane, (float)set[(int64_t)idx * kC + lane]);
}

// ---------------------------------------------------------------- pointer logits
template <typename T, int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_player_logits_kernel(
    NmhPlayerHeads ph, int n_rows, const T* __restrict__ ents, int64_t ent_stride, int R,
    const void* __restrict__ mask, int64_t ms, const float* __restrict__ pq, float* __restrict__ out, int64_t os) {
  __shared__ float s_pq[kRowsPerBlock][kMaxHeads * kQ];
  __shared__ float s_rows[kRowsPerBlock][kChunk * kC];
  __shared__ uint16_t s_list[kRowsPerBlock][kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const int H = ph.n_heads;
  float* spq = s_pq[w];
  float* rows = s_rows[w];
  uint16_t* list = s_list[w];
  for (int i = lane; i < H * kQ; i += 64) spq[i] = pq[r * H * kQ + i];
  const T* __restrict__ set = ents + r * ent_stride;
  float* __restrict__ orow = out + r * os;
  const int cnt = legal_list_heads<MK, true>(ph, mask, r * ms, R, list, orow);
#pragma unroll
  for (int h = 0; h < kMaxHeads; ++h)
    if (h < H && lane == h) orow[ph.out_off[h] + R] = 0.0f;  // the no-op entries
  wave_sync();
  for (int i0 = 0; i0 < cnt; i0 += kChunk) {
    const int n = min(kChunk, cnt - i0);
    set_dev::stage_rows<kC, kC>(set, list, i0, n, rows);
    wave_sync();
    if (lane < n) {
      const int entry = list[i0 + lane], j = entry & kJMask, hm = entry >> kHeadShift;
      const float* row = rows + lane * kC;
#pragma unroll
      for (int h = 0; h < kMaxHeads; ++h)
        if (h < H && (hm >> h & 1)) orow[ph.out_off[h] + j] = player_logit(spq + h * kQ, row);
    }
    wave_sync();  // the next chunk overwrites the rows
  }
}

template <typename T, int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_player_logits_backward_kernel(
    NmhPlayerHeads ph, int n_rows, const T* __restrict__ ents, int64_t ent_stride, int R,
    const void* __restrict__ mask, int64_t ms, const float* __restrict__ g_out, int64_t gs, float* __restrict__ g_pq) {
  __shared__ float s_rows[kRowsPerBlock][kChunk * kC];
  __shared__ float s_g[kRowsPerBlock][kMaxHeads][kChunk];
  __shared__ uint16_t s_list[kRowsPerBlock][kMaxRows];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), f = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const int H = ph.n_heads;
  float* rows = s_rows[w];
  uint16_t* list = s_list[w];
  const T* __restrict__ set = ents + r * ent_stride;
  const float* __restrict__ grow = g_out + r * gs;
  const int cnt = legal_list_heads<MK, false>(ph, mask, r * ms, R, list, nullptr);
  // the column feature f reads; the constant (f = 35) and the lanes beyond read column 0 and drop it
  const int col = f < kF ? feature_col(f) : 0;
  float acc[kMaxHeads] = {};
  wave_sync();
  for (int i0 = 0; i0 < cnt; i0 += kChunk) {
    const int n = min(kChunk, cnt - i0);
    set_dev::stage_rows<kC, kC>(set, list, i0, n, rows);
    if (f < n) {  // lane k: listed candidate k's g_out in the heads that allow it, no other entry
      const int entry = list[i0 + f], j = entry & kJMask, hm = entry >> kHeadShift;
#pragma unroll
      for (int h = 0; h < kMaxHeads; ++h)
        if (h < H && (hm >> h & 1)) s_g[w][h][f] = grow[ph.out_off[h] + j];
    }
    wave_sync();
    if (f <= kF) {
      for (int k = 0; k < n; ++k) {
        const int hm = list[i0 + k] >> kHeadShift;  // (wave-uniform)
        const float c = rows[k * kC + col];
        float x = c;
        if (f >= 1 && f <= kTypes) x = npc_class(c) == f - 1 ? 1.0f : 0.0f;
        if (f == kF) x = 1.0f;
#pragma unroll
        for (int h = 0; h < kMaxHeads; ++h)
          if (h < H && (hm >> h & 1)) acc[h] = fmaf(s_g[w][h][k], x, acc[h]);
      }
    }
    wave_sync();  // the next chunk overwrites the rows and s_g
  }
  if (f < kQ) {
#pragma unroll
    for (int h = 0; h < kMaxHeads; ++h)
      if (h < H) g_pq[(r * H + h) * kQ + f] = acc[h];  // the pads' lanes added nothing: 0
  }
}

}  // namespace

extern "C" {

int nmh_player_features(int32_t n_sets, const void* ents, int64_t ent_stride, int32_t ent_kind, int32_t set_rows,
                        const void* ids, int64_t id_stride, int32_t id_kind, float* features, float* sums,
                        float* mine, int32_t* mine_idx, void* stream) {
  const char* fn = "nmh_player_features";
  if (n_sets < 0) return heads_fail(NMH_E_INVALID, "%s: n_sets %d is negative", fn, n_sets);
  int rc = check_set(fn, kEntitySets, ents, ent_stride, ent_kind, set_rows);
  if (rc != NMH_OK) return rc;
  if (!features && !sums && !mine && !mine_idx)
    return heads_fail(NMH_E_INVALID, "%s: features, sums, mine and mine_idx are all NULL", fn);
  if (mine || mine_idx) rc = check_ids(fn, ids, id_stride, id_kind, "mine or mine_idx is");
  if (rc != NMH_OK) return rc;
  if (n_sets == 0) return NMH_OK;
  const bool f32 = ent_kind == NMH_PLAYER_F32;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!features && !sums) {
    const dim3 grid((unsigned)((n_sets + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
    if (f32)
      hipLaunchKernelGGL(nmh_player_own_kernel<float>, grid, block, 0, st, n_sets, static_cast<const float*>(ents),
                         ent_stride, set_rows, ids, id_stride, id_kind, mine, mine_idx);
    else
      hipLaunchKernelGGL(nmh_player_own_kernel<int16_t>, grid, block, 0, st, n_sets,
                         static_cast<const int16_t*>(ents), ent_stride, set_rows, ids, id_stride, id_kind, mine,
                         mine_idx);
    return heads_launched(fn);
  }
  const dim3 grid((unsigned)n_sets), block(kThreads);
  if (f32)
    hipLaunchKernelGGL(nmh_player_features_kernel<float>, grid, block, 0, st, static_cast<const float*>(ents),
                       ent_stride, set_rows, ids, id_stride, id_kind, features, sums, mine, mine_idx);
  else
    hipLaunchKernelGGL(nmh_player_features_kernel<int16_t>, grid, block, 0, st, static_cast<const int16_t*>(ents),
                       ent_stride, set_rows, ids, id_stride, id_kind, features, sums, mine, mine_idx);
  return heads_launched(fn);
}

int nmh_player_logits(const NmhPlayerHeads* ph, int32_t n_rows, const void* ents, int64_t ent_stride,
                      int32_t ent_kind, int32_t set_rows, const void* mask, int64_t mask_stride, int32_t mask_kind,
                      const float* pq, float* out, int64_t out_stride, void* stream) {
  const char* fn = "nmh_player_logits";
  const int rc = check_forward(fn, kEntitySets, ph, n_rows, ents, ent_stride, ent_kind, set_rows, 1, mask, mask_stride,
                               mask_kind, pq, out, out_stride);
  if (rc != NMH_OK || n_rows == 0) return rc;
  HEADS_SET_LAUNCH(nmh_player_logits_kernel, ent_kind, mask_kind, kRowsPerBlock, stream, ph, n_rows, ents, ent_stride,
                   set_rows, mask, mask_stride, pq, out, out_stride);
  return heads_launched(fn);
}

int nmh_player_logits_backward(const NmhPlayerHeads* ph, int32_t n_rows, const void* ents, int64_t ent_stride,
                               int32_t ent_kind, int32_t set_rows, const void* mask, int64_t mask_stride,
                               int32_t mask_kind, const float* g_out, int64_t g_stride, float* g_pq, void* stream) {
  const char* fn = "nmh_player_logits_backward";
  const int rc = check_backward(fn, kEntitySets, ph, n_rows, ents, ent_stride, ent_kind, set_rows, 1, mask,
                                mask_stride, mask_kind, g_out, g_stride, g_pq);
  if (rc != NMH_OK || n_rows == 0) return rc;
  HEADS_SET_LAUNCH(nmh_player_logits_backward_kernel, ent_kind, mask_kind, kRowsPerBlock, stream, ph, n_rows, ents,
                   ent_stride, set_rows, mask, mask_stride, g_out, g_stride, g_pq);
  return heads_launched(fn);
}

}  // extern "C"
