// decoder.hip — all action heads of the start-kit Baseline's decoder from the obs rows in one
// launch (SPEC.md §23; include/nmmo_heads.h, nmh_decoder_forward / nmh_decoder_backward; DESIGN.md
// §3.20). Part of libnmmo_heads.so.
//
// The call is the composition the library already has -- nmh_item_logits / nmh_player_logits into a
// logits row, nmh_forward on it, nmh_backward and the two *_logits_backward -- without the logits
// row: a pointer head's logits go from the candidates' own columns straight into the LDS tile that
// head_forward (heads_dev.h) reads. Every value is computed by the same device function on the same
// operands in the same order as in the composition, so the outputs are the same bits.
//
// One wave per obs row, 4 rows per workgroup (2 where four waves' LDS would pass 64 KiB), no
// workgroup barrier. LDS of a wave:
//   tile   sum(dims) floats   head k's staged logits at off[k] (forward); g_j by list position (backward)
//   pq     40 floats per pointer head, the row's projected queries
//   U      one region used by one head at a time:
//            item head    uint16 list[R]: the legal j, ascending
//            entity head  uint16 list[R], then 64 x 31 floats: the listed candidates' columns, 64 at a time
// For the nmmo heads that is 6,344 + 1,280 + 8,136 = 15,760 bytes a wave, 63,040 a workgroup.
//
// Forward, per pointer head: legal_list (heads_dev.h) fills the head's tile entries with -inf and
// lists the legal candidates; an item head then takes one listed candidate per lane (load_item,
// item_logit: item_dev.h), an entity head stages 64 listed candidates' rows and takes one per lane
// (stage_rows: set_dev.h; player_logit: player_dev.h). Candidates no head allows are never addressed.
// Backward, per pointer head: the same list; g_j = nmh_backward_kernel's expression on the recomputed
// logit, kept in LDS by list position; then lane f owns feature f of the head's query and walks the
// list in ascending order with one fmaf per candidate. No atomics: the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "heads_dev.h"
#include "heads_host.h"  // heads_fail, heads_launched, aligned16, check_head_plan
#include "item_dev.h"
#include "player_dev.h"
#include "set_dev.h"
#include "../../include/nmmo_heads.h"

using namespace nmmo;

namespace {

constexpr int kRowsPerBlock = 4;  // 2 where 4 waves' LDS would exceed kMaxLds
constexpr int kMaxLds = 64 * 1024;
constexpr int kChunk = 64;  // listed entity candidates staged at a time
constexpr int kSlot = NMH_DECODER_QUERY;
constexpr int kRowsBytes = kChunk * player_dev::kC * 4;

static_assert(kSlot >= NMH_PLAYER_QUERY && kSlot >= NMH_ITEM_QUERY && kSlot <= 64, "a lane per float of a slot");
static_assert(NMH_ITEM_MAX_ROWS < (1 << set_dev::kHeadShift), "stage_rows masks a list entry to 12 bits");
static_assert(2 * (NMH_MAX_DIM * 4 + NMH_MAX_HEADS * kSlot * 4 + NMH_PLAYER_MAX_ROWS * 2 + kRowsBytes) <= kMaxLds &&
                  2 * (NMH_MAX_DIM * 4 + NMH_MAX_HEADS * kSlot * 4 + NMH_ITEM_MAX_ROWS * 2) <= kMaxLds,
              "two waves of any accepted shape fit 64 KiB");

// what the host works out once per call from NmhHeads + NmhDecoderSets
struct DecPlan {
  int32_t n_heads, n_ptr, total;
  int32_t u_off;     // bytes from a wave's LDS base to its U region
  int32_t rows_off;  // bytes from U to the entity rows (past the largest entity list)
  int32_t dims[NMH_MAX_HEADS];
  int32_t off[NMH_MAX_HEADS];  // head k's first entry in the tile and in a mask row
  int32_t set[NMH_MAX_HEADS];  // -1: dense, else its candidate set
  int32_t src[NMH_MAX_HEADS];  // dense: its first column in a dense row; pointer: its pq slot p
  int32_t rule[NMH_MAX_SETS];
  int32_t share[NMH_MAX_SETS];
  int64_t stride[NMH_MAX_SETS];
  const void* base[NMH_MAX_SETS];
};

struct WaveLds {
  float* s;        // the tile
  float* pq;       // the row's slots
  uint16_t* list;  // U
  float* rows;     // U + rows_off
};

__device__ __forceinline__ WaveLds wave_lds(const DecPlan& pl, float* staged, int w, int wave_bytes) {
  char* base = reinterpret_cast<char*>(staged) + (size_t)w * wave_bytes;
  WaveLds m;
  m.s = reinterpret_cast<float*>(base);
  m.pq = m.s + pl.total;
  m.list = reinterpret_cast<uint16_t*>(base + pl.u_off);
  m.rows = reinterpret_cast<float*>(base + pl.u_off + pl.rows_off);
  return m;
}

// row r's candidates of set `set`, read in place
template <typename T>
__device__ __forceinline__ const T* set_of(const DecPlan& pl, int set, int64_t r) {
  return static_cast<const T*>(pl.base[set]) + (r / pl.share[set]) * pl.stride[set];
}

// SEL (heads_dev.h): kDraw samples or evaluates actions_in; kArgmax selects greedily (SPEC.md §24)
template <typename T, int MK, int SEL>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_decoder_forward_kernel(
    DecPlan pl, int n_rows, int wave_bytes, const float* __restrict__ pq, const float* __restrict__ dense, int64_t ds,
    const void* __restrict__ mask, int64_t ms, const int32_t* __restrict__ actions_in, uint32_t seed_lo,
    uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi, uint32_t row_base, int32_t* __restrict__ actions_out,
    float* __restrict__ logprob, float* __restrict__ entropy, float* __restrict__ lse,
    float* __restrict__ head_entropy) {
  extern __shared__ float staged[];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const WaveLds m = wave_lds(pl, staged, w, wave_bytes);
  float* s = m.s;
  for (int i = lane; i < pl.n_ptr * kSlot; i += 64) m.pq[i] = pq[r * pl.n_ptr * kSlot + i];
  for (int k = 0; k < pl.n_heads; k++) {
    const int n = pl.dims[k], off = pl.off[k], set = pl.set[k];
    const int64_t mbase = r * ms + off;
    if (set < 0) {  // dense: the given logit where legal
      const float* x = dense + r * ds + pl.src[k];
      for (int i = lane; i < n; i += 64) s[off + i] = legal_at<MK>(mask, mbase + i) ? x[i] : -INFINITY;
      continue;
    }
    const int R = n - 1;
    const int cnt = legal_list<MK>(mask, mbase, R, s + off, -INFINITY, m.list);
    if (lane == 0) s[off + R] = legal_at<MK>(mask, mbase + R) ? 0.f : -INFINITY;  // the no-op entry
    wave_sync();
    const float* q = m.pq + pl.src[k] * kSlot;
    const T* __restrict__ cand = set_of<T>(pl, set, r);
    if (pl.rule[set] == NMH_SET_ITEM) {
      for (int i = lane; i < cnt; i += 64) {
        const int j = m.list[i];
        s[off + j] = item_dev::item_logit(q, item_dev::load_item(cand + (int64_t)j * item_dev::kC));
      }
    } else {
      for (int i0 = 0; i0 < cnt; i0 += kChunk) {
        const int c = min(kChunk, cnt - i0);
        set_dev::stage_rows<player_dev::kC, player_dev::kC>(cand, m.list, i0, c, m.rows);
        wave_sync();
        if (lane < c) s[off + m.list[i0 + lane]] = player_dev::player_logit(q, m.rows + lane * player_dev::kC);
        wave_sync();  // the next chunk overwrites the rows
      }
    }
    wave_sync();  // the next head rebuilds the list
  }
  wave_sync();
  float lp = 0.f, ent = 0.f;
  tile_heads<SEL>(s, pl.dims, 0, pl.n_heads, pl.n_heads, r, true, actions_in, seed_lo, seed_hi, off_lo, off_hi,
                  row_base, actions_out, lse, head_entropy, lp, ent);
  if (lane == 0) {
    logprob[r] = lp;
    entropy[r] = ent;
  }
}

template <typename T, int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_decoder_backward_kernel(
    DecPlan pl, int n_rows, int wave_bytes, const float* __restrict__ pq, const float* __restrict__ dense, int64_t ds,
    const void* __restrict__ mask, int64_t ms, const int32_t* __restrict__ actions, const float* __restrict__ lse,
    const float* __restrict__ head_entropy, const float* __restrict__ g_logprob, const float* __restrict__ g_entropy,
    float* __restrict__ g_dense, int64_t gds, float* __restrict__ g_pq) {
  constexpr int kU = 8;  // item candidates in flight per lane
  extern __shared__ float staged[];
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), f = lane_id();
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  const WaveLds m = wave_lds(pl, staged, w, wave_bytes);
  float* sg = m.s;  // g_j of the head in hand, by list position
  if (g_pq)
    for (int i = f; i < pl.n_ptr * kSlot; i += 64) m.pq[i] = pq[r * pl.n_ptr * kSlot + i];
  const float glp = g_logprob ? g_logprob[r] : 0.f, gen = g_entropy ? g_entropy[r] : 0.f;
  for (int k = 0; k < pl.n_heads; k++) {
    const int n = pl.dims[k], set = pl.set[k];
    const int64_t mbase = r * ms + pl.off[k], hq = r * pl.n_heads + k;
    const int a = actions[hq];
    const float L = lse[hq], H = head_entropy[hq];
    auto grad = [&](int i, float x) {  // nmh_backward_kernel's expression
      const float logp = x - L;
      const float p = expf(logp);
      return glp * ((i == a ? 1.f : 0.f) - p) - gen * (p * (logp + H));
    };
    if (set < 0) {
      if (!g_dense) continue;
      const float* x = dense + r * ds + pl.src[k];
      float* gx = g_dense + r * gds + pl.src[k];
      for (int i = f; i < n; i += 64) {
        const bool l = legal_at<MK>(mask, mbase + i);
        const float g = grad(i, x[i]);
        gx[i] = l ? g : 0.f;
      }
      continue;
    }
    if (!g_pq) continue;
    const int R = n - 1;
    const int cnt = legal_list<MK>(mask, mbase, R, sg, 0.f, m.list);
    wave_sync();
    const float* q = m.pq + pl.src[k] * kSlot;
    const T* __restrict__ cand = set_of<T>(pl, set, r);
    float acc = 0.0f;
    if (pl.rule[set] == NMH_SET_ITEM) {
      for (int i = f; i < cnt; i += 64) {
        const int j = m.list[i];
        sg[i] = grad(j, item_dev::item_logit(q, item_dev::load_item(cand + (int64_t)j * item_dev::kC)));
      }
      wave_sync();
      if (f <= item_dev::kF) {  // lane f: feature f; f = 32: the constant
        const int col = item_dev::feature_col(min(f, item_dev::kF - 1));
        for (int i0 = 0; i0 < cnt; i0 += kU) {
          T c[kU];
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            c[u] = (T)0;
            if (i0 + u < cnt && f < item_dev::kF) c[u] = cand[(int64_t)m.list[i0 + u] * item_dev::kC + col];
          }
#pragma unroll
          for (int u = 0; u < kU; ++u)
            if (i0 + u < cnt) acc = fmaf(sg[i0 + u], f < item_dev::kF ? item_dev::item_feature(f, c[u]) : 1.0f, acc);
        }
      }
    } else {
      // the column feature f reads; the constant (f = 35) and the lanes beyond read column 0 and drop it
      const int col = f < player_dev::kF ? player_dev::feature_col(f) : 0;
      for (int i0 = 0; i0 < cnt; i0 += kChunk) {
        const int c = min(kChunk, cnt - i0);
        set_dev::stage_rows<player_dev::kC, player_dev::kC>(cand, m.list, i0, c, m.rows);
        wave_sync();
        if (f < c) sg[f] = grad(m.list[i0 + f], player_dev::player_logit(q, m.rows + f * player_dev::kC));
        wave_sync();
        if (f <= player_dev::kF) {
          for (int e = 0; e < c; ++e) {
            const float v = m.rows[e * player_dev::kC + col];
            float x = v;
            if (f >= 1 && f <= player_dev::kTypes) x = player_dev::npc_class(v) == f - 1 ? 1.0f : 0.0f;
            if (f == player_dev::kF) x = 1.0f;
            acc = fmaf(sg[e], x, acc);
          }
        }
        wave_sync();  // the next chunk overwrites the rows and sg
      }
    }
    if (f < kSlot) g_pq[(r * pl.n_ptr + pl.src[k]) * kSlot + f] = acc;  // the unused floats' lanes added nothing: 0
    wave_sync();  // the next head rebuilds the list and sg
  }
}

// The argument rules both entry points share (SPEC.md §23, "Limits"); fills the plan, *wave_bytes
// and *dense_total (the dense heads' columns).
int check_decoder(const char* fn, const NmhHeads* hd, const NmhDecoderSets* st, int32_t n_rows, const float* pq,
                  const float* dense, int64_t ds, const void* mask, int64_t ms, int32_t mask_kind, DecPlan* pl,
                  int* wave_bytes, int64_t* dense_total) {
  if (!hd) return heads_fail(NMH_E_INVALID, "%s: hd is NULL", fn);
  if (!st) return heads_fail(NMH_E_INVALID, "%s: sets is NULL", fn);
  if (hd->n_heads < 1 || hd->n_heads > NMH_MAX_HEADS)
    return heads_fail(NMH_E_INVALID, "%s: n_heads %d outside 1..%d", fn, hd->n_heads, NMH_MAX_HEADS);
  if (st->n_sets < 0 || st->n_sets > NMH_MAX_SETS)
    return heads_fail(NMH_E_INVALID, "%s: n_sets %d outside 0..%d", fn, st->n_sets, NMH_MAX_SETS);
  if (st->elem_kind != NMH_ELEM_F32 && st->elem_kind != NMH_ELEM_I16)
    return heads_fail(NMH_E_INVALID, "%s: unknown elem_kind %d", fn, st->elem_kind);
  *pl = DecPlan{};
  int max_item = 0, max_ent = 0;
  for (int s = 0; s < st->n_sets; s++) {
    const int rule = st->rule[s], R = st->set_rows[s];
    if (rule != NMH_SET_ENTITY && rule != NMH_SET_ITEM)
      return heads_fail(NMH_E_INVALID, "%s: unknown rule[%d] %d", fn, s, rule);
    const int cols = rule == NMH_SET_ITEM ? NMH_ITEM_COLS : NMH_PLAYER_COLS;
    const int max_rows = rule == NMH_SET_ITEM ? NMH_ITEM_MAX_ROWS : NMH_PLAYER_MAX_ROWS;
    if (R < 1 || R > max_rows)
      return heads_fail(NMH_E_INVALID, "%s: set_rows[%d] = %d outside 1..%d", fn, s, R, max_rows);
    if (st->share[s] < 1) return heads_fail(NMH_E_INVALID, "%s: share[%d] %d < 1", fn, s, st->share[s]);
    if (st->stride[s] < (int64_t)cols * R)
      return heads_fail(NMH_E_INVALID, "%s: stride[%d] %lld < %d set_rows = %d", fn, s, (long long)st->stride[s], cols,
                        cols * R);
    if (!st->base[s]) return heads_fail(NMH_E_INVALID, "%s: base[%d] is NULL", fn, s);
    if (rule == NMH_SET_ITEM) max_item = std::max(max_item, R);
    else max_ent = std::max(max_ent, R);
    pl->rule[s] = rule;
    pl->share[s] = st->share[s];
    pl->stride[s] = st->stride[s];
    pl->base[s] = st->base[s];
  }
  int64_t sum;
  const int rc = check_head_plan(fn, hd, st->n_sets, st->set_rows, st->head_set, "set", n_rows, dense, ds, mask, ms,
                                 mask_kind, {&pl->n_heads, &pl->n_ptr, pl->dims, pl->off, pl->set, pl->src}, &sum,
                                 dense_total);
  if (rc != NMH_OK) return rc;
  if (pl->n_ptr > 0) {
    if (!pq) return heads_fail(NMH_E_INVALID, "%s: pq is NULL with pointer heads", fn);
    if (!aligned16(pq)) return heads_fail(NMH_E_INVALID, "%s: pq is not 16-byte aligned", fn);
  }
  pl->total = (int32_t)sum;
  pl->u_off = (int32_t)(sum * 4 + pl->n_ptr * kSlot * 4);
  pl->rows_off = (max_ent * 2 + 3) & ~3;
  const int u_bytes = std::max(max_item * 2, max_ent ? pl->rows_off + kRowsBytes : 0);
  *wave_bytes = (pl->u_off + u_bytes + 15) & ~15;
  return NMH_OK;
}

// launches K(element type, mask kind), one of the two kernel names below, on n_rows rows: 4 waves a
// workgroup where their LDS fits 64 KiB, else 2
#define DEC_LAUNCH(K, ...)                                                                              \
  do {                                                                                                  \
    const int rpb = kRowsPerBlock * wave_bytes <= kMaxLds ? kRowsPerBlock : 2;                          \
    const dim3 grid((unsigned)((n_rows + rpb - 1) / rpb)), block(64 * rpb);                             \
    hipStream_t hs = static_cast<hipStream_t>(stream);                                                  \
    const bool mf = mask_kind == NMH_MASK_F32;                                                          \
    auto* kern = st->elem_kind == NMH_ELEM_F32 ? (mf ? K(float, NMH_MASK_F32) : K(float, NMH_MASK_U8))   \
                                               : (mf ? K(int16_t, NMH_MASK_F32) : K(int16_t, NMH_MASK_U8)); \
    hipLaunchKernelGGL(kern, grid, block, (size_t)rpb* wave_bytes, hs, pl, n_rows, wave_bytes, __VA_ARGS__); \
  } while (0)
#define DEC_FWD(T, MK) nmh_decoder_forward_kernel<T, MK, SEL>  // where a template's SEL is in scope
#define DEC_BWD(T, MK) nmh_decoder_backward_kernel<T, MK>

// nmh_decoder_forward (SEL = kDraw) and nmh_decoder_forward_argmax (kArgmax: no actions, no counter)
template <int SEL>
int decoder_forward(const char* fn, const NmhHeads* hd, const NmhDecoderSets* st, int32_t n_rows, const float* pq,
                    const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride, int32_t mask_kind,
                    const int32_t* actions_in, uint64_t seed, uint64_t offset, uint32_t row_base, int32_t* actions_out,
                    float* logprob, float* entropy, float* lse, float* head_entropy, void* stream) {
  DecPlan pl;
  int wave_bytes;
  int64_t dense_total;
  const int rc = check_decoder(fn, hd, st, n_rows, pq, dense, dense_stride, mask, mask_stride, mask_kind, &pl,
                               &wave_bytes, &dense_total);
  if (rc != NMH_OK) return rc;
  if (!actions_out || !logprob || !entropy || !lse || !head_entropy)
    return heads_fail(NMH_E_INVALID, "%s: an output pointer is NULL", fn);
  if (n_rows == 0) return NMH_OK;
  DEC_LAUNCH(DEC_FWD, pq, dense, dense_stride, mask, mask_stride, actions_in, (uint32_t)seed, (uint32_t)(seed >> 32),
             (uint32_t)offset, (uint32_t)(offset >> 32), row_base, actions_out, logprob, entropy, lse, head_entropy);
  return heads_launched(fn);
}

}  // namespace

extern "C" {

int nmh_decoder_forward(const NmhHeads* hd, const NmhDecoderSets* st, int32_t n_rows, const float* pq,
                        const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride,
                        int32_t mask_kind, const int32_t* actions_in, uint64_t seed, uint64_t offset,
                        uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy, float* lse,
                        float* head_entropy, void* stream) {
  return decoder_forward<kDraw>("nmh_decoder_forward", hd, st, n_rows, pq, dense, dense_stride, mask, mask_stride,
                                mask_kind, actions_in, seed, offset, row_base, actions_out, logprob, entropy, lse,
                                head_entropy, stream);
}

int nmh_decoder_forward_argmax(const NmhHeads* hd, const NmhDecoderSets* st, int32_t n_rows, const float* pq,
                               const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride,
                               int32_t mask_kind, int32_t* actions_out, float* logprob, float* entropy, float* lse,
                               float* head_entropy, void* stream) {
  return decoder_forward<kArgmax>("nmh_decoder_forward_argmax", hd, st, n_rows, pq, dense, dense_stride, mask,
                                  mask_stride, mask_kind, nullptr, 0, 0, 0, actions_out, logprob, entropy, lse,
                                  head_entropy, stream);
}

int nmh_decoder_backward(const NmhHeads* hd, const NmhDecoderSets* st, int32_t n_rows, const float* pq,
                         const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride,
                         int32_t mask_kind, const int32_t* actions, const float* lse, const float* head_entropy,
                         const float* g_logprob, const float* g_entropy, float* g_dense, int64_t g_dense_stride,
                         float* g_pq, void* stream) {
  const char* fn = "nmh_decoder_backward";
  DecPlan pl;
  int wave_bytes;
  int64_t dense_total;
  const int rc = check_decoder(fn, hd, st, n_rows, pq, dense, dense_stride, mask, mask_stride, mask_kind, &pl,
                               &wave_bytes, &dense_total);
  if (rc != NMH_OK) return rc;
  if (!actions || !lse || !head_entropy)
    return heads_fail(NMH_E_INVALID, "%s: actions, lse or head_entropy is NULL", fn);
  if (g_dense && g_dense_stride < dense_total)
    return heads_fail(NMH_E_INVALID, "%s: g_dense_stride %lld < the dense heads' %lld columns", fn,
                      (long long)g_dense_stride, (long long)dense_total);
  if (g_pq && !aligned16(g_pq)) return heads_fail(NMH_E_INVALID, "%s: g_pq is not 16-byte aligned", fn);
  if (dense_total == 0) g_dense = nullptr;
  if (pl.n_ptr == 0) g_pq = nullptr;
  if (n_rows == 0 || (!g_dense && !g_pq)) return NMH_OK;
  DEC_LAUNCH(DEC_BWD, pq, dense, dense_stride, mask, mask_stride, actions, lse, head_entropy,
             g_logprob, g_entropy, g_dense, g_dense_stride, g_pq);
  return heads_launched(fn);
}

}  // extern "C"
