// heads_host.h — the host code that the translation units of libnmmo_heads.so share (heads.hip,
// tile_enc.hip, item_enc.hip, player_enc.hip, embed_enc.hip, decoder.hip): the library's one error text, the
// launch-error and alignment helpers, the argument rules of "heads over a candidate set"
// (nmh_item_logits / nmh_player_logits / nmh_embed_logits and their backwards) and the head plan of the calls that mix
// dense and pointer heads (nmh_pointer_*, nmh_decoder_*). Host only; no kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmmo_heads.h"

// Records the message nmh_last_error() returns and returns `code`: `return heads_fail(E, "...", ...)`.
// Defined in heads.hip next to the one error text. Hidden visibility: not an export.
int heads_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// after a launch: NMH_OK, or NMH_E_HIP with the runtime's error text (heads.hip)
int heads_launched(const char* fn);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------- heads over a candidate set
static_assert(NMH_ITEM_F32 == NMH_ELEM_F32 && NMH_PLAYER_F32 == NMH_ELEM_F32 && NMH_ITEM_I16 == NMH_ELEM_I16 &&
                  NMH_PLAYER_I16 == NMH_ELEM_I16,
              "one pair of element kinds");

// a kind of candidate set: its shape, and what its entry points call their arguments
struct SetKind {
  int cols, max_rows;
  const char *set, *stride, *kind, *heads;
};
constexpr SetKind kItemSets = {NMH_ITEM_COLS, NMH_ITEM_MAX_ROWS, "items", "item_stride", "item_kind", "ih"};
constexpr SetKind kEntitySets = {NMH_PLAYER_COLS, NMH_PLAYER_MAX_ROWS, "ents", "ent_stride", "ent_kind", "ph"};

inline int check_set(const char* fn, const SetKind& k, const void* set, int64_t stride, int32_t elem_kind,
                     int32_t set_rows) {
  if (!set) return heads_fail(NMH_E_INVALID, "%s: %s is NULL", fn, k.set);
  if (elem_kind != NMH_ELEM_F32 && elem_kind != NMH_ELEM_I16)
    return heads_fail(NMH_E_INVALID, "%s: unknown %s %d", fn, k.kind, elem_kind);
  if (set_rows < 1 || set_rows > k.max_rows)
    return heads_fail(NMH_E_INVALID, "%s: set_rows %d outside 1..%d", fn, set_rows, k.max_rows);
  if (stride < (int64_t)k.cols * set_rows)
    return heads_fail(NMH_E_INVALID, "%s: %s %lld < %d set_rows = %d", fn, k.stride, (long long)stride, k.cols,
                      k.cols * set_rows);
  return NMH_OK;
}

// the rows' ids of a features call that asks for the own row; `mine` names the outputs that need them
inline int check_ids(const char* fn, const void* ids, int64_t id_stride, int32_t id_kind, const char* mine) {
  if (!ids) return heads_fail(NMH_E_INVALID, "%s: ids is NULL but %s not", fn, mine);
  if (id_kind != NMH_ELEM_F32 && id_kind != NMH_ELEM_I16)
    return heads_fail(NMH_E_INVALID, "%s: unknown id_kind %d", fn, id_kind);
  if (id_stride < 1) return heads_fail(NMH_E_INVALID, "%s: id_stride %lld < 1", fn, (long long)id_stride);
  return NMH_OK;
}

// the rules a *_logits entry point and its backward share; `out` names the [n_rows, out_stride]
// argument. Entity sets are not shared between rows: their entry points pass share = 1.
inline int check_logits(const char* fn, const SetKind& k, const NmhSetHeads* sh, int32_t n_rows, const void* set,
                        int64_t stride, int32_t elem_kind, int32_t set_rows, int32_t share, const void* mask,
                        int64_t mask_stride, int32_t mask_kind, const char* out_name, const void* out,
                        const char* stride_name, int64_t out_stride) {
  if (!sh) return heads_fail(NMH_E_INVALID, "%s: %s is NULL", fn, k.heads);
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "%s: n_rows %d is negative", fn, n_rows);
  if (sh->n_heads < 1 || sh->n_heads > NMH_ITEM_MAX_HEADS)
    return heads_fail(NMH_E_INVALID, "%s: n_heads %d outside 1..%d", fn, sh->n_heads, NMH_ITEM_MAX_HEADS);
  const int rc = check_set(fn, k, set, stride, elem_kind, set_rows);
  if (rc != NMH_OK) return rc;
  if (share < 1) return heads_fail(NMH_E_INVALID, "%s: share %d < 1", fn, share);
  if (!mask) return heads_fail(NMH_E_INVALID, "%s: mask is NULL", fn);
  if (mask_kind != NMH_MASK_F32 && mask_kind != NMH_MASK_U8)
    return heads_fail(NMH_E_INVALID, "%s: unknown mask_kind %d", fn, mask_kind);
  if (!out) return heads_fail(NMH_E_INVALID, "%s: %s is NULL", fn, out_name);
  for (int h = 0; h < sh->n_heads; ++h) {
    if (sh->mask_off[h] < 0 || sh->out_off[h] < 0)
      return heads_fail(NMH_E_INVALID, "%s: mask_off[%d] %d or out_off[%d] %d is negative", fn, h, sh->mask_off[h], h,
                        sh->out_off[h]);
    if (mask_stride < (int64_t)sh->mask_off[h] + set_rows + 1)
      return heads_fail(NMH_E_INVALID, "%s: mask_stride %lld < mask_off[%d] + set_rows + 1 = %lld", fn,
                        (long long)mask_stride, h, (long long)sh->mask_off[h] + set_rows + 1);
    if (out_stride < (int64_t)sh->out_off[h] + set_rows + 1)
      return heads_fail(NMH_E_INVALID, "%s: %s %lld < out_off[%d] + set_rows + 1 = %lld", fn, stride_name,
                        (long long)out_stride, h, (long long)sh->out_off[h] + set_rows + 1);
  }
  return NMH_OK;
}

// every rule of a *_logits entry point: check_logits on out / out_stride, then the projected queries
inline int check_forward(const char* fn, const SetKind& k, const NmhSetHeads* sh, int32_t n_rows, const void* set,
                         int64_t stride, int32_t elem_kind, int32_t set_rows, int32_t share, const void* mask,
                         int64_t mask_stride, int32_t mask_kind, const float* pq, const float* out,
                         int64_t out_stride) {
  const int rc = check_logits(fn, k, sh, n_rows, set, stride, elem_kind, set_rows, share, mask, mask_stride, mask_kind,
                              "out", out, "out_stride", out_stride);
  if (rc != NMH_OK) return rc;
  if (!pq) return heads_fail(NMH_E_INVALID, "%s: pq is NULL", fn);
  if (!aligned16(pq)) return heads_fail(NMH_E_INVALID, "%s: pq is not 16-byte aligned", fn);
  return NMH_OK;
}

// every rule of a *_logits_backward entry point: check_logits on g_out / g_stride, then g_pq
inline int check_backward(const char* fn, const SetKind& k, const NmhSetHeads* sh, int32_t n_rows, const void* set,
                          int64_t stride, int32_t elem_kind, int32_t set_rows, int32_t share, const void* mask,
                          int64_t mask_stride, int32_t mask_kind, const float* g_out, int64_t g_stride,
                          const float* g_pq) {
  const int rc = check_logits(fn, k, sh, n_rows, set, stride, elem_kind, set_rows, share, mask, mask_stride, mask_kind,
                              "g_out", g_out, "g_stride", g_stride);
  if (rc != NMH_OK) return rc;
  if (!g_pq) return heads_fail(NMH_E_INVALID, "%s: g_pq is NULL", fn);
  return NMH_OK;
}

// launches K<element type, mask kind>(*sh, n_rows, set as const element*, ...) with one wave per row,
// rows_per_block waves a workgroup
#define HEADS_SET_LAUNCH(K, elem_kind, mask_kind, rows_per_block, stream, sh, n_rows, set, ...)                   \
  do {                                                                                                            \
    const dim3 grid((unsigned)(((n_rows) + (rows_per_block)-1) / (rows_per_block))), block(64 * (rows_per_block)); \
    hipStream_t st = static_cast<hipStream_t>(stream);                                                            \
    const bool mf = (mask_kind) == NMH_MASK_F32;                                                                  \
    if ((elem_kind) == NMH_ELEM_F32) {                                                                            \
      auto* kern = mf ? K<float, NMH_MASK_F32> : K<float, NMH_MASK_U8>;                                           \
      hipLaunchKernelGGL(kern, grid, block, 0, st, *(sh), n_rows, static_cast<const float*>(set), __VA_ARGS__);   \
    } else {                                                                                                      \
      auto* kern = mf ? K<int16_t, NMH_MASK_F32> : K<int16_t, NMH_MASK_U8>;                                       \
      hipLaunchKernelGGL(kern, grid, block, 0, st, *(sh), n_rows, static_cast<const int16_t*>(set), __VA_ARGS__); \
    }                                                                                                             \
  } while (0)

// ---------------------------------------------------------------- the head plan
// where a caller's plan (heads.hip PtrPlan, decoder.hip DecPlan) keeps what check_head_plan fills
struct HeadPlan {
  int32_t *n_heads, *n_ptr;  // n_ptr: the pointer heads, counted from the caller's 0
  int32_t *dims, *off, *set, *src;
};

// The rules the calls with dense and pointer heads share, once hd, n_heads and the sets themselves
// are known to be sound: per head its size, its set (head_set[k], -1 = dense) and dims[k] ==
// set_rows + 1; sum(dims); every set used (`set_noun` is what the caller's messages call a set); then
// n_rows, the mask and the dense logits. Fills the plan, *total = sum(dims) and *dense_total = the
// dense heads' columns.
inline int check_head_plan(const char* fn, const NmhHeads* hd, int32_t n_sets, const int32_t* set_rows,
                           const int32_t* head_set, const char* set_noun, int32_t n_rows, const float* dense,
                           int64_t ds, const void* mask, int64_t ms, int32_t mask_kind, const HeadPlan& pl,
                           int64_t* total, int64_t* dense_total) {
  *pl.n_heads = hd->n_heads;
  int64_t sum = 0, dsum = 0;
  unsigned used = 0;
  for (int k = 0; k < hd->n_heads; k++) {
    const int n = hd->dims[k], s = head_set[k];
    if (n < 1 || n > NMH_MAX_DIM)
      return heads_fail(NMH_E_INVALID, "%s: dims[%d] = %d outside 1..%d", fn, k, n, NMH_MAX_DIM);
    if (s < -1 || s >= n_sets)
      return heads_fail(NMH_E_INVALID, "%s: head_set[%d] = %d outside -1..%d", fn, k, s, n_sets - 1);
    if (s >= 0 && n != set_rows[s] + 1)
      return heads_fail(NMH_E_INVALID, "%s: dims[%d] = %d is not set_rows[%d] + 1 = %d", fn, k, n, s, set_rows[s] + 1);
    pl.dims[k] = n;
    pl.off[k] = (int32_t)sum;
    pl.set[k] = s;
    if (s < 0) {
      pl.src[k] = (int32_t)dsum;
      dsum += n;
    } else {
      pl.src[k] = (*pl.n_ptr)++;
      used |= 1u << s;
    }
    sum += n;
  }
  if (sum > NMH_MAX_DIM)
    return heads_fail(NMH_E_INVALID, "%s: sum(dims) %lld exceeds NMH_MAX_DIM %d", fn, (long long)sum, NMH_MAX_DIM);
  for (int s = 0; s < n_sets; s++)
    if (!(used >> s & 1u)) return heads_fail(NMH_E_INVALID, "%s: no head uses %s %d (head_set)", fn, set_noun, s);
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "%s: n_rows %d is negative", fn, n_rows);
  if (!mask) return heads_fail(NMH_E_INVALID, "%s: mask is NULL", fn);
  if (mask_kind != NMH_MASK_F32 && mask_kind != NMH_MASK_U8)
    return heads_fail(NMH_E_INVALID, "%s: unknown mask_kind %d", fn, mask_kind);
  if (ms < sum)
    return heads_fail(NMH_E_INVALID, "%s: mask_stride %lld < sum(dims) %lld", fn, (long long)ms, (long long)sum);
  if (dsum > 0 && !dense) return heads_fail(NMH_E_INVALID, "%s: dense is NULL with dense heads", fn);
  if (dsum > 0 && ds < dsum)
    return heads_fail(NMH_E_INVALID, "%s: dense_stride %lld < the dense heads' %lld columns", fn, (long long)ds,
                      (long long)dsum);
  *total = sum;
  *dense_total = dsum;
  return NMH_OK;
}
