// heads.hip — libnmmo_heads.so (include/nmmo_heads.h): the masked multi-head categorical that
// ends every reference policy (baseline_policy.py:245-262), fused. SPEC.md §15 holds the
// semantics; DESIGN.md §3.12 the kernel notes. The pointer-head kernels further down (SPEC.md §18,
// DESIGN.md §3.15) also compute the logits, query . key, of the heads that choose a candidate.
//
// Forward: one wave per row, 4 rows per 256-thread workgroup. The wave first stages its row in
// LDS with coalesced dword loads -- logits[i] where the mask allows entry i, -inf elsewhere, as
// many whole heads as fit a tile (all 12 nmmo heads: 1,586 floats) -- so a row costs one round
// of global loads instead of one or two per head; a first version that read each head straight
// into registers was bound by those round trips. Per head each lane then owns a
// contiguous chunk of the tile, so the inclusive sums of exp(x - max) are ordered across lanes:
// the sample is a wave scan of per-lane partial sums, a ballot for the first lane past u * S,
// and that lane's serial walk over its chunk. Logits and mask are read from HBM exactly once.
// Backward is elementwise given the saved lse and head entropy: lanes stride each head, so loads
// and stores are coalesced dwords (rows are not 16-byte aligned: the flat obs row stride is
// 23,987 floats, a logits row 1,586).
#include <math.h>

#include <algorithm>

#include "common.h"
#include "heads_dev.h"  // head_forward, tile_heads, legal_list, wave_sync: shared with decoder.hip
#include "heads_host.h"
#include "host_api.h"  // g_err and fail(): the library's one error text lives in this translation unit
#include "../../include/nmmo_heads.h"

using namespace nmmo;

namespace {

constexpr int kRowsPerBlock = 4;
constexpr int kStage = 16;  // staging loads in flight per lane and kind

// tile: floats of LDS per wave = min(sum(dims), NMH_MAX_DIM), so any one head fits. SEL (heads_dev.h):
// kDraw samples or evaluates actions_in; kArgmax selects greedily and ignores actions_in .. row_base.
template <int MK, int SEL>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_forward_kernel(
    NmhHeads hd, int n_rows, int tile, const float* __restrict__ logits, int64_t ls, const void* __restrict__ mask,
    int64_t ms, const int32_t* __restrict__ actions_in, uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo,
    uint32_t off_hi, uint32_t row_base, int32_t* __restrict__ actions_out, float* __restrict__ logprob,
    float* __restrict__ entropy, float* __restrict__ lse, float* __restrict__ head_entropy) {
  extern __shared__ float staged[];
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  float* s = staged + w * tile;
  // every wave runs to the end (the tiles are separated by workgroup barriers): a wave past the
  // last row recomputes that row and stores nothing
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock + w;
  const bool live = r0 < n_rows;
  const int64_t r = live ? r0 : n_rows - 1;
  const float* xrow = logits + r * ls;
  float lp = 0.f, ent = 0.f;
  int k0 = 0, off = 0;
  while (k0 < hd.n_heads) {
    // heads [k0, k1): as many whole heads as fit the tile
    int k1 = k0, len = 0;
    while (k1 < hd.n_heads && len + hd.dims[k1] <= tile) len += hd.dims[k1++];
    __syncthreads();  // the previous tile has been read
    // kStage unconditional loads of each kind in flight per lane (a lane past the end re-reads
    // the last entry): left to itself the loop is one mask load, a branch, one logits load
    for (int i0 = lane_id(); i0 < len; i0 += 64 * kStage) {
      float xv[kStage];
      bool lg[kStage];
#pragma unroll
      for (int j = 0; j < kStage; j++) {
        const int i = min(i0 + 64 * j, len - 1);
        xv[j] = xrow[off + i];
        lg[j] = legal_at<MK>(mask, r * ms + off + i);
      }
#pragma unroll
      for (int j = 0; j < kStage; j++) {
        const int i = i0 + 64 * j;
        if (i < len) s[i] = lg[j] ? xv[j] : -INFINITY;
      }
    }
    __syncthreads();
    tile_heads<SEL>(s, hd.dims, k0, k1, hd.n_heads, r, live, actions_in, seed_lo, seed_hi, off_lo, off_hi,
                    row_base, actions_out, lse, head_entropy, lp, ent);
    off += len;
    k0 = k1;
  }
  if (live && lane_id() == 0) {
    logprob[r] = lp;
    entropy[r] = ent;
  }
}

// g_i = g_logprob (1[i = a] - p_i) - g_entropy p_i (log p_i + H) on the legal set, 0 elsewhere;
// p_i = exp(x_i - lse). An empty head has no legal entry, so it is all zeros.
template <int MK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_backward_kernel(
    NmhHeads hd, int n_rows, const float* __restrict__ logits, int64_t ls, const void* __restrict__ mask, int64_t ms,
    const int32_t* __restrict__ actions, const float* __restrict__ lse, const float* __restrict__ head_entropy,
    const float* __restrict__ g_logprob, const float* __restrict__ g_entropy, float* __restrict__ g_logits,
    int64_t gs) {
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + __builtin_amdgcn_readfirstlane(wave_id());
  if (r >= n_rows) return;
  const float* xrow = logits + r * ls;
  float* grow = g_logits + r * gs;
  const float glp = g_logprob ? g_logprob[r] : 0.f, gen = g_entropy ? g_entropy[r] : 0.f;
  int off = 0;
  for (int k = 0; k < hd.n_heads; k++) {
    const int n = hd.dims[k];
    const int64_t q = r * hd.n_heads + k;
    const int a = actions[q];
    const float L = lse[q], H = head_entropy[q];
    for (int i = lane_id(); i < n; i += 64) {
      const bool l = legal_at<MK>(mask, r * ms + off + i);
      const float logp = xrow[off + i] - L;
      const float p = expf(logp);
      const float g = glp * ((i == a ? 1.f : 0.f) - p) - gen * (p * (logp + H));
      grow[off + i] = l ? g : 0.f;
    }
    off += n;
  }
}

// ---------------------------------------------------------------- pointer heads (SPEC.md §18)
// The same wave-per-row kernels with one more way to fill the tile: a pointer head's logits are
// dot products of the row's query with the row's candidate keys. The wave reads the head's mask
// first and compacts the legal candidates' indices into a list in LDS (ballot + rank), then walks
// the list, one candidate per 16-lane row and 16 bytes of a key row per lane, so the key rows of
// illegal candidates are never touched and a head costs what its legal entries cost. The tile then
// holds what nmh_forward_kernel would have staged from materialised logits, and head_forward runs
// on it unchanged. DESIGN.md §3.15.

// what the host works out once per call from NmhHeads + NmhPointer
struct PtrPlan {
  int32_t n_heads, n_sets, n_ptr, key_dim;
  int32_t dims[NMH_MAX_HEADS];
  int32_t off[NMH_MAX_HEADS];  // head k's first entry in the tile and in a mask row
  int32_t set[NMH_MAX_HEADS];  // -1: dense, else its key set
  int32_t src[NMH_MAX_HEADS];  // dense: its first column in a dense row; pointer: its query's index p
  int32_t set_rows[NMH_MAX_SETS];
  const float* keys[NMH_MAX_SETS];
};
struct KeyGrads {
  float* p[NMH_MAX_SETS];
};

// LDS of one wave: the tile of `total` floats, then the index list of `max_rows` uint16
__host__ __device__ inline int wave_lds_bytes(int total, int max_rows) { return (total * 4 + max_rows * 2 + 15) & ~15; }

// sum over each 16-lane row, in every lane of it: four row_ror steps (all lanes active)
__device__ __forceinline__ float row16_sum(float x) {
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, false));  // row_ror:8
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, false));  // row_ror:4
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x122, 0xF, 0xF, false));  // row_ror:2
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x121, 0xF, 0xF, false));  // row_ror:1
  return x;
}

// the query of one pointer head: lane l of every 16-lane row holds floats [4 (l + 16 c), + 4)
template <int NC>
__device__ __forceinline__ void load_query(const float* __restrict__ q, int D, float4 (&out)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const int d4 = (lane_id() & 15) + 16 * c;
    out[c] = 4 * d4 < D ? reinterpret_cast<const float4*>(q)[d4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// Walks the listed candidates of one head: 16-lane row g of the wave takes list[i0 + 4 u + g], each
// lane loads 16 B of that key row per 64-float chunk (NC chunks cover D), kU candidates per row in
// flight. f(j, x_j, the lane's piece of key row j) runs in all 16 lanes of the row that took j.
template <int NC, class Fn>
__device__ __forceinline__ void for_listed_keys(const uint16_t* list, int cnt, const float* __restrict__ krow, int D,
                                                const float4 (&q)[NC], Fn&& f) {
  constexpr int kU = NC == 1 ? 4 : 2;
  const int g = lane_id() >> 4, l = lane_id() & 15, nd4 = D >> 2;
  const float4* k4 = reinterpret_cast<const float4*>(krow);
  for (int i0 = 0; i0 < cnt; i0 += 4 * kU) {
    int j[kU];
    float4 kv[kU][NC];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const int i = i0 + 4 * u + g;
      j[u] = i < cnt ? (int)list[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < kU; u++) {
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const int d4 = l + 16 * c;
        kv[u][c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j[u] >= 0 && d4 < nd4) kv[u][c] = k4[(int64_t)j[u] * nd4 + d4];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; u++) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NC; c++) {
        acc = fmaf(kv[u][c].x, q[c].x, acc);
        acc = fmaf(kv[u][c].y, q[c].y, acc);
        acc = fmaf(kv[u][c].z, q[c].z, acc);
        acc = fmaf(kv[u][c].w, q[c].w, acc);
      }
      const float x = row16_sum(acc);
      if (j[u] >= 0) f(j[u], x, kv[u]);
    }
  }
}

template <int MK, int NC, int SEL>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_pointer_forward_kernel(
    PtrPlan pl, int n_rows, int total, int wave_bytes, const float* __restrict__ queries,
    const float* __restrict__ dense, int64_t ds, const void* __restrict__ mask, int64_t ms,
    const int32_t* __restrict__ actions_in, uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi,
    uint32_t row_base, int32_t* __restrict__ actions_out, float* __restrict__ logprob, float* __restrict__ entropy,
    float* __restrict__ lse, float* __restrict__ head_entropy) {
  extern __shared__ float staged[];
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;  // (waves share nothing: no workgroup barrier below)
  float* s = reinterpret_cast<float*>(reinterpret_cast<char*>(staged) + (size_t)w * wave_bytes);
  uint16_t* list = reinterpret_cast<uint16_t*>(s + total);
  const int D = pl.key_dim;
  for (int k = 0; k < pl.n_heads; k++) {
    const int n = pl.dims[k], off = pl.off[k], set = pl.set[k];
    const int64_t mbase = r * ms + off;
    if (set < 0) {  // dense: the given logit where legal
      const float* x = dense + r * ds + pl.src[k];
      for (int i = lane_id(); i < n; i += 64) s[off + i] = legal_at<MK>(mask, mbase + i) ? x[i] : -INFINITY;
      continue;
    }
    const int m = n - 1;
    const int cnt = legal_list<MK>(mask, mbase, m, s + off, -INFINITY, list);
    if (lane_id() == 0) s[off + m] = legal_at<MK>(mask, mbase + m) ? 0.f : -INFINITY;  // the no-op entry
    wave_sync();
    float4 q[NC];
    load_query<NC>(queries + (r * pl.n_ptr + pl.src[k]) * D, D, q);
    for_listed_keys<NC>(list, cnt, pl.keys[set] + r * m * D, D, q, [&](int j, float x, const float4(&)[NC]) {
      if ((lane_id() & 15) == 0) s[off + j] = x;
    });
    wave_sync();  // the next head rebuilds the list
  }
  wave_sync();
  float lp = 0.f, ent = 0.f;
  tile_heads<SEL>(s, pl.dims, 0, pl.n_heads, pl.n_heads, r, true, actions_in, seed_lo, seed_hi, off_lo, off_hi,
                  row_base, actions_out, lse, head_entropy, lp, ent);
  if (lane_id() == 0) {
    logprob[r] = lp;
    entropy[r] = ent;
  }
}

// Pass 1, per head: g_j as in nmh_backward_kernel. A dense head's goes straight to g_dense. A pointer
// head recomputes x_j from the key row it has just loaded, keeps g_j in the tile (0 off the legal
// set) and adds g_j K_j to the query's gradient from the same registers. Pass 2, per key set: every
// gK row, the sum over the set's heads in head order of g_j Q, as float4 stores along D.
template <int MK, int NC>
__global__ __launch_bounds__(64 * kRowsPerBlock) void nmh_pointer_backward_kernel(
    PtrPlan pl, int n_rows, int total, int wave_bytes, const float* __restrict__ queries,
    const float* __restrict__ dense, int64_t ds, const void* __restrict__ mask, int64_t ms,
    const int32_t* __restrict__ actions, const float* __restrict__ lse, const float* __restrict__ head_entropy,
    const float* __restrict__ g_logprob, const float* __restrict__ g_entropy, float* __restrict__ g_dense, int64_t gds,
    float* __restrict__ g_queries, KeyGrads gk) {
  extern __shared__ float staged[];
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + w;
  if (r >= n_rows) return;
  float* s = reinterpret_cast<float*>(reinterpret_cast<char*>(staged) + (size_t)w * wave_bytes);
  uint16_t* list = reinterpret_cast<uint16_t*>(s + total);
  const int D = pl.key_dim, nd4 = D >> 2;
  const float glp = g_logprob ? g_logprob[r] : 0.f, gen = g_entropy ? g_entropy[r] : 0.f;
  for (int k = 0; k < pl.n_heads; k++) {
    const int n = pl.dims[k], off = pl.off[k], set = pl.set[k];
    const int64_t mbase = r * ms + off, hq = r * pl.n_heads + k;
    const int a = actions[hq];
    const float L = lse[hq], H = head_entropy[hq];
    auto grad = [&](int i, float x) {
      const float logp = x - L;
      const float p = expf(logp);
      return glp * ((i == a ? 1.f : 0.f) - p) - gen * (p * (logp + H));
    };
    if (set < 0) {
      if (!g_dense) continue;
      const float* x = dense + r * ds + pl.src[k];
      float* gx = g_dense + r * gds + pl.src[k];
      for (int i = lane_id(); i < n; i += 64) {
        const bool l = legal_at<MK>(mask, mbase + i);
        const float g = grad(i, x[i]);
        gx[i] = l ? g : 0.f;
      }
      continue;
    }
    if (!g_queries && !gk.p[set]) continue;
    const int m = n - 1;
    const int cnt = legal_list<MK>(mask, mbase, m, s + off, 0.f, list);
    wave_sync();
    float4 q[NC], gq[NC];
    load_query<NC>(queries + (r * pl.n_ptr + pl.src[k]) * D, D, q);
#pragma unroll
    for (int c = 0; c < NC; c++) gq[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    for_listed_keys<NC>(list, cnt, pl.keys[set] + r * m * D, D, q, [&](int j, float x, const float4(&kv)[NC]) {
      const float g = grad(j, x);
      if ((lane_id() & 15) == 0) s[off + j] = g;
#pragma unroll
      for (int c = 0; c < NC; c++) {
        gq[c].x = fmaf(g, kv[c].x, gq[c].x);
        gq[c].y = fmaf(g, kv[c].y, gq[c].y);
        gq[c].z = fmaf(g, kv[c].z, gq[c].z);
        gq[c].w = fmaf(g, kv[c].w, gq[c].w);
      }
    });
    if (g_queries) {  // the four 16-lane rows' partial sums, in a fixed order
      float4* out = reinterpret_cast<float4*>(g_queries + (r * pl.n_ptr + pl.src[k]) * D);
#pragma unroll
      for (int c = 0; c < NC; c++) {
        float4 v = gq[c];
        v.x += __shfl_xor(v.x, 16), v.y += __shfl_xor(v.y, 16), v.z += __shfl_xor(v.z, 16), v.w += __shfl_xor(v.w, 16);
        v.x += __shfl_xor(v.x, 32), v.y += __shfl_xor(v.y, 32), v.z += __shfl_xor(v.z, 32), v.w += __shfl_xor(v.w, 32);
        const int d4 = lane_id() + 16 * c;
        if (lane_id() < 16 && d4 < nd4) out[d4] = v;
      }
    }
    wave_sync();
  }
  for (int set = 0; set < pl.n_sets; set++) {
    if (!gk.p[set]) continue;
    const int n4 = pl.set_rows[set] * nd4;  // float4s of this row's gK: <= 2047 * 64
    float4* out = reinterpret_cast<float4*>(gk.p[set]) + r * n4;
    for (int f = lane_id(); f < n4; f += 64) {
      const int j = f / nd4, d4 = f - j * nd4;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < pl.n_heads; k++) {
        if (pl.set[k] != set) continue;
        const float g = s[pl.off[k] + j];
        if (g != 0.f) {  // (most entries: illegal, g = 0; the query is then not fetched)
          const float4 qv = reinterpret_cast<const float4*>(queries + (r * pl.n_ptr + pl.src[k]) * D)[d4];
          acc.x = fmaf(g, qv.x, acc.x);
          acc.y = fmaf(g, qv.y, acc.y);
          acc.z = fmaf(g, qv.z, acc.z);
          acc.w = fmaf(g, qv.w, acc.w);
        }
      }
      out[f] = acc;
    }
  }
}

// the argument checks both entry points share; *total gets sum(dims)
int check_args(const char* fn, const NmhHeads* hd, int32_t n_rows, const void* logits, int64_t ls, const void* mask,
               int64_t ms, int32_t mask_kind, int64_t* total) {
  if (!hd) return fail(NMH_E_INVALID, "%s: hd is NULL", fn);
  if (hd->n_heads < 1 || hd->n_heads > NMH_MAX_HEADS)
    return fail(NMH_E_INVALID, "%s: n_heads %d outside 1..%d", fn, hd->n_heads, NMH_MAX_HEADS);
  int64_t sum = 0;
  for (int k = 0; k < hd->n_heads; k++) {
    if (hd->dims[k] < 1 || hd->dims[k] > NMH_MAX_DIM)
      return fail(NMH_E_INVALID, "%s: dims[%d] = %d outside 1..%d", fn, k, hd->dims[k], NMH_MAX_DIM);
    sum += hd->dims[k];
  }
  if (n_rows < 0) return fail(NMH_E_INVALID, "%s: n_rows %d is negative", fn, n_rows);
  if (!logits || !mask) return fail(NMH_E_INVALID, "%s: logits or mask is NULL", fn);
  if (mask_kind != NMH_MASK_F32 && mask_kind != NMH_MASK_U8)
    return fail(NMH_E_INVALID, "%s: unknown mask_kind %d", fn, mask_kind);
  if (ls < sum) return fail(NMH_E_INVALID, "%s: logits_stride %lld < sum(dims) %lld", fn, (long long)ls, (long long)sum);
  if (ms < sum) return fail(NMH_E_INVALID, "%s: mask_stride %lld < sum(dims) %lld", fn, (long long)ms, (long long)sum);
  *total = sum;
  return NMH_OK;
}

// The argument checks the two pointer entry points share (SPEC.md §18, "Limits"); fills the plan,
// *dense_total (the dense heads' columns) and *max_rows (the largest set_rows in use).
int check_pointer(const char* fn, const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                  const float* const* keys, const float* dense, int64_t ds, const void* mask, int64_t ms,
                  int32_t mask_kind, PtrPlan* pl, int64_t* total, int64_t* dense_total, int* max_rows) {
  if (!hd) return fail(NMH_E_INVALID, "%s: hd is NULL", fn);
  if (!pt) return fail(NMH_E_INVALID, "%s: pt is NULL", fn);
  if (hd->n_heads < 1 || hd->n_heads > NMH_MAX_HEADS)
    return fail(NMH_E_INVALID, "%s: n_heads %d outside 1..%d", fn, hd->n_heads, NMH_MAX_HEADS);
  if (pt->n_sets < 0 || pt->n_sets > NMH_MAX_SETS)
    return fail(NMH_E_INVALID, "%s: n_sets %d outside 0..%d", fn, pt->n_sets, NMH_MAX_SETS);
  const int D = pt->key_dim;
  if (pt->n_sets > 0 && (D < 4 || D > NMH_MAX_KEY_DIM || D % 4))
    return fail(NMH_E_INVALID, "%s: key_dim %d is not a multiple of 4 in 4..%d", fn, D, NMH_MAX_KEY_DIM);
  *max_rows = 0;  // every set is in use once the plan stands
  for (int s = 0; s < pt->n_sets; s++) {
    if (pt->set_rows[s] < 1 || pt->set_rows[s] >= NMH_MAX_DIM)
      return fail(NMH_E_INVALID, "%s: set_rows[%d] = %d outside 1..%d", fn, s, pt->set_rows[s], NMH_MAX_DIM - 1);
    *max_rows = std::max(*max_rows, pt->set_rows[s]);
  }
  *pl = PtrPlan{};
  pl->n_sets = pt->n_sets;
  pl->key_dim = D;
  const int rc = check_head_plan(fn, hd, pt->n_sets, pt->set_rows, pt->head_set, "key set", n_rows, dense, ds, mask, ms,
                                 mask_kind, {&pl->n_heads, &pl->n_ptr, pl->dims, pl->off, pl->set, pl->src}, total,
                                 dense_total);
  if (rc != NMH_OK) return rc;
  if (pl->n_ptr > 0) {
    if (!queries || !keys) return fail(NMH_E_INVALID, "%s: queries or keys is NULL with pointer heads", fn);
    if (!aligned16(queries)) return fail(NMH_E_INVALID, "%s: queries is not 16-byte aligned", fn);
    for (int s = 0; s < pt->n_sets; s++) {
      if (!keys[s]) return fail(NMH_E_INVALID, "%s: keys[%d] is NULL", fn, s);
      if (!aligned16(keys[s])) return fail(NMH_E_INVALID, "%s: keys[%d] is not 16-byte aligned", fn, s);
      pl->set_rows[s] = pt->set_rows[s];
      pl->keys[s] = keys[s];
    }
  }
  return NMH_OK;
}

// launches K(mask kind, 64-float chunks of a key row), one of the two kernel names below, on n_rows rows
#define NMH_POINTER_LAUNCH(K, fn, ...)                                                                           \
  do {                                                                                                           \
    const dim3 grid((unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);        \
    const int wave_bytes = wave_lds_bytes((int)total, max_rows), nc = (pl.key_dim + 63) / 64;                    \
    const bool f32 = mask_kind == NMH_MASK_F32;                                                                  \
    auto* kern = nc <= 1   ? (f32 ? K(NMH_MASK_F32, 1) : K(NMH_MASK_U8, 1))                                      \
                 : nc == 2 ? (f32 ? K(NMH_MASK_F32, 2) : K(NMH_MASK_U8, 2))                                      \
                           : (f32 ? K(NMH_MASK_F32, 4) : K(NMH_MASK_U8, 4));                                     \
    hipLaunchKernelGGL(kern, grid, block, (size_t)kRowsPerBlock* wave_bytes, static_cast<hipStream_t>(stream), pl, \
                       n_rows, (int)total, wave_bytes, __VA_ARGS__);                                             \
    return heads_launched(fn);                                                                                   \
  } while (0)
#define NMH_POINTER_FWD(MK, NC) nmh_pointer_forward_kernel<MK, NC, SEL>  // where a template's SEL is in scope
#define NMH_POINTER_BWD(MK, NC) nmh_pointer_backward_kernel<MK, NC>

// nmh_forward (SEL = kDraw) and nmh_forward_argmax (kArgmax, which passes no actions and no counter)
template <int SEL>
int forward(const char* fn, const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride,
            const void* mask, int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in, uint64_t seed,
            uint64_t offset, uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy, float* lse,
            float* head_entropy, void* stream) {
  int64_t total;
  const int rc = check_args(fn, hd, n_rows, logits, logits_stride, mask, mask_stride, mask_kind, &total);
  if (rc != NMH_OK) return rc;
  if (!actions_out || !logprob || !entropy || !lse || !head_entropy)
    return fail(NMH_E_INVALID, "%s: an output pointer is NULL", fn);
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  auto* kern = mask_kind == NMH_MASK_F32 ? nmh_forward_kernel<NMH_MASK_F32, SEL> : nmh_forward_kernel<NMH_MASK_U8, SEL>;
  const int tile = (int)std::min<int64_t>(total, NMH_MAX_DIM);
  hipLaunchKernelGGL(kern, grid, block, sizeof(float) * kRowsPerBlock * tile, static_cast<hipStream_t>(stream), *hd,
                     n_rows, tile, logits, logits_stride, mask, mask_stride, actions_in, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), row_base, actions_out,
                     logprob, entropy, lse, head_entropy);
  return heads_launched(fn);
}

// nmh_pointer_forward and nmh_pointer_forward_argmax likewise
template <int SEL>
int pointer_forward(const char* fn, const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                    const float* const* keys, const float* dense, int64_t dense_stride, const void* mask,
                    int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in, uint64_t seed, uint64_t offset,
                    uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy, float* lse,
                    float* head_entropy, void* stream) {
  PtrPlan pl;
  int64_t total, dense_total;
  int max_rows;
  const int rc = check_pointer(fn, hd, pt, n_rows, queries, keys, dense, dense_stride, mask, mask_stride, mask_kind,
                               &pl, &total, &dense_total, &max_rows);
  if (rc != NMH_OK) return rc;
  if (!actions_out || !logprob || !entropy || !lse || !head_entropy)
    return fail(NMH_E_INVALID, "%s: an output pointer is NULL", fn);
  if (n_rows == 0) return NMH_OK;
  NMH_POINTER_LAUNCH(NMH_POINTER_FWD, fn, queries, dense, dense_stride, mask, mask_stride, actions_in, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), row_base, actions_out,
                     logprob, entropy, lse, head_entropy);
}

}  // namespace

// heads_host.h: the library's other translation units report through these two, so that every
// message lands in the g_err nmh_last_error() reads.
int heads_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fail(code, "%s", buf);
}

int heads_launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NMH_OK : fail(NMH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
}

extern "C" {

const char* nmh_last_error(void) { return g_err.c_str(); }
const char* nmh_build_info(void) { return NMMO_BUILD_INFO; }

int nmh_forward(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride, const void* mask,
                int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in, uint64_t seed, uint64_t offset,
                uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy, float* lse,
                float* head_entropy, void* stream) {
  return forward<kDraw>("nmh_forward", hd, n_rows, logits, logits_stride, mask, mask_stride, mask_kind, actions_in,
                        seed, offset, row_base, actions_out, logprob, entropy, lse, head_entropy, stream);
}

int nmh_forward_argmax(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride,
                       const void* mask, int64_t mask_stride, int32_t mask_kind, int32_t* actions_out, float* logprob,
                       float* entropy, float* lse, float* head_entropy, void* stream) {
  return forward<kArgmax>("nmh_forward_argmax", hd, n_rows, logits, logits_stride, mask, mask_stride, mask_kind,
                          nullptr, 0, 0, 0, actions_out, logprob, entropy, lse, head_entropy, stream);
}

int nmh_backward(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride, const void* mask,
                 int64_t mask_stride, int32_t mask_kind, const int32_t* actions, const float* lse,
                 const float* head_entropy, const float* g_logprob, const float* g_entropy, float* g_logits,
                 int64_t g_stride, void* stream) {
  int64_t total;
  const int rc = check_args("nmh_backward", hd, n_rows, logits, logits_stride, mask, mask_stride, mask_kind, &total);
  if (rc != NMH_OK) return rc;
  if (!actions || !lse || !head_entropy || !g_logits)
    return fail(NMH_E_INVALID, "nmh_backward: actions, lse, head_entropy or g_logits is NULL");
  if (g_stride < total)
    return fail(NMH_E_INVALID, "nmh_backward: g_stride %lld < sum(dims) %lld", (long long)g_stride, (long long)total);
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  auto* kern = mask_kind == NMH_MASK_F32 ? nmh_backward_kernel<NMH_MASK_F32> : nmh_backward_kernel<NMH_MASK_U8>;
  hipLaunchKernelGGL(kern, grid, block, 0, static_cast<hipStream_t>(stream), *hd, n_rows, logits, logits_stride, mask,
                     mask_stride, actions, lse, head_entropy, g_logprob, g_entropy, g_logits, g_stride);
  return heads_launched("nmh_backward");
}

int nmh_pointer_forward(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                        const float* const* keys, const float* dense, int64_t dense_stride, const void* mask,
                        int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in, uint64_t seed,
                        uint64_t offset, uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy,
                        float* lse, float* head_entropy, void* stream) {
  return pointer_forward<kDraw>("nmh_pointer_forward", hd, pt, n_rows, queries, keys, dense, dense_stride, mask,
                                mask_stride, mask_kind, actions_in, seed, offset, row_base, actions_out, logprob,
                                entropy, lse, head_entropy, stream);
}

int nmh_pointer_forward_argmax(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                               const float* const* keys, const float* dense, int64_t dense_stride, const void* mask,
                               int64_t mask_stride, int32_t mask_kind, int32_t* actions_out, float* logprob,
                               float* entropy, float* lse, float* head_entropy, void* stream) {
  return pointer_forward<kArgmax>("nmh_pointer_forward_argmax", hd, pt, n_rows, queries, keys, dense, dense_stride,
                                  mask, mask_stride, mask_kind, nullptr, 0, 0, 0, actions_out, logprob, entropy, lse,
                                  head_entropy, stream);
}

int nmh_pointer_backward(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                         const float* const* keys, const float* dense, int64_t dense_stride, const void* mask,
                         int64_t mask_stride, int32_t mask_kind, const int32_t* actions, const float* lse,
                         const float* head_entropy, const float* g_logprob, const float* g_entropy, float* g_dense,
                         int64_t g_dense_stride, float* g_queries, float* const* g_keys, void* stream) {
  PtrPlan pl;
  int64_t total, dense_total;
  int max_rows;
  const int rc = check_pointer("nmh_pointer_backward", hd, pt, n_rows, queries, keys, dense, dense_stride, mask,
                               mask_stride, mask_kind, &pl, &total, &dense_total, &max_rows);
  if (rc != NMH_OK) return rc;
  if (!actions || !lse || !head_entropy)
    return fail(NMH_E_INVALID, "nmh_pointer_backward: actions, lse or head_entropy is NULL");
  if (g_dense && g_dense_stride < dense_total)
    return fail(NMH_E_INVALID, "nmh_pointer_backward: g_dense_stride %lld < the dense heads' %lld columns",
                (long long)g_dense_stride, (long long)dense_total);
  if (g_queries && !aligned16(g_queries))
    return fail(NMH_E_INVALID, "nmh_pointer_backward: g_queries is not 16-byte aligned");
  KeyGrads gk{};
  for (int s = 0; g_keys && s < pl.n_sets; s++) {
    if (!aligned16(g_keys[s]))
      return fail(NMH_E_INVALID, "nmh_pointer_backward: g_keys[%d] is not 16-byte aligned", s);
    gk.p[s] = g_keys[s];
  }
  if (dense_total == 0) g_dense = nullptr;
  if (pl.n_ptr == 0) g_queries = nullptr;
  if (n_rows == 0) return NMH_OK;
  NMH_POINTER_LAUNCH(NMH_POINTER_BWD, "nmh_pointer_backward", queries, dense, dense_stride, mask,
                     mask_stride, actions, lse, head_entropy, g_logprob, g_entropy, g_dense, g_dense_stride,
                     g_queries, gk);
}

}  // extern "C"
