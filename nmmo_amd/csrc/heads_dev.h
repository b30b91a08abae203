// heads_dev.h — the device functions of the masked heads that more than one translation unit of
// libnmmo_heads.so uses: wave_sync and legal_at (heads.hip, decoder.hip, item_enc.hip,
// player_enc.hip) and, for heads.hip and decoder.hip, the float wave reductions, one head of one row
// on one wave from its staged tile (SPEC.md §15), the heads of a tile in sequence, and the legal list
// of a pointer head (SPEC.md §18). Internal linkage: every translation unit compiles its own copy.
#pragma once

#include <math.h>

#include "common.h"
#include "../../include/nmmo_heads.h"

namespace nmmo {
namespace {

// ---- float wave reductions in the style of common.h's wave_incl_scan: four row_shr steps scan
// each 16-lane row, row_bcast:15 / :31 carry row totals upward. Lanes whose DPP source is out of
// the row, and rows the row mask disables, read `old` = the identity.
template <class Op>
__device__ __forceinline__ float wave_incl_scan_f(float x, float ident, Op op) {
  const int id = __float_as_int(ident);
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x111, 0xF, 0xF, false)));
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x112, 0xF, 0xF, false)));
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x114, 0xF, 0xF, false)));
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x118, 0xF, 0xF, false)));
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x142, 0xA, 0xF, false)));
  x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(id, __float_as_int(x), 0x143, 0xC, 0xF, false)));
  return x;
}
__device__ __forceinline__ float lane63(float x) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ float wave_scan_add(float x) {
  return wave_incl_scan_f(x, 0.f, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ float wave_max_f(float x) {
  return lane63(wave_incl_scan_f(x, -INFINITY, [](float a, float b) { return fmaxf(a, b); }));
}

template <int MK>
__device__ __forceinline__ bool legal_at(const void* mask, int64_t i) {
  if (MK == NMH_MASK_F32) return static_cast<const float*>(mask)[i] > 0.f;
  return static_cast<const uint8_t*>(mask)[i] != 0;
}

struct HeadOut {
  int action;
  float logprob, lse, entropy;
};

// How a forward kernel chooses a head's action, a compile-time parameter of the kernel. kDraw is
// one instantiation for both of the calls that have `actions_in`: NULL samples, else it is evaluated.
// kArgmax is the greedy selection of SPEC.md §24; it reads neither actions_in nor the philox counter.
enum Select { kDraw = 0, kArgmax = 1 };

// One head of one row on one wave (all 64 lanes active) from its staged copy s[0, n): the logit
// where legal, -inf where not. Lane l owns entries [l c, min(n, (l + 1) c)); c is odd, so the
// lanes' reads s[l c + j] fall on distinct LDS banks. kDraw: `sample` draws with u, else a_in is
// evaluated. kArgmax: the smallest index whose logit is the head's maximum (0 if nothing is legal),
// then evaluated like a given action; sample, u and a_in are not looked at.
template <int SEL>
__device__ __forceinline__ HeadOut head_forward(const float* s, int n, bool sample, float u, int a_in) {
  const int c = ((n + 63) >> 6) | 1;
  const int lo = min(n, lane_id() * c), hi = min(n, lo + c);
  float m = -INFINITY;
  int first = lo;  // kArgmax: the lane's first index of its maximum
  for (int i = lo; i < hi; i++) {
    const float x = s[i];
    if (SEL == kArgmax) first = x > m ? i : first;
    m = fmaxf(m, x);
  }
  const uint64_t has = __ballot(m != -INFINITY);  // lanes that own a legal entry
  HeadOut o;
  if (has == 0) {  // empty legal set: contributes nothing; a sampled action is uniform over n
    o.action = SEL == kArgmax ? 0 : sample ? min(n - 1, (int)(u * (float)n)) : a_in;
    o.logprob = o.lse = o.entropy = 0.f;
    return o;
  }
  const bool mine = m != -INFINITY;
  const float lane_max = m;
  m = wave_max_f(m);
  float sum = 0.f, ts = 0.f;
  for (int i = lo; i < hi; i++) {
    const float x = s[i], t = x - m;
    const bool l = x != -INFINITY;
    const float ev = l ? expf(t) : 0.f;
    sum += ev;
    ts += l ? ev * t : 0.f;
  }
  const float P = wave_scan_add(sum);  // inclusive sums over lanes, in entry order
  const float S = lane63(P);
  const float T = lane63(wave_scan_add(ts));
  const float logS = logf(S);
  o.lse = m + logS;
  o.entropy = logS - T / S;  // = lse - sum p x, without the cancellation against m
  int a = a_in;
  if (SEL == kArgmax) {
    // Lanes own ascending ranges, so the lowest lane whose maximum is the wave's holds the smallest
    // index. fmaxf returns one of its operands: some lane's maximum equals m bit for bit (a NaN logit
    // is outside the contract; lane 0's index keeps the action in range then).
    const uint64_t top = __ballot(mine && lane_max == m);
    a = __builtin_amdgcn_readlane(first, top ? __ffsll((unsigned long long)top) - 1 : 0);
  } else if (sample) {
    const float tgt = u * S;
    // first lane with a legal entry whose inclusive sum passes tgt; u * S can round up to S, and
    // the scan's lane sums are not exactly monotone, so fall back to the last lane that has one
    const uint64_t hit = __ballot(P > tgt && mine);
    const int L = hit ? __ffsll((unsigned long long)hit) - 1 : 63 - __clzll((long long)has);
    float acc = P - sum;
    int pick = -1, last = -1;
    for (int i = lo; i < hi; i++) {
      const float x = s[i];
      if (x != -INFINITY) {
        acc += expf(x - m);
        last = i;
        pick = (pick < 0 && acc > tgt) ? i : pick;
      }
    }
    pick = pick < 0 ? last : pick;  // (the serial walk can end a rounding short of the scan's P)
    a = __builtin_amdgcn_readlane(pick, L);
  }
  o.action = a;
  const float xa = (a >= 0 && a < n) ? s[a] : -INFINITY;
  o.logprob = xa != -INFINITY ? (xa - m) - logS : -1e9f - o.lse;  // illegal: what masked_fill(-1e9) yields
  return o;
}

// Heads [k0, k1) of row r from their staged copies, which lie back to back from s: draws, reads or
// (kArgmax) selects the action of each, stores its per-head outputs (a live wave's lane 0) and adds
// its logprob and entropy to lp / ent.
template <int SEL>
__device__ __forceinline__ void tile_heads(const float* s, const int32_t* dims, int k0, int k1, int n_heads, int64_t r,
                                           bool live, const int32_t* __restrict__ actions_in, uint32_t seed_lo,
                                           uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi, uint32_t row_base,
                                           int32_t* __restrict__ actions_out, float* __restrict__ lse,
                                           float* __restrict__ head_entropy, float& lp, float& ent) {
  const bool sample = SEL == kDraw && actions_in == nullptr;
  int o_s = 0;
  for (int k = k0; k < k1; k++) {
    const int n = dims[k];
    float u = 0.f;
    int a_in = 0;
    if (sample) {
      u = (float)(philox(row_base + (uint32_t)r, (uint32_t)k, off_lo, off_hi, seed_lo, seed_hi).x >> 8) * 0x1p-24f;
    } else if (SEL == kDraw) {
      a_in = actions_in[r * n_heads + k];
    }
    const HeadOut o = head_forward<SEL>(s + o_s, n, sample, u, a_in);
    lp += o.logprob;
    ent += o.entropy;
    if (live && lane_id() == 0) {
      const int64_t q = r * n_heads + k;
      actions_out[q] = o.action;
      lse[q] = o.lse;
      head_entropy[q] = o.entropy;
    }
    o_s += n;
  }
}

// orders this wave's LDS stores before its later LDS loads from other lanes
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The mask of one pointer head's m candidates (mask entries mbase + [0, m)): s[j] = fill for every
// j < m, and the legal j in ascending order in list[0, cnt). Returns cnt (wave-uniform).
template <int MK>
__device__ __forceinline__ int legal_list(const void* __restrict__ mask, int64_t mbase, int m, float* s, float fill,
                                          uint16_t* list) {
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
      if (j < m) s[j] = fill;
      if (lg) list[cnt + __popcll(b & lanes_below())] = (uint16_t)j;
      cnt += __popcll(b);
    }
  }
  return cnt;
}

}  // namespace
}  // namespace nmmo
