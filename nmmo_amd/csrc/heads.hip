// heads.hip — libnmmo_heads.so (include/nmmo_heads.h): the masked multi-head categorical that
// ends every reference policy (baseline_policy.py:245-262), fused. SPEC.md §15 holds the
// semantics; DESIGN.md §3.12 the kernel notes.
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
#include "host_api.h"
#include "../../include/nmmo_heads.h"

using namespace nmmo;

namespace {

constexpr int kRowsPerBlock = 4;
constexpr int kStage = 16;  // staging loads in flight per lane and kind

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

// One head of one row on one wave (all 64 lanes active) from its staged copy s[0, n): the logit
// where legal, -inf where not. Lane l owns entries [l c, min(n, (l + 1) c)); c is odd, so the
// lanes' reads s[l c + j] fall on distinct LDS banks. `sample`: draw with u, else evaluate a_in.
__device__ __forceinline__ HeadOut head_forward(const float* s, int n, bool sample, float u, int a_in) {
  const int c = ((n + 63) >> 6) | 1;
  const int lo = min(n, lane_id() * c), hi = min(n, lo + c);
  float m = -INFINITY;
  for (int i = lo; i < hi; i++) m = fmaxf(m, s[i]);
  const uint64_t has = __ballot(m != -INFINITY);  // lanes that own a legal entry
  HeadOut o;
  if (has == 0) {  // empty legal set: contributes nothing; a sampled action is uniform over n
    o.action = sample ? min(n - 1, (int)(u * (float)n)) : a_in;
    o.logprob = o.lse = o.entropy = 0.f;
    return o;
  }
  const bool mine = m != -INFINITY;
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
  if (sample) {
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

// tile: floats of LDS per wave = min(sum(dims), NMH_MAX_DIM), so any one head fits
template <int MK>
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
  const bool sample = actions_in == nullptr;
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
    int o_s = 0;
    for (int k = k0; k < k1; k++) {
      const int n = hd.dims[k];
      float u = 0.f;
      int a_in = 0;
      if (sample) {
        u = (float)(philox(row_base + (uint32_t)r, (uint32_t)k, off_lo, off_hi, seed_lo, seed_hi).x >> 8) * 0x1p-24f;
      } else {
        a_in = actions_in[r * hd.n_heads + k];
      }
      const HeadOut o = head_forward(s + o_s, n, sample, u, a_in);
      lp += o.logprob;
      ent += o.entropy;
      if (live && lane_id() == 0) {
        const int64_t q = r * hd.n_heads + k;
        actions_out[q] = o.action;
        lse[q] = o.lse;
        head_entropy[q] = o.entropy;
      }
      o_s += n;
    }
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

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NMH_OK : fail(NMH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
}

}  // namespace

extern "C" {

const char* nmh_last_error(void) { return g_err.c_str(); }
const char* nmh_build_info(void) { return NMMO_BUILD_INFO; }

int nmh_forward(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride, const void* mask,
                int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in, uint64_t seed, uint64_t offset,
                uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy, float* lse,
                float* head_entropy, void* stream) {
  int64_t total;
  const int rc = check_args("nmh_forward", hd, n_rows, logits, logits_stride, mask, mask_stride, mask_kind, &total);
  if (rc != NMH_OK) return rc;
  if (!actions_out || !logprob || !entropy || !lse || !head_entropy)
    return fail(NMH_E_INVALID, "nmh_forward: an output pointer is NULL");
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  auto* kern = mask_kind == NMH_MASK_F32 ? nmh_forward_kernel<NMH_MASK_F32> : nmh_forward_kernel<NMH_MASK_U8>;
  const int tile = (int)std::min<int64_t>(total, NMH_MAX_DIM);
  hipLaunchKernelGGL(kern, grid, block, sizeof(float) * kRowsPerBlock * tile, static_cast<hipStream_t>(stream), *hd,
                     n_rows, tile, logits, logits_stride, mask, mask_stride, actions_in, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset,
                     (uint32_t)(offset >> 32), row_base, actions_out, logprob, entropy, lse, head_entropy);
  return launched("nmh_forward");
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
  return launched("nmh_backward");
}

}  // extern "C"
