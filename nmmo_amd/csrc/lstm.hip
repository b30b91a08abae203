// lstm.hip — libnmmo_lstm.so (include/nmmo_lstm.h): the recurrence of a torch.nn.LSTM layer.
// SPEC.md §17 holds the semantics and the closed-form backward; DESIGN.md §3.14 the kernel notes.
//
// nml_cell_kernel is one elementwise pass: a thread owns kVec consecutive hidden units of one row,
// reads their four gate pre-activations and c, and stores h, c (and the activated gates).
//
// The sequence kernels partition by batch rows: a workgroup owns kRows rows and walks all T steps
// for them. Rows never exchange data, so there is no communication between workgroups of any kind:
// no grid barrier, no flags, no atomics. Per step the workgroup multiplies its rows' h (forward) or
// gate gradients (backward), held in LDS and read as broadcasts, by W_hh streamed from L2 with
// coalesced loads: forward reads the transposed matrix (a thread wants column j of a gate block),
// backward the stored one. A workgroup is 1, 2 or 4 slices of H threads (as many as fit 1,024
// threads): forward splits the four gates over the slices, backward the 4H terms of its dot
// product, so that a step's chain of dependent loads is shared by up to 16 waves.
//
// Dot products are two-level: chains of kChunk float FMAs, whose sums are added in float64. The
// pre-activation is summed in float64 and rounded to float32 once. The order depends on H alone,
// so results are bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <math.h>

#include "host_api.h"
#include "../../include/nmmo_lstm.h"

namespace {

constexpr int kRows = NML_ROWS;
constexpr int kChunk = 16;  // float FMAs per chain; divides NML_H_STEP
constexpr int kCellThreads = 256;
static_assert(NML_H_STEP % kChunk == 0 && kChunk % 4 == 0, "chunks tile H");

// 1 / (1 + e^-x) with the accurate expf: e^100 overflows to +inf and 1 / inf = 0; e^-100 is below
// half an ulp of 1, so the sum is 1. No argument gives a NaN but a NaN.
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct Gates {
  float i, f, g, o;
};

// The cell from its four pre-activations: the activated gates, and c and h by reference.
__device__ __forceinline__ Gates cell(float pi, float pf, float pg, float po, float c_prev, float& c, float& h) {
  const Gates a{sigmoid(pi), sigmoid(pf), tanhf(pg), sigmoid(po)};
  c = a.f * c_prev + a.i * a.g;
  h = a.o * tanhf(c);
  return a;
}

template <int kVec>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
};
template <>
struct alignas(16) Vec<4> {
  float v[4];
};

template <int kVec>
__device__ __forceinline__ Vec<kVec> ld(const float* p) {
  return *reinterpret_cast<const Vec<kVec>*>(p);
}
template <int kVec>
__device__ __forceinline__ void st(float* p, const Vec<kVec>& x) {
  *reinterpret_cast<Vec<kVec>*>(p) = x;
}

// n = B * H / kVec threads of work; c_prev / c_out and ga / gates_out may be the same buffers.
template <int kVec>
__global__ __launch_bounds__(kCellThreads) void nml_cell_kernel(size_t n, int H, const float* ga, const float* gb,
                                                                const float* __restrict__ b_ih,
                                                                const float* __restrict__ b_hh, const float* c_prev,
                                                                float* h_out, float* c_out, float* gates_out) {
  const size_t idx = (size_t)blockIdx.x * kCellThreads + threadIdx.x;
  if (idx >= n) return;
  const int per_row = H / kVec;
  const size_t row = idx / per_row;
  const int j = (int)(idx - row * per_row) * kVec;
  Vec<kVec> pre[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const size_t at = row * 4 * H + (size_t)g * H + j;
    pre[g] = ld<kVec>(ga + at);
    if (b_ih) {
      const Vec<kVec> b = ld<kVec>(b_ih + g * H + j);
#pragma unroll
      for (int u = 0; u < kVec; u++) pre[g].v[u] += b.v[u];
    }
    if (gb) {
      const Vec<kVec> b = ld<kVec>(gb + at);
#pragma unroll
      for (int u = 0; u < kVec; u++) pre[g].v[u] += b.v[u];
    }
    if (b_hh) {
      const Vec<kVec> b = ld<kVec>(b_hh + g * H + j);
#pragma unroll
      for (int u = 0; u < kVec; u++) pre[g].v[u] += b.v[u];
    }
  }
  const Vec<kVec> cp = ld<kVec>(c_prev + row * H + j);
  Vec<kVec> c, h, act[4];
#pragma unroll
  for (int u = 0; u < kVec; u++) {
    const Gates a = cell(pre[0].v[u], pre[1].v[u], pre[2].v[u], pre[3].v[u], cp.v[u], c.v[u], h.v[u]);
    act[0].v[u] = a.i, act[1].v[u] = a.f, act[2].v[u] = a.g, act[3].v[u] = a.o;
  }
  st<kVec>(c_out + row * H + j, c);
  st<kVec>(h_out + row * H + j, h);
  if (gates_out) {
#pragma unroll
    for (int g = 0; g < 4; g++) st<kVec>(gates_out + row * 4 * H + (size_t)g * H + j, act[g]);
  }
}

// acc[r][q] += sum over k < K of v[r][k] * w[k * ldw + q * qs + lane], r < kRows, q < kQ; v is in
// LDS (every lane reads the same address: a broadcast), w in global memory: a wave-uniform address
// plus the lane's 32-bit offset, so that the loads of a chunk share one address register and
// consecutive lanes read consecutive words. Chains of kChunk float FMAs, the chain sums added in
// float64.
template <int kQ>
__device__ __forceinline__ void rows_dot(double (&acc)[kRows][kQ], const float* v, int ldv, const float* __restrict__ w,
                                         unsigned lane, size_t ldw, size_t qs, int K) {
  // one chain at a time: four chains' loads issued together measured slower
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += kChunk) {
    float a[kRows][kQ];
#pragma unroll
    for (int r = 0; r < kRows; r++)
#pragma unroll
      for (int q = 0; q < kQ; q++) a[r][q] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < kChunk; kk += 4) {
      float4 x[kRows];
#pragma unroll
      for (int r = 0; r < kRows; r++) x[r] = *reinterpret_cast<const float4*>(v + r * ldv + k0 + kk);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        float wv[kQ];
#pragma unroll
        for (int q = 0; q < kQ; q++) wv[q] = (w + ((size_t)(k0 + kk + u) * ldw + q * qs))[lane];
#pragma unroll
        for (int r = 0; r < kRows; r++) {
          const float xv = u == 0 ? x[r].x : u == 1 ? x[r].y : u == 2 ? x[r].z : x[r].w;
#pragma unroll
          for (int q = 0; q < kQ; q++) a[r][q] = fmaf(xv, wv[q], a[r][q]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRows; r++)
#pragma unroll
      for (int q = 0; q < kQ; q++) acc[r][q] += (double)a[r][q];
  }
}

// How many slices of H threads a workgroup has: as many as fit 1,024 threads, at most 4, a divisor
// of 4 (the gates) and of kRows.
__host__ __device__ constexpr int slices_for(int H) { return H <= NML_MAX_H / 4 ? 4 : H <= NML_MAX_H / 2 ? 2 : 1; }
static_assert(kRows % 4 == 0, "every slice count divides the rows");

// grid = ceil(B / kRows), block = kS * H, dynamic LDS = forward_lds(H). Thread (s, j) computes the
// 4 / kS gates from s * 4 / kS on, of hidden unit j, for every row: the dot product with its
// columns of W_hh^T, the pre-activation and the activation. The gates then cross the workgroup
// through LDS, and the thread updates c and h of unit j of the rows r with r % kS == s, which it
// keeps in registers. A row past B holds zeros and stores nothing.
template <int kS>
__global__ __launch_bounds__(NML_MAX_H) void nml_seq_forward_kernel(
    int T, int B, int H, const float* __restrict__ xg, const float* __restrict__ whh_t, const float* __restrict__ b_ih,
    const float* __restrict__ b_hh, const float* __restrict__ h0, const float* __restrict__ c0, float* __restrict__ y,
    float* __restrict__ h_T, float* __restrict__ c_T, float* __restrict__ gates, float* __restrict__ cs) {
  constexpr int kQ = 4 / kS, kOwn = kRows / kS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hs = lds;                // [kRows][H]: h_{t-1}
  float* act = lds + kRows * H;   // [kRows][4][H]: the activated gates of step t (kS > 1 only)
  const int s = threadIdx.x / H, j = threadIdx.x - s * H;
  const int row0 = blockIdx.x * kRows;
  const int nr = min(kRows, B - row0);
  float c[kOwn], h[kOwn];
#pragma unroll
  for (int m = 0; m < kOwn; m++) {
    const int r = s + kS * m;
    const bool live = r < nr;
    h[m] = live ? h0[(size_t)(row0 + r) * H + j] : 0.0f;
    c[m] = live ? c0[(size_t)(row0 + r) * H + j] : 0.0f;
    hs[r * H + j] = h[m];
  }
  for (int t = 0; t < T; t++) {
    __syncthreads();  // hs holds h_{t-1} of every hidden unit
    double acc[kRows][kQ];
#pragma unroll
    for (int r = 0; r < kRows; r++)
#pragma unroll
      for (int q = 0; q < kQ; q++) acc[r][q] = 0.0;
    rows_dot<kQ>(acc, hs, H, whh_t, (unsigned)(s * kQ * H + j), (size_t)4 * H, (size_t)H, H);
    if constexpr (kS == 1) __syncthreads();  // every thread is done reading hs
#pragma unroll
    for (int r = 0; r < kRows; r++) {
      if (r >= nr) continue;
      const size_t at = (size_t)t * B + row0 + r;
      float a[kQ];
#pragma unroll
      for (int q = 0; q < kQ; q++) {
        const int g = s * kQ + q;
        const double bi = b_ih ? (double)b_ih[g * H + j] : 0.0, bh = b_hh ? (double)b_hh[g * H + j] : 0.0;
        const float pre = (float)((((double)xg[at * 4 * H + (size_t)g * H + j] + bi) + acc[r][q]) + bh);
        a[q] = g == 2 ? tanhf(pre) : sigmoid(pre);
        gates[at * 4 * H + (size_t)g * H + j] = a[q];
        if constexpr (kS > 1) act[(r * 4 + g) * H + j] = a[q];
      }
      if constexpr (kS == 1) {  // the thread holds all four gates of its unit: update the row now
        c[r] = a[1] * c[r] + a[0] * a[2];
        h[r] = a[3] * tanhf(c[r]);
        cs[at * H + j] = c[r];
        y[at * H + j] = h[r];
        hs[r * H + j] = h[r];
      }
    }
    if constexpr (kS > 1) {
      __syncthreads();  // every thread is done reading hs, and act is complete
#pragma unroll
      for (int m = 0; m < kOwn; m++) {
        const int r = s + kS * m;
        if (r >= nr) continue;
        const float i = act[(r * 4 + 0) * H + j], f = act[(r * 4 + 1) * H + j], g = act[(r * 4 + 2) * H + j];
        const float o = act[(r * 4 + 3) * H + j];
        c[m] = f * c[m] + i * g;
        h[m] = o * tanhf(c[m]);
        const size_t at = (size_t)t * B + row0 + r;
        cs[at * H + j] = c[m];
        y[at * H + j] = h[m];
        hs[r * H + j] = h[m];
      }
    }
  }
#pragma unroll
  for (int m = 0; m < kOwn; m++) {
    const int r = s + kS * m;
    if (r >= nr) continue;
    h_T[(size_t)(row0 + r) * H + j] = h[m];
    c_T[(size_t)(row0 + r) * H + j] = c[m];
  }
}

size_t forward_lds(int H) { return (size_t)kRows * H * sizeof(float) * (slices_for(H) > 1 ? 5 : 1); }

// grid = ceil(B / kRows), block = kS * H, dynamic LDS = backward_lds(H). Thread (s, k) does the
// elementwise step for hidden unit k of the rows r with r % kS == s, then the part of
// dh_{t-1} = dG_t W_hh over the gate units n of slice s, [s * 4H / kS, (s + 1) * 4H / kS), for
// every row; the kS partial sums meet in LDS and are added in slice order.
template <int kS>
__global__ __launch_bounds__(NML_MAX_H) void nml_seq_backward_kernel(
    int T, int B, int H, const float* __restrict__ dy, const float* __restrict__ dh_T, const float* __restrict__ dc_T,
    const float* __restrict__ gates, const float* __restrict__ cs, const float* __restrict__ c0,
    const float* __restrict__ whh, float* __restrict__ dG, float* __restrict__ dh0, float* __restrict__ dc0) {
  constexpr int kOwn = kRows / kS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* dgs = lds;                                                   // [kRows][4H]: dG_t
  double* part = reinterpret_cast<double*>(lds + kRows * 4 * H);      // [kS][kRows][H] (kS > 1 only)
  const int s = threadIdx.x / H, k = threadIdx.x - s * H;
  const int row0 = blockIdx.x * kRows;
  const int nr = min(kRows, B - row0);
  const int span = 4 * H / kS;  // gate units per slice
  float dh[kOwn], dc[kOwn];
#pragma unroll
  for (int m = 0; m < kOwn; m++) {
    const int r = s + kS * m;
    const bool live = r < nr;
    dh[m] = live ? dh_T[(size_t)(row0 + r) * H + k] : 0.0f;
    dc[m] = live ? dc_T[(size_t)(row0 + r) * H + k] : 0.0f;
#pragma unroll
    for (int q = 0; q < 4; q++) dgs[r * 4 * H + q * H + k] = 0.0f;  // rows past B stay zero
  }
  for (int t = T - 1; t >= 0; t--) {
#pragma unroll
    for (int m = 0; m < kOwn; m++) {
      const int r = s + kS * m;
      if (r >= nr) continue;
      const size_t at = (size_t)t * B + row0 + r;
      const float* gp = gates + at * 4 * H + k;
      const float i = gp[0], f = gp[H], g = gp[2 * (size_t)H], o = gp[3 * (size_t)H];
      const float c_prev = t ? cs[(at - B) * H + k] : c0[(size_t)(row0 + r) * H + k];
      const float tc = tanhf(cs[at * H + k]);
      const float dht = dy[at * H + k] + dh[m];
      const float dct = dc[m] + dht * o * (1.0f - tc * tc);
      const float d[4] = {dct * g * (i * (1.0f - i)), dct * c_prev * (f * (1.0f - f)), dct * i * (1.0f - g * g),
                          dht * tc * (o * (1.0f - o))};
      dc[m] = dct * f;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        dG[at * 4 * H + (size_t)q * H + k] = d[q];
        dgs[r * 4 * H + q * H + k] = d[q];
      }
    }
    __syncthreads();  // dgs holds dG_t of every gate unit
    double acc[kRows][1];
#pragma unroll
    for (int r = 0; r < kRows; r++) acc[r][0] = 0.0;
    rows_dot<1>(acc, dgs + s * span, 4 * H, whh, (unsigned)(s * span * H + k), (size_t)H, 0, span);
    if constexpr (kS > 1) {
#pragma unroll
      for (int r = 0; r < kRows; r++) part[(s * kRows + r) * H + k] = acc[r][0];
    }
    __syncthreads();  // every thread is done reading dgs, and part is complete
#pragma unroll
    for (int m = 0; m < kOwn; m++) {
      const int r = s + kS * m;
      if constexpr (kS > 1) {
        double sum = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < kS; s2++) sum += part[(s2 * kRows + r) * H + k];
        dh[m] = (float)sum;
      } else {
        dh[m] = (float)acc[r][0];
      }
    }
    // the next step's part is written behind its first barrier, after these reads
  }
#pragma unroll
  for (int m = 0; m < kOwn; m++) {
    const int r = s + kS * m;
    if (r >= nr) continue;
    dh0[(size_t)(row0 + r) * H + k] = dh[m];
    dc0[(size_t)(row0 + r) * H + k] = dc[m];
  }
}

size_t backward_lds(int H) {
  const int S = slices_for(H);
  return (size_t)kRows * 4 * H * sizeof(float) + (S > 1 ? (size_t)S * kRows * H * sizeof(double) : 0);
}

// 0, or the error of a call named `fn` whose B, H (and T, when has_t) are out of range
int check_shape(const char* fn, bool has_t, int T, int B, int H) {
  if (has_t && (T < 1 || T > NML_MAX_T)) return fail(NML_E_INVALID, "%s: T %d outside 1..%d", fn, T, NML_MAX_T);
  if (B < 0 || B > NML_MAX_B) return fail(NML_E_INVALID, "%s: B %d outside 0..%d", fn, B, NML_MAX_B);
  if (H < NML_H_STEP || H > NML_MAX_H || H % NML_H_STEP)
    return fail(NML_E_INVALID, "%s: H %d is not a multiple of %d in %d..%d", fn, H, NML_H_STEP, NML_H_STEP, NML_MAX_H);
  return NML_OK;
}

struct Named {
  const char* name;
  const void* p;
};

template <int N>
int check_ptrs(const char* fn, const Named (&ptrs)[N]) {
  for (const Named& a : ptrs)
    if (!a.p) return fail(NML_E_INVALID, "%s: %s is NULL", fn, a.name);
  return NML_OK;
}

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NML_OK : fail(NML_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

const char* nml_last_error(void) { return g_err.c_str(); }
const char* nml_build_info(void) { return NMMO_BUILD_INFO; }

int nml_cell(int32_t B, int32_t H, const float* ga, const float* gb, const float* b_ih, const float* b_hh,
             const float* c_prev, float* h_out, float* c_out, float* gates_out, void* stream) {
  if (int rc = check_shape("nml_cell", false, 1, B, H)) return rc;
  const Named req[] = {{"ga", ga}, {"c_prev", c_prev}, {"h_out", h_out}, {"c_out", c_out}};
  if (int rc = check_ptrs("nml_cell", req)) return rc;
  if (B == 0) return NML_OK;
  // 16-byte accesses when every buffer allows them (H is a multiple of 4 by the check above)
  const bool vec = aligned16(ga) && aligned16(gb) && aligned16(b_ih) && aligned16(b_hh) && aligned16(c_prev) &&
                   aligned16(h_out) && aligned16(c_out) && aligned16(gates_out);
  const size_t n = (size_t)B * H / (vec ? 4 : 1);
  const dim3 grid((unsigned)((n + kCellThreads - 1) / kCellThreads));
  auto* kern = vec ? nml_cell_kernel<4> : nml_cell_kernel<1>;
  hipLaunchKernelGGL(kern, grid, dim3(kCellThreads), 0, static_cast<hipStream_t>(stream), n, H, ga, gb, b_ih, b_hh,
                     c_prev, h_out, c_out, gates_out);
  return launched("nml_cell");
}

int nml_seq_forward(int32_t T, int32_t B, int32_t H, const float* xg, const float* whh_t, const float* b_ih,
                    const float* b_hh, const float* h0, const float* c0, float* y, float* h_T, float* c_T, float* gates,
                    float* cs, void* stream) {
  if (int rc = check_shape("nml_seq_forward", true, T, B, H)) return rc;
  const Named req[] = {{"xg", xg}, {"whh_t", whh_t}, {"h0", h0},       {"c0", c0}, {"y", y},
                       {"h_T", h_T}, {"c_T", c_T},   {"gates", gates}, {"cs", cs}};
  if (int rc = check_ptrs("nml_seq_forward", req)) return rc;
  if (B == 0) return NML_OK;
  const int S = slices_for(H);
  auto* kern = S == 4 ? nml_seq_forward_kernel<4> : S == 2 ? nml_seq_forward_kernel<2> : nml_seq_forward_kernel<1>;
  hipLaunchKernelGGL(kern, dim3((B + kRows - 1) / kRows), dim3(S * H), forward_lds(H), static_cast<hipStream_t>(stream),
                     T, B, H, xg, whh_t, b_ih, b_hh, h0, c0, y, h_T, c_T, gates, cs);
  return launched("nml_seq_forward");
}

int nml_seq_backward(int32_t T, int32_t B, int32_t H, const float* dy, const float* dh_T, const float* dc_T,
                     const float* gates, const float* cs, const float* c0, const float* whh, float* dG, float* dh0,
                     float* dc0, void* stream) {
  if (int rc = check_shape("nml_seq_backward", true, T, B, H)) return rc;
  const Named req[] = {{"dy", dy}, {"dh_T", dh_T}, {"dc_T", dc_T}, {"gates", gates}, {"cs", cs},
                       {"c0", c0}, {"whh", whh},   {"dG", dG},     {"dh0", dh0},     {"dc0", dc0}};
  if (int rc = check_ptrs("nml_seq_backward", req)) return rc;
  if (B == 0) return NML_OK;
  const int S = slices_for(H);
  auto* kern = S == 4 ? nml_seq_backward_kernel<4> : S == 2 ? nml_seq_backward_kernel<2> : nml_seq_backward_kernel<1>;
  hipLaunchKernelGGL(kern, dim3((B + kRows - 1) / kRows), dim3(S * H), backward_lds(H),  // at most 64 KiB
                     static_cast<hipStream_t>(stream), T, B, H, dy, dh_T, dc_T, gates, cs, c0, whh, dG, dh0, dc0);
  return launched("nml_seq_backward");
}

}  // extern "C"
