// tile_enc.hip — the tile encoder's embedding + first 3x3 convolution + ReLU as one table lookup
// (SPEC.md §19; include/nmmo_heads.h, nmh_tile_forward / nmh_tile_backward). Part of
// libnmmo_heads.so.
//
// The embedding and the convolution are both linear and the embedding's input is an index, so
//   conv1(embed(tile))[n][o][y][x] = b1[o] + sum_{ky,kx,f} T[f][idx[n][(y+ky)*15 + x+kx][f]][ky*3+kx][o]
// with T [3, 256, 9, 32] a function of the weights alone (nmmo_amd/tile.py, tile_table). Per row
// that is 169 x 27 reads of 32 consecutive floats and 146 k additions instead of 4.67 M
// multiply-adds, and the [N, 96, 15, 15] embedding tensor never exists.
//
// Forward: a workgroup of 256 threads takes kFwdRows rows. The 675 indices of a row are computed
// from the obs row in place and kept in LDS as bytes. 8 lanes share one output position, each with
// 4 consecutive channels, so a table read is 8 x 16 B = the 128 contiguous bytes of T[f][v][k][:],
// served by L1 / L2 (the whole table is 864 KiB). Each channel's 28 additions are made in the order
// SPEC §19 fixes, by one lane. The [32][169] result goes through LDS so that the stores to `out`
// are contiguous.
//
// Backward: a workgroup of 512 threads owns the (feature f, tap k) slice [256][32] of the table
// gradient, 32 KiB of LDS, for one chunk of rows. Entry (v, o) belongs to one thread: wave v & 7,
// lane (o, (v >> 3) & 1). The workgroup walks its rows and the 169 positions of each in ascending
// order; lane j of every wave holds the indices of positions j, j + 64 and j + 128, a ballot gives
// the wave the positions it owns, and it visits only those: the owner alone adds dz[n][o][p] to
// its entry. The next row's out, g_out and indices are loaded while the row is added up.
// No atomics, one fixed order of additions per entry: the same bits on every run. The slice is
// stored whole at the end, zeros included. The workgroup of slice (0, 0) also sums the bias
// gradient of its chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_api.h"
#include "../../include/nmmo_heads.h"

// heads.hip: the message goes into the error text nmh_last_error() returns
int heads_record_error(int code, const char* msg);

namespace {

constexpr int kT = NMH_TILE_TILES, kF = NMH_TILE_FEATURES, kV = NMH_TILE_VALUES, kK = NMH_TILE_TAPS;
constexpr int kO = NMH_TILE_CHANNELS, kSide = 15, kOutSide = 13, kP = kOutSide * kOutSide;
constexpr int kRowIdx = kT * kF;   // 675 entries of a row's Tile section
constexpr int kRowOut = kO * kP;   // 5408 floats of a row's output
constexpr int kCentre = 112;
constexpr int kFwdRows = NMH_TILE_FWD_ROWS, kFwdThreads = 256;
constexpr int kBwdThreads = 512;
constexpr int kSlices = kF * kK;  // 27 (feature, tap) slices

static_assert(kRowOut % 4 == 0, "a row of out is whole float4s");
static_assert(kT == kSide * kSide && kK == 9 && kO == 32 && kV == 256 && kF == 3, "the start-kit shape");

#define TILE_FAIL(code, ...) heads_record_error(fail(code, __VA_ARGS__), g_err.c_str())

// SPEC §19's index rule. float32: (v - c) + 7 in two roundings, truncated, clamped, NaN -> 0.
__device__ inline int tile_index(float v, float c, bool relative) {
  const float t = relative ? (v - c) + 7.0f : v;
  return t >= 0.0f ? (t >= 255.0f ? 255 : (int)t) : 0;
}
__device__ inline int tile_index(int16_t v, int16_t c, bool relative) {
  const int t = relative ? ((int)v - (int)c) + 7 : (int)v;
  return t < 0 ? 0 : (t > 255 ? 255 : t);
}

template <typename T>
__global__ __launch_bounds__(kFwdThreads) void nmh_tile_forward_kernel(
    int n_rows, const T* __restrict__ tile, int64_t tile_stride, const float* __restrict__ table,
    const float* __restrict__ bias, float* __restrict__ out, uint8_t* __restrict__ idx_out) {
  __shared__ uint8_t s_idx[kRowIdx + 1];
  __shared__ float s_out[kRowOut];
  const int tid = threadIdx.x;
  const int oq = tid & 7, slot = tid >> 3;  // channels 4 oq .. 4 oq + 3 of positions slot, slot + 32, ...
  const float4 b4 = reinterpret_cast<const float4*>(bias)[oq];
  const float4* __restrict__ table4 = reinterpret_cast<const float4*>(table) + oq;
  const int64_t row0 = (int64_t)blockIdx.x * kFwdRows;
  for (int r = 0; r < kFwdRows; ++r) {
    const int64_t n = row0 + r;
    if (n >= n_rows) break;  // uniform over the workgroup
    const T* __restrict__ row = tile + n * tile_stride;
    const T c0 = row[kCentre * kF], c1 = row[kCentre * kF + 1];
    for (int e = tid; e < kRowIdx; e += kFwdThreads) {
      const int f = e % kF;
      const int i = tile_index(row[e], f == 0 ? c0 : c1, f < 2);
      s_idx[e] = (uint8_t)i;
      if (idx_out) idx_out[n * kRowIdx + e] = (uint8_t)i;
    }
    __syncthreads();
    for (int p = slot; p < kP; p += kFwdThreads / 8) {
      const int y = p / kOutSide, x = p - y * kOutSide;
      float4 z = b4;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const uint8_t* ip = s_idx + ((y + ky) * kSide + x + kx) * kF;
#pragma unroll
          for (int f = 0; f < kF; ++f) {
            const float4 t = table4[((f * kV + (int)ip[f]) * kK + ky * 3 + kx) * (kO / 4)];
            z.x += t.x;
            z.y += t.y;
            z.z += t.z;
            z.w += t.w;
          }
        }
      }
      float* so = s_out + (4 * oq) * kP + p;
      so[0] = fmaxf(z.x, 0.0f);
      so[kP] = fmaxf(z.y, 0.0f);
      so[2 * kP] = fmaxf(z.z, 0.0f);
      so[3 * kP] = fmaxf(z.w, 0.0f);
    }
    __syncthreads();
    float* __restrict__ orow = out + n * kRowOut;
    for (int i = tid; i < kRowOut; i += kFwdThreads) orow[i] = s_out[i];
    // no third barrier: the next row's s_idx writes come after this row's last s_idx read (the
    // barrier above), and its s_out writes after its own first barrier, which every thread
    // reaches only after these reads of s_out
  }
}

__global__ __launch_bounds__(kBwdThreads) void nmh_tile_backward_kernel(
    int n_rows, int rows_per_chunk, const uint8_t* __restrict__ idx, const float* __restrict__ out,
    const float* __restrict__ g_out, float* __restrict__ g_table_parts, float* __restrict__ g_bias_parts) {
  __shared__ float s_acc[kV * kO];  // this (feature, tap) slice of the chunk's table gradient
  __shared__ __attribute__((aligned(16))) float s_dz[kRowOut];  // the row's dz, [o][p] as in g_out
  __shared__ float s_red[(kBwdThreads / kO) * kO];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int o = lane & 31, half = lane >> 5;
  const int chunk = blockIdx.x / kSlices, slice = blockIdx.x - chunk * kSlices;
  const int f = slice / kK, k = slice - f * kK;
  const int ky = k / 3, kx = k - ky * 3;
  const int64_t lo = (int64_t)chunk * rows_per_chunk;
  const int64_t hi = lo + rows_per_chunk < n_rows ? lo + rows_per_chunk : n_rows;
  for (int i = tid; i < kV * kO; i += kBwdThreads) s_acc[i] = 0.0f;
  // lane j holds the indices of positions j, j + 64 and j + 128: the Tile entries its taps read
  int toff[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int p = lane + 64 * q < kP ? lane + 64 * q : kP - 1;
    const int y = p / kOutSide, x = p - y * kOutSide;
    toff[q] = ((y + ky) * kSide + x + kx) * kF + f;
  }
  float bsum = 0.0f;  // slice 0 only: thread (o, g = tid / 32) sums positions g, g + 16, ... of every row
  // A row's out and g_out are 1,352 float4 each, up to 3 per thread, and its 3 index bytes per
  // lane: all loaded a row ahead, so that they are in flight while the row before is added up.
  constexpr int kQuads = kRowOut / 4, kPer = (kQuads + kBwdThreads - 1) / kBwdThreads;
  float4 po[kPer], pg[kPer];
  int pv[3];
  auto prefetch = [&](int64_t n) {
    const float4* __restrict__ orow = reinterpret_cast<const float4*>(out + n * kRowOut);
    const float4* __restrict__ grow = reinterpret_cast<const float4*>(g_out + n * kRowOut);
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * kBwdThreads;
      if (i < kQuads) {
        po[u] = orow[i];
        pg[u] = grow[i];
      }
    }
    const uint8_t* __restrict__ irow = idx + n * kRowIdx;
#pragma unroll
    for (int q = 0; q < 3; ++q) pv[q] = irow[toff[q]];
  };
  if (lo < hi) prefetch(lo);
  for (int64_t n = lo; n < hi; ++n) {
    __syncthreads();  // the previous row's readers of s_dz are done (and s_acc is zeroed)
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * kBwdThreads;
      if (i < kQuads)
        reinterpret_cast<float4*>(s_dz)[i] =
            make_float4(po[u].x > 0.0f ? pg[u].x : 0.0f, po[u].y > 0.0f ? pg[u].y : 0.0f,
                        po[u].z > 0.0f ? pg[u].z : 0.0f, po[u].w > 0.0f ? pg[u].w : 0.0f);
    }
    const int v0 = pv[0], v1 = pv[1], v2 = pv[2];
    __syncthreads();
    if (n + 1 < hi) prefetch(n + 1);
    if (slice == 0)
      for (int p = tid >> 5; p < kP; p += kBwdThreads / kO) bsum += s_dz[o * kP + p];
    const float* dzo = s_dz + o * kP;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int vq = q == 0 ? v0 : (q == 1 ? v1 : v2);
      // the positions 64 q + j whose entry this wave owns, as a bit per lane j: visited in
      // ascending order, the others cost nothing
      unsigned long long mine = __ballot(lane + 64 * q < kP && (vq & 7) == wave);
      while (mine) {
        const int j = __builtin_ctzll(mine);
        mine &= mine - 1;
        const int v = __builtin_amdgcn_readlane(vq, j);  // wave-uniform
        if (((v >> 3) & 1) == half) s_acc[v * kO + o] += dzo[64 * q + j];
      }
    }
  }
  __syncthreads();
  // the slice, whole: g_table_parts [chunk][f][v][k][o]
  float* __restrict__ gt = g_table_parts + (int64_t)chunk * (kF * kV * kK * kO) + ((int64_t)f * kV * kK + k) * kO;
  for (int i = tid; i < kV * kO; i += kBwdThreads) gt[(int64_t)(i >> 5) * (kK * kO) + (i & 31)] = s_acc[i];
  if (slice == 0) {
    s_red[tid] = bsum;  // [g][o]
    __syncthreads();
    if (tid < kO) {
      float s = 0.0f;
      for (int g = 0; g < kBwdThreads / kO; ++g) s += s_red[g * kO + tid];
      g_bias_parts[(int64_t)chunk * kO + tid] = s;
    }
  }
}

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NMH_OK : TILE_FAIL(NMH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int nmh_tile_forward(int32_t n_rows, const void* tile, int64_t tile_stride, int32_t tile_kind, const float* table,
                     const float* bias, float* out, uint8_t* idx_out, void* stream) {
  if (n_rows < 0) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: n_rows %d is negative", n_rows);
  if (!tile) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: tile is NULL");
  if (!table) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: table is NULL");
  if (!bias) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: bias is NULL");
  if (!out) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: out is NULL");
  if (tile_kind != NMH_TILE_F32 && tile_kind != NMH_TILE_I16)
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: unknown tile_kind %d", tile_kind);
  if (tile_stride < kRowIdx)
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: tile_stride %lld < %d", (long long)tile_stride, kRowIdx);
  if (!aligned16(table) || !aligned16(bias))
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_forward: table or bias is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kFwdRows - 1) / kFwdRows)), block(kFwdThreads);
  if (tile_kind == NMH_TILE_F32)
    hipLaunchKernelGGL(nmh_tile_forward_kernel<float>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const float*>(tile), tile_stride, table, bias, out, idx_out);
  else
    hipLaunchKernelGGL(nmh_tile_forward_kernel<int16_t>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const int16_t*>(tile), tile_stride, table, bias, out, idx_out);
  return launched("nmh_tile_forward");
}

int nmh_tile_backward(int32_t n_rows, const uint8_t* idx, const float* out, const float* g_out, int32_t n_chunks,
                      float* g_table_parts, float* g_bias_parts, void* stream) {
  if (n_rows < 0) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: n_rows %d is negative", n_rows);
  if (!idx) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: idx is NULL");
  if (!out) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: out is NULL");
  if (!g_out) return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: g_out is NULL");
  if (!g_table_parts || !g_bias_parts)
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: g_table_parts or g_bias_parts is NULL");
  if (n_chunks < 1 || n_chunks > NMH_TILE_MAX_CHUNKS)
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: n_chunks %d outside 1..%d", n_chunks, NMH_TILE_MAX_CHUNKS);
  if (!aligned16(out) || !aligned16(g_out))
    return TILE_FAIL(NMH_E_INVALID, "nmh_tile_backward: out or g_out is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const int rows_per_chunk = (int)(((int64_t)n_rows + n_chunks - 1) / n_chunks);
  hipLaunchKernelGGL(nmh_tile_backward_kernel, dim3((unsigned)(n_chunks * kSlices)), dim3(kBwdThreads), 0,
                     static_cast<hipStream_t>(stream), n_rows, rows_per_chunk, idx, out, g_out, g_table_parts,
                     g_bias_parts);
  return launched("nmh_tile_backward");
}

}  // extern "C"
