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
//
// With the second convolution (SPEC.md §22; nmh_tile2_forward / nmh_tile2_backward): the forward
// kernel keeps a row's a1 = relu(conv1(embed(tile))) [32][169] in LDS, where the plain forward stages
// it for its stores, and runs tile_conv_2 and its ReLU on that copy. Thread (g = tid / 128,
// p = tid % 128 < 121) owns output position p of channels 4 g .. 4 g + 3 and adds the 288 terms of
// each in the order c, ky, kx; g is uniform over a wave, so the weights come by scalar loads and
// W2 takes no LDS. Only the 968 floats of out2 leave the CU. Backward is two launches. Stage 1, one
// workgroup of 256 threads per part of rows: per row it recomputes a1 in LDS from the saved
// indices, stages dz2 = g_out2 * (out2 > 0) in LDS inside a border of two zeros, stores the gated
// dz1 row (wave w owns channels w, w + 4, ..: W2 again by scalar loads) and adds the row to its
// part of g_W2, thread (o2, c) = (tid / 32, tid % 32) owning the 9 taps of that pair; thread
// (o2, 0) also sums g_b2[o2]. Stage 2 is the backward kernel above over dz1, which is gated
// already: it is a template on that.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heads_host.h"  // heads_fail, heads_launched, aligned16
#include "../../include/nmmo_heads.h"

namespace {

constexpr int kT = NMH_TILE_TILES, kF = NMH_TILE_FEATURES, kV = NMH_TILE_VALUES, kK = NMH_TILE_TAPS;
constexpr int kO = NMH_TILE_CHANNELS, kSide = 15, kOutSide = 13, kP = kOutSide * kOutSide;
constexpr int kRowIdx = kT * kF;   // 675 entries of a row's Tile section
constexpr int kRowOut = kO * kP;   // 5408 floats of a row's output
constexpr int kCentre = 112;
constexpr int kFwdRows = NMH_TILE_FWD_ROWS, kFwdThreads = 256;
constexpr int kBwdThreads = 512;
constexpr int kSlices = kF * kK;  // 27 (feature, tap) slices
// the second convolution (SPEC §22): 32 -> 8 channels, 3 x 3, 13 x 13 -> 11 x 11
constexpr int kO2 = NMH_TILE2_CHANNELS, kOut2Side = 11, kP2 = kOut2Side * kOut2Side;
constexpr int kRowOut2 = kO2 * kP2;       // 968 floats of a row's out2
constexpr int kW2 = kO2 * kO * kK;        // 2304 weights
constexpr int kFwd2Rows = NMH_TILE2_FWD_ROWS;
constexpr int kPadSide = kOut2Side + 4, kPad = kPadSide * kPadSide;  // dz2 inside a border of two zeros

static_assert(kRowOut % 4 == 0, "a row of out is whole float4s");
static_assert(kT == kSide * kSide && kK == 9 && kO == 32 && kV == 256 && kF == 3, "the start-kit shape");
static_assert(kO2 == 8 && kP2 == NMH_TILE2_OUT && kO2 * kO == kFwdThreads, "one thread per (o2, c) pair of g_W2");

// SPEC §19's index rule. float32: (v - c) + 7 in two roundings, truncated, clamped, NaN -> 0.
__device__ inline int tile_index(float v, float c, bool relative) {
  const float t = relative ? (v - c) + 7.0f : v;
  return t >= 0.0f ? (t >= 255.0f ? 255 : (int)t) : 0;
}
__device__ inline int tile_index(int16_t v, int16_t c, bool relative) {
  const int t = relative ? ((int)v - (int)c) + 7 : (int)v;
  return t < 0 ? 0 : (t > 255 ? 255 : t);
}

// A row's 675 indices into s_idx, and to idx_row when it is not NULL, by kFwdThreads threads.
template <typename T>
__device__ inline void tile_row_indices(const T* __restrict__ row, int tid, uint8_t* s_idx, uint8_t* __restrict__ idx_row) {
  const T c0 = row[kCentre * kF], c1 = row[kCentre * kF + 1];
  for (int e = tid; e < kRowIdx; e += kFwdThreads) {
    const int f = e % kF;
    const int i = tile_index(row[e], f == 0 ? c0 : c1, f < 2);
    s_idx[e] = (uint8_t)i;
    if (idx_row) idx_row[e] = (uint8_t)i;
  }
}

// A row's a1 = relu(conv1(embed(tile))) [32][169] into s_out from its indices in s_idx, by
// kFwdThreads threads: 8 lanes share a position, lane oq with channels 4 oq .. 4 oq + 3 (table4 is
// the table + oq, b4 the bias's float4 oq), and add in §19's order.
__device__ inline void tile_row_a1(const uint8_t* s_idx, const float4* __restrict__ table4, float4 b4, int oq, int slot,
                                   float* s_out) {
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
    tile_row_indices(tile + n * tile_stride, tid, s_idx, idx_out ? idx_out + n * kRowIdx : nullptr);
    __syncthreads();
    tile_row_a1(s_idx, table4, b4, oq, slot, s_out);
    __syncthreads();
    float* __restrict__ orow = out + n * kRowOut;
    for (int i = tid; i < kRowOut; i += kFwdThreads) orow[i] = s_out[i];
    // no third barrier: the next row's s_idx writes come after this row's last s_idx read (the
    // barrier above), and its s_out writes after its own first barrier, which every thread
    // reaches only after these reads of s_out
  }
}

// SPEC §22 forward: a1 stays in LDS and tile_conv_2 + ReLU run on it. Thread (g, p2) adds the 288
// terms of out2[4 g + j][p2], j < 4, in the order c, ky, kx, each one multiply and one add; g is
// uniform over a wave, so W2[4 g + j][c][.][.] is read by scalar loads.
template <typename T>
__global__ __launch_bounds__(kFwdThreads) void nmh_tile2_forward_kernel(
    int n_rows, const T* __restrict__ tile, int64_t tile_stride, const float* __restrict__ table,
    const float* __restrict__ bias1, const float* __restrict__ w2, const float* __restrict__ bias2,
    float* __restrict__ out2, uint8_t* __restrict__ idx_out) {
  __shared__ uint8_t s_idx[kRowIdx + 1];
  __shared__ float s_a1[kRowOut];
  const int tid = threadIdx.x;
  const int oq = tid & 7, slot = tid >> 3;
  const float4 b4 = reinterpret_cast<const float4*>(bias1)[oq];
  const float4* __restrict__ table4 = reinterpret_cast<const float4*>(table) + oq;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 7);  // channels 4 g .. 4 g + 3
  const int p2 = tid & 127, pc = p2 < kP2 ? p2 : kP2 - 1;   // lanes 121..127 compute position 120 again and store nothing
  const int y2 = pc / kOut2Side, x2 = pc - y2 * kOut2Side;
  const float* a = s_a1 + y2 * kOutSide + x2;
  const float* __restrict__ wg = w2 + g * 4 * (kO * kK);
  const float4 bz = reinterpret_cast<const float4*>(bias2)[g];
  const int64_t row0 = (int64_t)blockIdx.x * kFwd2Rows;
  for (int r = 0; r < kFwd2Rows; ++r) {
    const int64_t n = row0 + r;
    if (n >= n_rows) break;  // uniform over the workgroup
    tile_row_indices(tile + n * tile_stride, tid, s_idx, idx_out ? idx_out + n * kRowIdx : nullptr);
    __syncthreads();
    tile_row_a1(s_idx, table4, b4, oq, slot, s_a1);
    __syncthreads();
    float z0 = bz.x, z1 = bz.y, z2 = bz.z, z3 = bz.w;
    for (int c = 0; c < kO; ++c) {
      const float* ac = a + c * kP;
      const float* __restrict__ wc = wg + c * kK;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float v = ac[ky * kOutSide + kx];
          const int k = ky * 3 + kx;
          z0 += wc[k] * v;
          z1 += wc[kO * kK + k] * v;
          z2 += wc[2 * kO * kK + k] * v;
          z3 += wc[3 * kO * kK + k] * v;
        }
      }
    }
    if (p2 < kP2) {
      float* __restrict__ orow = out2 + n * kRowOut2 + (4 * g) * kP2 + p2;  // 64 and 57 consecutive floats per wave and channel
      orow[0] = fmaxf(z0, 0.0f);
      orow[kP2] = fmaxf(z1, 0.0f);
      orow[2 * kP2] = fmaxf(z2, 0.0f);
      orow[3 * kP2] = fmaxf(z3, 0.0f);
    }
    // no third barrier, as above: the next row's s_a1 writes come after its first barrier, which
    // every thread reaches after its own reads of s_a1
  }
}

// SPEC §22 backward, stage 1: part `blockIdx.x` of rows. Per row: indices and dz2 into LDS, a1
// recomputed, the gated dz1 row stored, the row added to the part's g_W2 and g_b2, which are stored
// once at the end (zeros for an empty part). The `unroll 1` loops keep the kernel at 130 VGPRs,
// three workgroups per CU; unrolled it took 258.
__global__ __launch_bounds__(kFwdThreads) void nmh_tile2_backward_kernel(
    int n_rows, int rows_per_part, const uint8_t* __restrict__ idx, const float* __restrict__ out2,
    const float* __restrict__ g_out2, const float* __restrict__ table, const float* __restrict__ bias1,
    const float* __restrict__ w2, float* __restrict__ dz1, float* __restrict__ g_w2_parts,
    float* __restrict__ g_bias2_parts) {
  __shared__ uint8_t s_idx[kRowIdx + 1];
  __shared__ float s_a1[kRowOut];
  __shared__ float s_dz2[kO2 * kPad];  // [o2][15][15]: dz2[o2][y][x] at (y + 2, x + 2), zeros around it
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int oq = tid & 7, slot = tid >> 3;
  const float4 b4 = reinterpret_cast<const float4*>(bias1)[oq];
  const float4* __restrict__ table4 = reinterpret_cast<const float4*>(table) + oq;
  const int o2 = tid >> 5, c = tid & 31;  // the owner of g_W2[o2][c][.][.]
  const int64_t lo = (int64_t)blockIdx.x * rows_per_part;
  const int64_t hi = lo + rows_per_part < n_rows ? lo + rows_per_part : n_rows;
  for (int i = tid; i < kO2 * kPad; i += kFwdThreads) s_dz2[i] = 0.0f;  // the border stays zero
  float gw[kK] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float gb = 0.0f;
  for (int64_t n = lo; n < hi; ++n) {
    __syncthreads();  // the previous row's readers of s_idx, s_a1 and s_dz2 are done
    const uint8_t* __restrict__ irow = idx + n * kRowIdx;
    for (int e = tid; e < kRowIdx; e += kFwdThreads) s_idx[e] = irow[e];
    const float* __restrict__ orow = out2 + n * kRowOut2;
    const float* __restrict__ grow = g_out2 + n * kRowOut2;
    for (int i = tid; i < kRowOut2; i += kFwdThreads) {
      const int o = i / kP2, p = i - o * kP2;
      const int y = p / kOut2Side, x = p - y * kOut2Side;
      s_dz2[o * kPad + (y + 2) * kPadSide + x + 2] = orow[i] > 0.0f ? grow[i] : 0.0f;
    }
    __syncthreads();
    tile_row_a1(s_idx, table4, b4, oq, slot, s_a1);
    __syncthreads();
    // dz1[c1][p] = (a1[c1][p] > 0) * sum over o2, ky, kx in that order of W2[o2][c1][ky][kx] *
    // dz2[o2][y - ky][x - kx], the taps outside the 11 x 11 output reading the zero border
    float* __restrict__ drow = dz1 + n * kRowOut;
#pragma unroll 1
    for (int ci = 0; ci < kO / 4; ++ci) {
      const int c1 = wave + 4 * ci;  // wave-uniform: W2 by scalar loads
      const float* __restrict__ wc = w2 + c1 * kK;
#pragma unroll 1
      for (int q = 0; q < 3; ++q) {
        const int p = lane + 64 * q;
        if (p < kP) {
          const int y = p / kOutSide, x = p - y * kOutSide;
          const float* d = s_dz2 + (y + 2) * kPadSide + x + 2;
          float s = 0.0f;
#pragma unroll
          for (int o = 0; o < kO2; ++o) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
              for (int kx = 0; kx < 3; ++kx)
                s += wc[o * (kO * kK) + ky * 3 + kx] * d[o * kPad - ky * kPadSide - kx];
            }
          }
          drow[c1 * kP + p] = s_a1[c1 * kP + p] > 0.0f ? s : 0.0f;
        }
      }
    }
    // g_W2[o2][c][ky][kx] += sum over y, x ascending of dz2[o2][y][x] * a1[c][y + ky][x + kx]
    const float* d = s_dz2 + o2 * kPad + 2 * kPadSide + 2;
    const float* ac = s_a1 + c * kP;
    float row_sum = 0.0f;  // g_b2: a line's 11 values, then the row's 11 lines, then the part's rows
#pragma unroll 1
    for (int y = 0; y < kOut2Side; ++y) {
      float line_sum = 0.0f;
      float rows[3][kOutSide];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int x = 0; x < kOutSide; ++x) rows[ky][x] = ac[(y + ky) * kOutSide + x];
      }
#pragma unroll
      for (int x = 0; x < kOut2Side; ++x) {
        const float v = d[y * kPadSide + x];
        line_sum += v;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) gw[ky * 3 + kx] += v * rows[ky][x + kx];
        }
      }
      row_sum += line_sum;
    }
    gb += row_sum;
  }
  float* __restrict__ gp = g_w2_parts + (int64_t)blockIdx.x * kW2 + (o2 * kO + c) * kK;
#pragma unroll
  for (int k = 0; k < kK; ++k) gp[k] = gw[k];
  if (c == 0) g_bias2_parts[(int64_t)blockIdx.x * kO2 + o2] = gb;
}

// kGated: g_out is dz itself (stage 2 of SPEC §22's backward) and `out` is not read.
template <bool kGated>
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
        if constexpr (!kGated) po[u] = orow[i];
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
      if (i < kQuads) {
        if constexpr (kGated)
          reinterpret_cast<float4*>(s_dz)[i] = make_float4(pg[u].x, pg[u].y, pg[u].z, pg[u].w);
        else
          reinterpret_cast<float4*>(s_dz)[i] =
              make_float4(po[u].x > 0.0f ? pg[u].x : 0.0f, po[u].y > 0.0f ? pg[u].y : 0.0f,
                          po[u].z > 0.0f ? pg[u].z : 0.0f, po[u].w > 0.0f ? pg[u].w : 0.0f);
      }
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

}  // namespace

extern "C" {

int nmh_tile_forward(int32_t n_rows, const void* tile, int64_t tile_stride, int32_t tile_kind, const float* table,
                     const float* bias, float* out, uint8_t* idx_out, void* stream) {
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "nmh_tile_forward: n_rows %d is negative", n_rows);
  if (!tile) return heads_fail(NMH_E_INVALID, "nmh_tile_forward: tile is NULL");
  if (!table) return heads_fail(NMH_E_INVALID, "nmh_tile_forward: table is NULL");
  if (!bias) return heads_fail(NMH_E_INVALID, "nmh_tile_forward: bias is NULL");
  if (!out) return heads_fail(NMH_E_INVALID, "nmh_tile_forward: out is NULL");
  if (tile_kind != NMH_TILE_F32 && tile_kind != NMH_TILE_I16)
    return heads_fail(NMH_E_INVALID, "nmh_tile_forward: unknown tile_kind %d", tile_kind);
  if (tile_stride < kRowIdx)
    return heads_fail(NMH_E_INVALID, "nmh_tile_forward: tile_stride %lld < %d", (long long)tile_stride, kRowIdx);
  if (!aligned16(table) || !aligned16(bias))
    return heads_fail(NMH_E_INVALID, "nmh_tile_forward: table or bias is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kFwdRows - 1) / kFwdRows)), block(kFwdThreads);
  if (tile_kind == NMH_TILE_F32)
    hipLaunchKernelGGL(nmh_tile_forward_kernel<float>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const float*>(tile), tile_stride, table, bias, out, idx_out);
  else
    hipLaunchKernelGGL(nmh_tile_forward_kernel<int16_t>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const int16_t*>(tile), tile_stride, table, bias, out, idx_out);
  return heads_launched("nmh_tile_forward");
}

int nmh_tile_backward(int32_t n_rows, const uint8_t* idx, const float* out, const float* g_out, int32_t n_chunks,
                      float* g_table_parts, float* g_bias_parts, void* stream) {
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "nmh_tile_backward: n_rows %d is negative", n_rows);
  if (!idx) return heads_fail(NMH_E_INVALID, "nmh_tile_backward: idx is NULL");
  if (!out) return heads_fail(NMH_E_INVALID, "nmh_tile_backward: out is NULL");
  if (!g_out) return heads_fail(NMH_E_INVALID, "nmh_tile_backward: g_out is NULL");
  if (!g_table_parts || !g_bias_parts)
    return heads_fail(NMH_E_INVALID, "nmh_tile_backward: g_table_parts or g_bias_parts is NULL");
  if (n_chunks < 1 || n_chunks > NMH_TILE_MAX_CHUNKS)
    return heads_fail(NMH_E_INVALID, "nmh_tile_backward: n_chunks %d outside 1..%d", n_chunks, NMH_TILE_MAX_CHUNKS);
  if (!aligned16(out) || !aligned16(g_out))
    return heads_fail(NMH_E_INVALID, "nmh_tile_backward: out or g_out is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const int rows_per_chunk = (int)(((int64_t)n_rows + n_chunks - 1) / n_chunks);
  hipLaunchKernelGGL(nmh_tile_backward_kernel<false>, dim3((unsigned)(n_chunks * kSlices)), dim3(kBwdThreads), 0,
                     static_cast<hipStream_t>(stream), n_rows, rows_per_chunk, idx, out, g_out, g_table_parts,
                     g_bias_parts);
  return heads_launched("nmh_tile_backward");
}

int nmh_tile2_forward(int32_t n_rows, const void* tile, int64_t tile_stride, int32_t tile_kind, const float* table,
                      const float* bias1, const float* w2, const float* bias2, float* out2, uint8_t* idx_out,
                      void* stream) {
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: n_rows %d is negative", n_rows);
  if (!tile) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: tile is NULL");
  if (!table) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: table is NULL");
  if (!bias1) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: bias1 is NULL");
  if (!w2) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: w2 is NULL");
  if (!bias2) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: bias2 is NULL");
  if (!out2) return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: out2 is NULL");
  if (tile_kind != NMH_TILE_F32 && tile_kind != NMH_TILE_I16)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: unknown tile_kind %d", tile_kind);
  if (tile_stride < kRowIdx)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: tile_stride %lld < %d", (long long)tile_stride, kRowIdx);
  if (!aligned16(table) || !aligned16(bias1) || !aligned16(w2) || !aligned16(bias2))
    return heads_fail(NMH_E_INVALID, "nmh_tile2_forward: table, bias1, w2 or bias2 is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const dim3 grid((unsigned)((n_rows + kFwd2Rows - 1) / kFwd2Rows)), block(kFwdThreads);
  if (tile_kind == NMH_TILE_F32)
    hipLaunchKernelGGL(nmh_tile2_forward_kernel<float>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const float*>(tile), tile_stride, table, bias1, w2, bias2, out2, idx_out);
  else
    hipLaunchKernelGGL(nmh_tile2_forward_kernel<int16_t>, grid, block, 0, static_cast<hipStream_t>(stream), n_rows,
                       static_cast<const int16_t*>(tile), tile_stride, table, bias1, w2, bias2, out2, idx_out);
  return heads_launched("nmh_tile2_forward");
}

int nmh_tile2_backward(int32_t n_rows, const uint8_t* idx, const float* out2, const float* g_out2, const float* table,
                       const float* bias1, const float* w2, int32_t n_table_chunks, int32_t n_w2_parts,
                       float* dz1_scratch, float* g_table_parts, float* g_bias1_parts, float* g_w2_parts,
                       float* g_bias2_parts, void* stream) {
  if (n_rows < 0) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: n_rows %d is negative", n_rows);
  if (!idx) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: idx is NULL");
  if (!out2) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: out2 is NULL");
  if (!g_out2) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: g_out2 is NULL");
  if (!table) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: table is NULL");
  if (!bias1) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: bias1 is NULL");
  if (!w2) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: w2 is NULL");
  if (!dz1_scratch) return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: dz1_scratch is NULL");
  if (!g_table_parts || !g_bias1_parts)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: g_table_parts or g_bias1_parts is NULL");
  if (!g_w2_parts || !g_bias2_parts)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: g_w2_parts or g_bias2_parts is NULL");
  if (n_table_chunks < 1 || n_table_chunks > NMH_TILE_MAX_CHUNKS)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: n_table_chunks %d outside 1..%d", n_table_chunks,
                      NMH_TILE_MAX_CHUNKS);
  if (n_w2_parts < 1 || n_w2_parts > NMH_TILE2_MAX_PARTS)
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: n_w2_parts %d outside 1..%d", n_w2_parts,
                      NMH_TILE2_MAX_PARTS);
  if (!aligned16(table) || !aligned16(bias1) || !aligned16(w2))
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: table, bias1 or w2 is not 16-byte aligned");
  if (!aligned16(dz1_scratch))
    return heads_fail(NMH_E_INVALID, "nmh_tile2_backward: dz1_scratch is not 16-byte aligned");
  if (n_rows == 0) return NMH_OK;
  const int rows_per_part = (int)(((int64_t)n_rows + n_w2_parts - 1) / n_w2_parts);
  hipLaunchKernelGGL(nmh_tile2_backward_kernel, dim3((unsigned)n_w2_parts), dim3(kFwdThreads), 0,
                     static_cast<hipStream_t>(stream), n_rows, rows_per_part, idx, out2, g_out2, table, bias1, w2,
                     dz1_scratch, g_w2_parts, g_bias2_parts);
  const int rc = heads_launched("nmh_tile2_backward");
  if (rc != NMH_OK) return rc;
  const int rows_per_chunk = (int)(((int64_t)n_rows + n_table_chunks - 1) / n_table_chunks);
  hipLaunchKernelGGL(nmh_tile_backward_kernel<true>, dim3((unsigned)(n_table_chunks * kSlices)), dim3(kBwdThreads), 0,
                     static_cast<hipStream_t>(stream), n_rows, rows_per_chunk, idx, static_cast<const float*>(nullptr),
                     static_cast<const float*>(dz1_scratch), g_table_parts, g_bias1_parts);
  return heads_launched("nmh_tile2_backward");
}

}  // extern "C"
