// ppo.hip — libnmmo_ppo.so (include/nmmo_ppo.h): the PPO minibatch loss of the reference trainer
// (clean_pufferl.py:476-523), its statistics and its gradients in one launch. SPEC.md §16 holds
// the semantics and the closed-form gradients; DESIGN.md §3.13 the kernel notes.
//
// The workload is a minibatch of 1,024 rows: seven vectors of 4 KiB, bound by launch latency, so
// the whole call is ONE workgroup of 1,024 threads (16 waves) and every reduction stays inside
// it. Thread t owns rows t, t + 1024, ...; with n <= 1024 it loads its row once, up front, and
// keeps it in registers across the three dependent reductions (advantage sum -> squared
// deviations -> the six loss / statistic sums, reduced together behind one barrier). A reduction
// is a float64 DPP scan per wave, lane 63's total to LDS, and a serial sum of the 16 wave totals
// in wave order: no atomics, and an order that depends on n alone, so results are bit-identical
// from run to run. Elementwise terms are evaluated in float64 from the float32 inputs and every
// output is rounded to float32 once.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>

#include "host_api.h"
#include "../../include/nmmo_ppo.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kSums = 6;  // pg, v, entropy, old_kl, kl, clip count

// x + (the DPP-moved x), 0.0 where the move has no source (out of row, or a row the mask disables)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ double dpp_add(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, kRowMask, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, kRowMask, 0xF, false);
  return x + __hiloint2double(hi, lo);
}
// Sum over the 64 lanes of a wave (all lanes active), wave-uniform: the inclusive scan of
// common.h's wave_incl_scan on a double, read at lane 63.
__device__ __forceinline__ double wave_sum(double x) {
  x = dpp_add<0x111, 0xF>(x);  // row_shr:1
  x = dpp_add<0x112, 0xF>(x);  // row_shr:2
  x = dpp_add<0x114, 0xF>(x);  // row_shr:4
  x = dpp_add<0x118, 0xF>(x);  // row_shr:8
  x = dpp_add<0x142, 0xA>(x);  // row_bcast:15 -> rows 1, 3
  x = dpp_add<0x143, 0xC>(x);  // row_bcast:31 -> rows 2, 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 63),
                          __builtin_amdgcn_readlane(__double2loint(x), 63));
}

// Block sums of K values behind one barrier; buf rows are used by this call alone (no reuse, so
// no second barrier). Every thread gets every total, summed in wave order.
template <int K>
__device__ __forceinline__ void block_sums(double (&x)[K], double (*buf)[kWaves]) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const double s = wave_sum(x[k]);
    if (lane == 0) buf[k][w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) t += buf[k][i];
    x[k] = t;
  }
}

struct Row {
  float nlp, ent, v, olp, a, R, V;
};

struct Ptrs {
  const float *nlp, *ent, *v, *olp, *a, *R, *V;
};

__device__ __forceinline__ Row load_row(const Ptrs& in, int i) {
  return Row{in.nlp[i], in.ent[i], in.v[i], in.olp[i], in.a[i], in.R[i], in.V[i]};
}

__device__ __forceinline__ double clampd(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// kSmall: n <= kThreads, each thread holds at most one row in registers.
template <bool kSmall>
__global__ __launch_bounds__(kThreads) void nmp_loss_kernel(NmpParams p, int n, Ptrs in, float* __restrict__ loss,
                                                            float* __restrict__ stats, float* __restrict__ g_nlp,
                                                            float* __restrict__ g_ent, float* __restrict__ g_v,
                                                            double* __restrict__ accum) {
  __shared__ double red[2 + kSums][kWaves];
  const int tid = threadIdx.x;
  const double N = (double)n;
  Row mine{};  // zeros: a thread without a row adds nothing to any sum
  if (kSmall && tid < n) mine = load_row(in, tid);

  double mean = 0.0, sd = 1.0, scale = 1.0;
  if (p.norm_adv) {
    double s[1] = {0.0};
    if (kSmall) {
      s[0] = (double)mine.a;
    } else {
      for (int i = tid; i < n; i += kThreads) s[0] += (double)in.a[i];
    }
    block_sums(s, &red[0]);
    mean = s[0] / N;
    double q[1] = {0.0};
    if (kSmall) {
      const double d = (double)mine.a - mean;
      q[0] = tid < n ? d * d : 0.0;
    } else {
      for (int i = tid; i < n; i += kThreads) {
        const double d = (double)in.a[i] - mean;
        q[0] += d * d;
      }
    }
    block_sums(q, &red[1]);
    sd = sqrt(q[0] / (N - 1.0));
    scale = sd + 1e-8;
  }

  const double lo = 1.0 - p.clip_coef, hi = 1.0 + p.clip_coef, k = p.vf_clip_coef;
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto one = [&](const Row& r, int i) {
    const double lr = (double)r.nlp - (double)r.olp;
    const double ratio = exp(lr);
    acc[3] += -lr;
    acc[4] += (ratio - 1.0) - lr;
    acc[5] += fabs(ratio - 1.0) > p.clip_coef ? 1.0 : 0.0;
    const double A = p.norm_adv ? ((double)r.a - mean) / scale : (double)r.a;
    // policy: max(-A ratio, -A clamp(ratio)); a tie gives half the gradient to each side, the
    // clamp passes it on [lo, hi] inclusive
    const double p1 = -A * ratio, p2 = -A * clampd(ratio, lo, hi);
    acc[0] += fmax(p1, p2);
    const double w1 = p1 > p2 ? 1.0 : p1 == p2 ? 0.5 : 0.0;
    const bool inside = ratio >= lo && ratio <= hi;
    const double g_ratio = w1 * -A + (inside ? (1.0 - w1) * -A : 0.0);
    g_nlp[i] = (float)(g_ratio * ratio / N);
    // value
    const double du = (double)r.v - (double)r.R;
    const double u = du * du;
    double gv;
    if (p.clip_vloss) {
      const double d = (double)r.v - (double)r.V;
      const double dcl = ((double)r.V + clampd(d, -k, k)) - (double)r.R;
      const double cl = dcl * dcl;
      acc[1] += fmax(u, cl);
      const double wu = u > cl ? 1.0 : u == cl ? 0.5 : 0.0;
      const bool inside_v = d >= -k && d <= k;
      gv = wu * (2.0 * du) + (inside_v ? (1.0 - wu) * (2.0 * dcl) : 0.0);
    } else {
      acc[1] += u;
      gv = 2.0 * du;
    }
    g_v[i] = (float)(p.vf_coef * (0.5 * gv / N));
    acc[2] += (double)r.ent;
    g_ent[i] = (float)(-p.ent_coef / N);
  };
  if (kSmall) {
    if (tid < n) one(mine, tid);
  } else {
    for (int i = tid; i < n; i += kThreads) one(load_row(in, i), i);
  }
  block_sums(acc, &red[2]);

  if (tid == 0) {
    const double pg = acc[0] / N, vl = 0.5 * (acc[1] / N), ent = acc[2] / N;
    float out[NMP_N_OUT];
    out[NMP_LOSS] = (float)(pg - p.ent_coef * ent + vl * p.vf_coef);
    out[NMP_PG_LOSS] = (float)pg;
    out[NMP_V_LOSS] = (float)vl;
    out[NMP_ENTROPY] = (float)ent;
    out[NMP_OLD_APPROX_KL] = (float)(acc[3] / N);
    out[NMP_APPROX_KL] = (float)(acc[4] / N);
    out[NMP_CLIPFRAC] = (float)(acc[5] / N);
    out[NMP_ADV_MEAN] = (float)mean;
    out[NMP_ADV_STD] = (float)sd;
    *loss = out[NMP_LOSS];
#pragma unroll
    for (int j = 0; j < NMP_N_OUT; j++) stats[j] = out[j];
    if (accum) {  // launches on one stream are ordered: a plain read, add and store
#pragma unroll
      for (int j = 0; j < NMP_N_STATS; j++) accum[j] = accum[j] + (double)out[j];
      accum[NMP_N_STATS] = accum[NMP_N_STATS] + 1.0;
    }
  }
}

bool coef_ok(double c) { return std::isfinite(c) && c >= 0.0; }

}  // namespace

extern "C" {

const char* nmp_last_error(void) { return g_err.c_str(); }
const char* nmp_build_info(void) { return NMMO_BUILD_INFO; }

int nmp_loss(const NmpParams* params, int32_t n, const float* newlogprob, const float* entropy, const float* newvalue,
             const float* old_logprob, const float* advantages, const float* returns, const float* old_values,
             float* loss, float* stats, float* g_newlogprob, float* g_entropy, float* g_newvalue, double* accum,
             void* stream) {
  if (!params) return fail(NMP_E_INVALID, "nmp_loss: params is NULL");
  if (!coef_ok(params->clip_coef)) return fail(NMP_E_INVALID, "nmp_loss: clip_coef %g is negative or not finite", params->clip_coef);
  if (!coef_ok(params->vf_clip_coef))
    return fail(NMP_E_INVALID, "nmp_loss: vf_clip_coef %g is negative or not finite", params->vf_clip_coef);
  if (!coef_ok(params->ent_coef)) return fail(NMP_E_INVALID, "nmp_loss: ent_coef %g is negative or not finite", params->ent_coef);
  if (!coef_ok(params->vf_coef)) return fail(NMP_E_INVALID, "nmp_loss: vf_coef %g is negative or not finite", params->vf_coef);
  if (n < 0 || n > NMP_MAX_N) return fail(NMP_E_INVALID, "nmp_loss: n %d outside 0..%d", n, NMP_MAX_N);
  if (params->norm_adv && n == 1) return fail(NMP_E_INVALID, "nmp_loss: n 1 with norm_adv (the unbiased std needs n >= 2)");
  if (!newlogprob || !entropy || !newvalue || !old_logprob || !advantages || !returns || !old_values)
    return fail(NMP_E_INVALID, "nmp_loss: an input pointer is NULL");
  if (!loss || !stats || !g_newlogprob || !g_entropy || !g_newvalue)
    return fail(NMP_E_INVALID, "nmp_loss: an output pointer is NULL");
  if (n == 0) return NMP_OK;
  const Ptrs in{newlogprob, entropy, newvalue, old_logprob, advantages, returns, old_values};
  auto* kern = n <= kThreads ? nmp_loss_kernel<true> : nmp_loss_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), *params, n, in, loss, stats,
                     g_newlogprob, g_entropy, g_newvalue, accum);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NMP_OK : fail(NMP_E_HIP, "nmp_loss: launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
