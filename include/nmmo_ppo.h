/*
 * nmmo_ppo.h — C-ABI of the fused PPO minibatch loss (libnmmo_ppo.so).
 *
 * Between the agent's forward and loss.backward() the reference trainer (clean_pufferl.py:476-523)
 * evaluates the clipped PPO objective as a chain of elementwise ops and full reductions over seven
 * vectors of one minibatch. nmp_loss computes that loss, its statistics and its gradients with
 * respect to the three vectors the agent produced in one gfx950 kernel launch. The semantics are
 * frozen in SPEC.md §16.
 *
 * Conventions (those of nmmo_hip.h): every call returns 0 or a negative NMP_E_* code and never
 * aborts; nmp_last_error() returns a thread-local message. Argument errors are reported without
 * touching a GPU. Every buffer is a caller-owned DEVICE pointer; work is enqueued on `stream`
 * (a hipStream_t, NULL = default stream) with no synchronisation and no allocation inside.
 */
#ifndef NMMO_PPO_H
#define NMMO_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMP_API __attribute__((visibility("default")))

#define NMP_OK 0
#define NMP_E_INVALID (-1) /* bad argument */
#define NMP_E_HIP (-2)     /* HIP runtime error */

#define NMP_MAX_N 16777216 /* 2^24 rows per call */

/* stats[NMP_N_OUT], float32. The first NMP_N_STATS are the per-minibatch statistics the trainer
 * averages; the last two are the advantage mean and (unbiased) std the normalisation used
 * (0 and 1 when norm_adv is off: none was applied). */
#define NMP_LOSS 0
#define NMP_PG_LOSS 1
#define NMP_V_LOSS 2
#define NMP_ENTROPY 3
#define NMP_OLD_APPROX_KL 4
#define NMP_APPROX_KL 5
#define NMP_CLIPFRAC 6
#define NMP_N_STATS 7
#define NMP_ADV_MEAN 7
#define NMP_ADV_STD 8
#define NMP_N_OUT 9

/* Coefficients of one call; each must be finite and >= 0. */
typedef struct NmpParams {
  double clip_coef;
  double vf_clip_coef;
  double ent_coef;
  double vf_coef;
  int32_t norm_adv;   /* != 0: advantages are normalised over the call's n rows */
  int32_t clip_vloss; /* != 0: the clipped value loss */
} NmpParams;

/* The seven inputs are float32 [n]. 0 <= n <= NMP_MAX_N, and n >= 2 when norm_adv is on; n == 0
 * is a no-op that writes nothing.
 *
 * loss[1] and stats[NMP_N_OUT] get the scalars (stats[NMP_LOSS] == *loss). g_newlogprob,
 * g_entropy, g_newvalue [n] get d loss / d newlogprob, entropy, newvalue; every entry is stored,
 * nothing past n is touched.
 *
 * accum: NULL, or float64 [NMP_N_STATS + 1] that the call adds to: accum[k] += stats[k] (the
 * float32 values, added in float64) for k < NMP_N_STATS and accum[NMP_N_STATS] += 1. The update
 * is a plain read, add and store by one thread: calls that share an accumulator must be ordered
 * (one stream). The caller zeroes it. */
NMP_API int nmp_loss(const NmpParams* params, int32_t n, const float* newlogprob, const float* entropy,
                     const float* newvalue, const float* old_logprob, const float* advantages,
                     const float* returns, const float* old_values, float* loss, float* stats,
                     float* g_newlogprob, float* g_entropy, float* g_newvalue, double* accum, void* stream);

NMP_API const char* nmp_last_error(void);
/* "src=<hash of the sources the library was compiled from> arch=gfx950 fp_contract=off" */
NMP_API const char* nmp_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
