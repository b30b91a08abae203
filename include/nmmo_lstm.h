/*
 * nmmo_lstm.h — C-ABI of the fused LSTM recurrence (libnmmo_lstm.so).
 *
 * The reference's default learner is recurrent (train.py:65-71 wraps every policy in pufferlib's
 * Recurrent, an nn.LSTM between encoder and decoder; clean_pufferl.py:310-324 and :454-469 carry
 * its state). The input and recurrent GEMMs over whole batches stay with torch; what is here is the
 * recurrence itself: nml_cell, the gate math and state update of one step over any number of rows,
 * and nml_seq_forward / nml_seq_backward, a whole [T, B] window of one layer in one launch each.
 * The semantics are torch.nn.LSTM's, frozen in SPEC.md §17.
 *
 * Conventions (those of nmmo_ppo.h): every call returns 0 or a negative NML_E_* code and never
 * aborts; nml_last_error() returns a thread-local message. Argument errors are reported without
 * touching a GPU. Every buffer is a caller-owned DEVICE pointer to float32; work is enqueued on
 * `stream` (a hipStream_t, NULL = default stream) with no synchronisation and no allocation
 * inside. Tensors are dense and row-major in the shapes given. B == 0 is a successful no-op.
 */
#ifndef NMMO_LSTM_H
#define NMMO_LSTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NML_API __attribute__((visibility("default")))

#define NML_OK 0
#define NML_E_INVALID (-1) /* bad argument */
#define NML_E_HIP (-2)     /* HIP runtime error */

/* The hidden size H must be a multiple of NML_H_STEP in NML_H_STEP..NML_MAX_H. */
#define NML_H_STEP 64
#define NML_MAX_H 1024
#define NML_MAX_B 16777216 /* 2^24 rows per call */
#define NML_MAX_T 4096     /* steps per window */
/* Batch rows one workgroup of the sequence kernels owns (a test shape, not a contract). */
#define NML_ROWS 4

/* One step, elementwise over [B, H]. Gate order i, f, g, o along the 4H axis.
 *   pre = ga + b_ih + gb + b_hh   (left to right; a NULL gb, b_ih or b_hh is left out)
 *   i, f, o = sigmoid(pre), g = tanh(pre);  c = f * c_prev + i * g;  h = o * tanh(c)
 * ga [B, 4H], gb [B, 4H] or NULL, b_ih / b_hh [4H] or NULL, c_prev [B, H].
 * h_out, c_out [B, H]; gates_out [B, 4H] or NULL gets the activated gates. Every element of every
 * output is stored. c_out may be c_prev, and gates_out may be ga: an element is read before the
 * same thread stores it. No other overlap is allowed. */
NML_API int nml_cell(int32_t B, int32_t H, const float* ga, const float* gb, const float* b_ih, const float* b_hh,
                     const float* c_prev, float* h_out, float* c_out, float* gates_out, void* stream);

/* One layer over a window of T steps, 1 <= T <= NML_MAX_T: for t = 0..T-1
 *   pre_t = xg[t] + b_ih + h_{t-1} * W_hh^T + b_hh, then the cell above.
 * xg [T, B, 4H] is x * W_ih^T. whh_t [H, 4H] is W_hh TRANSPOSED (the layout the kernel reads
 * coalesced). b_ih / b_hh [4H] or NULL. h0, c0 [B, H].
 * y [T, B, H] gets h_t; h_T, c_T [B, H] the last state; gates [T, B, 4H] the activated gates and
 * cs [T, B, H] the c_t, both for nml_seq_backward. Outputs must not overlap inputs. */
NML_API int nml_seq_forward(int32_t T, int32_t B, int32_t H, const float* xg, const float* whh_t, const float* b_ih,
                            const float* b_hh, const float* h0, const float* c0, float* y, float* h_T, float* c_T,
                            float* gates, float* cs, void* stream);

/* The reverse walk. dy [T, B, H], dh_T, dc_T [B, H]: the gradients of y, h_T, c_T. gates, cs as
 * nml_seq_forward left them, c0 as it got it, whh [4H, H] is W_hh as stored (not transposed).
 * dG [T, B, 4H] gets the gradient of pre_t; dh0, dc0 [B, H] that of h0, c0. The reductions over
 * rows (dW_hh = dG^T [h0; y_{:-1}], dW_ih = dG^T x, dx = dG W_ih, db = sum dG) are the caller's. */
NML_API int nml_seq_backward(int32_t T, int32_t B, int32_t H, const float* dy, const float* dh_T, const float* dc_T,
                             const float* gates, const float* cs, const float* c0, const float* whh, float* dG,
                             float* dh0, float* dc0, void* stream);

NML_API const char* nml_last_error(void);
/* "src=<hash of the sources the library was compiled from> arch=gfx950 fp_contract=off" */
NML_API const char* nml_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
