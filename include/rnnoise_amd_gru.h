/* rnnoise_amd_gru.h -- librnnoise_amd_gru.so: the recurrence of a float GRU layer over a sequence, forward and backward, on the device.
 *
 * A library of its own beside the product, the score library and the train library (it links nothing of them and they link nothing of
 * it): two kernels, rn_gru_step_kernel and rn_gru_step_grad_kernel, and the five calls below.  It knows no network: the caller
 * computes the input projection of all steps as one product, this library runs what has to go step by step, and the caller adds up
 * the weight gradients from what the backward call leaves.  rnnoise_amd/gru_native.py wraps it as a torch.autograd.Function;
 * float_net.FloatNet(gru_impl="native") runs its three GRUs through it.
 *
 * DEFINITIONS (torch's gate order r, z, n; H = hidden, N = n_rows, T = n_frames; y[-1] = h0, zeros where h0 is NULL):
 *     gh   = w_hh . y[t-1] + b_hh                       w_hh [3H][H], b_hh [3H], dense
 *     r    = sigmoid(gi_r + gh_r)                       gi[t][s][3H] = W_ih x + b_ih, the caller's
 *     z    = sigmoid(gi_z + gh_z)
 *     hn   = gh_n
 *     n    = tanh(gi_n + r hn)
 *     y[t] = (1 - z) n + z y[t-1]
 * saved[t][s][4H] = r, z, n, hn (H floats each) is what the backward call reads.  Backward, t = T-1 .. 0, dh starting as dhT (NULL:
 * zeros):
 *     dh  += dy[t]
 *     a_n  = dh (1 - z) (1 - n^2)
 *     a_z  = dh (y[t-1] - n) z (1 - z)
 *     a_r  = a_n hn r (1 - r)
 *     dgi[t] = [a_r, a_z, a_n]
 *     dgh[t] = [a_r, a_z, a_n r]
 *     dh   = dh z + w_hh^T . dgh[t]
 * and the last dh is dh0.  dW_hh = sum_t dgh[t]^T y[t-1] and db_hh = sum dgh are the caller's: one product and one sum over all steps.
 *
 * SLOTS.  gi, y, dy and dgi take a frame stride and a row stride in floats: slot (t, s) lies at t * frame_stride + s * row_stride, so
 * both [T][N][.] and torch's batch-first [N][T][.] buffers are read and written where they lie.  Strides are explicit (no 0, 0
 * shorthand) and must keep the slots of a buffer apart in one of the two orders: rows within a frame, or frames within a row.
 * The kernels move four floats at a time: these four pointers, w_hh, h0, dhT, dh0, saved, dgh and the scratch are 16-byte aligned, and
 * the strides are multiples of 4 (H is a multiple of 16, so dense buffers are).  saved [T][N][4H], dgh [T][N][3H], h0, dhT, dh0
 * [N][H] and the scratch are dense.
 *
 * LAUNCHES.  One plain launch per step, issued by a loop inside the call: T launches forward, T backward, no atomics, no workgroup
 * waits for another, no graph.  A workgroup of four waves owns 16 hidden units x 16 rows; each wave takes a quarter of the sum with
 * the exact float32 matrix instruction (v_mfma_f32_16x16x4_f32) and the quarters are added through LDS in wave order, so the floats
 * depend on neither the cut of the steps into calls nor on N.  Rows are independent: what one row holds never reaches another.
 * The backward step reads the whole dh of the step before while it writes its own, so dh alternates between the two halves of the
 * scratch and is never updated in place; dh0 may not overlap dhT.
 */
#ifndef RNNOISE_AMD_GRU_H
#define RNNOISE_AMD_GRU_H

#include <stddef.h>

#ifndef RNNOISE_EXPORT
#if defined(__GNUC__)
#define RNNOISE_EXPORT __attribute__((visibility("default")))
#else
#define RNNOISE_EXPORT
#endif
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RNNOISE_AMD_GRU_TILE 16         /* hidden units, and rows, of a workgroup; hidden is a multiple of it */
#define RNNOISE_AMD_GRU_MIN_HIDDEN 16   /* the range of hidden the kernels support */
#define RNNOISE_AMD_GRU_MAX_HIDDEN 4096
#define RNNOISE_AMD_GRU_MAX_ROWS 1048560 /* 16 * 65535: the row tiles are the grid's second dimension */

typedef struct RNNoiseGruSeq {
  const float *gi; /* slots of 3H floats */
  long gi_frame_stride, gi_row_stride;
  const float *w_hh, *b_hh;
  const float *h0; /* [N][H], or NULL: zeros */
  float *y;        /* slots of H floats; y[T-1] is the final state */
  long y_frame_stride, y_row_stride;
  int n_rows, n_frames, hidden;
} RNNoiseGruSeq;

typedef struct RNNoiseGruSeqGrad {
  const float *dy; /* slots of H floats: the gradient with respect to y */
  long dy_frame_stride, dy_row_stride;
  const float *y; /* the forward call's output */
  long y_frame_stride, y_row_stride;
  const float *w_hh;
  const float *h0;  /* the forward call's, or NULL */
  const float *dhT; /* [N][H]: a gradient with respect to the final state beside dy[T-1], or NULL: zeros */
  float *dgi;       /* slots of 3H floats */
  long dgi_frame_stride, dgi_row_stride;
  float *dgh; /* [T][N][3H] */
  float *dh0; /* [N][H] */
  int n_rows, n_frames, hidden;
} RNNoiseGruSeqGrad;

/* Host only: 0 when the forward call accepts *call, -1 when it refuses it: a NULL call, gi, w_hh, b_hh or y; n_rows < 1 or above
 * RNNOISE_AMD_GRU_MAX_ROWS; n_frames < 0; hidden not a multiple of 16 or outside 16 .. 4096; a pointer that is not 16-byte aligned
 * (b_hh: 4-byte) or a stride that is not a multiple of 4; strides (non-positive ones among them) that let the slots of gi or y
 * overlap; sizes beyond LONG_MAX floats.  Nothing is dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_gru_check(const RNNoiseGruSeq *call);

/* Host only: the same for the backward call: a NULL call, dy, y, w_hh, dgi, dgh or dh0; the counts, alignment and strides as above
 * (dy, y, dgi); a dh0 that overlaps dhT. */
RNNOISE_EXPORT int rnnoise_amd_gru_grad_check(const RNNoiseGruSeqGrad *call);

/* Host only: the floats of the two work buffers for the call's n_rows, n_frames and hidden (its pointers and strides are not looked
 * at): saved_floats = T * N * 4H, scratch_floats = 2 * N * H.  Either result pointer may be NULL.  -1 for a NULL call or counts the
 * check refuses. */
RNNOISE_EXPORT int rnnoise_amd_gru_workspace(const RNNoiseGruSeq *call, size_t *saved_floats, size_t *scratch_floats);

/* Forward: every pointer is memory of HIP device `device`; asynchronous on hip_stream (a hipStream_t, NULL: the default stream), T
 * launches.  Writes y and d_saved (saved_floats floats).  -1, with nothing launched, where the check refuses, for a NULL d_saved and
 * where the device cannot be selected; 0 otherwise, also when n_frames is 0 (nothing is launched or written: the final state of an
 * empty call is the caller's h0). */
RNNOISE_EXPORT int rnnoise_amd_gru_forward_device(int device, const RNNoiseGruSeq *call, float *d_saved, void *hip_stream);

/* Backward: likewise, T launches from step T-1 down.  Reads d_saved as the forward call of the same sizes left it, writes dgi, dgh
 * and dh0, and uses d_scratch (scratch_floats floats) for dh between steps.  -1, with nothing launched, where the check refuses and
 * for a NULL d_saved or d_scratch; 0 otherwise, also when n_frames is 0 (nothing is written: dh0 of an empty call is the caller's
 * dhT). */
RNNOISE_EXPORT int rnnoise_amd_gru_backward_device(int device, const RNNoiseGruSeqGrad *call, const float *d_saved, float *d_scratch,
                                                   void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
