/* rnnoise_amd_gru_stack.h -- librnnoise_amd_gru_stack.so: three chained float GRU layers over a sequence as one diagonal launch a step,
 * forward and backward, on the device.
 *
 * A library of its own beside the product, the score, train and gru libraries (it links nothing of them and they link nothing of
 * it): two kernels, rn_gru_stack_kernel and rn_gru_stack_grad_kernel, and the five calls below.  Layer 0's input projection stays the
 * caller's (one product over all steps); the projections of layers 1 and 2 run inside the step kernel, and the caller adds up the
 * weight gradients from what the backward call leaves.  rnnoise_amd/gru_stack.py wraps it as a torch.autograd.Function;
 * float_net.FloatNet(gru_impl="stack") runs its three GRUs through it.
 *
 * DEFINITIONS (torch's gate order r, z, n; H = hidden, N = n_rows, T = n_frames; layers l = 0, 1, 2; y_l[-1] = h0[l], zeros where it
 * is NULL; every weight matrix [3H][H] and every bias [3H], dense).  One layer is rnnoise_amd_gru.h's:
 *     gi_0[t] = gi0[t]                                   the caller's W_ih x + b_ih
 *     gi_l[t] = w_ih[l] . y_{l-1}[t] + b_ih[l]           l >= 1
 *     gh   = w_hh[l] . y_l[t-1] + b_hh[l]
 *     r    = sigmoid(gi_r + gh_r)
 *     z    = sigmoid(gi_z + gh_z)
 *     hn   = gh_n
 *     n    = tanh(gi_n + r hn)
 *     y_l[t] = (1 - z) n + z y_l[t-1]
 * saved[l][t][s][4H] = r, z, n, hn (H floats each) is what the backward call reads.  Backward, t = T-1 .. 0, dh_l starting as dhT[l]
 * (NULL: zeros):
 *     d    = dy[l][t]                                    l = 2
 *     d    = dy[l][t] + dx_{l+1}[t]                      l <= 1:  dx_{l+1}[t] = w_ih[l+1]^T . dgi_{l+1}[t]
 *     dh   = dh_l + d
 *     a_n  = dh (1 - z) (1 - n^2)
 *     a_z  = dh (y_l[t-1] - n) z (1 - z)
 *     a_r  = a_n hn r (1 - r)
 *     dgi_l[t] = [a_r, a_z, a_n]
 *     dgh_l[t] = [a_r, a_z, a_n r]
 *     dh_l = dh z + w_hh[l]^T . dgh_l[t]
 * and the last dh_l is dh0[l].  dW_hh[l] = sum_t dgh_l[t]^T y_l[t-1], db_hh[l] = sum dgh_l, and for l >= 1 dW_ih[l] = sum_t
 * dgi_l[t]^T y_{l-1}[t], db_ih[l] = sum dgi_l are the caller's: products and sums over all steps.
 *
 * THE ORDER OF EVERY SUM.  A workgroup of four waves owns 16 hidden units x 16 rows of one layer.  A product over k = 0 .. H-1 is cut
 * into the quarters w = 0 .. 3 of H/4 consecutive k; wave w adds its quarter with the exact float32 matrix instruction
 * (v_mfma_f32_16x16x4_f32) in ascending k, P_w.  Forward, with P^hh over y_l[t-1] and P^ih over y_{l-1}[t]:
 *     layer 0:  S_g = ((P^hh_0 + P^hh_1) + P^hh_2) + P^hh_3,   r = sigmoid(gi_r + (S_r + b_hh_r)), z likewise, hn = S_n + b_hh_n
 *     l >= 1:   Q_w = P^hh_w + P^ih_w for r and z,  S_g = ((Q_0 + Q_1) + Q_2) + Q_3,  r = sigmoid(S_r + (b_ih_r + b_hh_r)), z likewise;
 *               hn = S^hh_n + b_hh_n and gi_n = S^ih_n + b_ih_n are sums of their own (each ((P_0 + P_1) + P_2) + P_3)
 * Backward, a wave adds its quarter of the units u in ascending u, each gate a chain of its own, then P_w = (P_r + P_z) + P_n, and
 *     dh_l = dh z + (((P_0 + P_1) + P_2) + P_3),    dx_l[t] = ((P'_0 + P'_1) + P'_2) + P'_3   (P' over w_ih[l] and dgi_l)
 *     dh   = dh_l + (dy[l][t] + dx_{l+1}[t])
 * Nothing else is added anywhere, so the floats depend on neither N nor the cut of the steps into calls.  Rows are independent: what
 * one row holds never reaches another.
 *
 * SLOTS.  gi0, y[l], dy[l] and dgi[0] take a frame stride and a row stride in floats: slot (t, s) lies at t * frame_stride + s *
 * row_stride, so [T][N][.] and torch's batch-first [N][T][.] buffers are read and written where they lie, and the three y (or dy) may
 * be slices of one [N][T][4H] concatenation buffer.  Strides are explicit and must keep the slots of a buffer apart in one of the two
 * orders: rows within a frame, or frames within a row.  The kernels move four floats at a time: these pointers, the weights, h0, dhT,
 * dh0, saved, dgi[1..2], dgh and the scratch are 16-byte aligned (biases: 4-byte), and the strides are multiples of 4.  saved
 * [3][T][N][4H], dgi[1..2] and dgh[l] [T][N][3H], h0[l], dhT[l], dh0[l] [N][H] and the scratch are dense.  Two of the three y of a
 * forward call must be apart: either their extents (first to last float) do not meet, or they have the same strides and lie side by
 * side within one slot pitch (the concatenation buffer's case); anything else is refused.
 *
 * LAUNCHES.  Forward makes T + 2 plain launches from a loop inside the call: launch s runs layer l at step t = s - l where 0 <= t < T
 * (the grid holds the layers that have a step: (layers x H/16) x ceil(N/16) workgroups, the layer is blockIdx.x / (H/16) plus the
 * first live layer).  Backward is the mirror image: launch s runs layer 2 at t = T-1-s, layer 1 at t + 1, layer 0 at t + 2.  No
 * atomics, no workgroup waits for another, no graph, no persistent kernel: the kernel boundary is the only ordering.
 *
 * WHY ONE LAUNCH OF OFFSET PER LAYER SUFFICES.  Forward, layer l at step t reads y_l[t-1] and y_{l-1}[t]: both were written by launch
 * s - 1.  It writes y_l[t], which nobody reads in launch s: layer l + 1 reads y_l[t-1] there.  Backward, the gate gradients of layer
 * l need the complete dy[l][t] + dx_{l+1}[t].  A workgroup of layer l + 1 computes the dgi and dgh it feeds on the fly from saved, dh,
 * dy and y[t-1] (as the gru library's does for dgh) and from the same operands accumulates, beside w_hh^T dgh + dh z, a second result
 * dx_{l+1}[t] = w_ih[l+1]^T dgi_{l+1}[t] for its 16 units x 16 rows (the third gate takes a_n, not a_n r), and stores it into a dx
 * buffer; layer l reads it one launch later.  dx is read by all workgroups of layer l of a row tile while layer l + 1 writes the next
 * step's, so it alternates between two halves exactly as dh does.  The scratch is three dh pairs and two dx pairs: (3 + 2) 2 N H
 * floats.  dh0[l] may not overlap dhT[l].
 */
#ifndef RNNOISE_AMD_GRU_STACK_H
#define RNNOISE_AMD_GRU_STACK_H

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

#define RNNOISE_AMD_GRU_STACK_LAYERS 3        /* the depth of the chain: fixed */
#define RNNOISE_AMD_GRU_STACK_TILE 16         /* hidden units, and rows, of a workgroup; hidden is a multiple of it */
#define RNNOISE_AMD_GRU_STACK_MIN_HIDDEN 16   /* the range of hidden the kernels support */
#define RNNOISE_AMD_GRU_STACK_MAX_HIDDEN 4096
#define RNNOISE_AMD_GRU_STACK_MAX_ROWS 1048560 /* 16 * 65535: the row tiles are the grid's second dimension */

typedef struct RNNoiseGruStack {
  const float *gi0; /* slots of 3H floats: layer 0's input projection */
  long gi0_frame_stride, gi0_row_stride;
  const float *w_ih[3], *b_ih[3]; /* [1], [2]; [0] is not looked at */
  const float *w_hh[3], *b_hh[3];
  const float *h0[3]; /* [N][H] each, or NULL: zeros */
  float *y[3];        /* slots of H floats; y[l][T-1] is layer l's final state */
  long y_frame_stride[3], y_row_stride[3];
  int n_rows, n_frames, hidden;
} RNNoiseGruStack;

typedef struct RNNoiseGruStackGrad {
  const float *dy[3]; /* slots of H floats: the gradient with respect to each layer's output, apart from what the layer above adds */
  long dy_frame_stride[3], dy_row_stride[3];
  const float *y[3]; /* the forward call's outputs */
  long y_frame_stride[3], y_row_stride[3];
  const float *w_ih[3]; /* [1], [2]; [0] is not looked at */
  const float *w_hh[3];
  const float *h0[3];  /* the forward call's, or NULL */
  const float *dhT[3]; /* [N][H]: a gradient with respect to the final state beside dy[l][T-1], or NULL: zeros */
  float *dgi[3];       /* [0]: slots of 3H floats; [1], [2]: [T][N][3H] */
  long dgi0_frame_stride, dgi0_row_stride;
  float *dgh[3]; /* [T][N][3H] each */
  float *dh0[3]; /* [N][H] each */
  int n_rows, n_frames, hidden;
} RNNoiseGruStackGrad;

/* Host only: 0 when the forward call accepts *call, -1 when it refuses it: a NULL call, gi0, w_hh[l], b_hh[l], y[l], w_ih[1..2] or
 * b_ih[1..2]; n_rows < 1 or above RNNOISE_AMD_GRU_STACK_MAX_ROWS; n_frames < 0; hidden not a multiple of 16 or outside 16 .. 4096; a
 * pointer that is not 16-byte aligned (biases: 4-byte) or a stride that is not a multiple of 4; strides (non-positive ones among
 * them) that let the slots of gi0 or of a y[l] overlap; two y that are not apart (SLOTS above); sizes beyond LONG_MAX floats.
 * Nothing is dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_gru_stack_check(const RNNoiseGruStack *call);

/* Host only: the same for the backward call: a NULL call, dy[l], y[l], w_hh[l], w_ih[1..2], dgi[l], dgh[l] or dh0[l]; the counts,
 * alignment and strides as above (dy[l], y[l], dgi[0]); a dh0[l] that overlaps dhT[l]. */
RNNOISE_EXPORT int rnnoise_amd_gru_stack_grad_check(const RNNoiseGruStackGrad *call);

/* Host only: the floats of the two work buffers for the call's n_rows, n_frames and hidden (its pointers and strides are not looked
 * at): saved_floats = 3 * T * N * 4H, scratch_floats = (3 + 2) * 2 * N * H.  Either result pointer may be NULL.  -1 for a NULL call
 * or counts the check refuses. */
RNNOISE_EXPORT int rnnoise_amd_gru_stack_workspace(const RNNoiseGruStack *call, size_t *saved_floats, size_t *scratch_floats);

/* Forward: every pointer is memory of HIP device `device`; asynchronous on hip_stream (a hipStream_t, NULL: the default stream), T + 2
 * launches.  Writes y[0..2] and d_saved (saved_floats floats).  -1, with nothing launched, where the check refuses, for a NULL or
 * unaligned d_saved and where the device cannot be selected; 0 otherwise, also when n_frames is 0 (nothing is launched or written:
 * the final states of an empty call are the caller's h0). */
RNNOISE_EXPORT int rnnoise_amd_gru_stack_forward_device(int device, const RNNoiseGruStack *call, float *d_saved, void *hip_stream);

/* Backward: likewise, T + 2 launches from step T-1 down.  Reads d_saved as the forward call of the same sizes left it, writes dgi,
 * dgh and dh0, and uses d_scratch (scratch_floats floats) for dh and dx between steps.  -1, with nothing launched, where the check
 * refuses and for a NULL or unaligned d_saved or d_scratch; 0 otherwise, also when n_frames is 0 (nothing is written: dh0 of an empty
 * call is the caller's dhT). */
RNNOISE_EXPORT int rnnoise_amd_gru_stack_backward_device(int device, const RNNoiseGruStackGrad *call, const float *d_saved,
                                                         float *d_scratch, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
