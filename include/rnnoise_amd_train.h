/* rnnoise_amd_train.h -- librnnoise_amd_train.so: the reference trainer's loss with its gradient, on the device, in double.
 *
 * A library of its own beside the product (librnnoise_amd.so links nothing of it and it links nothing of the product): two kernels,
 * rn_train_loss_kernel and rn_train_loss_sums_kernel, and the three calls below.  It knows no batch and no network: it reads the
 * predictions of a network of the caller's and the 98-float training records where they lie, through device pointers and strides,
 * adds the loss's sums per row and writes the gradient of the loss with respect to the predictions.  rnnoise_amd/train_loss.py wraps
 * it as a torch.autograd.Function; rnnoise_amd/train.py trains with it.
 *
 * SLOTS.  Record t of row s lies at records[t * rec_frame_stride + s * rec_row_stride], 98 floats of which only the 33 targets
 * (floats 65 .. 97: 32 band gains, one VAD) are read; records holds the sequences from record 0.  The predictions of step t0 + f of
 * row s lie at gains[f * gain_frame_stride + s * gain_row_stride] (32 floats) and vad[f * vad_frame_stride + s * vad_row_stride]
 * (1 float): gains and vad hold the call's n_frames steps from step t0.  grad_gains and grad_vad are laid out as gains and vad.
 * Strides are in floats and explicit (no 0, 0 shorthand); they must keep the slots of a buffer apart, in one of the two orders
 * rnnoise_batch_set_pcm_layout knows (include/rnnoise_amd.h): rows within a frame, or frames within a row.
 *
 * ALIGNMENT AND TERMS are those of rnnoise_batch_score_records (include/rnnoise_amd.h, "Score calls" and "Feature calls"): step t is
 * scored against record t - 1 for t >= max(first, 1), so a call with t0 > 0 reads record t0 - 1; with g a band's gain target, v the
 * VAD target, p the predicted gain and q the predicted VAD, everything converted to double,
 *     tg = max(g, 0) * tanh(8 max(g, 0))^2,   m = min(g + 1, 1),   pw = p^gamma,   d = pw - tg^gamma
 *     gain term of a band   (1 + 5 v) m d^2
 *     VAD term of a frame   |2 v - 1| (-v log(.01 + q) - (1 - v) log(1.01 - q))
 *
 * SUMS.  sums[n_rows][4] doubles {gain terms, VAD terms, frames scored, 0}: the calls ADD to the first three -- zero them first -- and
 * leave the fourth alone.  A frame's 32 gain terms are summed by the butterfly a = a + a[lane ^ m], m = 16, 8, 4, 2, 1; a row's sums
 * then take  sum = sum + frame's value,  frame after frame in ascending t.  These are the expressions and the order of
 * rnnoise_batch_score_records_device (both libraries compile rnnoise_amd/csrc/eval_terms.h), so the doubles are those of that call on
 * the same buffers bit for bit, whatever the cut of the frames into calls.
 *
 * GRADIENTS, computed in double and rounded once to float; w_gain and w_vad are the weights of the two sums in the caller's loss
 * (the trainer's means: w_gain = 1 / (32 F), w_vad = .001 / F, F the scored frames of all rows):
 *     grad_gains = (float)(w_gain * 2 (1 + 5 v) m d gamma pw / p)       for p > 0
 *     grad_gains = 0                                                    for p <= 0 or a NaN p
 *     grad_vad   = (float)(w_vad * |2 v - 1| (-v / (.01 + q) + (1 - v) / (1.01 - q)))
 * For gamma < 1 the trainer's formula is infinite at p = 0 (pw / p) and not a number below it; this library gives 0 there, so that
 * a prediction a sigmoid has rounded to 0 stops moving instead of poisoning the step.  Steps of the call that are not scored
 * (t < max(first, 1)) get zeros.  With both gradient pointers NULL only the sums are computed.
 *
 * LAUNCHES.  Two per call, no atomics, no workgroup waits for another.  rn_train_loss_kernel: a grid over (row, block of
 * RNNOISE_AMD_TRAIN_FRAME_BLOCK steps), a wave per step at a time; it writes the gradients and the scored step's two doubles --
 * the butterfly's sum of the gain terms, the VAD term -- to frame_terms[n_rows][n_frames][2] at [s][f] (unscored steps are left
 * untouched).  rn_train_loss_sums_kernel: one lane per row adds the row's frame terms to sums in ascending f.
 */
#ifndef RNNOISE_AMD_TRAIN_H
#define RNNOISE_AMD_TRAIN_H

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

#define RNNOISE_AMD_TRAIN_RECORD 98      /* floats of a record: 65 features, 32 gain targets, 1 VAD target */
#define RNNOISE_AMD_TRAIN_BANDS 32
#define RNNOISE_AMD_TRAIN_SUMS 4         /* doubles of a row of sums */
#define RNNOISE_AMD_TRAIN_FRAME_BLOCK 16 /* steps of a workgroup of rn_train_loss_kernel */

typedef struct RNNoiseTrainLoss {
  const float *records;
  long rec_frame_stride, rec_row_stride;
  const float *gains;
  long gain_frame_stride, gain_row_stride;
  const float *vad;
  long vad_frame_stride, vad_row_stride;
  float *grad_gains, *grad_vad; /* laid out as gains / vad; both NULL: sums only */
  int n_rows, t0, n_frames, first;
  double gamma, w_gain, w_vad;
} RNNoiseTrainLoss;

/* Host only: 0 when the two calls below accept *call, -1 when they refuse it: a NULL call, records, gains or vad; n_rows < 1; a
 * negative t0, n_frames or first; t0 + n_frames beyond INT_MAX; a gamma that is not finite or not positive; a weight that is not
 * finite; one gradient pointer without the other; strides (non-positive ones among them) that let the slots of records (98 floats,
 * records 0 .. t0 + n_frames - 2), gains (32 floats) or vad (1 float, n_frames steps each) overlap.  Nothing is dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_train_loss_check(const RNNoiseTrainLoss *call);

/* Device form: every pointer is memory of HIP device `device`; asynchronous on hip_stream (a hipStream_t, NULL: the default stream),
 * two launches whatever n_frames is.  d_frame_terms is the caller's workspace of n_rows * n_frames * 2 doubles.  -1, with nothing
 * launched, where the check refuses, for a NULL d_sums or d_frame_terms, and where the device cannot be selected; 0 otherwise, also
 * when n_frames is 0. */
RNNOISE_EXPORT int rnnoise_amd_train_loss_device(int device, double *d_sums, double *d_frame_terms, const RNNoiseTrainLoss *call,
                                                 void *hip_stream);

/* Host form: every pointer is host memory; synchronous.  The buffers go up as they lie, the sums, the gradients and -- where
 * frame_terms is not NULL -- the frame terms come back; the doubles and floats are those of the device form. */
RNNOISE_EXPORT int rnnoise_amd_train_loss(int device, double *sums, double *frame_terms, const RNNoiseTrainLoss *call);

#ifdef __cplusplus
}
#endif
#endif
