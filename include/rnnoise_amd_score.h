/* rnnoise_amd_score.h -- librnnoise_amd_score.so: denoised audio scored against the clean signal, on the device.
 *
 * A library of its own beside the product (librnnoise_amd.so links nothing of it and it links nothing of the product): one kernel,
 * rn_audio_score_kernel, and the three calls below.  It knows no batch: it reads three float32 PCM planes at 48 kHz through device
 * pointers -- ref (clean), in (noisy), out (denoised) -- and adds eight double-precision sums per sequence, from which
 * rnnoise_amd/audio_score.py computes SNR, SI-SDR and the segmental SNR.
 *
 * PLANES.  Sample i of frame t of row (sequence) s of a plane lies at  p[t * frame_stride + s * row_stride + i],  strides in floats:
 * the meaning rnnoise_batch_set_pcm_layout gives its strides (include/rnnoise_amd.h).  [T][N][480] -- what
 * rnnoise_batch_train_mix_device leaves and rnnoise_batch_process_device takes -- is (N * 480, 480); a stream-contiguous [N][T * 480]
 * tensor is (480, T * 480), padded rows (480, T * 480 + pad).  Every pointer is 16-byte aligned and every stride a multiple of 4 and
 * at least 480.  A plane holds its sequence from frame 0.  The planes are only read and may be the same memory.
 *
 * DELAY.  With n = t * 480 + i the sample index of a row, out sample n is compared with ref / in sample n - delay; delay is any
 * non-negative sample count.  The denoiser's own path has RNNOISE_AMD_SCORE_DELAY = 960: one frame from the delayed spectra (the
 * reference's src/denoise.c:478-502) and one from the overlap-add.
 *
 * WHAT IS SCORED.  The output frames t of [t0, t0 + n_frames) with t >= first.  first * 480 >= delay is required, so that every
 * scored sample has its ref / in sample.
 *
 * TERMS.  For every scored sample, with r, x, y the ref, in, out floats converted to double, slot k of a record takes
 *     0: r*r   1: x*x   2: y*y   3: x*r   4: y*r   5: (x-r)*(x-r)   6: (y-r)*(y-r)   7: 1.0
 *
 * ORDER -- part of the interface; tests/audio_score_ref.py restates it in numpy and the kernel is held to it bit for bit.
 *   - One wave of 64 lanes serves one row and walks its frames in ascending t.
 *   - Within a frame lane l takes the output samples i with (i >> 2) & 63 == l, in ascending i: the float4 granules l and l + 64.
 *     Lanes 0..55 get eight samples, lanes 56..63 four.
 *   - Each lane's eight accumulators start at 0.0 in every frame and take plain IEEE double multiplies, subtractions and adds, one
 *     rounding each, never a fused multiply-add:  acc[k] = acc[k] + term[k].
 *   - The lanes combine by a butterfly,  a = a + a[lane ^ m]  for m = 32, 16, 8, 4, 2, 1.  IEEE addition commutes, so every lane
 *     ends with the same eight doubles: the FRAME RECORD.
 *   - The row's eight totals start from sums[s][k] and become  total = total + frame record,  frame after frame; they are stored once.
 *   The order is defined on OUTPUT sample indices, so the bits depend on neither the delay's alignment nor the layout, and a sequence
 *   scored in several calls (cuts of [t0, t0 + n_frames)) gives the bits of one call.  A NaN or an infinity stays in its row.
 *
 * OUTPUTS.  sums[n_rows][RNNOISE_AMD_SCORE_SLOTS] doubles: the calls ADD to them -- zero them first.  frame_terms, or NULL:
 * [n_rows][terms_frames][RNNOISE_AMD_SCORE_SLOTS] doubles, terms_frames >= t0 + n_frames; the record of every scored frame is written
 * at its t, every other record is left untouched.
 */
#ifndef RNNOISE_AMD_SCORE_H
#define RNNOISE_AMD_SCORE_H

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

#define RNNOISE_AMD_SCORE_FRAME 480 /* samples of a frame, 10 ms at 48 kHz */
#define RNNOISE_AMD_SCORE_SLOTS 8   /* doubles of a record */
#define RNNOISE_AMD_SCORE_DELAY 960 /* samples by which rnnoise_batch_process* delays its input */

typedef struct RNNoiseAudioPlane {
  const float *p;
  long frame_stride, row_stride; /* floats */
} RNNoiseAudioPlane;

typedef struct RNNoiseAudioScore {
  RNNoiseAudioPlane ref, in, out;
  int n_rows;       /* >= 1 */
  int t0, n_frames; /* the output frames of this call: t0 >= 0, n_frames >= 0, t0 + n_frames representable */
  int first;        /* frames below it are not scored; first >= 0 and first * 480 >= delay */
  int delay;        /* samples, >= 0 */
  int terms_frames; /* frames of a row of frame_terms; read only with frame_terms, then >= t0 + n_frames */
} RNNoiseAudioScore;

/* Host only: 0 when the two calls below accept *call, -1 when they refuse it: a NULL call or plane, a plane pointer that is not
 * 16-byte aligned, a stride below 480 or no multiple of 4, n_rows < 1, a negative t0, n_frames, first or delay, t0 + n_frames beyond
 * INT_MAX, first * 480 < delay, or a plane whose last slot lies beyond LONG_MAX floats.  terms_frames is not looked at (the calls do,
 * where they get frame_terms).  Nothing is dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_audio_score_check(const RNNoiseAudioScore *call);

/* Device form: every pointer is memory of HIP device `device`; asynchronous on hip_stream (a hipStream_t, NULL: the default stream),
 * ONE launch whatever n_frames is.  -1, with nothing launched, where the check refuses, for a NULL d_sums, for terms_frames <
 * t0 + n_frames beside a d_frame_terms, and where the device cannot be selected; 0 otherwise, also when no frame is to be scored. */
RNNOISE_EXPORT int rnnoise_amd_audio_score_device(int device, double *d_sums, double *d_frame_terms, const RNNoiseAudioScore *call,
                                                  void *hip_stream);

/* Host form: every pointer is host memory; synchronous.  The rows go through device memory in pieces of at most 48 MiB of PCM (one
 * row at least), only the frames the call reads; the doubles are those of the device form. */
RNNOISE_EXPORT int rnnoise_amd_audio_score(int device, double *sums, double *frame_terms, const RNNoiseAudioScore *call);

#ifdef __cplusplus
}
#endif
#endif
