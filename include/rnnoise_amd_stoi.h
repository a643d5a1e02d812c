/* rnnoise_amd_stoi.h -- librnnoise_amd_stoi.so: STOI and ESTOI of denoised audio against the clean signal, on the device.
 *
 * A library of its own beside the product and the other side libraries (it links none of them and none links it): five kernels,
 * rn_stoi_resample_kernel, rn_stoi_keep_kernel, rn_stoi_bands_kernel, rn_stoi_segments_kernel and rn_stoi_sum_kernel, and the four
 * calls below.  It reads three float32 PCM planes at 48 kHz through device pointers -- ref (clean), in (noisy, may be absent), out
 * (denoised) -- and writes eight doubles per sequence: the sums over segments of the short-time objective intelligibility measure
 * (Taal et al. 2011) and of its extended form (Jensen and Taal 2016), for in against ref and for out against ref, with the counts
 * that turn them into means.  rnnoise_amd/stoi.py binds it; tests/stoi_ref.py restates the definition below in numpy float64.
 *
 * The constants are the published algorithm's; the numbers are NOT bit-compatible with any published implementation, because the
 * 48 -> 10 kHz resampler is this project's own.
 *
 * PLANES.  As in rnnoise_amd_score.h: sample i of frame t of row (sequence) s of a plane lies at
 * p[t * frame_stride + s * row_stride + i], strides in floats; pointers 16-byte aligned, strides multiples of 4 and at least 480.
 * A plane holds its sequence from frame 0 to frame n_frames - 1.  in.p may be NULL (its strides are then not looked at).  The
 * planes are only read and may be the same memory.
 *
 * DEFINITION.  All arithmetic after the float32 loads is IEEE double, one rounding per operation, no fused multiply-add.
 * eps = 2^-52.
 *   Span.  The scored samples of a row are the output samples n of [first * 480, n_frames * 480); degraded (in / out) sample n is
 *     compared with ref sample n - delay -- in is read at n - delay too, as the score library reads it.  With
 *     L = (n_frames - first) * 480, x[0..L) is a signal's span; samples outside it count as 0.
 *   Resampling.  h[k], k = 0..2304, is a Kaiser-windowed sinc on the 240 kHz grid: beta = 0.1102 (75 - 8.7), cutoff 4750 Hz, unit
 *     DC gain (rnnoise_amd/stoi_tables.py holds the 2,305 doubles).  The 10 kHz signal is
 *         y[m] = 5 * sum_n h[1152 + 24 m - 5 n] * x[n],   m = 0 .. L10 - 1,  L10 = 5 L / 24 = 100 (n_frames - first)
 *   Frames.  Length 256, hop 128, window w = hanning(258)[1:-1]; F = floor((L10 - 256) / 128) + 1 frames (0 where L10 < 256).
 *   Silent frames.  e_j = 20 log10(||w * ref_frame_j|| + eps); frame j is kept where e_j > max_j e_j - 40.  The K kept frames,
 *     windowed, are overlap-added at hop 128 in their compact order -- the same indices for ref and for the degraded signal.
 *   STFT.  The compacted signals are cut again into M = K - 1 frames of 256 at hop 128, windowed with w and zero-padded to 512.
 *   Bands.  15 third-octave bands from 150 Hz, over the bins [a, b) of
 *         [7,9) [9,11) [11,14) [14,17) [17,22) [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138) [138,174) [174,219)
 *     X[b, j] = sqrt(sum |bin|^2).
 *   Segments.  One for every m = 30 .. M, of the columns m - 30 .. m - 1: K - 30 segments, none where K < 31.
 *   STOI term, x the ref and y the degraded segment, per band row over its 30 columns: alpha = ||x|| / (||y|| + eps);
 *     y' = min(alpha y, x (1 + 10^(15/20))); the row means are subtracted and the rows divided by (norm + eps); the term is the
 *     sum of the 450 products, divided by 15.
 *   ESTOI term: the rows of x and of y (unclipped) have their means subtracted and are divided by (norm + eps); then the columns
 *     of the results likewise; the term is the sum of the 450 products, divided by 30.
 *
 * ORDER -- every sum has one order, so two runs give the same bits whatever n_rows and the layout are.
 *   - Taps: y[m] is one accumulator from 0.0 over k = 1152 + 24 m - 5 n ascending (n descending), acc = acc + h[k] * x[n], all 461
 *     taps of the phase (zeros outside the span included); then 5 * acc.
 *   - Frame norms: one accumulator over i = 0..255 ascending of (w[i] * y[128 j + i])^2, then the square root.  The kernel compares
 *     (norm_j + eps) > (max norm + eps) * 0.01: the inequality of the definition without the logarithms; a frame within rounding of
 *     the threshold may fall on either side of it (tests/stoi_ref.py reports each row's margin).  A NaN norm makes the maximum NaN,
 *     and then no frame is kept.
 *   - Overlap-add: a compacted sample is (the term of the lower kept frame) + (that of the higher).
 *   - Transform: every frame of every signal has a transform of its own, so nothing of one signal reaches another's spectrum and
 *     an all-zero frame has an all-zero spectrum.  The 512 real samples go as 256 complex points z[j] = x[2 j] + i x[2 j + 1]
 *     through a radix-2 decimation-in-time FFT; with E[k] = (Z[k] + conj Z[256 - k]) / 2 and O[k] = (Z[k] - conj Z[256 - k]) / 2i,
 *     bin k is E[k] + exp(-2 pi i k / 512) O[k].
 *   - Band sums: |bin|^2 = re * re + im * im, one accumulator over the bins ascending.
 *   - 30-column sums (norms, means, products of a band row): one accumulator over the columns ascending; the 15 row results are then
 *     added in ascending band order.  ESTOI's column sums run over the bands ascending, and the 30 column results are added in
 *     ascending column order.
 *   - Segments: one accumulator per sum over m ascending.
 *   A NaN or an infinity stays in its row.
 *
 * RESULTS.  results[n_rows][RNNOISE_AMD_STOI_SLOTS] doubles, WRITTEN (not added to):
 *     0: sum of the STOI terms, in / ref    1: sum of the ESTOI terms, in / ref    2: segments    3: kept frames K
 *     4: sum of the STOI terms, out / ref   5: sum of the ESTOI terms, out / ref   6: segments    7: kept frames K
 *   Slots 0 to 3 are zeros where in.p is NULL.  STOI is slot 0 / slot 2, and so on; a row with K < 31 has 0 segments and sums 0.0.
 *
 * LIMITS.  n_rows <= RNNOISE_AMD_STOI_MAX_ROWS, n_frames <= RNNOISE_AMD_STOI_MAX_FRAMES.
 */
#ifndef RNNOISE_AMD_STOI_H
#define RNNOISE_AMD_STOI_H

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

#define RNNOISE_AMD_STOI_FRAME 480        /* samples of a frame, 10 ms at 48 kHz */
#define RNNOISE_AMD_STOI_SLOTS 8          /* doubles of a row of results */
#define RNNOISE_AMD_STOI_MAX_ROWS 32768   /* largest n_rows */
#define RNNOISE_AMD_STOI_MAX_FRAMES 8192  /* largest n_frames */

typedef struct RNNoiseStoiPlane {
  const float *p;
  long frame_stride, row_stride; /* floats */
} RNNoiseStoiPlane;

typedef struct RNNoiseStoi {
  RNNoiseStoiPlane ref, in, out; /* in.p may be NULL */
  int n_rows;   /* 1 .. RNNOISE_AMD_STOI_MAX_ROWS */
  int n_frames; /* the whole sequence, T: 0 .. RNNOISE_AMD_STOI_MAX_FRAMES */
  int first;    /* frames below it are not scored; 0 <= first <= n_frames and first * 480 >= delay */
  int delay;    /* samples, >= 0 */
} RNNoiseStoi;

/* Host only: 0 when the two calls below accept *call, -1 when they refuse it: a NULL call, a NULL ref.p or out.p, a plane pointer
 * that is not 16-byte aligned, a stride below 480 or no multiple of 4, n_rows or n_frames outside the limits, a negative first or
 * delay, first > n_frames, first * 480 < delay, or a plane whose last slot lies beyond LONG_MAX floats.  Nothing is dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_stoi_check(const RNNoiseStoi *call);

/* Host only: the bytes of scratch the device form needs for n_rows rows of n_frames frames (whatever first is), or -1 outside the
 * limits.  With C = 100 * n_frames and G = C < 256 ? 0 : (C - 256) / 128 + 1:
 *     n_rows * (8 * (3 * C + 50 * G) + 4 * (G + G % 2) + 8)
 * -- the three 10 kHz signals, and per frame a norm, 3 x 15 band envelopes, 4 segment terms and an index; 5.4 MB a row at 2,000
 * frames. */
RNNOISE_EXPORT long long rnnoise_amd_stoi_workspace(int n_rows, int n_frames);

/* Device form: every pointer is memory of HIP device `device`; asynchronous on hip_stream (a hipStream_t, NULL: the default stream);
 * at most FIVE launches whatever n_frames is, no other work.  d_scratch: 8-byte aligned, scratch_bytes of it, at least
 * rnnoise_amd_stoi_workspace(n_rows, n_frames); its contents before and after the call mean nothing.  -1, with nothing launched,
 * where the check refuses, for a NULL d_results, a NULL or misaligned or too small scratch, and where the device cannot be
 * selected; 0 otherwise. */
RNNOISE_EXPORT int rnnoise_amd_stoi_device(int device, double *d_results, void *d_scratch, long long scratch_bytes,
                                           const RNNoiseStoi *call, void *hip_stream);

/* Host form: every pointer is host memory; synchronous.  The rows go through device memory in pieces whose PCM and scratch together
 * take at most 256 MiB (one row at least); the doubles are those of the device form. */
RNNOISE_EXPORT int rnnoise_amd_stoi(int device, double *results, const RNNoiseStoi *call);

#ifdef __cplusplus
}
#endif
#endif
