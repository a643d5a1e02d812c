/* rnnoise_amd_debug.h -- test and measurement taps.  NOT part of the product library: these entry points exist only in the
 * instrumented build (rnnoise_amd/librnnoise_amd_instr.so: the same sources compiled with -DRN_INSTRUMENT=1, which also
 * compiles the stage taps and shader-clock probes into the kernels, plus the probe kernels of csrc/fft_probe.hip).
 * librnnoise_amd.so / librnnoise.so.0 export the symbols of rnnoise.h and rnnoise_amd.h and nothing else. */
#ifndef RNNOISE_AMD_DEBUG_H
#define RNNOISE_AMD_DEBUG_H

#include "rnnoise_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pitch-analysis stage taps ([N][RN_DBG_FLOATS], layout rn_layout.h RN_DBG_*).  The first
 * call arms the taps (dst may be NULL); later calls copy the last step's record. Tests only. */
RNNOISE_EXPORT int rnnoise_batch_debug_pitch(RNNoiseBatch *b, float *dst);

/* Test tap: n independent 960-point transforms through the register-resident FFT of the analysis / synthesis kernels
 * (rnnoise_amd/csrc/fft_reg.h; reference: rnn_fft_c, src/kiss_fft.c:566-586), `reps` passes each with the spectrum fed
 * back as the next input.  in/out: [n][960][2] host floats, natural order.  variant 0/1 = exchange implementation.
 * clocks[n] (optional): shader clocks per wave; xlane[2][6][64] (optional): source lanes of the exchange primitives. */
RNNOISE_EXPORT int rnnoise_amd_debug_fft(int device, int variant, float *out, const float *in, int n, int reps,
                                         unsigned long long *clocks, int *xlane);

/* Test tap: out[i] = (float)log10(1e-2 + (double)ex[i]) evaluated on `device` by the feature stage's own function (src/denoise.c:383
 * is the one libm call of the path: the kernels restate the host libm's algorithm, rnnoise_amd/csrc/log10_glibc.h). Host buffers. 0 / -1.
 * _range: ex == NULL sweeps the n floats whose bit patterns are first_bits, first_bits + 1, ... (exhaustive sweeps);
 * model 0 = what this process's kernels use (rnnoise_amd_log10_model()), 1 = the device library's log10. */
RNNOISE_EXPORT int rnnoise_amd_debug_log_energy(int device, float *out, const float *ex, int n);
RNNOISE_EXPORT int rnnoise_amd_debug_log_energy_range(int device, float *out, const float *ex, unsigned first_bits, unsigned n, int model);

/* The Viterbi VAD of training-data generation on the device (rnnoise_batch_train_levels_vad_device) evaluates the host libm's log()
 * and pow() (rnnoise_amd/csrc/pow_glibc.h).
 * _libm: those device functions against THIS host's libm, for the n floats f with bit patterns first_bits, first_bits + stride, ...:
 *   mode 1 pow((double)((1.f - f) / f), .5), 2 log(1e-15 + (double)f), 3 log((double)f); *mismatches = how many doubles differ in a
 *   bit (two NaNs count as equal), *first_bad = the bits of the first such f.  0 / -1.
 * _selfcheck: forced = 0 or 1 replaces the answer of rnnoise_amd_train_vad_device_available() (0: the device call refuses as on a
 *   host with a foreign libm), -1 gives it back to the self-check.  Host only. */
RNNOISE_EXPORT int rnnoise_amd_debug_train_vad_libm(int device, int mode, unsigned first_bits, unsigned stride, unsigned n,
                                                    unsigned long long *mismatches, unsigned *first_bad);
RNNOISE_EXPORT void rnnoise_amd_debug_train_vad_selfcheck(int forced);

#ifdef __cplusplus
}
#endif
#endif
