/* rn_train_vad.h -- INTERNAL (not part of the API, like rn_layout.h): the Viterbi VAD of training-data generation as device code,
 * the epilogue of rn_train_levels (rnnoise_amd/csrc/train_mix.hip), and the tables of the host libm's
 * log() and pow() that it evaluates (rnnoise_amd/csrc/pow_glibc.h).  It lives under include/ because tests/csrc/hip_emul compiles
 * train_mix.hip as host C++ from a directory that holds only the unit and train_common.h, with include/ on the search path; the
 * two restated-libm headers stay beside log10_glibc.h and are reached from here by their relative path.
 *
 * rn_vad_row() is rnnoise_amd_train_vad's vad_levels / vad_observation / vad_decode (train_mix.hip, the reference's
 * src/dump_features.c:199-254) for one row, statement for statement: every quantity the reference holds in a float is rounded to
 * float, every sub-expression it evaluates in double stays double, the two limits are the same two ternaries (a NaN passes both),
 * the sums are serial in frame order.  What differs is where log, pow and sqrt come from:
 *   log, pow   the host libm's algorithm, restated (pow_glibc.h: bit-equal to GNU libc >= 2.28 on an FMA host over the whole domain);
 *   sqrt, /    the operators.  Both are IEEE correctly rounded in double on gfx950 as this library is built (no fast-math flag):
 *              a / b is the v_div_scale / v_rcp / Newton / v_div_fmas / v_div_fixup sequence, sqrt the v_rsq_f64 sequence whose
 *              last step is the fused-residual correction; float a / b likewise (the compiler's default for HIP).
 * The two predecessor bits of a frame go into the row's own output byte; the back-trace replaces them with the decision.  No
 * workspace, no LDS. */
#pragma once
#include "../rnnoise_amd/csrc/pow_glibc.h"

#ifdef __HIPCC__
#define RN_VAD_DEVICE_TABLE(type, name, ...) \
  static const type name##_host[] = {__VA_ARGS__}; \
  static __device__ __constant__ const type name##_dev[] = {__VA_ARGS__};
#else
#define RN_VAD_DEVICE_TABLE(type, name, ...) static const type name##_host[] = {__VA_ARGS__};
#endif
RN_VAD_DEVICE_TABLE(double, rn_vad_log_tab, RN_LOG_TAB_VALUES)
RN_VAD_DEVICE_TABLE(double, rn_vad_pow_log_tab, RN_POW_LOG_TAB_VALUES)
RN_VAD_DEVICE_TABLE(uint64_t, rn_vad_exp_tab, RN_EXP_TAB_VALUES)
#ifdef __HIP_DEVICE_COMPILE__
#define RN_VAD_TAB(name) name##_dev /* (a __constant__ array: read with global loads) */
#else
#define RN_VAD_TAB(name) name##_host
#endif

RN_HD double rn_vad_log(double x) { return rn_log_glibc_full(x, RN_VAD_TAB(rn_vad_log_tab)); }
RN_HD double rn_vad_pow_half(double x) { return rn_pow_glibc_fma(x, 0.5, RN_VAD_TAB(rn_vad_pow_log_tab), RN_VAD_TAB(rn_vad_exp_tab)); }

/* one row: n frame energies -> n bytes, the first `lead` of them cleared (RNN_CLEAR(vad, start_pos / 480), :437) */
RN_HD void rn_vad_row(const float *energy, int n, unsigned char *vad, int lead) {
  /* vad_levels */
  float sq = 1e-30, inv = 1e-30;
  for (int f = 0; f < n; f++) sq += energy[f] * energy[f];
  const float speech = __builtin_sqrt((double)(sq / n));
  for (int f = 0; f < n; f++) inv += 1.f / (1e-8 * speech * speech + energy[f] * energy[f]);
  const float noise = 1.f / __builtin_sqrt((double)(inv / n));
  /* vad_observation's two levels, the same for every frame */
  const double log_noise = rn_vad_log((double)noise);
  const double span = .01 + rn_vad_log((double)speech) - log_noise;
  float belief = 0.5;
  for (int f = 0; f < n; f++) {
    float where = (rn_vad_log(1e-15 + energy[f]) - log_noise) / span;
    where = .1f > where ? .1f : where;
    where = .9f < where ? .9f : where;
    const float obs = 1.f / (1.f + rn_vad_pow_half((double)((1.f - where) / where)));
    const float quiet = 1 - belief;
    const bool speech_stays = belief * 0.99f > quiet * 0.01f, noise_stays = quiet * 0.99f > belief * 0.01f;
    vad[f] = (unsigned char)((speech_stays ? 2 : 0) | (noise_stays ? 0 : 1)); /* bit s: the predecessor of state s */
    const float into_speech = (speech_stays ? belief * 0.99f : quiet * 0.01f) * obs;
    const float into_noise = (noise_stays ? quiet * 0.99f : belief * 0.01f) * (1 - obs);
    belief = into_speech / (into_speech + into_noise);
  }
  unsigned state = belief > .5;
  for (int f = n - 1; f >= 0; f--) {
    const unsigned from = vad[f];
    vad[f] = (unsigned char)state;
    state = (from >> state) & 1;
  }
  for (int f = 0; f + 1 < n; f++) vad[f] |= vad[f + 1];
  for (int f = n - 1; f > 0; f--) vad[f] |= vad[f - 1];
  for (int f = 0; f < lead; f++) vad[f] = 0;
}
