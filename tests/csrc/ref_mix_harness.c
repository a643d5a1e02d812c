/* ref_mix_harness.c -- the reference's own mixing-stage functions made callable.  TEST INFRASTRUCTURE, compiled by
 * tests/test_train_mix_cpu.py into pytest's temporary directory where the reference's sources are mounted; nothing of it is kept.
 *
 * weighted_rms, viterbi_vad and clear_vad are static functions of src/dump_features.c, beside a main() that does file I/O and
 * random draws: this TU #includes that file where it lies (REF_DUMP_FEATURES_C) with main renamed and wraps the three, and
 * rnn_biquad of src/denoise.c, which the test links from the reference's source.  Nothing is restated here.  The reference fixes
 * the sequence at SEQUENCE_LENGTH = 2000 frames. */
#define main ref_dump_features_main
#include REF_DUMP_FEATURES_C
#undef main

int refm_sequence_frames(void) { return SEQUENCE_LENGTH; }
void refm_biquad(float *y, float *mem, const float *x, const float *b, const float *a, int n) { rnn_biquad(y, mem, x, b, a, n); }
float refm_weighted_rms(float *x) { return weighted_rms(x); }
void refm_viterbi_vad(const float *E, int *vad) { viterbi_vad(E, vad); }
void refm_clear_vad(float *x, int *vad) { clear_vad(x, vad); }
