/* ref_dump_harness.c -- the reference's own training-stage functions made callable.  TEST INFRASTRUCTURE, compiled by
 * tests/train_support.py (reference_dump_features) where the reference's sources are mounted; nothing of it is kept.
 *
 * weighted_rms, viterbi_vad, clear_vad, load_rir and rir_filter_sequence are static functions of src/dump_features.c, beside a main()
 * that does file I/O and random draws: this TU #includes that file where it lies (REF_DUMP_FEATURES_C) with main renamed and wraps
 * them, rnn_biquad of src/denoise.c and the 65,536-point kiss_fft tables, which the build links from the reference's source.  Nothing
 * is restated here.  The reference fixes the sequence at SEQUENCE_LENGTH = 2000 frames. */
#define main ref_dump_features_main
#include REF_DUMP_FEATURES_C
#undef main

/* ---- the mixing stage (tests/test_train_mix_cpu.py) ---- */
int refm_sequence_frames(void) { return SEQUENCE_LENGTH; }
void refm_biquad(float *y, float *mem, const float *x, const float *b, const float *a, int n) { rnn_biquad(y, mem, x, b, a, n); }
float refm_weighted_rms(float *x) { return weighted_rms(x); }
void refm_viterbi_vad(const float *E, int *vad) { viterbi_vad(E, vad); }
void refm_clear_vad(float *x, int *vad) { clear_vad(x, vad); }

/* ---- the RIR stage (tests/test_train_rir_cpu.py) ---- */
static struct rir_list list;

static void setup(void) {
  if (!list.fft) list.fft = rnn_fft_alloc_twiddles(RIR_FFT_SIZE, NULL, NULL, NULL, 0);
}

int refr_fft_size(void) { return RIR_FFT_SIZE; }
int refr_sequence_frames(void) { return SEQUENCE_LENGTH; }

void refr_tables(float *twiddles, int *bitrev, int *factors) {
  setup();
  memcpy(twiddles, list.fft->twiddles, sizeof(kiss_twiddle_cpx) * RIR_FFT_SIZE);
  for (int i = 0; i < RIR_FFT_SIZE; i++) bitrev[i] = list.fft->bitrev[i];
  for (int i = 0; i < 2 * MAXFACTORS; i++) factors[i] = list.fft->factors[i];
}

/* load_rir of a file -> spec[65536][2] */
void refr_load_rir(const char *file, int early, float *spec) {
  setup();
  kiss_fft_cpx *X = load_rir(file, list.fft, early);
  memcpy(spec, X, sizeof(*X) * RIR_FFT_SIZE);
  free(X);
}

/* rir_filter_sequence on audio[SEQUENCE_SAMPLES] with the spectrum spec[65536][2] */
void refr_filter(float *audio, const float *spec) {
  setup();
  kiss_fft_cpx *Y = (kiss_fft_cpx *)spec;
  list.nb_rirs = 1;
  list.rir = &Y;
  list.early = &Y;
  rir_filter_sequence(&list, audio, 0, 0);
}
