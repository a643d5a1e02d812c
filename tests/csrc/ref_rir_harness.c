/* ref_rir_harness.c -- TEST INFRASTRUCTURE: the reference's own load_rir, rir_filter_sequence and 65,536-point kiss_fft tables,
 * callable: src/dump_features.c is included where it lies, with its main renamed (as tests/csrc/ref_mix_harness.c does).  Nothing of
 * the reference is restated here.  Compiled by tests/test_train_rir_cpu.py where the reference's sources are. */
#define main ref_dump_features_main
#include REF_DUMP_FEATURES_C
#undef main

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
