// vad_main.cpp -- rn_train_levels with its Viterbi-VAD epilogue (rnnoise_amd/csrc/train_mix.hip, include/rn_train_vad.h) on the host
// (shim.h beside this file), against rnnoise_amd_train_vad of the same unit and tests/csrc/mix_oracle.c.  TEST INFRASTRUCTURE, a
// stand-alone program built with the address and undefined-behaviour sanitizers: every buffer is a heap block of its exact size, so
// any access outside a row is reported, and every output is compared bit for bit.  Exit status 0: all equal.
// $VAD_EMUL_DUMP names a file: the run at 2000 frames leaves its energies, start positions and VAD bytes there (int32 n, T; float32
// energy[n][T]; int32 start[n]; uint8 vad[n][T]) for the comparison with the reference's own viterbi_vad (tests/test_train_vad_cpu.py).
#include "shim.h"
#include <random>
extern "C" {
void mixo_vad(const float *, int, int, unsigned char *);
int rnnoise_batch_train_levels_device(RNNoiseBatch *, float *, float *, const short *, const short *, const short *, long long, long long, long long, const RNNoiseTrainMix *, int, void *);
int rnnoise_batch_train_levels_vad_device(RNNoiseBatch *, float *, float *, unsigned char *, const short *, const short *, const short *, long long, long long, long long, const RNNoiseTrainMix *, const int *, int, void *);
int rnnoise_amd_train_vad(const float *, int, int, const int *, unsigned char *);
int rnnoise_amd_train_vad_device_available(void);
}
// the speech rows, by sequence: 0 speech-like bursts with silent stretches, 1 digital silence, 2 one loud frame, 3 every frame the
// same, 4 loud and all-zero frames in turn, 5 a level that climbs over the sequence, 6 quiet noise
constexpr int KINDS = 7;
static short speech_sample(int kind, long long i, int T, std::mt19937 &rng) {
  const long long f = i / 480;
  const int r = (int)(rng() % 40001) - 20000;
  switch (kind) {
    case 0: return (short)(r * ((i / 700) % 3 ? 1 : 0));
    case 1: return 0;
    case 2: return f == T / 2 ? (short)r : 0;
    case 3: return (short)(((i % 480) * 37) % 2001 - 1000);
    case 4: return (f / 3) % 2 ? (short)r : 0;
    case 5: return (short)(r * (double)(f + 1) / T);
    default: return (short)(r / 2000);
  }
}
static int run(int n, int T, bool odd_base, bool null_start, bool dump) {
  std::mt19937 rng(n * 131 + T);
  const long long span = 480LL * T, stride = span + 2, len[3] = {stride * n, span + 778, span + 1};
  short *base[3], *c[3];
  for (int k = 0; k < 3; k++) {
    base[k] = (short *)malloc((len[k] + (odd_base ? 1 : 0)) * 2);   // exact size: any read outside a corpus is reported
    c[k] = base[k] + (odd_base ? 1 : 0);
    for (long long i = 0; i < len[k]; i++) c[k][i] = (short)((int)(rng() % 2001) - 1000);
  }
  std::vector<RNNoiseTrainMix> mix(n);
  std::vector<int> start(n);
  for (int s = 0; s < n; s++) {
    RNNoiseTrainMix &p = mix[s];
    memset(&p, 0, sizeof p);
    p.speech_pos = s * stride + (s & 1);  // even and odd corpus positions; a row's two spare samples belong to it
    for (long long i = 0; i < stride; i++) c[0][s * stride + i] = speech_sample(s % KINDS, i > 0 ? i - (s & 1) : 0, T, rng);
    p.noise_pos = (s * 39LL + 1) % (len[1] - span + 1);
    p.fgnoise_pos = s & 1;
    p.speech_gain = 1.f;
    p.noise_gain = .5f;
    p.fgnoise_gain = s % 3 ? 0.f : .8f;
    p.a_sig[0] = -0.6838f, p.a_sig[1] = 0.3025f;
    const int starts[] = {0, 479, 480, 480 * (T / 2) + 7, 480 * T + 900, 961, 480 * T};
    start[s] = starts[(s / KINDS + s) % 7];
  }
  RNNoiseBatch b{n, 0};
  float *energy = (float *)malloc(sizeof(float) * n * T), *rms = (float *)malloc(sizeof(float) * n * 3);
  float *energy0 = (float *)malloc(sizeof(float) * n * T), *rms0 = (float *)malloc(sizeof(float) * n * 3);
  unsigned char *vad = (unsigned char *)malloc((size_t)n * T), *want = (unsigned char *)malloc((size_t)n * T);
  memset(vad, 0xA5, (size_t)n * T);
  const int *sp = null_start ? nullptr : start.data();
  if (rnnoise_batch_train_levels_vad_device(&b, energy, rms, vad, c[0], c[1], c[2], len[0], len[1], len[2], mix.data(), sp, T, nullptr)) return 1;
  if (rnnoise_batch_train_levels_device(&b, energy0, rms0, c[0], c[1], c[2], len[0], len[1], len[2], mix.data(), T, nullptr)) return 2;
  if (rnnoise_amd_train_vad(energy, n, T, sp, want)) return 3;
  int bad = 0, vsum = 0, silent = 0;
  bad += memcmp(energy, energy0, sizeof(float) * n * T) != 0;  // the levels call without the VAD runs what it ran
  bad += memcmp(rms, rms0, sizeof(float) * n * 3) != 0;
  bad += memcmp(vad, want, (size_t)n * T) != 0;
  std::vector<unsigned char> ov(T);
  for (int s = 0; s < n; s++) {
    mixo_vad(energy + (size_t)s * T, T, null_start ? 0 : start[s], ov.data());
    bad += memcmp(ov.data(), vad + (size_t)s * T, T) != 0;
    for (int f = 0; f < T; f++) vsum += ov[f];
    if (s % KINDS == 1)
      for (int f = 0; f < T; f++) silent += energy[(size_t)s * T + f] != 0.f;
  }
  bad += silent != 0;  // (the silent rows are silent: log(0), NaN through the limits)
  if (dump && getenv("VAD_EMUL_DUMP")) {
    FILE *f = fopen(getenv("VAD_EMUL_DUMP"), "wb");
    if (!f) return 4;
    const int hdr[2] = {n, T};
    std::vector<int> st(n, 0);
    if (!null_start) st = start;
    fwrite(hdr, 4, 2, f), fwrite(energy, 4, (size_t)n * T, f), fwrite(st.data(), 4, n, f), fwrite(vad, 1, (size_t)n * T, f);
    fclose(f);
  }
  printf("n=%d T=%d odd_base=%d null_start=%d: %d mismatching blocks, %d active frames of %d\n", n, T, odd_base, null_start, bad, vsum, n * T);
  for (int k = 0; k < 3; k++) free(base[k]);
  free(energy); free(rms); free(energy0); free(rms0); free(vad); free(want); free(b.train_mix_buf);
  return bad;
}
int main() {
  if (!rnnoise_amd_train_vad_device_available()) {
    printf("this host's libm is not the restated one\n");
    return 1;
  }
  int bad = 0, k = 0;
  for (int T : {1, 2, 7, 300})
    for (int n : {1, 65, 130}) bad += run(n, T, k++ & 1, false, false);
  bad += run(65, 7, false, true, false) + run(1, 2, true, true, false);  // start_pos NULL
  bad += run(65, 2000, true, false, true);
  printf(bad ? "FAILED\n" : "all equal\n");
  return bad != 0;
}
