// mix_main.cpp -- the loops of rnnoise_amd/csrc/train_mix.hip on the host (shim.h beside this file), against tests/csrc/mix_oracle.c.  TEST
// INFRASTRUCTURE, a stand-alone program built with the address and undefined-behaviour sanitizers: every buffer is a heap block of its
// exact size (the corpora at even and at odd addresses), so any access outside a corpus or an output is reported, and every output is
// compared bit for bit.  Exit status 0: all equal.
#include "shim.h"
#include <random>
extern "C" {
void mixo_levels(const short *, const short *, const short *, const RNNoiseTrainMix *, int, float *, float *);
void mixo_vad(const float *, int, int, unsigned char *);
void mixo_mix(const short *, const short *, const short *, const RNNoiseTrainMix *, const float *, const unsigned char *, int, float *, float *, float *, int *);
int rnnoise_batch_train_levels_device(RNNoiseBatch *, float *, float *, const short *, const short *, const short *, long long, long long, long long, const RNNoiseTrainMix *, int, void *);
int rnnoise_batch_train_mix_device(RNNoiseBatch *, float *, float *, float *, int *, const short *, const short *, const short *, long long, long long, long long, const RNNoiseTrainMix *, const float *, const unsigned char *, int, void *);
int rnnoise_amd_train_vad(const float *, int, int, const int *, unsigned char *);
}
static int run(int n, int T, bool odd_base) {
  std::mt19937 rng(n * 131 + T);
  const long long span = 480LL * T, len[3] = {span + 2001, span + 778, span + 1};
  short *base[3], *c[3];
  for (int k = 0; k < 3; k++) {
    base[k] = (short *)malloc((len[k] + (odd_base ? 1 : 0)) * 2);   // exact size: any read outside a corpus is reported
    c[k] = base[k] + (odd_base ? 1 : 0);
    for (long long i = 0; i < len[k]; i++) c[k][i] = (short)((int)(rng() % 40001) - 20000) * ((i / 700) % 3 ? 1 : 0);
  }
  const float F[4][2] = {{0, 0}, {-0.6838f, 0.3025f}, {-0.31f, -0.1922f}, {-1.3731f, 0.4761f}};
  std::vector<RNNoiseTrainMix> mix(n);
  std::vector<int> start(n);
  for (int s = 0; s < n; s++) {
    RNNoiseTrainMix &p = mix[s];
    p.speech_pos = s == n - 1 ? len[0] - span : (s * 37LL) % (len[0] - span + 1);
    p.noise_pos = s == n - 1 ? len[1] - span : (s * 39LL + 1) % (len[1] - span + 1);
    p.fgnoise_pos = s == n - 1 ? len[2] - span : (s * 41LL + 2) % (len[2] - span + 1);
    p.speech_gain = s % 3 == 0 ? .3f : s % 3 == 1 ? 1.f : 3.1f;
    p.noise_gain = s % 5 == 1 || s % 5 == 3 ? 0.f : 4.f;
    p.fgnoise_gain = s % 5 == 2 || s % 5 == 3 ? 0.f : .8f;
    float *f[6] = {p.a_sig, p.b_sig, p.a_noise, p.b_noise, p.a_fgnoise, p.b_fgnoise};
    for (int k = 0; k < 6; k++) memcpy(f[k], F[(s + k + s / 4) % 4], 8);
    p.clip = s % 2;
    p.quantize = (s / 2) % 2;
    start[s] = s % 4 == 2 ? (s * 53) % (480 * T + 900) : 0;
  }
  RNNoiseBatch b{n, 0};
  float *energy = (float *)malloc(sizeof(float) * n * T), *rms = (float *)malloc(sizeof(float) * n * 3);
  float *clean = (float *)aligned_alloc(16, sizeof(float) * n * span), *noisy = (float *)aligned_alloc(16, sizeof(float) * n * span);
  float *target = (float *)malloc(sizeof(float) * n * T);
  int *nf = (int *)malloc(sizeof(int) * n);
  unsigned char *vad = (unsigned char *)malloc((size_t)n * T);
  if (rnnoise_batch_train_levels_device(&b, energy, rms, c[0], c[1], c[2], len[0], len[1], len[2], mix.data(), T, nullptr)) return 1;
  if (rnnoise_amd_train_vad(energy, n, T, start.data(), vad)) return 2;
  if (rnnoise_batch_train_mix_device(&b, clean, noisy, target, nf, c[0], c[1], c[2], len[0], len[1], len[2], mix.data(), rms, vad, T, nullptr)) return 3;
  int bad = 0, vsum = 0;
  std::vector<float> e(T), oc(span), on(span), ot(T);
  std::vector<unsigned char> ov(T);
  for (int s = 0; s < n; s++) {
    float r3[3];
    int onf;
    mixo_levels(c[0], c[1], c[2], &mix[s], T, e.data(), r3);
    mixo_vad(e.data(), T, start[s], ov.data());
    mixo_mix(c[0], c[1], c[2], &mix[s], r3, ov.data(), T, oc.data(), on.data(), ot.data(), &onf);
    bad += memcmp(e.data(), energy + (size_t)s * T, 4 * T) != 0;
    bad += memcmp(r3, rms + s * 3, 12) != 0;
    bad += memcmp(ov.data(), vad + (size_t)s * T, T) != 0;
    bad += onf != nf[s];
    for (int f = 0; f < T; f++) {
      vsum += ov[f];
      bad += memcmp(&oc[f * 480], clean + ((size_t)f * n + s) * 480, 1920) != 0;
      bad += memcmp(&on[f * 480], noisy + ((size_t)f * n + s) * 480, 1920) != 0;
      bad += memcmp(&ot[f], target + (size_t)f * n + s, 4) != 0;
    }
  }
  printf("n=%d T=%d odd_base=%d: %d mismatching blocks, %d active frames of %d\n", n, T, odd_base, bad, vsum, n * T);
  for (int k = 0; k < 3; k++) free(base[k]);
  free(energy); free(rms); free(clean); free(noisy); free(target); free(nf); free(vad); free(b.train_mix_buf);
  return bad;
}
int main() {
  int bad = run(1, 7, false) + run(65, 7, true) + run(70, 3, false) + run(2, 40, true) + run(3, 1, true);
  printf(bad ? "FAILED\n" : "all equal\n");
  return bad != 0;
}
