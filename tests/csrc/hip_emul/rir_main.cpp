// rir_main.cpp -- the kernels of rnnoise_amd/csrc/train_rir.hip on the host (shim.h beside this file), against tests/csrc/rir_oracle.c.  TEST
// INFRASTRUCTURE, a stand-alone program built with the address and undefined-behaviour sanitizers: every buffer is a heap block of its
// exact size, so any access outside the frames, the spectra, the responses or the workspace is reported, and every output is compared
// bit for bit.  The workspace holds one unit: every slab is one transform pair.  Exit status 0: all equal.
#include "shim.h"
#include <random>
extern "C" {
void riro_load(const float *, int, int, float *);
void riro_filter(float *, int, const float *);
void riro_clip_quantize(float *, long, int, int);
long long rnnoise_amd_train_rir_work_bytes(long long);
int rnnoise_batch_train_rir_load_device(RNNoiseBatch *, float *, const float *, const int *, int, void *);
int rnnoise_batch_train_rir_device(RNNoiseBatch *, float *, float *, const float *, int, const RNNoiseTrainRir *, void *, long long, int, void *);
}
constexpr int NR = 2, RIR = 32768, SPEC = 2 * 65536;
static int run(RNNoiseBatch &b, const float *spectra, int n, int T) {
  std::mt19937 rng(n * 131 + T);
  const size_t count = (size_t)T * n * 480;
  float *clean = (float *)aligned_alloc(16, count * 4), *noisy = (float *)aligned_alloc(16, count * 4);
  for (size_t i = 0; i < count; i++) {
    clean[i] = (float)((int)(rng() % 20001) - 10000) * .37f;
    noisy[i] = clean[i] + (float)((int)(rng() % 90001) - 45000) * .91f;   // (beyond +-32767 here and there)
  }
  // sequence 0: response 1, clipped; sequence 1: not filtered, clipped and quantised; sequence 2: response 0, quantised
  const RNNoiseTrainRir rec[3] = {{1, 1, 0}, {-1, 1, 1}, {0, 0, 1}};
  std::vector<float> wc((size_t)n * T * 480), wn(wc.size());
  for (int s = 0; s < n; s++) {
    float *c = &wc[(size_t)s * T * 480], *x = &wn[(size_t)s * T * 480];
    for (int f = 0; f < T; f++) {
      memcpy(c + f * 480, clean + ((size_t)f * n + s) * 480, 1920);
      memcpy(x + f * 480, noisy + ((size_t)f * n + s) * 480, 1920);
    }
    if (rec[s].rir_id >= 0) {
      riro_filter(c, T, spectra + ((size_t)rec[s].rir_id * 2 + 1) * SPEC);
      riro_filter(x, T, spectra + ((size_t)rec[s].rir_id * 2 + 0) * SPEC);
    }
    riro_clip_quantize(x, (long)T * 480, rec[s].clip, rec[s].quantize);
  }
  const long long wb = rnnoise_amd_train_rir_work_bytes(1);
  void *work = aligned_alloc(16, wb);
  if (rnnoise_batch_train_rir_device(&b, clean, noisy, spectra, NR, rec, work, wb, T, nullptr)) return 1000;
  int bad = 0;
  for (int s = 0; s < n; s++)
    for (int f = 0; f < T; f++) {
      bad += memcmp(&wc[((size_t)s * T + f) * 480], clean + ((size_t)f * n + s) * 480, 1920) != 0;
      bad += memcmp(&wn[((size_t)s * T + f) * 480], noisy + ((size_t)f * n + s) * 480, 1920) != 0;
    }
  printf("n=%d T=%d: %d mismatching frames\n", n, T, bad);
  free(clean); free(noisy); free(work);
  return bad;
}
int main() {
  RNNoiseBatch b{3, 0};
  // two responses: a short one that ends inside the early form's fade, and one of full length with a decaying tail
  std::mt19937 rng(5);
  const int lens[NR] = {601, RIR};
  float *rir = (float *)aligned_alloc(16, sizeof(float) * NR * RIR), *spectra = (float *)aligned_alloc(16, sizeof(float) * NR * 2 * SPEC);
  for (int r = 0; r < NR; r++)
    for (int i = 0; i < RIR; i++) rir[r * RIR + i] = (float)((int)(rng() % 2001) - 1000) * 1e-3f * expf(-i / (r ? 3000.f : 150.f));
  if (rnnoise_batch_train_rir_load_device(&b, spectra, rir, lens, NR, nullptr)) return 2;
  int bad = 0;
  std::vector<float> want(SPEC);
  for (int r = 0; r < NR; r++)
    for (int early = 0; early < 2; early++) {
      riro_load(rir + r * RIR, lens[r], early, want.data());
      const int d = memcmp(want.data(), spectra + ((size_t)r * 2 + early) * SPEC, sizeof(float) * SPEC) != 0;
      printf("spectrum %d early=%d: %s\n", r, early, d ? "DIFFERS" : "equal");
      bad += d;
    }
  bad += run(b, spectra, 3, 7) + run(b, spectra, 3, 69);
  printf(bad ? "FAILED\n" : "all equal\n");
  free(rir); free(spectra); free(b.train_rir_tw); free(b.train_rir_buf);
  return bad != 0;
}
