/* mix_oracle.c -- the mixing stage of training-data generation (include/rnnoise_amd.h: RNNoiseTrainMix) restated in plain C for
 * explicit parameters and any number of frames.  TEST INFRASTRUCTURE: compiled by tests/mix_oracle.py (gcc -O2 -ffp-contract=off)
 * into a library of its own; tests/test_train_mix_cpu.py holds it to the reference's own functions (tests/csrc/ref_dump_harness.c).
 *
 * What it restates, with the types of every intermediate as C gives them to the reference's expressions:
 *   mixo_biquad        rnn_biquad, src/denoise.c:409-419
 *   mixo_weighted_rms  weighted_rms, src/dump_features.c:283-293
 *   mixo_viterbi       viterbi_vad, :199-254, with n frames for SEQUENCE_LENGTH
 *   mixo_clear_vad     clear_vad, :256-281
 *   mixo_levels        :409-412 (frame energies) and :420-435 (the six biquads, the three levels) of one sequence
 *   mixo_vad           :418 and :437 of one sequence
 *   mixo_mix           :420-431 and :437-465 of one sequence, without the RIR (:449-453) */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rnnoise_amd.h"

#define FRAME 480

void mixo_biquad(float *y, float mem[2], const float *x, const float *b, const float *a, int n) {
  for (int i = 0; i < n; i++) {
    float in = x[i];
    float out = in + mem[0];
    double t0 = b[0] * (double)in - a[0] * (double)out;
    double t1 = b[1] * (double)in - a[1] * (double)out;
    mem[0] = mem[1] + t0;
    mem[1] = t1;
    y[i] = out;
  }
}

float mixo_weighted_rms(const float *x, int n) {
  const float wb[2] = {-2.f, 1.f}, wa[2] = {-1.89f, .895f};
  float mem[2] = {0, 0}, acc = 1e-15f;
  float *w = malloc(sizeof(float) * n);
  mixo_biquad(w, mem, x, wb, wa, n);
  for (int i = 0; i < n; i++) acc += w[i] * w[i];
  free(w);
  return 0.9506 * sqrt(acc / n);
}

void mixo_viterbi(const float *E, int n, int *vad) {
  const float stay = 0.99f, leave = 0.01f, scale = 0.5f;
  int *from = malloc(sizeof(int) * 2 * n); /* from[2*i + state]: the best predecessor of `state` at frame i */
  float sig = 1e-30, noise = 1e-30, p = 0.5;
  for (int i = 0; i < n; i++) sig += E[i] * E[i];
  sig = sqrt(sig / n);
  for (int i = 0; i < n; i++) noise += 1.f / (1e-8 * sig * sig + E[i] * E[i]);
  noise = 1.f / sqrt(noise / n);
  for (int i = 0; i < n; i++) {
    float obs, before, ps, pn;
    obs = (log(1e-15 + E[i]) - log(noise)) / (.01 + log(sig) - log(noise));
    obs = .1f > obs ? .1f : obs; /* (in this order and form a NaN stays a NaN, as in MIN16(.9f, MAX16(.1f, p0))) */
    obs = .9f < obs ? .9f : obs;
    obs = 1.f / (1.f + pow((1.f - obs) / obs, scale));
    if (p * stay > (1 - p) * leave) {
      from[2 * i + 1] = 1;
      before = p * stay;
    } else {
      from[2 * i + 1] = 0;
      before = (1 - p) * leave;
    }
    ps = before * obs;
    if ((1 - p) * stay > p * leave) {
      from[2 * i] = 0;
      before = (1 - p) * stay;
    } else {
      from[2 * i] = 1;
      before = p * leave;
    }
    pn = before * (1 - obs);
    p = ps / (ps + pn);
  }
  vad[n - 1] = p > .5;
  for (int i = n - 1; i > 0; i--) vad[i - 1] = from[2 * i + (vad[i] ? 1 : 0)];
  for (int i = 0; i + 1 < n; i++)
    if (vad[i + 1]) vad[i] = 1;
  for (int i = n - 1; i > 0; i--)
    if (vad[i - 1]) vad[i] = 1;
  free(from);
}

void mixo_clear_vad(float *x, const int *vad, int n_frames) {
  int on = vad[0];
  for (int f = 0; f < n_frames; f++) {
    float *fr = x + (size_t)f * FRAME;
    if (!on && f + 1 < n_frames && vad[f + 1]) {
      for (int j = 0; j < FRAME; j++) fr[j] *= j / (float)FRAME;
      on = 1;
    } else if (!on) {
      memset(fr, 0, sizeof(float) * FRAME);
    } else if (f > 0 && !vad[f] && !vad[f - 1]) {
      for (int j = 0; j < FRAME; j++) fr[j] *= 1.f - j / (float)FRAME;
      on = 0;
    }
  }
}

/* the three signals of a sequence after the fixed high-pass and their own filter: sig[k] = n floats each (malloc'ed) */
static void filtered(const short *const corpus[3], const RNNoiseTrainMix *p, int n, float *sig[3]) {
  static const float a_hp[2] = {-1.99599, 0.99600}, b_hp[2] = {-2, 1};
  const long long pos[3] = {p->speech_pos, p->noise_pos, p->fgnoise_pos};
  const float *fa[3] = {p->a_sig, p->a_noise, p->a_fgnoise}, *fb[3] = {p->b_sig, p->b_noise, p->b_fgnoise};
  for (int k = 0; k < 3; k++) {
    float mem[2] = {0, 0};
    sig[k] = malloc(sizeof(float) * n);
    for (int i = 0; i < n; i++) sig[k][i] = corpus[k][pos[k] + i];
    mixo_biquad(sig[k], mem, sig[k], b_hp, a_hp, n);
    mem[0] = mem[1] = 0;
    mixo_biquad(sig[k], mem, sig[k], fb[k], fa[k], n);
  }
}

void mixo_levels(const short *speech, const short *noise, const short *fgnoise, const RNNoiseTrainMix *p, int n_frames, float *energy,
                 float *rms3) {
  const short *const corpus[3] = {speech, noise, fgnoise};
  const int n = FRAME * n_frames;
  float *sig[3];
  for (int f = 0; f < n_frames; f++) {
    energy[f] = 0;
    for (int j = 0; j < FRAME; j++) {
      float s = speech[p->speech_pos + (long long)f * FRAME + j];
      energy[f] += s * s;
    }
  }
  filtered(corpus, p, n, sig);
  for (int k = 0; k < 3; k++) {
    rms3[k] = mixo_weighted_rms(sig[k], n);
    free(sig[k]);
  }
}

void mixo_vad(const float *energy, int n_frames, int start_pos, unsigned char *vad) {
  int *v = malloc(sizeof(int) * n_frames);
  int lead = start_pos / FRAME;
  mixo_viterbi(energy, n_frames, v);
  for (int f = 0; f < n_frames; f++) vad[f] = f < lead ? 0 : v[f];
  free(v);
}

/* clean, noisy: [n_frames * 480] of this sequence; vad_target: [n_frames] */
void mixo_mix(const short *speech, const short *noise, const short *fgnoise, const RNNoiseTrainMix *p, const float *rms3,
              const unsigned char *vad, int n_frames, float *clean, float *noisy, float *vad_target, int *noise_free) {
  const short *const corpus[3] = {speech, noise, fgnoise};
  const int n = FRAME * n_frames;
  float *sig[3];
  float gs = p->speech_gain, gn = p->noise_gain, gf = p->fgnoise_gain;
  int *v = malloc(sizeof(int) * n_frames);
  for (int f = 0; f < n_frames; f++) v[f] = vad[f];
  filtered(corpus, p, n, sig);
  mixo_clear_vad(sig[0], v, n_frames);
  gs *= 3000.f / (1 + rms3[0]);
  gn *= 3000.f / (1 + rms3[1]);
  gf *= 3000.f / (1 + rms3[2]);
  for (int i = 0; i < n; i++) {
    sig[0][i] *= gs;
    sig[1][i] *= gn;
    sig[2][i] *= gf;
    noisy[i] = sig[0][i] + sig[1][i] + sig[2][i];
    clean[i] = sig[0][i];
  }
  if (p->clip)
    for (int i = 0; i < n; i++) {
      float t = noisy[i];
      t = -32767.f > t ? -32767.f : t;
      noisy[i] = 32767.f < t ? 32767.f : t;
    }
  if (p->quantize)
    for (int i = 0; i < n; i++) noisy[i] = floor(.5f + noisy[i]);
  for (int f = 0; f < n_frames; f++) vad_target[f] = v[f];
  *noise_free = gn == 0 && gf == 0;
  for (int k = 0; k < 3; k++) free(sig[k]);
  free(v);
}
