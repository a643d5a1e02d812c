/* ctl_oracle.c -- the per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls) restated on the
 * oracle.  TEST INFRASTRUCTURE: compiled by tests/ctl_oracle.py with the flags of oracle/Makefile's liboracle.so
 * (gcc -O2 -ffp-contract=off -mfma -I oracle -I rnnoise_amd/csrc) into a library of its own.
 *
 * rno_process_frame_ctl is rno_process_frame (oracle/rn_oracle.c) with three steps added:
 *   counter  voice = thr > 0 ? vad >= thr : 1 (a NaN vad is no voice); *c = voice ? 0 : min(*c + 1, 65536), on every frame, silent
 *            ones included (vad 0), before the gate is decided;
 *   floor    non-silent frames, after the decay cap and the lastg update (both on the un-floored gain): g' = g < floor ? floor : g
 *            per band, nothing at all when floor == 0; the per-bin gains come from g';
 *   gate     thr > 0 && *c > hold: the spectrum to be synthesised is zero, so the frame's transform is +0 everywhere -- the output
 *            is the previous synthesis tail (+ 0) and the new synthesis tail is +0.
 * The controls are taken as the kernel takes a table entry: NaN reads as 0, each value is clamped into its range ([0, 1], [0, 1],
 * [0, 65535]) and hold is truncated. */
#include "rn_oracle.c"

static float ctl_clamp(float x, float hi) { return x > 0 ? (x < hi ? x : hi) : 0; }

float rno_process_frame_ctl(const RnoModel *m, float *st, int *c, float floor_gain, float thr, float hold, float *out, const float *in,
                            RnoRecord *rec) {
  cpx X[NFREQ], P[NFREQ];
  float x[NFRAME], xw[NWIN];
  float Ex[NB], Ep[NB], Exp[NB], features[RN_NB_FEATURES], g[NB], gf[NFREQ];
  float vad_prob = 0, gain;
  cpx *dX = (cpx *)(st + RN_OFF_DELAYED_X);
  int i, pitch_index, silence, voice, closed, ihold;
  tables_init();
  if (rec) memset(rec, 0, sizeof *rec);
  floor_gain = ctl_clamp(floor_gain, 1.f);
  thr = ctl_clamp(thr, 1.f);
  ihold = (int)ctl_clamp(hold, 65535.f);

  biquad_hp(x, st + RN_OFF_MEM_HP, in);
  silence = frame_features(st, X, P, Ex, Ep, Exp, features, x, 0, NFREQ, &pitch_index, &gain);
  if (rec) {
    rec->pitch = pitch_index;
    rec->pitch_gain = gain;
    rec->silence = silence;
  }

  if (!silence) {
    rno_compute_rnn(m, st, g, &vad_prob, features);
    if (rec) {
      memcpy(rec->features, features, sizeof features);
      memcpy(rec->gains, g, sizeof g);
      rec->vad = vad_prob;
    }
  }
  /* counter, then gate: the frame's own VAD already counts */
  voice = thr > 0 ? vad_prob >= thr : 1;
  *c = voice ? 0 : (*c + 1 < 65536 ? *c + 1 : 65536);
  closed = thr > 0 && *c > ihold;

  if (!silence) {
    pitch_filter(dX, (const cpx *)(st + RN_OFF_DELAYED_P), st + RN_OFF_DELAYED_EX, st + RN_OFF_DELAYED_EP,
                 st + RN_OFF_DELAYED_EXP, g);
    for (i = 0; i < NB; i++) { /* denoise.c:479-487, on the un-floored gain */
      float alpha = .6f;
      float *lastg = st + RN_OFF_LASTG;
      double q;
      g[i] = (g[i] > alpha * lastg[i]) ? g[i] : alpha * lastg[i];
      q = g[i] * (st[RN_OFF_DELAYED_EX + i] + 1e-3) / (Ex[i] + 1e-3);
      lastg[i] = (float)((1.f < q) ? 1.f : q);
    }
    if (floor_gain > 0)
      for (i = 0; i < NB; i++) g[i] = (g[i] < floor_gain) ? floor_gain : g[i];
    interp_band_gain(gf, g);
    for (i = 0; i < NFREQ; i++) {
      dX[i].r *= gf[i];
      dX[i].i *= gf[i];
    }
  }

  /* frame_synthesis, denoise.c:400-407 */
  if (closed) memset(xw, 0, sizeof xw);
  else inverse_transform(xw, dX);
  apply_window(xw);
  for (i = 0; i < NFRAME; i++) out[i] = xw[i] + st[RN_OFF_SYNTHESIS + i];
  memcpy(st + RN_OFF_SYNTHESIS, xw + NFRAME, NFRAME * sizeof(float));

  memcpy(dX, X, sizeof X);
  memcpy(st + RN_OFF_DELAYED_P, P, sizeof P);
  memcpy(st + RN_OFF_DELAYED_EX, Ex, sizeof Ex);
  memcpy(st + RN_OFF_DELAYED_EP, Ep, sizeof Ep);
  memcpy(st + RN_OFF_DELAYED_EXP, Exp, sizeof Exp);
  return vad_prob;
}
