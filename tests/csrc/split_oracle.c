/* split_oracle.c -- the split calls (include/rnnoise_amd.h: rnnoise_batch_analyze, rnnoise_batch_synthesize) restated on the oracle.
 * TEST INFRASTRUCTURE: compiled by tests/split_oracle.py with the flags of oracle/Makefile's liboracle.so
 * (gcc -O2 -ffp-contract=off -mfma -I oracle -I rnnoise_amd/csrc) into a library of its own.
 *
 * rno_process_frame_ctl (tests/csrc/ctl_oracle.c) cut in two at the network:
 *   rno_split_analyze     the high-pass and rnn_compute_frame_features of one frame: the features out, the frame's spectra, band
 *                         energies and silence word into a pending record.  It moves what the analysis side owns and nothing else.
 *   rno_split_synthesize  the rest of the frame on a pending record, with the caller's gains and vad where that function has the
 *                         network's: counter and gate, pitch filter, decay cap, floor, per-bin gains, frame_synthesis, and the record's
 *                         spectra into the delayed_* fields.  On a silent frame gains and vad are not read and the vad counts as 0.
 * Any number of frames may be analysed before the first is synthesised; they are synthesised in order.  The network state is not
 * touched: fed rno_process_frame's own gains and vad the pair leaves every other float of the state as that function leaves it. */
#include "rn_oracle.c"

typedef struct {
  cpx X[NFREQ], P[NFREQ];
  float Ex[NB], Ep[NB], Exp[NB];
  int silence;
} RnoPending;

static float ctl_clamp(float x, float hi) { return x > 0 ? (x < hi ? x : hi) : 0; }

int rno_split_pending_bytes(void) { return (int)sizeof(RnoPending); }

/* returns the silence word; features[65] is written on every frame (zeros where frame_features leaves none) */
int rno_split_analyze(float *st, RnoPending *p, float *features, const float *in) {
  float x[NFRAME], gain;
  int pitch_index;
  tables_init();
  memset(features, 0, RN_NB_FEATURES * sizeof(float));
  biquad_hp(x, st + RN_OFF_MEM_HP, in);
  p->silence = frame_features(st, p->X, p->P, p->Ex, p->Ep, p->Exp, features, x, 0, NFREQ, &pitch_index, &gain);
  return p->silence;
}

void rno_split_synthesize(float *st, const RnoPending *p, int *c, float floor_gain, float thr, float hold, float *out, const float *gains,
                          const float *vad) {
  float xw[NWIN], g[NB], gf[NFREQ];
  cpx *dX = (cpx *)(st + RN_OFF_DELAYED_X);
  const float vad_prob = p->silence ? 0.f : *vad;
  int i, voice, closed, ihold;
  tables_init();
  floor_gain = ctl_clamp(floor_gain, 1.f);
  thr = ctl_clamp(thr, 1.f);
  ihold = (int)ctl_clamp(hold, 65535.f);
  voice = thr > 0 ? vad_prob >= thr : 1;
  *c = voice ? 0 : (*c + 1 < 65536 ? *c + 1 : 65536);
  closed = thr > 0 && *c > ihold;

  if (!p->silence) {
    memcpy(g, gains, sizeof g);
    pitch_filter(dX, (const cpx *)(st + RN_OFF_DELAYED_P), st + RN_OFF_DELAYED_EX, st + RN_OFF_DELAYED_EP,
                 st + RN_OFF_DELAYED_EXP, g);
    for (i = 0; i < NB; i++) { /* denoise.c:479-487, on the un-floored gain */
      float alpha = .6f;
      float *lastg = st + RN_OFF_LASTG;
      double q;
      g[i] = (g[i] > alpha * lastg[i]) ? g[i] : alpha * lastg[i];
      q = g[i] * (st[RN_OFF_DELAYED_EX + i] + 1e-3) / (p->Ex[i] + 1e-3);
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

  memcpy(dX, p->X, sizeof p->X);
  memcpy(st + RN_OFF_DELAYED_P, p->P, sizeof p->P);
  memcpy(st + RN_OFF_DELAYED_EX, p->Ex, sizeof p->Ex);
  memcpy(st + RN_OFF_DELAYED_EP, p->Ep, sizeof p->Ep);
  memcpy(st + RN_OFF_DELAYED_EXP, p->Exp, sizeof p->Exp);
}
