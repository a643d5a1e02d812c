/* link_oracle.c -- linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link) restated on the oracle.  TEST INFRASTRUCTURE:
 * compiled by tests/link_oracle.py with the flags of oracle/Makefile's liboracle.so (gcc -O2 -ffp-contract=off -mfma -I oracle
 * -I rnnoise_amd/csrc) into a library of its own.
 *
 * rno_link_group_frame advances the K rows of one link group by one frame, in three steps:
 *   1  every present row up to and including rno_compute_rnn (silent rows: up to the silence decision), as rno_process_frame_ctl
 *      (tests/csrc/ctl_oracle.c) does it;
 *   2  the two folds over the PARTICIPANTS -- the present rows whose frame is not silent -- in ascending row order:
 *        g_link[b]  m = the first participant's raw gain g[b]; for each further participant's x: m = (x < m) ? x : m
 *        vad_link   m = the first participant's VAD;           for each further participant's x: m = (x > m) ? x : m;  0 without one
 *      (so a NaN never replaces m and a NaN first value stays);
 *   3  the rest of rno_process_frame_ctl per present row: a participant with g_link where that function has the network's g (the
 *      pitch filter, the decay cap and the lastg update on the row's own lastg and energies, the floor, the per-bin gains), every
 *      present row with vad_link where it has its own VAD in the `voice` decision, on the row's own thr and hold.
 * An absent row is not touched.  The records and the returned VADs are each row's own raw values.  The controls are taken as
 * rno_process_frame_ctl takes them; a row with ctl = {0, 0, 0} has none (its counter still counts: 0 on every frame). */
#include "rn_oracle.c"

#define LINK_MAX 8

static float ctl_clamp(float x, float hi) { return x > 0 ? (x < hi ? x : hi) : 0; }

/* the two folds alone, for the tests of the rule: x[n][NB] and v[n] of the n participants in row order */
void rno_link_fold(int n, const float *x, const float *v, float *g_link, float *vad_link) {
  int j, b;
  *vad_link = 0;
  for (j = 0; j < n; j++) {
    for (b = 0; b < NB; b++) g_link[b] = !j ? x[b] : (x[j * NB + b] < g_link[b] ? x[j * NB + b] : g_link[b]);
    *vad_link = !j ? v[0] : (v[j] > *vad_link ? v[j] : *vad_link);
  }
}

/* m[K], st[K][RN_STATE_FLOATS], c[K], ctl[K][3] = floor, thr, hold, present[K], out[K][480], in[K][480], rec[K] (or NULL), vad[K]
 * (each row's own; 0 for a silent or an absent row), g_link[NB] and vad_link (or NULL: what step 2 found; g_link is left alone
 * without a participant).  Returns the number of participants, -1 for a K outside 1 .. 8 */
int rno_link_group_frame(int K, const RnoModel *const *m, float *st_all, int *c, const float *ctl, const int *present, float *out_all,
                         const float *in_all, RnoRecord *rec, float *vad, float *g_link_out, float *vad_link_out) {
  /* (per thread: tests/stream_mix.py runs one group per thread, and the ctypes call releases the GIL) */
  static _Thread_local cpx X[LINK_MAX][NFREQ], P[LINK_MAX][NFREQ];
  static _Thread_local float Ex[LINK_MAX][NB], Ep[LINK_MAX][NB], Exp[LINK_MAX][NB], g[LINK_MAX][NB];
  float x[NFRAME], xw[NWIN], features[RN_NB_FEATURES], gf[NFREQ], g_link[NB], part_g[LINK_MAX * NB], part_v[LINK_MAX];
  float vad_link = 0, gain;
  int silence[LINK_MAX];
  int k, i, n = 0, pitch_index;
  if (K < 1 || K > LINK_MAX) return -1;
  tables_init();
  /* 1 */
  for (k = 0; k < K; k++) {
    float *st = st_all + (size_t)k * RN_STATE_FLOATS;
    vad[k] = 0;
    if (rec) memset(rec + k, 0, sizeof *rec);
    if (!present[k]) continue;
    biquad_hp(x, st + RN_OFF_MEM_HP, in_all + (size_t)k * NFRAME);
    silence[k] = frame_features(st, X[k], P[k], Ex[k], Ep[k], Exp[k], features, x, 0, NFREQ, &pitch_index, &gain);
    if (rec) {
      rec[k].pitch = pitch_index;
      rec[k].pitch_gain = gain;
      rec[k].silence = silence[k];
    }
    if (!silence[k]) {
      rno_compute_rnn(m[k], st, g[k], &vad[k], features);
      if (rec) {
        memcpy(rec[k].features, features, sizeof features);
        memcpy(rec[k].gains, g[k], sizeof g[k]);
        rec[k].vad = vad[k];
      }
      memcpy(part_g + n * NB, g[k], sizeof g[k]);
      part_v[n++] = vad[k];
    }
  }
  /* 2 */
  rno_link_fold(n, part_g, part_v, g_link, &vad_link);
  if (g_link_out && n) memcpy(g_link_out, g_link, sizeof g_link);
  if (vad_link_out) *vad_link_out = vad_link;
  /* 3 */
  for (k = 0; k < K; k++) {
    float *st = st_all + (size_t)k * RN_STATE_FLOATS, *out = out_all + (size_t)k * NFRAME;
    cpx *dX = (cpx *)(st + RN_OFF_DELAYED_X);
    const float floor_gain = ctl_clamp(ctl[3 * k], 1.f), thr = ctl_clamp(ctl[3 * k + 1], 1.f);
    const int ihold = (int)ctl_clamp(ctl[3 * k + 2], 65535.f);
    int voice, closed;
    if (!present[k]) continue;
    /* counter, then gate: the frame's linked VAD already counts */
    voice = thr > 0 ? vad_link >= thr : 1;
    c[k] = voice ? 0 : (c[k] + 1 < 65536 ? c[k] + 1 : 65536);
    closed = thr > 0 && c[k] > ihold;

    if (!silence[k]) {
      float *gk = g[k];
      memcpy(gk, g_link, sizeof g_link);
      pitch_filter(dX, (const cpx *)(st + RN_OFF_DELAYED_P), st + RN_OFF_DELAYED_EX, st + RN_OFF_DELAYED_EP,
                   st + RN_OFF_DELAYED_EXP, gk);
      for (i = 0; i < NB; i++) { /* denoise.c:479-487, on the un-floored gain */
        float alpha = .6f;
        float *lastg = st + RN_OFF_LASTG;
        double q;
        gk[i] = (gk[i] > alpha * lastg[i]) ? gk[i] : alpha * lastg[i];
        q = gk[i] * (st[RN_OFF_DELAYED_EX + i] + 1e-3) / (Ex[k][i] + 1e-3);
        lastg[i] = (float)((1.f < q) ? 1.f : q);
      }
      if (floor_gain > 0)
        for (i = 0; i < NB; i++) gk[i] = (gk[i] < floor_gain) ? floor_gain : gk[i];
      interp_band_gain(gf, gk);
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

    memcpy(dX, X[k], sizeof X[k]);
    memcpy(st + RN_OFF_DELAYED_P, P[k], sizeof P[k]);
    memcpy(st + RN_OFF_DELAYED_EX, Ex[k], sizeof Ex[k]);
    memcpy(st + RN_OFF_DELAYED_EP, Ep[k], sizeof Ep[k]);
    memcpy(st + RN_OFF_DELAYED_EXP, Exp[k], sizeof Exp[k]);
  }
  return n;
}
