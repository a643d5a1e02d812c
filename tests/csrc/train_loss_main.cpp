// train_loss_main.cpp -- the kernel bodies of rnnoise_amd/csrc/train/train_loss.hip on the host, lane after lane, as a stand-alone
// program for the sanitizers (tests/test_train_loss_cpu.py builds it with -fsanitize=address,undefined and runs it as a subprocess).
//
//   train_loss_main JOB OUT
//
// JOB:  int64 header[16] = {n_rows, t_base, first, n_cuts, rec_fs, rec_rs, rec_floats, gain_fs, gain_rs, gain_floats, vad_fs, vad_rs,
//       vad_floats, want_grads, 0, 0}; double {gamma, w_gain, w_vad}; int64 cuts[n_cuts][2] = {t0, n_frames}; the records' floats
//       (from record 0), the predicted gains' and VADs' floats (from step t_base: a cut's pointers are moved by t0 - t_base frame
//       strides), each exactly as many as its header field says -- every buffer is a heap block of its own size, so that an access
//       past it is the sanitizer's; double sums[n_rows][4].
// OUT:  sums; then, when want_grads, the gradient buffers -- as large as gains and vad, filled with -7 before the first cut.
// Every cut gets a frame-terms workspace of exactly n_rows * n_frames * 2 doubles.
// Exit status 0: done; 3: a cut was refused (rn_tl_plan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "train_loss_shim.h"
#include "train_loss.hip"

static inline void rn_tl_terms(const RnTlIn (&in)[RN_TL_LANES], double gamma, int lane0, EvalTerms (&k)[RN_TL_LANES]) {
  RnTlReplay &r = g_replay;
  for (r.pass = 0;; r.pass++) {
    r.fresh = false;
    for (int l = 0; l < RN_TL_LANES; l++) {
      r.lane = lane0 + l, r.call = 0;
      k[l] = eval_frame_terms(in[l].gt, in[l].v, in[l].p, in[l].q, gamma, lane0 + l);
    }
    if (!r.fresh) return;
  }
}

static bool get(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

static float *block(FILE *f, int64_t floats) {
  float *p = static_cast<float *>(malloc(floats > 0 ? (size_t)floats * 4 : 4));
  if (!p || (f && !get(f, p, (size_t)floats * 4))) exit(2);
  if (!f)
    for (int64_t i = 0; i < floats; i++) p[i] = -7.f;
  return p;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  int64_t h[16];
  double par[3];
  if (!f || !get(f, h, sizeof h) || !get(f, par, sizeof par)) return 2;
  const int n_rows = (int)h[0], t_base = (int)h[1], n_cuts = (int)h[3];
  std::vector<int64_t> cuts((size_t)n_cuts * 2);
  if (!get(f, cuts.data(), cuts.size() * 8)) return 2;
  float *const rec = block(f, h[6]), *const gains = block(f, h[9]), *const vad = block(f, h[12]);
  float *const gg = h[13] ? block(nullptr, h[9]) : nullptr, *const gv = h[13] ? block(nullptr, h[12]) : nullptr;
  std::vector<double> sums((size_t)n_rows * RN_TL_SUMS);
  if (!get(f, sums.data(), sums.size() * 8)) return 2;
  fclose(f);
  RNNoiseTrainLoss c{};
  c.records = rec, c.rec_frame_stride = (long)h[4], c.rec_row_stride = (long)h[5];
  c.gain_frame_stride = (long)h[7], c.gain_row_stride = (long)h[8], c.vad_frame_stride = (long)h[10], c.vad_row_stride = (long)h[11];
  c.n_rows = n_rows, c.first = (int)h[2], c.gamma = par[0], c.w_gain = par[1], c.w_vad = par[2];
  for (int k = 0; k < n_cuts; k++) {
    c.t0 = (int)cuts[2 * k], c.n_frames = (int)cuts[2 * k + 1];
    const long long df = c.t0 - t_base;
    c.gains = gains + df * c.gain_frame_stride, c.vad = vad + df * c.vad_frame_stride;
    c.grad_gains = gg ? gg + df * c.gain_frame_stride : nullptr, c.grad_vad = gv ? gv + df * c.vad_frame_stride : nullptr;
    double *const terms = static_cast<double *>(malloc((size_t)n_rows * (c.n_frames > 0 ? c.n_frames : 1) * 2 * sizeof(double)));
    RnTlArgs a;
    const int plan = rn_tl_plan(&c, sums.data(), terms, a);
    if (plan < 0) return 3;
    if (plan == 1) {
      for (int row = 0; row < n_rows; row++)  // the first launch: every step of every row, one wave each
        for (int fr = 0; fr < a.n_frames; fr++) rn_tl_step(a, row, fr, 0);
      if (a.f_first < a.n_frames)
        for (int row = 0; row < n_rows; row++) rn_tl_row_sums(a, row);  // the second
    }
    free(terms);
  }
  FILE *o = fopen(argv[2], "wb");
  if (!o || !put(o, sums.data(), sums.size() * 8)) return 2;
  if (gg && (!put(o, gg, (size_t)h[9] * 4) || !put(o, gv, (size_t)h[12] * 4))) return 2;
  fclose(o);
  free(rec), free(gains), free(vad), free(gg), free(gv);
  return 0;
}
