// audio_score_main.cpp -- the kernel body of rnnoise_amd/csrc/score/audio_score.hip on the host, lane after lane, as a stand-alone
// program for the sanitizers (tests/test_audio_score_cpu.py builds it with -fsanitize=address,undefined and runs it as a subprocess).
//
//   audio_score_main JOB OUT
//
// JOB:  int64 header[16] = {n_rows, T, delay, first, n_cuts, ref_fs, ref_rs, ref_floats, in_fs, in_rs, in_floats, out_fs, out_rs,
//       out_floats, want_terms, 0}; int64 cuts[n_cuts][2] = {t0, n_frames}; the three planes' floats (ref, in, out), each exactly
//       as many as its header field says -- every plane is a heap block of its own size, so that a read past it is the sanitizer's;
//       double sums[n_rows][8]; double frame_terms[n_rows][T][8] when want_terms.
// OUT:  sums, then frame_terms when want_terms, after every cut has been scored in turn.
// Exit status 0: done; 3: a cut was refused (rn_as_plan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "audio_score_shim.h"
#include "audio_score.hip"

static bool get(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

static float *plane(FILE *f, int64_t floats) {
  const size_t bytes = ((size_t)floats * 4 + 15) & ~(size_t)15;
  float *p = static_cast<float *>(aligned_alloc(16, bytes ? bytes : 16));
  if (!p || !get(f, p, (size_t)floats * 4)) exit(2);
  return p;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  int64_t h[16];
  if (!f || !get(f, h, sizeof h)) return 2;
  const int n_rows = (int)h[0], T = (int)h[1], n_cuts = (int)h[4];
  std::vector<int64_t> cuts((size_t)n_cuts * 2);
  if (!get(f, cuts.data(), cuts.size() * 8)) return 2;
  RNNoiseAudioScore c{};
  float *const ref = plane(f, h[7]), *const in = plane(f, h[10]), *const out = plane(f, h[13]);
  c.ref = {ref, (long)h[5], (long)h[6]}, c.in = {in, (long)h[8], (long)h[9]}, c.out = {out, (long)h[11], (long)h[12]};
  c.n_rows = n_rows, c.first = (int)h[3], c.delay = (int)h[2], c.terms_frames = T;
  std::vector<double> sums((size_t)n_rows * RN_AS_SLOTS), terms(h[14] ? (size_t)n_rows * T * RN_AS_SLOTS : 0);
  if (!get(f, sums.data(), sums.size() * 8) || !get(f, terms.data(), terms.size() * 8)) return 2;
  fclose(f);
  for (int k = 0; k < n_cuts; k++) {
    c.t0 = (int)cuts[2 * k], c.n_frames = (int)cuts[2 * k + 1];
    RnAsArgs a;
    const int plan = rn_as_plan(&c, sums.data(), h[14] ? terms.data() : nullptr, a);
    if (plan < 0) return 3;
    if (plan == 0) continue;
    for (int row = 0; row < n_rows; row++) rn_as_wave(a, row, 0);  // the kernel: one wave per row
  }
  FILE *o = fopen(argv[2], "wb");
  if (!o || !put(o, sums.data(), sums.size() * 8) || !put(o, terms.data(), terms.size() * 8)) return 2;
  fclose(o);
  free(ref), free(in), free(out);
  return 0;
}
