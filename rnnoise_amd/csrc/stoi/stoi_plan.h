// stoi_plan.h -- the host-only half of librnnoise_amd_stoi.so (include/rnnoise_amd_stoi.h): the argument check, the sizes of a call
// and the layout of its scratch.  Plain C++ that dereferences nothing: stoi.hip includes it, and tests/csrc/stoi_check_main.cpp
// compiles it for the host under the sanitizers.  Needs ../side_host.h in front of it.
#pragma once
#include <limits.h>
#include <stddef.h>
#include "rnnoise_amd_stoi.h"

#define RN_STOI_FRAME RNNOISE_AMD_STOI_FRAME
#define RN_STOI_SLOTS RNNOISE_AMD_STOI_SLOTS
#define RN_STOI_WIN 256    // samples of a 10 kHz frame
#define RN_STOI_HOP 128
#define RN_STOI_BANDS 15
#define RN_STOI_SEG 30     // columns of a segment

// what the kernels get: the planes, the sizes and the scratch arrays of one call
struct RnStoiArgs {
  const float *ref, *in, *out;  // in: null where absent
  long long ref_fs, ref_rs, in_fs, in_rs, out_fs, out_rs;
  double *results;  // [n_rows][8]
  double *y10;      // [n_rows][3][C]      the 10 kHz signals: ref, in, out
  double *norm;     // [n_rows][G]         frame norms of ref
  double *env;      // [n_rows][3][G][15]  band envelopes: ref, in, out
  double *seg;      // [n_rows][G][4]      segment terms: STOI in, ESTOI in, STOI out, ESTOI out
  int *idx;         // [n_rows][G + G % 2] the kept frames, ascending
  int *cnt;         // [n_rows][2]         K
  int n_rows, first, delay;
  int L;            // samples of the span at 48 kHz
  int L10, F;       // samples and frames at 10 kHz
  int C, G;         // the capacities the scratch is laid out for: L10 and F of first = 0
};

namespace {
inline int stoi_frames(long long l10) { return l10 < RN_STOI_WIN ? 0 : (int)((l10 - RN_STOI_WIN) / RN_STOI_HOP + 1); }

inline bool stoi_sizes_ok(int n_rows, int n_frames) {
  return n_rows >= 1 && n_rows <= RNNOISE_AMD_STOI_MAX_ROWS && n_frames >= 0 && n_frames <= RNNOISE_AMD_STOI_MAX_FRAMES;
}

inline bool stoi_plane_ok(const RNNoiseStoiPlane &p, int n_rows, long long T) {
  if (!p.p || !aligned16(p.p)) return false;
  if (p.frame_stride < RN_STOI_FRAME || p.row_stride < RN_STOI_FRAME || (p.frame_stride & 3) || (p.row_stride & 3)) return false;
  const __int128 end = (__int128)(T > 0 ? T - 1 : 0) * p.frame_stride + (__int128)(n_rows - 1) * p.row_stride + RN_STOI_FRAME;
  return end <= (__int128)LONG_MAX;
}

inline bool stoi_call_ok(const RNNoiseStoi *c) {
  if (!c || !stoi_sizes_ok(c->n_rows, c->n_frames) || c->first < 0 || c->delay < 0 || c->first > c->n_frames) return false;
  if ((long long)c->first * RN_STOI_FRAME < c->delay) return false;
  if (c->in.p && !stoi_plane_ok(c->in, c->n_rows, c->n_frames)) return false;
  return stoi_plane_ok(c->ref, c->n_rows, c->n_frames) && stoi_plane_ok(c->out, c->n_rows, c->n_frames);
}

// bytes of scratch for n_rows rows of n_frames frames: the header's formula
inline long long stoi_workspace(int n_rows, int n_frames) {
  if (!stoi_sizes_ok(n_rows, n_frames)) return -1;
  const long long C = 100LL * n_frames, G = stoi_frames(C);
  return n_rows * (8 * (3 * C + 50 * G) + 4 * (G + G % 2) + 8);
}

// the kernels' arguments for a call whose planes, results and scratch lie where the call says; false: refused
inline bool stoi_plan(const RNNoiseStoi *call, double *results, void *scratch, long long scratch_bytes, RnStoiArgs &a) {
  if (!stoi_call_ok(call) || !results || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 7)) return false;
  const RNNoiseStoi &c = *call;
  if (scratch_bytes < stoi_workspace(c.n_rows, c.n_frames)) return false;
  a = RnStoiArgs{};
  a.ref = c.ref.p, a.ref_fs = c.ref.frame_stride, a.ref_rs = c.ref.row_stride;
  a.out = c.out.p, a.out_fs = c.out.frame_stride, a.out_rs = c.out.row_stride;
  if (c.in.p) a.in = c.in.p, a.in_fs = c.in.frame_stride, a.in_rs = c.in.row_stride;
  a.results = results;
  a.n_rows = c.n_rows, a.first = c.first, a.delay = c.delay;
  a.L = (c.n_frames - c.first) * RN_STOI_FRAME;
  a.L10 = 100 * (c.n_frames - c.first), a.F = stoi_frames(a.L10);
  a.C = 100 * c.n_frames, a.G = stoi_frames(a.C);
  const long long n = c.n_rows, C = a.C, G = a.G;
  double *d = static_cast<double *>(scratch);
  a.y10 = d, d += n * 3 * C;
  a.norm = d, d += n * G;
  a.env = d, d += n * 3 * G * RN_STOI_BANDS;
  a.seg = d, d += n * G * 4;
  a.idx = reinterpret_cast<int *>(d);
  a.cnt = a.idx + n * (G + G % 2);
  return true;
}
}  // namespace
