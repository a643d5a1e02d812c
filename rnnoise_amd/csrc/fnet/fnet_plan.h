// fnet_plan.h -- the host-only half of librnnoise_amd_fnet.so (include/rnnoise_amd_fnet.h) that needs no device: the limits, the
// checks on weights and rows, the byte arithmetic, and the launch schedule of a process call as a list the caller walks.  Plain C++:
// fnet.hip launches what the plan emits, tests/csrc/fnet_plan_main.cpp runs a host model of the same list under the sanitizers.
#pragma once
#include <limits.h>
#include <stdint.h>
#include "rnnoise_amd_fnet.h"
#include "../side_host.h"

#define RN_FNET_LAYERS 3
#define RN_FNET_K1 196        // conv1's K: 3 x 65 and one pad
#define RN_FNET_K1_LIVE 195   // inputs from here on read as zero
#define RN_FNET_HEAD_ROWS 48  // 32 gains and the vad row, padded to whole tiles of 16
#define RN_FNET_HIST (RNNOISE_AMD_FNET_LOOKAHEAD * RNNOISE_AMD_FNET_FEATURES)  // floats of a row's history

namespace {
inline bool rn_fnet_dims_ok(int C, int H, int N, int M) {
  if (C < RNNOISE_AMD_FNET_MIN_COND || C > RNNOISE_AMD_FNET_MAX_COND || C % 16) return false;
  if (H < RNNOISE_AMD_FNET_MIN_GRU || H > RNNOISE_AMD_FNET_MAX_GRU || H % 16) return false;
  return N >= 1 && N <= RNNOISE_AMD_FNET_MAX_ROWS && M >= 1 && M <= RNNOISE_AMD_FNET_MAX_FRAMES;
}

// the header's formula, term by term
inline long long rn_fnet_weight_bytes(long long C, long long H) {
  return 4 * (RN_FNET_K1 * C + C + 3 * C * H + H + 18 * H * H + 18 * H + RN_FNET_HEAD_ROWS * 4 * H + RN_FNET_HEAD_ROWS);
}
inline long long rn_fnet_state_bytes(long long H, long long N, long long M) {
  return 4 * (RNNOISE_AMD_FNET_FEATURES * (M + RNNOISE_AMD_FNET_LOOKAHEAD) * N + 3 * N * H) + 8 * N;
}
inline long long rn_fnet_work_bytes(long long C, long long H, long long N, long long M) {
  return 4 * ((M + 2) * N * C + 4 * M * N * H + 12 * N * H + N);
}
inline long long rn_fnet_bytes(int C, int H, int N, int M) {
  if (!rn_fnet_dims_ok(C, H, N, M)) return -1;
  return rn_fnet_weight_bytes(C, H) + rn_fnet_state_bytes(H, N, M) + rn_fnet_work_bytes(C, H, N, M);  // (< 2^59 at the limits)
}

inline bool rn_fnet_weights_ok(const RNNoiseFnetWeights *w, int n_rows, int max_frames) {
  if (!w || !rn_fnet_dims_ok(w->cond_size, w->gru_size, n_rows, max_frames)) return false;
  const float *one[] = {w->conv1_weight,     w->conv1_bias,     w->conv2_weight,     w->conv2_bias,
                        w->dense_out_weight, w->dense_out_bias, w->vad_dense_weight, w->vad_dense_bias};
  for (const float *p : one)
    if (!p || !aligned4(p)) return false;
  for (int l = 0; l < RN_FNET_LAYERS; l++) {
    const float *four[] = {w->gru_weight_ih[l], w->gru_weight_hh[l], w->gru_bias_ih[l], w->gru_bias_hh[l]};
    for (const float *p : four)
      if (!p || !aligned4(p)) return false;
  }
  return true;
}

// the strides of a buffer's rows (NULL or {0, 0}: [frame][n_rows][row]) -> fs, rs; false where the calls refuse them
inline bool rn_fnet_rows_ok(const RNNoiseFnetRows *r, int row_floats, int n_rows, long long n_frames, long *fs, long *rs) {
  if (row_floats < 1 || n_rows < 1 || n_frames < 0) return false;
  long f = r ? r->frame_stride : 0, s = r ? r->row_stride : 0;
  if (f == 0 && s == 0) f = (long)n_rows * row_floats, s = row_floats;
  if (!slots_fit(f, s, row_floats, n_rows, n_frames, 1)) return false;
  if (fs) *fs = f;
  if (rs) *rs = s;
  return true;
}

// ---- the launch schedule ----
enum RnFnetKind { RN_FNET_GATHER, RN_FNET_CONV1, RN_FNET_CONV2, RN_FNET_GRU, RN_FNET_HEADS };

// what the host knows of a runtime's time: the frames every row has had since the last reset of all rows, and where in a row's
// feature workspace its history lies (in frames: the frames of the piece before)
struct RnFnetClock {
  long long seen;
  int hist_at;
};

struct RnFnetLaunch {
  int kind;
  int t0;            // the piece's first frame within the call
  int T;             // the piece's frames, 1 .. max_frames
  int g0;            // the first frame of the piece the GRUs run on: max(0, 4 - seen), T where there is none
  long long seen;    // the clock at the piece's frame 0
  int hist_at;       // gather: the history's place when the piece begins
  int lo, hi;        // GRU: the layers of this launch,
  int t[RN_FNET_LAYERS];  // and the piece's frame each runs (index: the layer)
};

// whether layer l of a GRU launch reads its state before from the runtime's state (the piece's first GRU frame) or from the frame
// before in cat
inline bool rn_fnet_prev_is_state(const RnFnetLaunch &L, int l) { return L.t[l] == L.g0; }

// the GRU frames of a piece of T frames that begins at clock `seen`
inline int rn_fnet_gru_frames(int T, long long seen) {
  const long long warm = seen >= RNNOISE_AMD_FNET_LOOKAHEAD ? 0 : RNNOISE_AMD_FNET_LOOKAHEAD - seen;
  return warm >= T ? 0 : T - (int)warm;
}

// the header's formula: the launches of a call of n_frames frames on a runtime whose clock is at `seen`
inline long long rn_fnet_launches(int n_frames, int M, long long seen) {
  long long n = 0;
  for (int t0 = 0; t0 < n_frames; t0 += M) {
    const int T = n_frames - t0 < M ? n_frames - t0 : M, G = rn_fnet_gru_frames(T, seen + t0);
    n += 4 + (G > 0 ? G + 2 : 0);
  }
  return n;
}

// walks the launches of a call in order; emit(const RnFnetLaunch &) returns false to stop (-1).  The clock advances piece by piece,
// after the piece's last launch.  -> the launches made
template <class Emit>
inline long long rn_fnet_plan(int n_frames, int M, RnFnetClock &clock, Emit &&emit) {
  long long n = 0;
  for (int t0 = 0; t0 < n_frames; t0 += M) {
    RnFnetLaunch L{};
    L.t0 = t0, L.T = n_frames - t0 < M ? n_frames - t0 : M, L.seen = clock.seen, L.hist_at = clock.hist_at;
    const int G = rn_fnet_gru_frames(L.T, clock.seen);
    L.g0 = L.T - G;
    for (int kind : {RN_FNET_GATHER, RN_FNET_CONV1, RN_FNET_CONV2}) {
      L.kind = kind;
      if (!emit(L)) return -1;
      n++;
    }
    L.kind = RN_FNET_GRU;
    for (int s = 0; G > 0 && s < G + RN_FNET_LAYERS - 1; s++) {
      // launch s: layer l at the piece's frame g0 + s - l, for the layers lo .. hi that have one
      L.lo = s - (G - 1) > 0 ? s - (G - 1) : 0, L.hi = s < RN_FNET_LAYERS - 1 ? s : RN_FNET_LAYERS - 1;
      for (int l = 0; l < RN_FNET_LAYERS; l++) L.t[l] = l >= L.lo && l <= L.hi ? L.g0 + s - l : -1;
      if (!emit(L)) return -1;
      n++;
    }
    L.kind = RN_FNET_HEADS, L.lo = L.hi = 0;
    if (!emit(L)) return -1;
    n++;
    clock.seen += L.T, clock.hist_at = L.T;
  }
  return n;
}
}  // namespace
