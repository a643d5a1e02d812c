// train_loss_shim.h -- what rnnoise_amd/csrc/train/train_loss.hip and rnnoise_amd/csrc/eval_terms.h need to compile as plain C++
// (TEST INFRASTRUCTURE; its own, beside tests/csrc/audio_score_shim.h): a wave is an array of 64 lanes that the kernel's own loops
// run one after the other.  eval_frame_terms exchanges values between lanes in mid-function, so the 64 lanes of a step cannot simply
// run in turn; they are REPLAYED instead: pass n runs the function for every lane with the exchanges 0 .. n - 1 answered from what
// the lanes gave in earlier passes and exchange n recorded (its result, and everything after it, is not yet right in that pass).  The
// function is pure, so the pass in which no exchange is new has every lane's true result.
#pragma once
#include "rnnoise_amd_train.h"
#define RN_TL_HOST 1
#define RN_TL_LANES 64
#define RN_TL_FN inline
#define __device__
#define __forceinline__ inline

#define RN_TL_MAX_EXCHANGES 16
struct RnTlReplay {
  int lane, pass, call;
  bool fresh;
  double rec[RN_TL_MAX_EXCHANGES][RN_TL_LANES];
};
static RnTlReplay g_replay;
static inline double __shfl_xor(double v, int m, int) {
  RnTlReplay &r = g_replay;
  const int i = r.call++;
  if (i >= RN_TL_MAX_EXCHANGES) __builtin_trap();
  if (i < r.pass) return r.rec[i][r.lane ^ m];
  if (i == r.pass) r.rec[i][r.lane] = v, r.fresh = true;
  return v;
}

struct RnTlIn;
struct EvalTerms;
// (defined in train_loss_main.cpp, behind the unit's own text)
static inline void rn_tl_terms(const RnTlIn (&in)[RN_TL_LANES], double gamma, int lane0, EvalTerms (&k)[RN_TL_LANES]);
