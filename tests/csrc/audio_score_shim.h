// audio_score_shim.h -- what rnnoise_amd/csrc/score/audio_score.hip needs to compile as plain C++ (TEST INFRASTRUCTURE; its own,
// beside tests/csrc/hip_emul/shim.h): a wave is an array of 64 lanes that the kernel's own loops run one after the other, and the
// lane exchange works on the array of their accumulators.
#pragma once
#include "rnnoise_amd_score.h"
#define RN_AS_HOST 1
#define RN_AS_LANES 64
#define RN_AS_FN inline
#define RN_AS_ISSUED() ((void)0)
// acc = acc + acc[lane ^ m] for every lane at once, all eight slots
static inline void rn_as_exchange(double (&acc)[RN_AS_LANES][RNNOISE_AMD_SCORE_SLOTS], int m) {
  double old[RN_AS_LANES][RNNOISE_AMD_SCORE_SLOTS];
  for (int l = 0; l < RN_AS_LANES; l++)
    for (int k = 0; k < RNNOISE_AMD_SCORE_SLOTS; k++) old[l][k] = acc[l][k];
  for (int l = 0; l < RN_AS_LANES; l++)
    for (int k = 0; k < RNNOISE_AMD_SCORE_SLOTS; k++) acc[l][k] = old[l][k] + old[l ^ m][k];
}
