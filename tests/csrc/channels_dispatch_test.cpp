// tests/test_pcm_channels_cpu.py: the rules of interleaved channels (rnnoise_amd/csrc/dispatch.h: rn_pcm_channels_ok,
// rn_pcm_channels_fit; include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels) and the kernel forms of a step without a GPU, with the
// switches taken from this process's environment as the library takes them.  argv: cases, one line of output each --
//   ok:channels,n_streams                                    ->  1 | 0: what the setter accepts
//   fit:frame_stride,row_stride,M,channels,n_rows,n_frames   ->  1 | 0: whether a call's group slots are disjoint
//   plan:n,cus,pipelined,channels                            ->  K0 K1 K2 GRU K3 of a lock-step 48 kHz step of a new batch of n streams
//                                                                whose calls carry that channel count, shaped as batch.cpp shapes it
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../rnnoise_amd/csrc/dispatch.h"

static const char *const kHp[] = {"rn_hp_one_kernel", "rn_hp_kernel"};
static const char *const kK1[] = {"rn_analysis_single_kernel", "rn_analysis_kernel"};
static const char *const kNn[] = {"rn_nn_one_kernel", "rn_nn_vector_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel", "layers"};
static const char *const kGru[] = {"rn_nn_gru_kernel", "rn_nn_gru_w8_kernel", "unknown"};
static const char *const kK3[] = {"rn_synthesis_few_kernel", "rn_synthesis_kernel"};

int main(int argc, char **argv) {
  const RnKnobs k = rn_knobs_from_env();
  for (int i = 1; i < argc; i++) {
    long fs = 0, rs = 0;
    int v[4] = {0};
    if (!strncmp(argv[i], "ok:", 3) && sscanf(argv[i] + 3, "%d,%d", &v[0], &v[1]) == 2) {
      printf("%d\n", rn_pcm_channels_ok(v[0], v[1]) ? 1 : 0);
    } else if (!strncmp(argv[i], "fit:", 4) && sscanf(argv[i] + 4, "%ld,%ld,%d,%d,%d,%d", &fs, &rs, &v[0], &v[1], &v[2], &v[3]) == 6) {
      printf("%d\n", rn_pcm_channels_fit(fs, rs, v[0], v[1], v[2], v[3]) ? 1 : 0);
    } else if (!strncmp(argv[i], "plan:", 5) && sscanf(argv[i] + 5, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4) {
      if (!rn_pcm_channels_ok(v[3], v[0])) return 3;
      RnStepShape s{v[0], true, v[1], rn_default_nn_path(k, v[0]), v[2] != 0, false, rn_shape_low_rate(48000, false)};
      s.channels = v[3];
      const RnPlan p = rn_plan(k, s);
      printf("%s %s %s %s %s\n", kHp[p.hp], kK1[p.k1], kNn[p.nn], kGru[p.gru], kK3[p.k3]);
    } else {
      fprintf(stderr, "channels_dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
