// tests/test_dispatch_cpu.py: the dispatch rules of the library (rnnoise_amd/csrc/dispatch.h) without a GPU, with the switches taken
// from this process's environment as the library takes them.  argv: cases, one line of output each --
//   plan:n,whole,cus,nn_path,pipelined,per_stream,low_rate  ->  K0 K1 K2 GRU K3 kernel names (K2 "layers": the layer-wise network)
//   sched:n_frames,batch_schedule                            ->  pipelined side_k1
//   path:n                                                   ->  the network path of a new batch of n streams
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
    int v[7] = {0};
    if (!strncmp(argv[i], "plan:", 5) &&
        sscanf(argv[i] + 5, "%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7) {
      const RnPlan p = rn_plan(k, {v[0], v[1] != 0, v[2], v[3], v[4] != 0, v[5] != 0, v[6] != 0});
      printf("%s %s %s %s %s\n", kHp[p.hp], kK1[p.k1], kNn[p.nn], kGru[p.gru], kK3[p.k3]);
    } else if (!strncmp(argv[i], "sched:", 6) && sscanf(argv[i] + 6, "%d,%d", &v[0], &v[1]) == 2) {
      const RnSchedule s = rn_schedule(k, v[0], v[1]);
      printf("%d %d\n", s.pipelined ? 1 : 0, s.side_k1 ? 1 : 0);
    } else if (!strncmp(argv[i], "path:", 5) && sscanf(argv[i] + 5, "%d", &v[0]) == 1) {
      printf("%d\n", rn_default_nn_path(k, v[0]));
    } else {
      fprintf(stderr, "dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
