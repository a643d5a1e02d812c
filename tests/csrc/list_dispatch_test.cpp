// tests/test_stream_list_cpu.py: the kernel forms of a stream-list step (rnnoise_amd/csrc/dispatch.h: RnStepShape::listed) without a
// GPU, with the switches taken from this process's environment as the library takes them.  argv: cases, one line of output each --
//   list:batch,rows,cus,pipelined,low_rate[,nn_path] ->  K0 K1 K2 GRU K3 of a list step of `rows` rows on a new batch of `batch` streams
//                                                        (its default network path, or nn_path as rnnoise_batch_set_nn_path sets it),
//                                                        as batch.cpp shapes it: never whole, per-stream
//   plan:n,whole,cus,nn_path,pipelined,per_stream,low_rate  ->  the same names for a step that is no list call (listed left at its default)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../rnnoise_amd/csrc/dispatch.h"

static const char *const kHp[] = {"rn_hp_one_kernel", "rn_hp_kernel"};
static const char *const kK1[] = {"rn_analysis_single_kernel", "rn_analysis_kernel"};
static const char *const kNn[] = {"rn_nn_one_kernel", "rn_nn_vector_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel", "layers"};
static const char *const kGru[] = {"rn_nn_gru_kernel", "rn_nn_gru_w8_kernel", "unknown"};
static const char *const kK3[] = {"rn_synthesis_few_kernel", "rn_synthesis_kernel"};

static void print(const RnPlan &p) { printf("%s %s %s %s %s\n", kHp[p.hp], kK1[p.k1], kNn[p.nn], kGru[p.gru], kK3[p.k3]); }

int main(int argc, char **argv) {
  const RnKnobs k = rn_knobs_from_env();
  for (int i = 1; i < argc; i++) {
    int v[7] = {0};
    int got = 0;
    if (!strncmp(argv[i], "list:", 5) &&
        ((got = sscanf(argv[i] + 5, "%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5])) == 5 || got == 6)) {
      RnStepShape s{v[1], false, v[2], got == 6 ? v[5] : rn_default_nn_path(k, v[0]), v[3] != 0, true, v[4] != 0};
      s.listed = true;
      print(rn_plan(k, s));
    } else if (!strncmp(argv[i], "plan:", 5) &&
               sscanf(argv[i] + 5, "%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7) {
      print(rn_plan(k, {v[0], v[1] != 0, v[2], v[3], v[4] != 0, v[5] != 0, v[6] != 0}));
    } else {
      fprintf(stderr, "list_dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
