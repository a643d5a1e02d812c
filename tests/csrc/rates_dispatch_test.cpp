// tests/test_stream_rates_cpu.py: the kernel forms of a step of a batch with a per-stream rate table (rnnoise_amd/csrc/dispatch.h:
// rn_shape_low_rate), without a GPU, shaped as batch.cpp shapes a lock-step call.  argv: cases, one line of output each --
//   rates:n,pcm_rate,table,pipelined  ->  K0 K1 K2 GRU K3 of a step of a whole batch of n streams on its default network path
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
    int n, rate, table, pipelined;
    if (strncmp(argv[i], "rates:", 6) || sscanf(argv[i] + 6, "%d,%d,%d,%d", &n, &rate, &table, &pipelined) != 4) {
      fprintf(stderr, "rates_dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
    const RnStepShape s{n, true, 256, rn_default_nn_path(k, n), pipelined != 0, false, rn_shape_low_rate(rate, table != 0)};
    const RnPlan p = rn_plan(k, s);
    printf("%s %s %s %s %s\n", kHp[p.hp], kK1[p.k1], kNn[p.nn], kGru[p.gru], kK3[p.k3]);
  }
  return 0;
}
