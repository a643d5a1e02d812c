// tests/test_stream_formats_cpu.py: the kernel forms of a step of a batch with a per-stream format table (rnnoise_amd/csrc/dispatch.h:
// RnStepShape::companded), without a GPU.  argv: cases, one line of output each --
//   fmt:n,whole,cus,path,pipelined,per_stream,low_rate,listed,companded  ->  K0 K1 K2 GRU K3 of the step; companded = -1 leaves the
//   member at its default initialiser (the shape every caller written before the member builds)
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
    int n, whole, cus, path, pipelined, per_stream, low_rate, listed, companded;
    if (strncmp(argv[i], "fmt:", 4) || sscanf(argv[i] + 4, "%d,%d,%d,%d,%d,%d,%d,%d,%d", &n, &whole, &cus, &path, &pipelined, &per_stream,
                                              &low_rate, &listed, &companded) != 9) {
      fprintf(stderr, "formats_dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
    RnStepShape s{n, whole != 0, cus, path, pipelined != 0, per_stream != 0, low_rate != 0};
    s.listed = listed != 0;
    if (companded >= 0) s.companded = companded != 0;
    const RnPlan p = rn_plan(k, s);
    printf("%s %s %s %s %s\n", kHp[p.hp], kK1[p.k1], kNn[p.nn], kGru[p.gru], kK3[p.k3]);
  }
  return 0;
}
