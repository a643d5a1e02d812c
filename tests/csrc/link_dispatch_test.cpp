// tests/test_gain_link_cpu.py: the host-compilable parts of linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link) without a
// GPU -- what the setter accepts (rnnoise_amd/csrc/dispatch.h: rn_pcm_channels_ok, the rule of the channel count) and which stream
// member j of a row's link group is (rnnoise_amd/csrc/rn_dev.h: rn_link_stream).  argv: cases, one line of output each --
//   ok:k,n_streams                      ->  1 | 0: what the setter accepts
//   sib:row,k,j                         ->  the stream of member j of row's group in a call without a list
//   lsib:n_stride,row,k,j,e0,e1,...     ->  the same in a list call whose list is e0, e1, ... over a batch of n_stride streams
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rnnoise_amd/csrc/dispatch.h"
#include "../../rnnoise_amd/csrc/rn_dev.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    int v[3] = {0};
    if (!strncmp(argv[i], "ok:", 3) && sscanf(argv[i] + 3, "%d,%d", &v[0], &v[1]) == 2) {
      printf("%d\n", rn_pcm_channels_ok(v[0], v[1]) ? 1 : 0);
    } else if (!strncmp(argv[i], "sib:", 4) && sscanf(argv[i] + 4, "%d,%d,%d", &v[0], &v[1], &v[2]) == 3) {
      RnGroupDev g{};
      printf("%d\n", rn_link_stream(g, v[0], v[1], v[2]));
    } else if (!strncmp(argv[i], "lsib:", 5)) {
      std::vector<int> a;
      for (char *p = argv[i] + 5; *p;) {
        a.push_back((int)strtol(p, &p, 10));
        if (*p == ',') p++;
      }
      if (a.size() < 5) return 2;
      RnGroupDev g{};
      g.n_stride = a[0];
      g.list = a.data() + 4;
      g.list_n = (int)a.size() - 4;
      if (a[1] < 0 || a[1] >= g.list_n || g.list_n % a[2] || a[3] < 0 || a[3] >= a[2]) return 3;  // (what batch.cpp guarantees)
      printf("%d\n", rn_link_stream(g, a[1], a[2], a[3]));
    } else {
      fprintf(stderr, "link_dispatch_test: bad case %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
