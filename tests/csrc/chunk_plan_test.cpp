// The push rule of the chunk calls (rnnoise_amd/csrc/chunk_plan.h) at every fill and count: for M in 80, 160, 240, 320, 480, every r in
// [0, M) and every n in [0, 2M + 1] -- k, the new fill, out_fill = M - in_fill, enough output before the pop, k within the frame rows
// of the call, and the gather step's way back from the new fill to the old.  Prints the number of cases; exit 1 on the first miss.
#include <stdio.h>
#include "../../rnnoise_amd/csrc/chunk_plan.h"

#define CHECK(c)                                                                \
  if (!(c)) {                                                                   \
    fprintf(stderr, "chunk_plan_test: M=%d r=%d n=%d: %s\n", M, r, n, #c);      \
    return 1;                                                                   \
  }

int main() {
  long cases = 0;
  const int Ms[] = {80, 160, 240, 320, 480};
  for (int M : Ms)
    for (int r = 0; r < M; r++)
      for (int n = 0; n <= 2 * M + 1; n++, cases++) {
        const RnChunkPush p = rn_chunk_push(M, r, n);
        // the definition, by counting: samples go in one at a time, a frame leaves whenever M are pending
        int fill = r, k = 0;
        for (int i = 0; i < n; i++)
          if (++fill == M) fill = 0, k++;
        CHECK(p.k == k && p.in_fill == fill);
        CHECK(p.in_fill >= 0 && p.in_fill < M);
        CHECK(p.avail == (M - r) + k * M && p.avail >= n);
        CHECK(p.out_fill == M - p.in_fill && p.out_fill >= 1 && p.out_fill <= M);
        CHECK(p.k <= rn_chunk_frames(M, n));
        CHECK(rn_chunk_fill_before(M, p.in_fill, n) == r);
        CHECK(rn_chunk_count(n, 2 * M + 1) == n && rn_chunk_count(-n - 1, M) == 0 && rn_chunk_count(M + 1 + n, M) == M);
      }
  printf("%ld\n", cases);
  return 0;
}
