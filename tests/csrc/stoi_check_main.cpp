// stoi_check_main.cpp -- the host-only half of librnnoise_amd_stoi.so (rnnoise_amd/csrc/stoi/stoi_plan.h) as a program of its own, for the
// address and undefined-behaviour sanitizers: the check at the corners of its ranges, the workspace formula over every size, and the
// scratch layout of a plan -- every array inside the scratch, none overlapping.  Pointers are made-up addresses: nothing is dereferenced.
// Exit status 0: all as expected.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include "../../rnnoise_amd/csrc/side_host.h"
#include "../../rnnoise_amd/csrc/stoi/stoi_plan.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      failures++;                                                 \
    }                                                             \
  } while (0)

static RNNoiseStoi good() {
  const float *base = reinterpret_cast<const float *>(uintptr_t(1) << 20);
  RNNoiseStoi c{};
  c.ref = c.in = c.out = RNNoiseStoiPlane{base, 3 * 480, 480};
  c.n_rows = 3, c.n_frames = 10, c.first = 2, c.delay = 960;
  return c;
}

int main() {
  RNNoiseStoi c = good();
  EXPECT(stoi_call_ok(&c));
  EXPECT(!stoi_call_ok(nullptr));
  c.in.p = nullptr, c.in.frame_stride = -7, c.in.row_stride = 1;
  EXPECT(stoi_call_ok(&c));  // no noisy plane: its strides are not looked at
  for (int field = 0; field < 2; field++) {
    c = good();
    (field ? c.out : c.ref).p = nullptr;
    EXPECT(!stoi_call_ok(&c));
  }
  c = good(), c.out.p = reinterpret_cast<const float *>((uintptr_t(1) << 20) + 4);
  EXPECT(!stoi_call_ok(&c));
  c = good(), c.ref.frame_stride = LONG_MAX - 3, c.n_frames = RNNOISE_AMD_STOI_MAX_FRAMES;
  EXPECT(!stoi_call_ok(&c));  // the extent is computed wider than long
  c = good(), c.ref.row_stride = (LONG_MAX / 4) * 4, c.n_rows = RNNOISE_AMD_STOI_MAX_ROWS;
  EXPECT(!stoi_call_ok(&c));
  c = good(), c.first = INT_MAX, c.n_frames = RNNOISE_AMD_STOI_MAX_FRAMES, c.delay = INT_MAX;
  EXPECT(!stoi_call_ok(&c));
  c = good(), c.first = c.n_frames = RNNOISE_AMD_STOI_MAX_FRAMES, c.delay = RNNOISE_AMD_STOI_MAX_FRAMES * 480;
  EXPECT(stoi_call_ok(&c));
  c.delay += 1;
  EXPECT(!stoi_call_ok(&c));

  EXPECT(stoi_workspace(0, 10) == -1 && stoi_workspace(1, -1) == -1);
  EXPECT(stoi_workspace(RNNOISE_AMD_STOI_MAX_ROWS + 1, 10) == -1 && stoi_workspace(1, RNNOISE_AMD_STOI_MAX_FRAMES + 1) == -1);
  EXPECT(stoi_workspace(INT_MAX, INT_MAX) == -1 && stoi_workspace(INT_MIN, INT_MIN) == -1);
  EXPECT(stoi_workspace(1, 0) == 8 && stoi_workspace(1, 2) == 8 * 600 + 8 && stoi_workspace(2, 3) == 2 * (8 * (900 + 50) + 4 * 2 + 8));
  EXPECT(stoi_workspace(RNNOISE_AMD_STOI_MAX_ROWS, RNNOISE_AMD_STOI_MAX_FRAMES) > 0);

  // the layout: for every size, the arrays lie in order inside the scratch and end exactly where the formula says
  for (int rows : {1, 2, 65, RNNOISE_AMD_STOI_MAX_ROWS})
    for (int T : {0, 1, 2, 3, 4, 45, 120, 2000, RNNOISE_AMD_STOI_MAX_FRAMES})
      for (int first : {0, 2}) {
        if (first > T) continue;
        c = good(), c.n_rows = rows, c.n_frames = T, c.first = first, c.delay = first * 480;
        const long long bytes = stoi_workspace(rows, T);
        char *const scratch = reinterpret_cast<char *>(uintptr_t(1) << 40);
        double *const results = reinterpret_cast<double *>(uintptr_t(1) << 30);
        RnStoiArgs a;
        EXPECT(stoi_plan(&c, results, scratch, bytes, a));
        EXPECT(!stoi_plan(&c, results, scratch, bytes - 1, a) && !stoi_plan(&c, nullptr, scratch, bytes, a));
        EXPECT(!stoi_plan(&c, results, nullptr, bytes, a) && !stoi_plan(&c, results, scratch + 4, bytes + 4, a));
        EXPECT(stoi_plan(&c, results, scratch, bytes, a));
        const long long n = rows, C = a.C, G = a.G;
        EXPECT(a.L10 <= a.C && a.F <= a.G && a.L == (T - first) * 480 && a.L10 * 24 == a.L * 5);
        EXPECT(a.F == 0 || RN_STOI_HOP * (a.F - 1) + RN_STOI_WIN <= a.L10);
        EXPECT(reinterpret_cast<char *>(a.y10) == scratch && a.norm == a.y10 + n * 3 * C && a.env == a.norm + n * G);
        EXPECT(a.seg == a.env + n * 45 * G && reinterpret_cast<double *>(a.idx) == a.seg + n * 4 * G);
        EXPECT(a.cnt == a.idx + n * (G + G % 2) && reinterpret_cast<char *>(a.cnt + 2 * n) == scratch + bytes);
      }
  if (failures) fprintf(stderr, "%d failures\n", failures);
  return failures ? 1 : 0;
}
