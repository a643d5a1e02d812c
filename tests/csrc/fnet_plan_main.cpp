// The host-only half of librnnoise_amd_fnet.so (rnnoise_amd/csrc/fnet/fnet_plan.h) as a program of its own, for the address and
// undefined-behaviour sanitizers (tests/test_fnet_cpu.py builds and runs it): the limits and the byte arithmetic, the checks on
// weights and rows, and a host model of the launch schedule -- every launch of the plan reads and writes named slots (a row's feature
// frames, conv1's frames, the four parts of cat per frame, the three states, the gate scratch), and the model asserts that nothing is
// read before the launch that writes it has been issued, that no launch writes what a launch of the same step reads, and that the
// launches are as many as the header's formula says.
#include <assert.h>
#include <stdio.h>
#include <set>
#include <vector>
#include "../../rnnoise_amd/csrc/fnet/fnet_plan.h"

namespace {
int g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int limits_and_bytes() {
  const int ok_c[] = {16, 32, 128, 1008, 1024}, bad_c[] = {0, -16, 15, 17, 24, 1025, 1040};
  const int ok_h[] = {16, 48, 384, 4080, 4096}, bad_h[] = {0, -16, 8, 15, 17, 40, 4097, 4112};
  for (int c : ok_c)
    for (int h : ok_h) CHECK(rn_fnet_dims_ok(c, h, 1, 1) && rn_fnet_bytes(c, h, 1, 1) > 0);
  for (int c : bad_c) CHECK(!rn_fnet_dims_ok(c, 384, 1, 1) && rn_fnet_bytes(c, 384, 1, 1) == -1);
  for (int h : bad_h) CHECK(!rn_fnet_dims_ok(128, h, 1, 1) && rn_fnet_bytes(128, h, 1, 1) == -1);
  for (int n : {0, -1, RNNOISE_AMD_FNET_MAX_ROWS + 1}) CHECK(rn_fnet_bytes(128, 384, n, 1) == -1);
  for (int m : {0, -1, RNNOISE_AMD_FNET_MAX_FRAMES + 1}) CHECK(rn_fnet_bytes(128, 384, 1, m) == -1);
  CHECK(rn_fnet_bytes(128, 384, RNNOISE_AMD_FNET_MAX_ROWS, RNNOISE_AMD_FNET_MAX_FRAMES) > 0);
  CHECK(rn_fnet_bytes(RNNOISE_AMD_FNET_MAX_COND, RNNOISE_AMD_FNET_MAX_GRU, RNNOISE_AMD_FNET_MAX_ROWS, RNNOISE_AMD_FNET_MAX_FRAMES) > 0);
  // the formula by hand: cond 16, gru 16, one row, one frame
  const long long w = 4LL * (196 * 16 + 16 + 3 * 16 * 16 + 16 + 18 * 256 + 18 * 16 + 48 * 64 + 48);
  const long long s = 4LL * (65 * 5 + 48) + 8, k = 4LL * (3 * 16 + 64 + 12 * 16 + 1);
  CHECK(rn_fnet_bytes(16, 16, 1, 1) == w + s + k);
  return 0;
}

int weights_and_rows() {
  float t[4] = {0};
  RNNoiseFnetWeights w{};
  w.cond_size = 128, w.gru_size = 384;
  const float **all[] = {&w.conv1_weight,     &w.conv1_bias,       &w.conv2_weight,     &w.conv2_bias,       &w.gru_weight_ih[0],
                         &w.gru_weight_ih[1], &w.gru_weight_ih[2], &w.gru_weight_hh[0], &w.gru_weight_hh[1], &w.gru_weight_hh[2],
                         &w.gru_bias_ih[0],   &w.gru_bias_ih[1],   &w.gru_bias_ih[2],   &w.gru_bias_hh[0],   &w.gru_bias_hh[1],
                         &w.gru_bias_hh[2],   &w.dense_out_weight, &w.dense_out_bias,   &w.vad_dense_weight, &w.vad_dense_bias};
  for (const float **p : all) *p = t;
  CHECK(rn_fnet_weights_ok(&w, 1, 1) && rn_fnet_weights_ok(&w, RNNOISE_AMD_FNET_MAX_ROWS, RNNOISE_AMD_FNET_MAX_FRAMES));
  CHECK(!rn_fnet_weights_ok(nullptr, 1, 1) && !rn_fnet_weights_ok(&w, 0, 1) && !rn_fnet_weights_ok(&w, 1, 0));
  CHECK(!rn_fnet_weights_ok(&w, RNNOISE_AMD_FNET_MAX_ROWS + 1, 1));
  for (const float **p : all) {
    *p = nullptr;
    CHECK(!rn_fnet_weights_ok(&w, 1, 1));
    *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(t) + 2);
    CHECK(!rn_fnet_weights_ok(&w, 1, 1));
    *p = t;
  }
  long fs = 0, rs = 0;
  CHECK(rn_fnet_rows_ok(nullptr, 65, 7, 3, &fs, &rs) && fs == 7 * 65 && rs == 65);
  RNNoiseFnetRows r{0, 0};
  CHECK(rn_fnet_rows_ok(&r, 1, 7, 3, &fs, &rs) && fs == 7 && rs == 1);
  r = {65, 3 * 65};
  CHECK(rn_fnet_rows_ok(&r, 65, 7, 3, &fs, &rs) && fs == 65 && rs == 195);
  r = {7 * 67 + 5, 67};
  CHECK(rn_fnet_rows_ok(&r, 65, 7, 3, nullptr, nullptr));
  const RNNoiseFnetRows refused[] = {{65, 64}, {64, 7 * 65}, {7 * 65 - 1, 65}, {65, 3 * 65 - 1}, {0, 65}, {65, 0}, {-65, 65}, {65, -65},
                                     {LONG_MAX / 2, 65}};
  for (const RNNoiseFnetRows &bad : refused) CHECK(!rn_fnet_rows_ok(&bad, 65, 7, 3, nullptr, nullptr));
  CHECK(!rn_fnet_rows_ok(nullptr, 0, 7, 3, nullptr, nullptr) && !rn_fnet_rows_ok(nullptr, 65, 0, 3, nullptr, nullptr) &&
        !rn_fnet_rows_ok(nullptr, 65, 7, -1, nullptr, nullptr) && rn_fnet_rows_ok(nullptr, 65, 7, 0, nullptr, nullptr));
  return 0;
}

// ---- the model of the schedule ----
struct Model {
  int M;
  long long launch = 0;                // launches issued so far, resets included
  std::vector<long long> xin, c1;      // per frame slot: the launch that wrote it last, -1: never
  std::vector<long long> cat;          // [M][4]
  long long h[RN_FNET_LAYERS];         // the states
  explicit Model(int m) : M(m), xin(m + 4, -1), c1(m + 2, -1), cat(4 * m, -1) {
    for (long long &v : h) v = -1;
  }
  void reset(const RnFnetClock &clock) {  // what rn_fnet_reset_kernel writes
    for (int i = 0; i < 4; i++) xin[clock.hist_at + i] = launch;
    for (long long &v : h) v = launch;
    launch++;
  }
};

// one launch: -> false where it reads what was never written, what an earlier piece left in the workspace, or what it writes itself
bool issue(Model &m, const RnFnetLaunch &L, long long piece_began) {
  std::set<long long *> reads, writes;
  bool ok = true;
  auto fresh = [&](long long &slot) { ok = ok && slot >= piece_began && slot < m.launch, reads.insert(&slot); };  // of this piece
  auto kept = [&](long long &slot) { ok = ok && slot >= 0 && slot < m.launch, reads.insert(&slot); };               // of any earlier launch
  auto write = [&](long long &slot) { writes.insert(&slot); };
  switch (L.kind) {
    case RN_FNET_GATHER:
      // (a workgroup reads the history before it writes: the one launch that reads and writes the same slots, behind a barrier)
      for (int i = 0; i < 4; i++) ok = ok && m.xin[L.hist_at + i] >= 0 && m.xin[L.hist_at + i] < m.launch;
      for (int i = 0; i < L.T + 4; i++) write(m.xin[i]);
      break;
    case RN_FNET_CONV1:
      for (int j = 0; j < L.T + 2; j++) {
        for (int tap = 0; tap < 3; tap++) fresh(m.xin[j + tap]);
        write(m.c1[j]);
      }
      break;
    case RN_FNET_CONV2:
      for (int t = 0; t < L.T; t++) {
        for (int tap = 0; tap < 3; tap++) fresh(m.c1[t + tap]);
        write(m.cat[4 * t]);
      }
      break;
    case RN_FNET_GRU:
      ok = ok && L.lo <= L.hi;
      for (int l = L.lo; l <= L.hi; l++) {
        const int t = L.t[l];
        ok = ok && t >= L.g0 && t < L.T;
        if (!ok) return false;
        fresh(m.cat[4 * t + l]);  // c2 for layer 0, y_{l-1} above
        if (rn_fnet_prev_is_state(L, l))
          kept(m.h[l]);
        else
          fresh(m.cat[4 * (t - 1) + l + 1]);
        write(m.cat[4 * t + l + 1]);
      }
      break;
    default:
      for (int t = L.g0; t < L.T; t++)
        for (int part = 0; part < 4; part++) fresh(m.cat[4 * t + part]);
      if (L.g0 < L.T)
        for (long long &v : m.h) write(v);
  }
  for (long long *w : writes) {
    if (reads.count(w)) ok = false;  // written while the same launch still reads it
    *w = m.launch;
  }
  m.launch++;
  return ok;
}

int schedule() {
  for (int M : {1, 2, 16})
    for (int T : {0, 1, 2, 3, 4, 5, 35})
      for (int seen0 = 0; seen0 <= 4; seen0++)
        for (int second : {0, 1, 3, 35}) {  // a call of T frames, then one of `second`: the history and the states carry over
          Model m(M);
          RnFnetClock clock{0, 0};
          m.reset(clock);
          clock.seen = seen0;
          long long total = 0;
          for (int n_frames : {T, second}) {
            const long long want = rn_fnet_launches(n_frames, M, clock.seen);
            long long piece_began = m.launch, gru_frames = 0, heads = 0;
            int last_t0 = -1;
            bool ok = true;
            const long long made = rn_fnet_plan(n_frames, M, clock, [&](const RnFnetLaunch &L) {
              if (L.t0 != last_t0) piece_began = m.launch, last_t0 = L.t0;
              if (L.kind == RN_FNET_GRU) gru_frames += L.hi - L.lo + 1;
              if (L.kind == RN_FNET_HEADS) heads += L.T;
              ok = ok && L.T >= 1 && L.T <= M && issue(m, L, piece_began);
              return ok;
            });
            CHECK(ok && made == want);
            CHECK(heads == n_frames);
            total += made;
            // every layer ran every frame from the fourth since the reset on, and no other
            const long long before = clock.seen - n_frames;
            const long long live = n_frames - (before >= 4 ? 0 : (4 - before < n_frames ? 4 - before : n_frames));
            CHECK(gru_frames == RN_FNET_LAYERS * live);
          }
          CHECK(clock.seen == seen0 + T + second);
          CHECK(total == m.launch - 1);
          if (T == 0 && second == 0) CHECK(total == 0);
        }
  // the formula on its own: 35 frames in pieces of 16 from a reset: 3 pieces, 4 launches each, 31 GRU frames in 3 runs of + 2
  CHECK(rn_fnet_launches(35, 16, 0) == 3 * 4 + (12 + 2) + (16 + 2) + (3 + 2));
  CHECK(rn_fnet_launches(3, 16, 0) == 4 && rn_fnet_launches(3, 16, 1) == 4 && rn_fnet_launches(3, 16, 2) == 4 + 1 + 2);
  CHECK(rn_fnet_launches(1, 1, 100) == 4 + 3 && rn_fnet_launches(0, 4, 0) == 0);
  // a plan that stops: emit's refusal comes back as -1
  RnFnetClock c{0, 0};
  CHECK(rn_fnet_plan(5, 2, c, [](const RnFnetLaunch &) { return false; }) == -1);
  return 0;
}
}  // namespace

int main() {
  if (limits_and_bytes() || weights_and_rows() || schedule()) return 1;
  printf("fnet_plan_main: %d checks\n", g_checks);
  return 0;
}
