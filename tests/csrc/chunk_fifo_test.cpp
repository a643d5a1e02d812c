// The two staging steps of a chunk call (rnnoise_amd/csrc/chunk_fifo.h) on the host, as the state kernels run them: per stream, every
// lane's first half, the barrier, every lane's second half -- lane after lane, ascending on even pushes and descending on odd ones.
// 3 streams, 40 pushes with counts from a fixed seed, against two deques per stream.  Every buffer is a heap block of exactly its size,
// so that the sanitizers this program is built with (-fsanitize=address,undefined) see any access outside it.
//   usage: chunk_fifo_test LANES M MAX_COUNT S16 ALIAS      prints "ok <pushes> <frames>"; exit 1 and a message on the first difference
// The frames' "denoiser" between the two steps is y = x / 2 + 3 on the present frames only: the steps move samples, nothing else.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <vector>

#include "../../rnnoise_amd/csrc/chunk_fifo.h"

namespace {
uint32_t rng_state = 0x2545f491u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}
template <typename T>
struct Block {  // exactly n elements on the heap
  T *p;
  size_t n;
  explicit Block(size_t n_) : p(static_cast<T *>(malloc(n_ ? n_ * sizeof(T) : 1))), n(n_) {}
  ~Block() { free(p); }
};
float denoise(float x) { return x * .5f + 3.f; }
int fail(const char *what, int push, int s, long i) {
  fprintf(stderr, "chunk_fifo_test: push %d stream %d: %s at %ld\n", push, s, what, i);
  return 1;
}
bool same(float a, float b) { return !memcmp(&a, &b, 4); }
}  // namespace

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int nt = atoi(argv[1]), M = atoi(argv[2]), max_count = atoi(argv[3]), s16 = atoi(argv[4]), alias = atoi(argv[5]);
  const int N = 3, PUSHES = 40, F = rn_chunk_frames(M, max_count);
  if (nt <= 0 || M <= 0 || M > RN_CHUNK_FIFO_ROW || max_count <= 0) return 2;
  const size_t esz = s16 ? sizeof(short) : sizeof(float);
  const float POISON_F = 12345.25f;
  const short POISON_S = -21846;

  Block<float> fifo((size_t)N * RN_CHUNK_REC), stage((size_t)F * N * M), kept(M);
  Block<unsigned char> active((size_t)F * N);
  Block<char> in((size_t)N * max_count * esz), out_own((size_t)N * max_count * esz);
  Block<int> counts(N), frames(N);
  char *out = alias ? in.p : out_own.p;
  memset(fifo.p, 0, fifo.n * sizeof(float));  // (chunk_plan.h: a record of zeros is a restarted stream)

  std::deque<float> in_q[N], out_q[N];
  for (int s = 0; s < N; s++) out_q[s].assign(M, 0.f);
  long total_frames = 0;

  for (int push = 0; push < PUSHES; push++) {
    // the counts: anything in [0, max_count], and often one of the edges -- nothing, everything, exactly up to a frame boundary, one
    // sample either side of it
    for (int s = 0; s < N; s++) {
      const int r = (int)in_q[s].size(), pick = rnd() % 8;
      int n = rnd() % (max_count + 1);
      if (pick == 0) n = 0;
      else if (pick == 1) n = max_count;
      else if (pick == 2) n = M - r;
      else if (pick == 3) n = M - r - 1;
      else if (pick == 4) n = M - r + 1;
      counts.p[s] = n < 0 ? 0 : n > max_count ? max_count : n;
    }
    // the caller's rows: samples up to the count, poison behind it; `out` poisoned where it is a buffer of its own
    for (int s = 0; s < N; s++)
      for (int i = 0; i < max_count; i++) {
        const bool live = i < counts.p[s];
        if (s16) {
          reinterpret_cast<short *>(in.p)[(size_t)s * max_count + i] = live ? (short)(rnd() & 0xffff) : POISON_S;
          if (!alias) reinterpret_cast<short *>(out)[(size_t)s * max_count + i] = POISON_S;
        } else {
          reinterpret_cast<float *>(in.p)[(size_t)s * max_count + i] = live ? ((int)(rnd() % 60001) - 30000) + (rnd() % 8) * .125f : POISON_F;
          if (!alias) reinterpret_cast<float *>(out)[(size_t)s * max_count + i] = POISON_F;
        }
      }
    for (size_t i = 0; i < stage.n; i++) stage.p[i] = -777.f;  // (an absent frame's slot: read by nobody)
    memset(active.p, 0xee, active.n);
    // (a device count out of range reads clamped: stream 1 sometimes hands one in)
    std::vector<int> given(counts.p, counts.p + N);
    if (push % 5 == 1 && given[1] == 0) given[1] = -3;
    if (push % 5 == 2 && given[1] == max_count) given[1] = max_count + 5;
    Block<int> dev_counts(N);
    memcpy(dev_counts.p, given.data(), N * sizeof(int));

    RnChunkDev c{};
    c.fifo = fifo.p;
    c.M = M;
    c.N = N;
    c.max_count = max_count;
    c.F = F;
    c.s16 = s16;
    c.counts = dev_counts.p;
    c.in = in.p;
    c.out = out;
    c.stage = stage.p;
    c.active = active.p;
    c.frames = frames.p;
    auto lane = [&](int i) { return push & 1 ? nt - 1 - i : i; };

    // ---- step 1: scatter ----
    for (int s = 0; s < N; s++) {
      std::vector<RnChunkHead> h(nt);
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_scatter_head(c, s);
        rn_chunk_scatter_frames(c, s, h[lane(i)], lane(i), nt);
      }
      // (the barrier)
      for (int i = 0; i < nt; i++) rn_chunk_scatter_tail(c, s, h[lane(i)], lane(i), nt);
    }
    // the model: the samples join the input deque; whole frames leave it
    std::vector<std::vector<float>> want_frames[N];
    for (int s = 0; s < N; s++) {
      for (int i = 0; i < counts.p[s]; i++)
        in_q[s].push_back(s16 ? (float)reinterpret_cast<short *>(in.p)[(size_t)s * max_count + i]
                              : reinterpret_cast<float *>(in.p)[(size_t)s * max_count + i]);
      while ((int)in_q[s].size() >= M) {
        want_frames[s].emplace_back(in_q[s].begin(), in_q[s].begin() + M);
        in_q[s].erase(in_q[s].begin(), in_q[s].begin() + M);
      }
      const int k = (int)want_frames[s].size();
      if (k > F) return fail("more frames than rows", push, s, k);
      if (frames.p[s] != k) return fail("frames[s]", push, s, frames.p[s]);
      for (int j = 0; j < F; j++) {
        if (active.p[(size_t)j * N + s] != (j < k)) return fail("mask", push, s, j);
        for (int i = 0; i < M; i++) {
          const float got = stage.p[((size_t)j * N + s) * M + i];
          if (!same(got, j < k ? want_frames[s][j][i] : -777.f)) return fail("staged frame", push, s, (long)j * M + i);
        }
      }
      if (*rn_chunk_fill(c, s) != (int)in_q[s].size()) return fail("input fill", push, s, *rn_chunk_fill(c, s));
      for (size_t i = 0; i < in_q[s].size(); i++)
        if (!same(rn_chunk_in_fifo(c, s)[i], in_q[s][i])) return fail("input tail", push, s, (long)i);
    }

    // ---- step 2: the frames' processing, present frames only, in place ----
    for (int s = 0; s < N; s++)
      for (size_t j = 0; j < want_frames[s].size(); j++, total_frames++)
        for (int i = 0; i < M; i++) {
          float &v = stage.p[(j * N + s) * M + i];
          v = denoise(v);
          out_q[s].push_back(v);
        }

    // ---- step 3: gather ----
    for (int s = 0; s < N; s++) {
      std::vector<RnChunkHead> h(nt);
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_gather_head(c, s);
        rn_chunk_gather_pop(c, s, h[lane(i)], kept.p, lane(i), nt);
      }
      // (the barrier)
      for (int i = 0; i < nt; i++) rn_chunk_gather_keep(c, s, h[lane(i)], kept.p, lane(i), nt);
    }
    for (int s = 0; s < N; s++) {
      const int n = counts.p[s];
      if ((int)out_q[s].size() < n) return fail("the model ran dry", push, s, n);
      for (int i = 0; i < max_count; i++) {
        if (s16) {
          const short got = reinterpret_cast<short *>(out)[(size_t)s * max_count + i];
          short want = POISON_S;
          if (i < n) {
            const float v = out_q[s][i];
            want = (short)((v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000);
          }
          if (got != want) return fail(i < n ? "output sample" : "a sample behind the count was written", push, s, i);
        } else {
          const float got = reinterpret_cast<float *>(out)[(size_t)s * max_count + i];
          if (!same(got, i < n ? out_q[s][i] : POISON_F)) return fail(i < n ? "output sample" : "a sample behind the count was written", push, s, i);
        }
      }
      out_q[s].erase(out_q[s].begin(), out_q[s].begin() + n);
      if ((int)out_q[s].size() != M - (int)in_q[s].size()) return fail("out_fill != M - in_fill in the model", push, s, (long)out_q[s].size());
      for (size_t i = 0; i < out_q[s].size(); i++)
        if (!same(rn_chunk_out_fifo(c, s)[i], out_q[s][i])) return fail("output tail", push, s, (long)i);
    }
  }
  // ---- a restart: nothing pending, M zeros to give out, the other streams as they were ----
  {
    RnChunkDev c{};
    c.fifo = fifo.p;
    c.M = M;
    const std::vector<float> before(fifo.p, fifo.p + fifo.n);
    for (int t = 0; t < nt; t++) rn_chunk_restart(c, 1, t, nt);
    if (*rn_chunk_fill(c, 1) != 0) return fail("restart: fill", PUSHES, 1, 0);
    for (int i = 0; i < RN_CHUNK_FIFO_ROW; i++)
      if (!same(rn_chunk_out_fifo(c, 1)[i], 0.f)) return fail("restart: output FIFO", PUSHES, 1, i);
    for (int s = 0; s < N; s += 2)
      if (memcmp(fifo.p + (size_t)s * RN_CHUNK_REC, before.data() + (size_t)s * RN_CHUNK_REC, RN_CHUNK_REC * sizeof(float)))
        return fail("restart touched another stream", PUSHES, s, 0);
    RnChunkDev none{};
    rn_chunk_restart(none, 0, 0, nt);  // (a batch without FIFOs: nothing to do)
  }
  printf("ok %d %ld\n", PUSHES, total_frames);
  return 0;
}
