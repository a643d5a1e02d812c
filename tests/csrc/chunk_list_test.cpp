// The list forms of a chunk call's two staging steps and the FIFO record bodies (rnnoise_amd/csrc/chunk_fifo.h) on the host, as the
// state kernels run them: per row, every lane's first half, the barrier, every lane's second half -- lane after lane, ascending on
// even calls and descending on odd ones.  7 streams, 40 calls, against two deques per stream.  Every buffer is a heap block of exactly
// its size, so that the sanitizers this program is built with (-fsanitize=address,undefined) see any access outside it.
//   usage: chunk_list_test list  LANES M MAX_COUNT S16 ALIAS   lists of 0 .. 5 rows in shuffled order, some naming an entry outside the
//                                                              batch; prints "ok <calls> <frames> <absent rows>"
//          chunk_list_test mixed LANES M MAX_COUNT S16 ALIAS   the same, every third call through the full-size bodies instead
//          chunk_list_test records LANES M                     FIFO records: save, load into another stream, the refusals; "ok"
//   exit 1 and a message on the first difference
// The frames' "denoiser" between the two steps is y = x / 2 + 3 on the present frames only: the steps move samples, nothing else.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <vector>

#include "../../rnnoise_amd/csrc/chunk_fifo.h"

namespace {
uint32_t rng_state = 0x9e3779b9u;
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
int fail(const char *what, int call, int s, long i) {
  fprintf(stderr, "chunk_list_test: call %d stream/row %d: %s at %ld\n", call, s, what, i);
  return 1;
}
bool same(float a, float b) { return !memcmp(&a, &b, 4); }
short cast_s16(float v) { return (short)((v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000); }

const int S = 7;  // streams of the "batch"
const float POISON_F = 12345.25f;
const short POISON_S = -21846;

// one call through the bodies: the list forms where `list` is given, the full-size ones otherwise (then rows == S)
void run_scatter(const RnChunkDev &c, int nt, bool down) {
  auto lane = [&](int i) { return down ? nt - 1 - i : i; };
  for (int row = 0; row < c.N; row++) {
    std::vector<RnChunkHead> h(nt);
    if (c.list) {
      const int s = rn_chunk_row_stream(c, row);
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_list_scatter_head(c, row, s);
        rn_chunk_list_scatter_frames(c, row, s, h[lane(i)], lane(i), nt);
      }
      for (int i = 0; i < nt; i++) rn_chunk_list_scatter_tail(c, row, s, h[lane(i)], lane(i), nt);
    } else {
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_scatter_head(c, row);
        rn_chunk_scatter_frames(c, row, h[lane(i)], lane(i), nt);
      }
      for (int i = 0; i < nt; i++) rn_chunk_scatter_tail(c, row, h[lane(i)], lane(i), nt);
    }
  }
}
void run_gather(const RnChunkDev &c, float *kept, int nt, bool down) {
  auto lane = [&](int i) { return down ? nt - 1 - i : i; };
  for (int row = 0; row < c.N; row++) {
    std::vector<RnChunkHead> h(nt);
    if (c.list) {
      const int s = rn_chunk_row_stream(c, row);
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_list_gather_head(c, row, s);
        rn_chunk_list_gather_pop(c, row, s, h[lane(i)], kept, lane(i), nt);
      }
      for (int i = 0; i < nt; i++) rn_chunk_list_gather_keep(c, row, s, h[lane(i)], kept, lane(i), nt);
    } else {
      for (int i = 0; i < nt; i++) {
        h[lane(i)] = rn_chunk_gather_head(c, row);
        rn_chunk_gather_pop(c, row, h[lane(i)], kept, lane(i), nt);
      }
      for (int i = 0; i < nt; i++) rn_chunk_gather_keep(c, row, h[lane(i)], kept, lane(i), nt);
    }
  }
}

int calls_main(bool mixed, int nt, int M, int max_count, int s16, int alias) {
  const int CALLS = 40, F = rn_chunk_frames(M, max_count);
  const size_t esz = s16 ? sizeof(short) : sizeof(float);
  Block<float> fifo((size_t)S * RN_CHUNK_REC), kept(M);
  memset(fifo.p, 0, fifo.n * sizeof(float));  // (chunk_plan.h: a record of zeros is a restarted stream)
  std::deque<float> in_q[S], out_q[S];
  for (int s = 0; s < S; s++) out_q[s].assign(M, 0.f);
  long total_frames = 0, absent_rows = 0;

  for (int call = 0; call < CALLS; call++) {
    const bool full = mixed && call % 3 == 1;
    // the list: 0 .. 5 distinct streams in shuffled order; every fourth list call one entry names a stream outside the batch
    int perm[S];
    for (int s = 0; s < S; s++) perm[s] = s;
    for (int s = S - 1; s > 0; s--) std::swap(perm[s], perm[rnd() % (s + 1)]);
    const int R = full ? S : (int)(rnd() % 6);
    Block<int> list(R), counts(R), frames(R);
    std::vector<int> row_stream(R);  // -1: absent
    for (int i = 0; i < R; i++) row_stream[i] = list.p[i] = full ? i : perm[i];
    if (!full && R > 0 && call % 4 == 2) {
      const int i = rnd() % R;
      list.p[i] = (rnd() & 1) ? S + (int)(rnd() % 3) : -1 - (int)(rnd() % 3);
      row_stream[i] = -1;
      absent_rows++;
    }
    // the buffers of THIS call, exactly as large as its rows make them
    Block<float> stage((size_t)F * R * M);
    Block<unsigned char> active((size_t)F * R);
    Block<char> in((size_t)R * max_count * esz), out_own((size_t)R * max_count * esz);
    char *out = alias ? in.p : out_own.p;
    // the counts: anything in [0, max_count], often an edge -- nothing, everything, up to a frame boundary, one sample either side
    std::vector<int> means(R);
    for (int i = 0; i < R; i++) {
      const int s = row_stream[i], r = s < 0 ? 0 : (int)in_q[s].size(), pick = rnd() % 8;
      int n = rnd() % (max_count + 1);
      if (pick == 0) n = 0;
      else if (pick == 1) n = max_count;
      else if (pick == 2) n = M - r;
      else if (pick == 3) n = M - r - 1;
      else if (pick == 4) n = M - r + 1;
      means[i] = n < 0 ? 0 : n > max_count ? max_count : n;
      counts.p[i] = means[i];
      // (a device count out of range reads clamped)
      if (call % 5 == 1 && means[i] == 0) counts.p[i] = -3;
      if (call % 5 == 2 && means[i] == max_count) counts.p[i] = max_count + 5;
      frames.p[i] = -9;
    }
    for (int i = 0; i < R; i++)
      for (int x = 0; x < max_count; x++) {
        const bool live = x < means[i];
        if (s16) {
          reinterpret_cast<short *>(in.p)[(size_t)i * max_count + x] = live ? (short)(rnd() & 0xffff) : POISON_S;
          if (!alias) reinterpret_cast<short *>(out)[(size_t)i * max_count + x] = POISON_S;
        } else {
          reinterpret_cast<float *>(in.p)[(size_t)i * max_count + x] = live ? ((int)(rnd() % 60001) - 30000) + (rnd() % 8) * .125f : POISON_F;
          if (!alias) reinterpret_cast<float *>(out)[(size_t)i * max_count + x] = POISON_F;
        }
      }
    const std::vector<char> in_before(in.p, in.p + in.n);
    for (size_t i = 0; i < stage.n; i++) stage.p[i] = -777.f;  // (an absent frame's slot: read by nobody)
    memset(active.p, 0xee, active.n);
    const std::vector<float> fifo_before(fifo.p, fifo.p + fifo.n);

    RnChunkDev c{};
    c.fifo = fifo.p;
    c.M = M;
    c.N = R;
    c.max_count = max_count;
    c.F = F;
    c.s16 = s16;
    c.counts = counts.p;
    c.in = in.p;
    c.out = out;
    c.stage = stage.p;
    c.active = active.p;
    c.frames = frames.p;
    c.list = full ? nullptr : list.p;
    c.S = S;

    // ---- step 1: scatter ----
    run_scatter(c, nt, call & 1);
    std::vector<std::vector<std::vector<float>>> want_frames(R);
    for (int i = 0; i < R; i++) {
      const int s = row_stream[i];
      if (s >= 0) {
        for (int x = 0; x < means[i]; x++)
          in_q[s].push_back(s16 ? (float)reinterpret_cast<const short *>(in_before.data())[(size_t)i * max_count + x]
                                : reinterpret_cast<const float *>(in_before.data())[(size_t)i * max_count + x]);
        while ((int)in_q[s].size() >= M) {
          want_frames[i].emplace_back(in_q[s].begin(), in_q[s].begin() + M);
          in_q[s].erase(in_q[s].begin(), in_q[s].begin() + M);
        }
      }
      const int k = (int)want_frames[i].size();
      if (k > F) return fail("more frames than rows", call, i, k);
      if (frames.p[i] != k) return fail("frames[row]", call, i, frames.p[i]);
      for (int j = 0; j < F; j++) {
        if (active.p[(size_t)j * R + i] != (j < k)) return fail("mask", call, i, j);
        for (int x = 0; x < M; x++) {
          const float got = stage.p[((size_t)j * R + i) * M + x];
          if (!same(got, j < k ? want_frames[i][j][x] : -777.f)) return fail("staged frame", call, i, (long)j * M + x);
        }
      }
      if (s < 0) continue;
      if (*rn_chunk_fill(c, s) != (int)in_q[s].size()) return fail("input fill", call, s, *rn_chunk_fill(c, s));
      for (size_t x = 0; x < in_q[s].size(); x++)
        if (!same(rn_chunk_in_fifo(c, s)[x], in_q[s][x])) return fail("input tail", call, s, (long)x);
    }

    // ---- step 2: the frames' processing, present frames only, in place ----
    for (int i = 0; i < R; i++)
      for (size_t j = 0; j < want_frames[i].size(); j++, total_frames++)
        for (int x = 0; x < M; x++) {
          float &v = stage.p[(j * R + i) * M + x];
          v = denoise(v);
          out_q[row_stream[i]].push_back(v);
        }

    // ---- step 3: gather ----
    run_gather(c, kept.p, nt, call & 1);
    for (int i = 0; i < R; i++) {
      const int s = row_stream[i], n = s < 0 ? 0 : means[i];
      if (s >= 0 && (int)out_q[s].size() < n) return fail("the model ran dry", call, s, n);
      for (int x = 0; x < max_count; x++) {
        // behind the count, and in every sample of an absent row: the caller's bytes (the input's own where `in` is `out`)
        if (s16) {
          const short got = reinterpret_cast<short *>(out)[(size_t)i * max_count + x];
          const short keep = alias ? reinterpret_cast<const short *>(in_before.data())[(size_t)i * max_count + x] : POISON_S;
          if (got != (x < n ? cast_s16(out_q[s][x]) : keep)) return fail(x < n ? "output sample" : "a sample outside the count was written", call, i, x);
        } else {
          const float got = reinterpret_cast<float *>(out)[(size_t)i * max_count + x];
          const float keep = alias ? reinterpret_cast<const float *>(in_before.data())[(size_t)i * max_count + x] : POISON_F;
          if (!same(got, x < n ? out_q[s][x] : keep)) return fail(x < n ? "output sample" : "a sample outside the count was written", call, i, x);
        }
      }
      if (s < 0) continue;
      out_q[s].erase(out_q[s].begin(), out_q[s].begin() + n);
      if ((int)out_q[s].size() != M - (int)in_q[s].size()) return fail("out_fill != M - in_fill in the model", call, s, (long)out_q[s].size());
      for (size_t x = 0; x < out_q[s].size(); x++)
        if (!same(rn_chunk_out_fifo(c, s)[x], out_q[s][x])) return fail("output tail", call, s, (long)x);
    }
    // ---- the records of the unlisted streams: byte for byte what they were ----
    for (int s = 0; s < S; s++) {
      if (std::find(row_stream.begin(), row_stream.end(), s) != row_stream.end()) continue;
      if (memcmp(fifo.p + (size_t)s * RN_CHUNK_REC, fifo_before.data() + (size_t)s * RN_CHUNK_REC, RN_CHUNK_REC * sizeof(float)))
        return fail("the record of an unlisted stream changed", call, s, 0);
    }
  }
  printf("ok %d %ld %ld\n", CALLS, total_frames, absent_rows);
  return 0;
}

int records_main(int nt, int M) {
  Block<float> fifo((size_t)S * RN_CHUNK_REC);
  // FIFOs as calls leave them: r samples pending, M - r to give out, stale samples of earlier calls behind both, NaNs with payloads
  // among the live ones
  const int fills[S] = {0, 1, M / 2, M - 1, 7 % M, M - 2 > 0 ? M - 2 : 0, 3 % M};
  for (int s = 0; s < S; s++) {
    float *f = fifo.p + (size_t)s * RN_CHUNK_REC;
    for (int i = 0; i < 2 * RN_CHUNK_FIFO_ROW; i++) f[i] = (float)((int)(rnd() % 60001) - 30000) + .5f;
    const uint32_t nan_bits = 0x7fc12345u + s;
    if (fills[s] > 0) memcpy(f + fills[s] - 1, &nan_bits, 4);
    memcpy(f + RN_CHUNK_FIFO_ROW + (M - fills[s]) - 1, &nan_bits, 4);
    reinterpret_cast<int *>(f)[RN_CHUNK_OFF_FILL] = fills[s];
    for (int w = 1; w < 4; w++) reinterpret_cast<int *>(f)[RN_CHUNK_OFF_FILL + w] = 0x5a5a5a5a;  // (the padding: never read, never written)
  }
  const std::vector<float> fifo_before(fifo.p, fifo.p + fifo.n);
  auto run = [&](const RnChunkDev &c, bool load) {
    for (int row = 0; row < c.N; row++)
      for (int i = 0; i < nt; i++) load ? rn_chunk_rec_load(c, row, nt - 1 - i, nt) : rn_chunk_rec_save(c, row, i, nt);
  };
  // ---- save: the list in any order, one entry outside the batch ----
  const int order[5] = {4, 0, S + 2, 3, 6};
  Block<int> list(5);
  memcpy(list.p, order, sizeof order);
  Block<float> rec((size_t)5 * RN_CHUNK_REC), rec2((size_t)5 * RN_CHUNK_REC);
  RnChunkDev c{};
  c.fifo = fifo.p;
  c.M = M;
  c.N = 5;
  c.list = list.p;
  c.S = S;
  c.op = RN_CHUNK_OP_SAVE;
  for (Block<float> *b : {&rec, &rec2}) {
    memset(b->p, b == &rec ? 0xa5 : 0x3c, b->n * sizeof(float));  // (whatever the caller's memory held)
    c.rec = b->p;
    run(c, false);
  }
  if (memcmp(fifo.p, fifo_before.data(), fifo.n * sizeof(float))) return fail("save changed the batch", 0, 0, 0);
  for (int i = 0; i < 5; i++) {
    const float *r = rec.p + (size_t)i * RN_CHUNK_REC;
    const int *h = reinterpret_cast<const int *>(r);
    if (order[i] >= S) {  // magic 0, the rest of the row as it was
      if (h[RN_CHUNK_OFF_MAGIC] != 0) return fail("save: an entry outside the batch keeps a magic word", 0, i, 0);
      for (int w = 0; w < RN_CHUNK_REC; w++)
        if (w != RN_CHUNK_OFF_MAGIC && (uint32_t)h[w] != 0xa5a5a5a5u) return fail("save: an absent row was written", 0, i, w);
      continue;
    }
    if (memcmp(r, rec2.p + (size_t)i * RN_CHUNK_REC, RN_CHUNK_REC * sizeof(float))) return fail("save: two saves differ", 0, i, 0);
    const float *f = fifo_before.data() + (size_t)order[i] * RN_CHUNK_REC;
    const int fill = fills[order[i]];
    if (h[RN_CHUNK_OFF_FILL] != fill || h[RN_CHUNK_OFF_M] != M || h[RN_CHUNK_OFF_MAGIC] != RN_CHUNK_MAGIC || h[RN_CHUNK_OFF_MAGIC + 1] != 0)
      return fail("save: header", 0, i, 0);
    for (int w = 0; w < RN_CHUNK_FIFO_ROW; w++) {
      if (!same(r[w], w < fill ? f[w] : 0.f)) return fail("save: pending samples, zeros behind them", 0, i, w);
      if (!same(r[RN_CHUNK_FIFO_ROW + w], w < M - fill ? f[RN_CHUNK_FIFO_ROW + w] : 0.f)) return fail("save: output FIFO, zeros behind it", 0, i, w);
    }
  }
  // ---- a batch without FIFOs saves restarted records ----
  {
    RnChunkDev none{};
    none.M = M;
    none.N = 2;
    none.S = S;
    none.op = RN_CHUNK_OP_SAVE;
    none.rec = rec2.p;
    memset(rec2.p, 0x77, rec2.n * sizeof(float));
    run(none, false);
    for (int i = 0; i < 2; i++) {
      const int *h = reinterpret_cast<const int *>(rec2.p + (size_t)i * RN_CHUNK_REC);
      for (int w = 0; w < RN_CHUNK_REC; w++)
        if (h[w] != (w == RN_CHUNK_OFF_M ? M : w == RN_CHUNK_OFF_MAGIC ? RN_CHUNK_MAGIC : 0)) return fail("save without FIFOs", 0, i, w);
    }
  }
  // ---- load into other streams: 4 -> 1, 0 -> 5, (absent row), 3 -> 2, 6 -> outside the batch ----
  const int dest[5] = {1, 5, 0, 2, -1};
  memcpy(list.p, dest, sizeof dest);
  c.op = RN_CHUNK_OP_LOAD;
  c.rec = rec.p;
  run(c, true);
  for (int s = 0; s < S; s++) {
    const float *now = fifo.p + (size_t)s * RN_CHUNK_REC, *was = fifo_before.data() + (size_t)s * RN_CHUNK_REC;
    int from = -1;
    for (int i = 0; i < 5; i++)
      if (dest[i] == s && order[i] < S) from = order[i];
    if (from < 0) {  // not a destination, or the destination of the empty record
      if (memcmp(now, was, RN_CHUNK_REC * sizeof(float))) return fail("load touched a stream it had no record for", 1, s, 0);
      continue;
    }
    const float *src = fifo_before.data() + (size_t)from * RN_CHUNK_REC;
    const int fill = fills[from];
    if (reinterpret_cast<const int *>(now)[RN_CHUNK_OFF_FILL] != fill) return fail("load: fill", 1, s, 0);
    for (int w = 0; w < fill; w++)
      if (!same(now[w], src[w])) return fail("load: pending samples", 1, s, w);
    for (int w = 0; w < M - fill; w++)
      if (!same(now[RN_CHUNK_FIFO_ROW + w], src[RN_CHUNK_FIFO_ROW + w])) return fail("load: output FIFO", 1, s, w);
  }
  // ---- the refusals: another magic word, another M, r = -1, r = M -- nothing is touched ----
  const std::vector<float> fifo_loaded(fifo.p, fifo.p + fifo.n);
  for (int bad = 0; bad < 4; bad++) {
    Block<float> one(RN_CHUNK_REC);
    memcpy(one.p, rec.p, RN_CHUNK_REC * sizeof(float));  // (stream 4's record)
    int *h = reinterpret_cast<int *>(one.p);
    if (bad == 0) h[RN_CHUNK_OFF_MAGIC] ^= 0x100;
    if (bad == 1) h[RN_CHUNK_OFF_M] = M == 480 ? 160 : 480;
    if (bad == 2) h[RN_CHUNK_OFF_FILL] = -1;
    if (bad == 3) h[RN_CHUNK_OFF_FILL] = M;
    Block<int> to(1);
    to.p[0] = 3;
    RnChunkDev l = c;
    l.N = 1;
    l.list = to.p;
    l.rec = one.p;
    run(l, true);
    if (memcmp(fifo.p, fifo_loaded.data(), fifo.n * sizeof(float))) return fail("a refused record was loaded", 2, bad, 0);
  }
  // ---- no list: row i is stream i ----
  {
    Block<float> all((size_t)S * RN_CHUNK_REC);
    RnChunkDev a{};
    a.fifo = fifo.p;
    a.M = M;
    a.N = S;
    a.S = S;
    a.op = RN_CHUNK_OP_SAVE;
    a.rec = all.p;
    run(a, false);
    for (int s = 0; s < S; s++)
      if (reinterpret_cast<const int *>(all.p + (size_t)s * RN_CHUNK_REC)[RN_CHUNK_OFF_FILL] != reinterpret_cast<const int *>(fifo.p + (size_t)s * RN_CHUNK_REC)[RN_CHUNK_OFF_FILL])
        return fail("save without a list", 3, s, 0);
  }
  printf("ok\n");
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const bool mixed = !strcmp(argv[1], "mixed");
  if (!strcmp(argv[1], "records")) {
    if (argc != 4) return 2;
    const int nt = atoi(argv[2]), M = atoi(argv[3]);
    if (nt <= 0 || M <= 1 || M > RN_CHUNK_FIFO_ROW) return 2;
    return records_main(nt, M);
  }
  if ((!mixed && strcmp(argv[1], "list")) || argc != 7) return 2;
  const int nt = atoi(argv[2]), M = atoi(argv[3]), max_count = atoi(argv[4]), s16 = atoi(argv[5]), alias = atoi(argv[6]);
  if (nt <= 0 || M <= 0 || M > RN_CHUNK_FIFO_ROW || max_count <= 0) return 2;
  return calls_main(mixed, nt, M, max_count, s16, alias);
}
