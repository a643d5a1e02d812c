// chunk_fifo.h -- the per-stream bodies of a chunk call's two staging steps (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks;
// chunk_plan.h has the rule), which rn_state_scatter_kernel and rn_state_gather_kernel run as their third record kind, one workgroup
// per stream.  Every body is written for lane t of nt and in two halves with ONE barrier of the workgroup between them, which the
// caller places: everything a half reads of a FIFO that the other half rewrites in place is read before the barrier.  A plain host
// program can therefore run a body lane after lane, first halves, then second halves (tests/csrc/chunk_fifo_test.cpp).
//
//   scatter   cat = in_fifo[0, r) ++ in[s][0, n): frames j < k of cat go to the staging buffer, the mask column of the stream is
//             written whole, the tail cat[k M, r + n) becomes the input FIFO.
//   gather    vout = out_fifo[0, M - r) ++ staged frames [0, k): out[s][0, n) = vout[0, n), the rest becomes the output FIFO.
//
// The caller's rows are max_count samples apart and aligned as their element only, so every access to them is one element.  Samples
// are float in both FIFOs and in the staging buffer; an int16 call converts where it reads `in` (exact) and where it writes `out`,
// with the truncating cast K3 applies to its own int16 rows (dsp_kernels.hip: synthesis_body) -- a float call followed by that cast.
#pragma once
#include <stddef.h>
#include "chunk_plan.h"
#ifdef __HIPCC__
#define RN_CHUNK_FN __device__ __forceinline__
#else
#define RN_CHUNK_FN static inline
#endif

RN_CHUNK_FN float rn_chunk_load(const void *row, int i, int s16) {
  return s16 ? (float)static_cast<const short *>(row)[i] : static_cast<const float *>(row)[i];
}
RN_CHUNK_FN void rn_chunk_store(void *row, int i, float v, int s16) {
  if (s16) {
    const int q = (v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000;
    static_cast<short *>(row)[i] = (short)q;
  } else {
    static_cast<float *>(row)[i] = v;
  }
}
// row s of the caller's `in` / `out`
RN_CHUNK_FN const void *rn_chunk_row(const void *base, size_t s, int max_count, int s16) {
  return static_cast<const char *>(base) + s * (size_t)max_count * (s16 ? sizeof(short) : sizeof(float));
}
// sample x of the stream's staged frames, frame after frame
RN_CHUNK_FN float *rn_chunk_staged(const RnChunkDev &c, size_t s, int x) {
  const int j = x / c.M;
  return c.stage + ((size_t)j * c.N + s) * c.M + (x - j * c.M);
}

// the three parts of stream s's record (chunk_plan.h: RN_CHUNK_REC)
RN_CHUNK_FN float *rn_chunk_in_fifo(const RnChunkDev &c, size_t s) { return c.fifo + s * RN_CHUNK_REC; }
RN_CHUNK_FN float *rn_chunk_out_fifo(const RnChunkDev &c, size_t s) { return c.fifo + s * RN_CHUNK_REC + RN_CHUNK_FIFO_ROW; }
RN_CHUNK_FN int *rn_chunk_fill(const RnChunkDev &c, size_t s) {
  return reinterpret_cast<int *>(c.fifo + s * RN_CHUNK_REC + 2 * RN_CHUNK_FIFO_ROW);
}

// What every lane reads before it writes anything: the fill of the FIFO its body rewrites, as the call found it, and the count.
// Scatter: the pending samples r.  Gather: the output FIFO's M - r, from the fill the scatter step has left
struct RnChunkHead {
  int fill, n;
};
RN_CHUNK_FN RnChunkHead rn_chunk_scatter_head(const RnChunkDev &c, size_t s) {
  const int r = *rn_chunk_fill(c, s);
  return {r < 0 ? 0 : r >= c.M ? c.M - 1 : r, rn_chunk_count(c.counts[s], c.max_count)};
}
RN_CHUNK_FN RnChunkHead rn_chunk_gather_head(const RnChunkDev &c, size_t s) {
  RnChunkHead h = rn_chunk_scatter_head(c, s);
  h.fill = c.M - rn_chunk_fill_before(c.M, h.fill, h.n);
  return h;
}

// ---- scatter ----
// before the barrier: the k frames (the only reader of the pending samples, which go into frame 0), the mask, frames[s]
RN_CHUNK_FN void rn_chunk_scatter_frames(const RnChunkDev &c, size_t s, RnChunkHead h, int t, int nt) {
  const int r = h.fill, M = c.M, k = rn_chunk_push(M, r, h.n).k;
  const float *fifo = rn_chunk_in_fifo(c, s);
  const void *in = rn_chunk_row(c.in, s, c.max_count, c.s16);
  for (int j = 0; j < k; j++) {
    float *f = c.stage + ((size_t)j * c.N + s) * M;
    for (int i = t; i < M; i += nt) {
      const int x = j * M + i;
      f[i] = x < r ? fifo[x] : rn_chunk_load(in, x - r, c.s16);
    }
  }
  for (int j = t; j < c.F; j += nt) c.active[(size_t)j * c.N + s] = j < k;
  if (t == 0 && c.frames) c.frames[s] = k;
}
// after it: the tail of `in` as the pending samples -- appended where no frame completed, from the FIFO's start otherwise
RN_CHUNK_FN void rn_chunk_scatter_tail(const RnChunkDev &c, size_t s, RnChunkHead h, int t, int nt) {
  const int r = h.fill;
  const RnChunkPush p = rn_chunk_push(c.M, r, h.n);
  float *fifo = rn_chunk_in_fifo(c, s);
  const void *in = rn_chunk_row(c.in, s, c.max_count, c.s16);
  if (p.k == 0) {
    for (int i = t; i < h.n; i += nt) fifo[r + i] = rn_chunk_load(in, i, c.s16);
  } else {
    const int x0 = p.k * c.M - r;
    for (int i = t; i < p.in_fill; i += nt) fifo[i] = rn_chunk_load(in, x0 + i, c.s16);
  }
  if (t == 0) *rn_chunk_fill(c, s) = p.in_fill;
}

// ---- gather ----
// before the barrier: the n samples out, and what of the FIFO stays (only where no frame completed: n < fill) into tmp[0, fill - n),
// M floats the workgroup shares
RN_CHUNK_FN void rn_chunk_gather_pop(const RnChunkDev &c, size_t s, RnChunkHead h, float *tmp, int t, int nt) {
  const int of = h.fill, n = h.n;
  const float *fifo = rn_chunk_out_fifo(c, s);
  void *out = const_cast<void *>(rn_chunk_row(c.out, s, c.max_count, c.s16));
  for (int i = t; i < n; i += nt) rn_chunk_store(out, i, i < of ? fifo[i] : *rn_chunk_staged(c, s, i - of), c.s16);
  for (int i = n + t; i < of; i += nt) tmp[i - n] = fifo[i];
}
// after it: vout[n, fill + k M) as the output FIFO
RN_CHUNK_FN void rn_chunk_gather_keep(const RnChunkDev &c, size_t s, RnChunkHead h, const float *tmp, int t, int nt) {
  const int of = h.fill, n = h.n;
  const int left = rn_chunk_push(c.M, c.M - of, n).out_fill;
  float *fifo = rn_chunk_out_fifo(c, s);
  for (int j = t; j < left; j += nt) fifo[j] = j + n < of ? tmp[j] : *rn_chunk_staged(c, s, j + n - of);
}

// ---- restart ----
// stream s's FIFOs as a new stream has them: nothing pending, M zeros to give out.  Nothing where the batch has no FIFOs
RN_CHUNK_FN void rn_chunk_restart(const RnChunkDev &c, size_t s, int t, int nt) {
  if (!c.fifo) return;
  float *out = rn_chunk_out_fifo(c, s);
  for (int i = t; i < RN_CHUNK_FIFO_ROW; i += nt) out[i] = 0.f;
  if (t == 0) *rn_chunk_fill(c, s) = 0;
}
