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
// A call on a stream list runs the same two steps with a row distinct from the stream (the list forms below), and two more bodies
// move a stream's FIFOs to and from a saved record.
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

// ---- the same two steps on a stream list (chunk_plan.h: RnChunkDev::list) ----
// Row `row` of the caller's buffers, of counts / frames and of the staging buffer and its mask -- all c.N rows -- belongs to stream
// list[row], whose FIFO record is indexed by stream.  The same halves around the same barrier; every loop runs over one frame or one
// FIFO, so no sample costs a division.  An entry outside the batch makes its row absent: s < 0 below.
RN_CHUNK_FN int rn_chunk_row_stream(const RnChunkDev &c, int row) {
  const int s = c.list ? c.list[row] : row;
  return s >= 0 && s < c.S ? s : -1;
}
RN_CHUNK_FN RnChunkHead rn_chunk_list_scatter_head(const RnChunkDev &c, int row, int s) {
  if (s < 0) return {0, 0};
  const int r = *rn_chunk_fill(c, s);
  return {r < 0 ? 0 : r >= c.M ? c.M - 1 : r, rn_chunk_count(c.counts[row], c.max_count)};
}
RN_CHUNK_FN RnChunkHead rn_chunk_list_gather_head(const RnChunkDev &c, int row, int s) {
  RnChunkHead h = rn_chunk_list_scatter_head(c, row, s);
  h.fill = c.M - rn_chunk_fill_before(c.M, h.fill, h.n);
  return h;
}
RN_CHUNK_FN float *rn_chunk_list_frame(const RnChunkDev &c, int row, int j) { return c.stage + ((size_t)j * c.N + row) * c.M; }

// before the barrier.  An absent row: a zero mask column and frames[row] = 0, nothing else
RN_CHUNK_FN void rn_chunk_list_scatter_frames(const RnChunkDev &c, int row, int s, RnChunkHead h, int t, int nt) {
  const int r = h.fill, M = c.M, k = s < 0 ? 0 : rn_chunk_push(M, r, h.n).k;
  for (int j = t; j < c.F; j += nt) c.active[(size_t)j * c.N + row] = j < k;
  if (t == 0 && c.frames) c.frames[row] = k;
  if (k == 0) return;
  const float *fifo = rn_chunk_in_fifo(c, s);
  const void *in = rn_chunk_row(c.in, row, c.max_count, c.s16);
  float *f = rn_chunk_list_frame(c, row, 0);  // (the pending samples go into frame 0)
  for (int i = t; i < M; i += nt) f[i] = i < r ? fifo[i] : rn_chunk_load(in, i - r, c.s16);
  for (int j = 1; j < k; j++) {
    f = rn_chunk_list_frame(c, row, j);
    for (int i = t; i < M; i += nt) f[i] = rn_chunk_load(in, j * M - r + i, c.s16);
  }
}
// after it
RN_CHUNK_FN void rn_chunk_list_scatter_tail(const RnChunkDev &c, int row, int s, RnChunkHead h, int t, int nt) {
  if (s < 0) return;
  const int r = h.fill;
  const RnChunkPush p = rn_chunk_push(c.M, r, h.n);
  float *fifo = rn_chunk_in_fifo(c, s);
  const void *in = rn_chunk_row(c.in, row, c.max_count, c.s16);
  if (p.k == 0) {
    for (int i = t; i < h.n; i += nt) fifo[r + i] = rn_chunk_load(in, i, c.s16);
  } else {
    const int x0 = p.k * c.M - r;
    for (int i = t; i < p.in_fill; i += nt) fifo[i] = rn_chunk_load(in, x0 + i, c.s16);
  }
  if (t == 0) *rn_chunk_fill(c, s) = p.in_fill;
}
// before the barrier: out[row][0, n) = the output FIFO's `of` samples, then the k frames one after the other; what of the FIFO stays
// (only where no frame completed) into tmp
RN_CHUNK_FN void rn_chunk_list_gather_pop(const RnChunkDev &c, int row, int s, RnChunkHead h, float *tmp, int t, int nt) {
  if (s < 0) return;
  const int of = h.fill, n = h.n, M = c.M, k = rn_chunk_push(M, M - of, n).k;
  const float *fifo = rn_chunk_out_fifo(c, s);
  void *out = const_cast<void *>(rn_chunk_row(c.out, row, c.max_count, c.s16));
  for (int i = t; i < n && i < of; i += nt) rn_chunk_store(out, i, fifo[i], c.s16);
  for (int j = 0; j < k; j++) {
    const float *f = rn_chunk_list_frame(c, row, j);
    const int at = of + j * M;
    for (int i = t; i < M && at + i < n; i += nt) rn_chunk_store(out, at + i, f[i], c.s16);
  }
  for (int i = n + t; i < of; i += nt) tmp[i - n] = fifo[i];
}
// after it: with k > 0 the FIFO is the end of the last frame, from the new input fill on (r + n = k M + in_fill)
RN_CHUNK_FN void rn_chunk_list_gather_keep(const RnChunkDev &c, int row, int s, RnChunkHead h, const float *tmp, int t, int nt) {
  if (s < 0) return;
  const RnChunkPush p = rn_chunk_push(c.M, c.M - h.fill, h.n);
  float *fifo = rn_chunk_out_fifo(c, s);
  if (p.k == 0) {
    for (int j = t; j < p.out_fill; j += nt) fifo[j] = tmp[j];
  } else {
    const float *f = rn_chunk_list_frame(c, row, p.k - 1) + p.in_fill;
    for (int j = t; j < p.out_fill; j += nt) fifo[j] = f[j];
  }
}

// ---- FIFO records (chunk_plan.h: RN_CHUNK_OFF_*) ----
// Neither body rewrites what it reads: one half, no barrier.  Samples move as the bits they are.
// rec[row] <- the FIFOs of the row's stream: zeros outside the two valid ranges, so that equal FIFOs save as equal bytes; a batch
// without FIFOs saves restarted ones.  An entry outside the batch: magic 0, nothing else
RN_CHUNK_FN void rn_chunk_rec_save(const RnChunkDev &c, int row, int t, int nt) {
  float *rec = c.rec + (size_t)row * RN_CHUNK_REC;
  int *hdr = reinterpret_cast<int *>(rec);
  const int s = rn_chunk_row_stream(c, row), M = c.M;
  if (s < 0) {
    if (t == 0) hdr[RN_CHUNK_OFF_MAGIC] = 0;
    return;
  }
  int r = c.fifo ? *rn_chunk_fill(c, s) : 0;
  r = r < 0 ? 0 : r >= M ? M - 1 : r;
  for (int i = t; i < RN_CHUNK_REC; i += nt) {
    if (i >= RN_CHUNK_OFF_FILL) {
      hdr[i] = i == RN_CHUNK_OFF_FILL ? r : i == RN_CHUNK_OFF_M ? M : i == RN_CHUNK_OFF_MAGIC ? RN_CHUNK_MAGIC : 0;
    } else {
      const bool live = c.fifo && (i < RN_CHUNK_FIFO_ROW ? i < r : i - RN_CHUNK_FIFO_ROW < M - r);
      rec[i] = live ? c.fifo[(size_t)s * RN_CHUNK_REC + i] : 0.f;
    }
  }
}
// the FIFOs of the row's stream <- rec[row], where the record is one of this frame length (rn_chunk_rec_ok); nothing otherwise
RN_CHUNK_FN void rn_chunk_rec_load(const RnChunkDev &c, int row, int t, int nt) {
  const float *rec = c.rec + (size_t)row * RN_CHUNK_REC;
  const int *hdr = reinterpret_cast<const int *>(rec);
  const int s = rn_chunk_row_stream(c, row), M = c.M;
  if (s < 0 || !c.fifo) return;
  const int r = hdr[RN_CHUNK_OFF_FILL];
  if (!rn_chunk_rec_ok(hdr[RN_CHUNK_OFF_MAGIC], hdr[RN_CHUNK_OFF_M], r, M)) return;
  float *in = rn_chunk_in_fifo(c, s), *out = rn_chunk_out_fifo(c, s);
  for (int i = t; i < r; i += nt) in[i] = rec[i];
  for (int i = t; i < M - r; i += nt) out[i] = rec[RN_CHUNK_FIFO_ROW + i];
  if (t == 0) *rn_chunk_fill(c, s) = r;
}

// ---- restart ----
// stream s's FIFOs as a new stream has them: nothing pending, M zeros to give out.  Nothing where the batch has no FIFOs
RN_CHUNK_FN void rn_chunk_restart(const RnChunkDev &c, size_t s, int t, int nt) {
  if (!c.fifo) return;
  float *out = rn_chunk_out_fifo(c, s);
  for (int i = t; i < RN_CHUNK_FIFO_ROW; i += nt) out[i] = 0.f;
  if (t == 0) *rn_chunk_fill(c, s) = 0;
}
