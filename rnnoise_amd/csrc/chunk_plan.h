// chunk_plan.h -- the arithmetic of a chunk call (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks), as pure functions of the
// frame length M and a stream's fill and count, and what the two state kernels get for it (no HIP in here, as in dispatch.h, so that
// tests/test_chunks_cpu.py can run the rule at every fill and count without a GPU).
//
// Every stream owns an input FIFO of r pending samples, 0 <= r < M, and an output FIFO of M - r samples (M zeros and r = 0 after a
// restart).  A push of n samples completes k = (r + n) / M frames and leaves (r + n) % M samples pending; the k frames' outputs are
// appended to the output FIFO, whose first n samples are the push's result.  It always holds that many: before the pop it has
// (M - r) + k M samples, and k M > r + n - M.  After the pop it holds M - (r + n) % M: the invariant out_fill = M - in_fill.
#pragma once

// the frame rows of vad / gains (and of the staging buffer) a push of at most max_count samples can complete: the fullest FIFO,
// M - 1 samples, and max_count more.  0 for max_count == 0; -1 for a bad argument
static inline int rn_chunk_frames(int M, int max_count) {
  if (M <= 0 || max_count < 0) return -1;
  return (int)(((long long)M - 1 + max_count) / M);
}
// a count as the device forms read it: a negative entry is 0, one above max_count is max_count
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int rn_chunk_count(int n, int max_count) { return n < 0 ? 0 : n > max_count ? max_count : n; }

// one push of n samples (0 <= n) into a stream whose input FIFO holds r (0 <= r < M)
struct RnChunkPush {
  int k;         // frames the push completes
  int in_fill;   // samples pending afterwards
  int avail;     // samples in the output FIFO once the k frames are appended, before the n are popped (>= n)
  int out_fill;  // ... and after the pop: M - in_fill
};
#ifdef __HIPCC__
__host__ __device__
#endif
static inline RnChunkPush rn_chunk_push(int M, int r, int n) {
  RnChunkPush p;
  p.k = (r + n) / M;
  p.in_fill = r + n - p.k * M;
  p.avail = M - r + p.k * M;
  p.out_fill = p.avail - n;
  return p;
}

// the fill a push of n samples found, from the fill it left: the gather step runs behind the scatter step, which has stored the new one
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int rn_chunk_fill_before(int M, int in_fill, int n) {
  const int d = (in_fill - n) % M;
  return d < 0 ? d + M : d;
}

// A stream's FIFOs are one record of RN_CHUNK_REC floats: [0, 480) the pending input samples, [480, 960) the output FIFO -- rows of the
// longest frame (RN_FRAME_SIZE) whatever the batch's rate --, then the input fill r as an int32 and three words of padding (16-byte
// rows).  The output FIFO's fill is not stored: it is M - r between calls.  A record of zeros is a restarted stream.
#define RN_CHUNK_FIFO_ROW 480
#define RN_CHUNK_REC (2 * RN_CHUNK_FIFO_ROW + 4)
// What rn_state_scatter_kernel / rn_state_gather_kernel get beside the group (state_kernels.hip), by value.  fifo: the records of the
// group's streams, row by row -- a view of streams s.. gets it advanced --, or null: the batch has none (no chunk call yet; every
// drop-in pool).  The call's fields are read by chunk launches only; every other scatter launch restarts the FIFOs of the streams
// whose state it replaces and looks at nothing else.
struct RnChunkDev {
  float *fifo;                // [N][RN_CHUNK_REC]
  int M;                      // samples per frame at the batch's PCM rate
  // one chunk call (kind RN_REC_CHUNK)
  int N;                      // streams of the call: the rows of every buffer below
  int max_count, F, s16;      // samples between the rows of in / out; rn_chunk_frames(M, max_count); in / out hold int16
  const int *counts;          // [N] new samples of every stream, read through rn_chunk_count
  const void *in;             // [N][max_count] float or int16 (scatter)
  void *out;                  // [N][max_count] (gather)
  float *stage;               // [F][N][M] the frames of the masked call in between, in and out
  unsigned char *active;      // [F][N] its mask (scatter writes it)
  int *frames;                // [N] k of every stream, or null (scatter writes it)
  // a chunk call on a stream list (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks_list): N is the list's length, every
  // buffer above is indexed by list position (row), and row i's FIFO record is that of stream list[i] -- `fifo` then covers the
  // whole batch.  Null: row i is stream i, the full-size call
  const int *list;            // [N] the batch stream of every row
  int S;                      // streams of the batch: an entry outside [0, S) makes its row absent
  // FIFO records (rnnoise_batch_save_chunk_fifos_device / load): no call, N rows of `rec` <-> the FIFOs of streams list[i] (stream i
  // without a list)
  int op;                     // RN_CHUNK_OP_*
  float *rec;                 // [N][RN_CHUNK_REC] (load only reads it)
};
enum { RN_CHUNK_OP_CALL = 0, RN_CHUNK_OP_SAVE, RN_CHUNK_OP_LOAD };
// The saved record, RN_CHUNK_REC words like the one on the device: [0, r) the pending samples and zeros up to 480, [480, 480 + M - r)
// the output FIFO and zeros up to 960, then r, the frame length M the record belongs to, the magic word and a zero, as int32.
// (A FIFO record on the device is not one: samples behind the fills stay as they were, and the padding is never written.)
#define RN_CHUNK_OFF_FILL (2 * RN_CHUNK_FIFO_ROW)
#define RN_CHUNK_OFF_M (RN_CHUNK_OFF_FILL + 1)
#define RN_CHUNK_OFF_MAGIC (RN_CHUNK_OFF_FILL + 2)
#define RN_CHUNK_MAGIC 0x464b4301  // "\1CKF"
// whether load takes a record with this header on a batch whose frame is M
#ifdef __HIPCC__
__host__ __device__
#endif
static inline bool rn_chunk_rec_ok(int magic, int rec_M, int r, int M) { return magic == RN_CHUNK_MAGIC && rec_M == M && r >= 0 && r < M; }
