// batch_chunks.cpp -- chunk calls (include/rnnoise_amd.h)
// Any number of samples per stream and call: the streams' sample FIFOs live on the device (chunk_plan.h has the rule), and a call is
// three steps on the caller's stream -- the scatter kernel's chunk form (pending samples ++ the caller's rows -> whole frames in the
// batch's own staging buffer, their mask, the new tails), the masked float call on that buffer in place, the gather kernel's chunk form
// (output FIFO ++ the frames' output -> the caller's rows, the rest kept).  The int16 forms differ in the two staging steps alone.
#include "shim.h"

extern "C" int rnnoise_amd_chunk_frames(int frame_samples, int max_count) { return rn_chunk_frames(frame_samples, max_count); }

// every stream's FIFOs as after create; the caller has selected the device and drained it, and drains it again
int batch_chunk_restart_all(RNNoiseBatch *b) {
  if (!b->chunk_fifo) return 0;
  HIP_OK(hipMemset(b->chunk_fifo, 0, (size_t)b->n * RN_CHUNK_REC * sizeof(float)));  // (chunk_plan.h: a record of zeros)
  return 0;
}

// the FIFOs, where the batch has none yet: every stream's as after create, written on st ahead of what follows there
int batch_chunk_fifos_ready(RNNoiseBatch *b, hipStream_t st) {
  if (b->chunk_fifo) return 0;
  const size_t bytes = (size_t)b->n * RN_CHUNK_REC * sizeof(float);
  HIP_OK(hipMalloc((void **)&b->chunk_fifo, bytes));
  HIP_OK(hipMemsetAsync(b->chunk_fifo, 0, bytes, st));
  return 0;
}

namespace {
// One chunk call, as the entry points hand it to chunks_device (device memory, asynchronous on `stream`) or to chunks_host (host
// memory, synchronous; `stream` is not read).  listed: the list form -- every buffer has n_rows rows and row i belongs to stream
// list[i]; an empty list is a no-op even without a list pointer, never a full-size call.  Else the full-size form: list and n_rows
// are not read
struct ChunkCall {
  void *out = nullptr;  // PCM rows: float, or int16 with s16 set
  const void *in = nullptr;
  const int *counts = nullptr;
  int max_count = 0;
  const int *list = nullptr;
  int n_rows = 0;
  bool listed = false;
  float *vad = nullptr, *gains = nullptr;  // optional
  int *frames = nullptr;                   // optional
  void *stream = nullptr;
  bool s16 = false;
};
// What both forms refuse before anything moves: a chunk call does not combine with per-stream rates and formats, on the input or on
// the output side, a PCM layout, channels, linked gains (include/rnnoise_amd.h), and none runs while frames of a split call are pending
bool chunk_args_ok(const RNNoiseBatch *b, const ChunkCall &c) {
  if (!b || !c.out || !c.in || !c.counts || c.max_count < 0) return false;
  if (b->g.rs_Ls || b->g.pcm_fmt || b->out_Ls || b->out_fmt || b->row_stride || b->channels > 1 || b->link > 1) return false;
  if (batch_split_busy(b)) return false;
  return !c.listed || (c.n_rows >= 0 && c.n_rows <= b->n && (c.n_rows == 0 || c.list));
}
// The FIFOs, on the first chunk call (their first state written on the call's stream, ahead of the call), and a staging buffer for F
// frames of the call's rows with their mask behind them: frames of RN_FRAME_SIZE floats whatever the rate, so that a rate change keeps
// it.  It is sized in bytes and shared by the full-size and the list form: a call that fits leaves it alone.  Growing it drains the
// device first -- the old buffer may be in use by a call in flight on another stream.
int chunk_ready(RNNoiseBatch *b, const ChunkCall &c, int F) {
  if (batch_chunk_fifos_ready(b, static_cast<hipStream_t>(c.stream))) return -1;
  const size_t rows = c.listed ? c.n_rows : b->n, need = (size_t)F * rows * (RN_FRAME_SIZE * sizeof(float) + 1);
  if (need > b->chunk_stage_bytes) {
    if (b->chunk_stage) {
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipFree(b->chunk_stage));
      b->chunk_stage = nullptr;
      b->chunk_stage_bytes = 0;
    }
    HIP_OK(hipMalloc(&b->chunk_stage, need));
    b->chunk_stage_bytes = need;
  }
  return 0;
}

int chunks_device(RNNoiseBatch *b, const ChunkCall &c) {
  if (!chunk_args_ok(b, c)) return -1;
  if (c.max_count == 0 || (c.listed && c.n_rows == 0)) return 0;
  const int M = batch_frame_samples(b), F = rn_chunk_frames(M, c.max_count), rows = c.listed ? c.n_rows : b->n;
  const hipStream_t st = static_cast<hipStream_t>(c.stream);
  ON_DEVICE(b->device);
  if (chunk_ready(b, c, F)) return -1;
  RnChunkDev ck = batch_chunk_fifos(b, 0);
  ck.N = rows;
  ck.max_count = c.max_count;
  ck.F = F;
  ck.s16 = c.s16;
  ck.counts = c.counts;
  ck.in = c.in;
  ck.out = c.out;
  ck.stage = static_cast<float *>(b->chunk_stage);
  // (the mask behind the frames THIS call can have, at the longest frame: inside the allocation whatever it was sized for)
  ck.active = reinterpret_cast<unsigned char *>(ck.stage + (size_t)F * rows * RN_FRAME_SIZE);
  ck.frames = c.frames;
  ck.list = c.listed ? c.list : nullptr;
  ck.S = b->n;
  HIP_OK(rn_launch_state_scatter(&b->g, RN_REC_CHUNK, nullptr, nullptr, rows, 0, nullptr, &ck, st));
  // (the masked call reads frame f's rows in K0 and writes them in K3 of the same frame: in place.  The list form: the list call on
  //  the compact buffer -- every launch sized by n_rows)
  if (batch_process_device_impl(b, {.out = ck.stage, .in = ck.stage, .vad = c.vad, .gains = c.gains, .n_frames = F, .stream = c.stream,
                                    .active = ck.active, .list = ck.list, .n_rows = c.listed ? c.n_rows : 0, .packed = true}))
    return -1;
  HIP_OK(rn_launch_state_gather(&b->g, RN_REC_CHUNK, nullptr, nullptr, rows, 0, nullptr, &ck, st));
  return 0;
}

// the convenience form on host buffers: the counts (and the list: an entry outside the batch or listed twice) are checked before
// anything moves; whole rows go up, and only the first counts[i] samples of a row come back into the caller's `out`
int chunks_host(RNNoiseBatch *b, const ChunkCall &c) {
  if (!chunk_args_ok(b, c)) return -1;
  const size_t N = c.listed ? c.n_rows : b->n;
  if (c.listed && !host_list_ok(b, c.list, c.n_rows, true)) return -1;
  for (size_t i = 0; i < N; i++)
    if (c.counts[i] < 0 || c.counts[i] > c.max_count) return -1;
  if (c.max_count == 0 || N == 0) return 0;
  const size_t esz = c.s16 ? sizeof(short) : sizeof(float), row = (size_t)c.max_count * esz;
  const size_t fs = (size_t)rn_chunk_frames(batch_frame_samples(b), c.max_count) * N;
  ON_DEVICE(b->device);
  DevScratch d;
  const size_t o_in = d.carve(N * row), o_out = d.carve(N * row), o_counts = d.carve(N * sizeof(int)), o_vad = d.carve(fs * 4),
               o_gains = d.carve(fs * RN_NB_BANDS * 4), o_frames = d.carve(N * sizeof(int)), o_list = d.carve(c.listed ? N * sizeof(int) : 0);
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_in), c.in, N * row, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_counts), c.counts, N * sizeof(int), hipMemcpyHostToDevice));
  if (c.listed) HIP_OK(hipMemcpy(d.at<char>(o_list), c.list, N * sizeof(int), hipMemcpyHostToDevice));
  ChunkCall dc = c;  // the same call on the staged copies, on the null stream
  dc.out = d.at<char>(o_out), dc.in = d.at<char>(o_in), dc.counts = d.at<int>(o_counts);
  dc.list = c.listed ? d.at<int>(o_list) : nullptr;
  dc.vad = c.vad ? d.at<float>(o_vad) : nullptr, dc.gains = c.gains ? d.at<float>(o_gains) : nullptr;
  dc.frames = c.frames ? d.at<int>(o_frames) : nullptr;
  dc.stream = nullptr;
  if (chunks_device(b, dc)) return -1;
  HIP_OK(hipDeviceSynchronize());
  std::vector<char> rows(N * row);
  HIP_OK(hipMemcpy(rows.data(), d.at<char>(o_out), N * row, hipMemcpyDeviceToHost));
  for (size_t s = 0; s < N; s++) memcpy(static_cast<char *>(c.out) + s * row, rows.data() + s * row, (size_t)c.counts[s] * esz);
  if (c.vad) HIP_OK(hipMemcpy(c.vad, d.at<char>(o_vad), fs * 4, hipMemcpyDeviceToHost));
  if (c.gains) HIP_OK(hipMemcpy(c.gains, d.at<char>(o_gains), fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost));
  if (c.frames) HIP_OK(hipMemcpy(c.frames, d.at<char>(o_frames), N * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_process_device_chunks(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts, int max_count,
                                                   float *d_vad, float *d_gains, int *d_frames, void *hip_stream) {
  return chunks_device(b, {.out = d_out, .in = d_in, .counts = d_counts, .max_count = max_count, .vad = d_vad, .gains = d_gains,
                           .frames = d_frames, .stream = hip_stream});
}
extern "C" int rnnoise_batch_process_device_chunks_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                       int max_count, float *d_vad, float *d_gains, int *d_frames, void *hip_stream) {
  return chunks_device(b, {.out = d_out, .in = d_in, .counts = d_counts, .max_count = max_count, .vad = d_vad, .gains = d_gains,
                           .frames = d_frames, .stream = hip_stream, .s16 = true});
}
extern "C" int rnnoise_batch_process_chunks(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count, float *vad,
                                            float *gains, int *frames) {
  return chunks_host(b, {.out = out, .in = in, .counts = counts, .max_count = max_count, .vad = vad, .gains = gains, .frames = frames});
}
extern "C" int rnnoise_batch_process_chunks_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts, int max_count,
                                                float *vad, float *gains, int *frames) {
  return chunks_host(b, {.out = out, .in = in, .counts = counts, .max_count = max_count, .vad = vad, .gains = gains, .frames = frames,
                         .s16 = true});
}
// the same on a stream list (include/rnnoise_amd.h)
extern "C" int rnnoise_batch_process_device_chunks_list(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts,
                                                        int max_count, const int *d_streams, int n_rows, float *d_vad, float *d_gains,
                                                        int *d_frames, void *hip_stream) {
  return chunks_device(b, {.out = d_out, .in = d_in, .counts = d_counts, .max_count = max_count, .list = d_streams, .n_rows = n_rows,
                           .listed = true, .vad = d_vad, .gains = d_gains, .frames = d_frames, .stream = hip_stream});
}
extern "C" int rnnoise_batch_process_device_chunks_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                            int max_count, const int *d_streams, int n_rows, float *d_vad,
                                                            float *d_gains, int *d_frames, void *hip_stream) {
  return chunks_device(b, {.out = d_out, .in = d_in, .counts = d_counts, .max_count = max_count, .list = d_streams, .n_rows = n_rows,
                           .listed = true, .vad = d_vad, .gains = d_gains, .frames = d_frames, .stream = hip_stream, .s16 = true});
}
extern "C" int rnnoise_batch_process_chunks_list(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count,
                                                 const int *streams, int n_rows, float *vad, float *gains, int *frames) {
  return chunks_host(b, {.out = out, .in = in, .counts = counts, .max_count = max_count, .list = streams, .n_rows = n_rows,
                         .listed = true, .vad = vad, .gains = gains, .frames = frames});
}
extern "C" int rnnoise_batch_process_chunks_list_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts, int max_count,
                                                     const int *streams, int n_rows, float *vad, float *gains, int *frames) {
  return chunks_host(b, {.out = out, .in = in, .counts = counts, .max_count = max_count, .list = streams, .n_rows = n_rows,
                         .listed = true, .vad = vad, .gains = gains, .frames = frames, .s16 = true});
}
extern "C" int rnnoise_batch_chunk_fill(RNNoiseBatch *b, int *fill) {
  if (!b || !fill) return -1;
  if (!b->chunk_fifo) {  // (no chunk call yet: nothing pending anywhere)
    memset(fill, 0, (size_t)b->n * sizeof(int));
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  // (one word of every record)
  HIP_OK(hipMemcpy2D(fill, sizeof(int), b->chunk_fifo + 2 * RN_CHUNK_FIFO_ROW, RN_CHUNK_REC * sizeof(float), sizeof(int), b->n,
                     hipMemcpyDeviceToHost));
  return 0;
}
