// batch_state.cpp -- the state of single streams of a batch: per-stream reset, state export / import, stream snapshots.  All of it
// goes through the gather / scatter / zero kernels of state_kernels.hip; the host forms drain the device first (the caller's streams
// are not known here) and return with the work done.
#include "shim.h"

namespace {
// zero state for the n streams of the device list d_list, on st; the layer-wise network's state images of their tiles follow
// (rn_dev.h: act_q) while they are in use, so that a reset costs no re-quantisation of the whole batch at the next step.  Every
// scatter launch of this file gets the streams' sample FIFOs to restart (shim.h: batch_chunk_fifos)
int reset_streams_on(RNNoiseBatch *b, const int *d_list, int n, hipStream_t st) {
  const RnChunkDev ck = batch_chunk_fifos(b, 0);
  const RnGroupDev g = batch_state_group(b);  // (both halves of the history restart, a batch with an out-rate table alone included)
  HIP_OK(rn_launch_state_zero(&g, d_list, n, &ck, st));
  if (b->img_valid) HIP_OK(rn_launch_nn_requant(&b->g, st, d_list, n));
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_reset_streams(RNNoiseBatch *b, const int *streams, int n) {
  if (!b || n < 0 || (n > 0 && !streams)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (n > 0 && !host_list_ok(b, streams, n, false)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  DevScratch d;
  const size_t o_list = d.carve((size_t)n * sizeof(int));
  if (d.alloc()) return -1;
  int *d_list = d.at<int>(o_list);
  HIP_OK(hipMemcpy(d_list, streams, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  if (reset_streams_on(b, d_list, n, nullptr)) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" int rnnoise_batch_reset_streams_device(RNNoiseBatch *b, const int *d_streams, int n, void *hip_stream) {
  if (!b || n < 0 || (n > 0 && !d_streams)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return reset_streams_on(b, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

namespace {
// what every state produced by the reference or by export_state satisfies, and what lets the batch not store analysis_mem (rn_dev.h)
bool analysis_is_pitch_tail(const float *f) {
  return !memcmp(f + RN_OFF_ANALYSIS, f + RN_OFF_PITCH_BUF + RN_PITCH_BUF_SIZE - RN_FRAME_SIZE, RN_FRAME_SIZE * sizeof(float));
}
// the one-state staging row of export / import (16-byte aligned, as the scatter kernel wants its records)
int stage_ready(RNNoiseBatch *b) {
  if (!b->state_stage) HIP_OK(hipMalloc((void **)&b->state_stage, RN_STATE_FLOATS * sizeof(float)));
  return 0;
}
// where the state kernels find the frame phases of streams s, s + 1, ... in per-stream mode (they read them on the device; null in
// lock-step mode, where the launch carries b->ring_slot: the slots its next frame writes, ring slot p % RN_RING_SLOTS, spectra slot
// p % RN_SPEC_SLOTS)
const int *phase_of(const RNNoiseBatch *b, int s) { return b->per_stream ? b->phase_buf + s : nullptr; }
}  // namespace

// State migration: one gather / scatter kernel (state_kernels.hip) and one copy per call.  Synchronous with everything
// the batch has in flight (the caller's streams are not known here, so the device is drained first).
extern "C" int rnnoise_batch_export_state(RNNoiseBatch *b, int s, float *f) {
  if (!b || !f || s < 0 || s >= b->n) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (stage_ready(b)) return -1;
  const RnGroupDev v = group_view(b->g, s, 1);
  HIP_OK(rn_launch_state_gather(&v, RN_REC_STATE, b->state_stage, nullptr, 1, b->ring_slot, phase_of(b, s), nullptr, nullptr));
  // (a blocking copy on the null stream: ordered after the kernel)
  HIP_OK(hipMemcpy(f, b->state_stage, RN_STATE_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rnnoise_batch_import_state(RNNoiseBatch *b, int s, const float *f) {
  if (!b || !f || s < 0 || s >= b->n) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!analysis_is_pitch_tail(f)) {
    fprintf(stderr, "[rnnoise_amd] import_state: analysis_mem differs from the tail of pitch_buf\n");
    return -1;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (stage_ready(b)) return -1;
  HIP_OK(hipMemcpy(b->state_stage, f, RN_STATE_FLOATS * sizeof(float), hipMemcpyHostToDevice));
  b->img_valid = false;
  const RnGroupDev v = group_view(batch_state_group(b), s, 1);
  const RnChunkDev ck = batch_chunk_fifos(b, s);
  HIP_OK(rn_launch_state_scatter(&v, RN_REC_STATE, b->state_stage, nullptr, 1, b->ring_slot, phase_of(b, s), &ck, nullptr));
  HIP_OK(hipStreamSynchronize(nullptr));
  return 0;
}

// ---- stream snapshots (include/rnnoise_amd.h: rnnoise_batch_save_streams) ----
// The device forms are two launches at the most, ordered on the caller's stream like rnnoise_batch_reset_streams_device.  Nothing
// has to be joined here: a pipelined call ends with the synthesis of its last frame on the caller's stream, which waited for that
// frame's analysis (cur_k1) on the side stream, which waited for its high-pass (cur_hp) on the other one -- both side streams run
// in frame order, so everything the call queued anywhere is complete before a kernel that follows it on the caller's stream; and the
// next pipelined call records ev_begin on the caller's stream behind these launches and makes both side streams wait for it.
static_assert(RNNOISE_AMD_SNAP_FLOATS == RN_SNAP_FLOATS && RN_SNAP_FLOATS % 4 == 0, "one record size for the kernels and the API");
namespace {
bool snap_args_ok(const RNNoiseBatch *b, const void *snap, const int *streams, int n) {
  if (!b || n < 0 || n > b->n || (n > 0 && !snap)) return false;
  if (batch_split_busy(b)) return false;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (n > 0 && !streams && n != b->n) return false;  // (no list: the whole batch, stream i = row i)
  return true;
}
int save_on(RNNoiseBatch *b, float *d_snap, const int *d_list, int n, hipStream_t st) {
  const RnGroupDev g = batch_state_group(b);
  HIP_OK(rn_launch_state_gather(&g, RN_REC_SNAP, d_snap, d_list, n, b->ring_slot, phase_of(b, 0), nullptr, st, b->out_Ls));
  return 0;
}
// the listed rows' tiles of the layer-wise network's state images follow the load while they are live (rn_dev.h: act_q), as after
// a per-stream reset; without a list that is every tile
int load_on(RNNoiseBatch *b, const float *d_snap, const int *d_list, int n, hipStream_t st) {
  const RnChunkDev ck = batch_chunk_fifos(b, 0);
  const RnGroupDev g = batch_state_group(b);
  HIP_OK(rn_launch_state_scatter(&g, RN_REC_SNAP, d_snap, d_list, n, b->ring_slot, phase_of(b, 0), &ck, st, b->out_Ls));
  if (b->img_valid) HIP_OK(rn_launch_nn_requant(&b->g, st, d_list, d_list ? n : 0));
  return 0;
}
constexpr int SNAP_CHUNK = 1024;  // rows of the host forms' staging buffer (27 MB)

// the host forms: the list is checked, the device drained (the caller's streams are not known here), then chunks of SNAP_CHUNK rows
// go through one staging allocation with blocking copies
int snap_host(RNNoiseBatch *b, float *snap, const int *streams, int n, bool load) {
  if (!snap_args_ok(b, snap, streams, n)) return -1;
  if (n == 0) return 0;
  if (!host_list_ok(b, streams, n, load)) return -1;  // (a save may name a stream twice)
  std::vector<int> list((size_t)n);
  for (int i = 0; i < n; i++) {
    if (load) {
      const float *f = snap + (size_t)i * RN_SNAP_FLOATS;
      int magic;
      memcpy(&magic, f + RN_SNAP_OFF_MAGIC, sizeof magic);
      if (magic != RN_SNAP_MAGIC) return -1;
      if (!analysis_is_pitch_tail(f)) {
        fprintf(stderr, "[rnnoise_amd] load_streams: row %d: analysis_mem differs from the tail of pitch_buf\n", i);
        return -1;
      }
    }
    list[i] = streams ? streams[i] : i;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  const size_t chunk = n < SNAP_CHUNK ? n : SNAP_CHUNK, row_bytes = RN_SNAP_FLOATS * sizeof(float);
  DevScratch d;
  const size_t o_snap = d.carve(chunk * row_bytes), o_list = d.carve(chunk * sizeof(int));
  if (d.alloc()) return -1;
  float *d_snap = d.at<float>(o_snap);
  int *d_list = d.at<int>(o_list);
  for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk) {
    const int rows = (int)std::min(chunk, (size_t)n - r0);
    float *h = snap + r0 * RN_SNAP_FLOATS;
    HIP_OK(hipMemcpy(d_list, list.data() + r0, rows * sizeof(int), hipMemcpyHostToDevice));
    if (load) {
      HIP_OK(hipMemcpy(d_snap, h, rows * row_bytes, hipMemcpyHostToDevice));
      if (load_on(b, d_snap, d_list, rows, nullptr)) return -1;
      HIP_OK(hipStreamSynchronize(nullptr));
    } else {
      if (save_on(b, d_snap, d_list, rows, nullptr)) return -1;
      HIP_OK(hipStreamSynchronize(nullptr));
      HIP_OK(hipMemcpy(h, d_snap, rows * row_bytes, hipMemcpyDeviceToHost));
    }
  }
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_save_streams_device(RNNoiseBatch *b, float *d_snap, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_snap, d_streams, n) || (reinterpret_cast<uintptr_t>(d_snap) & 15)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return save_on(b, d_snap, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_load_streams_device(RNNoiseBatch *b, const float *d_snap, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_snap, d_streams, n) || (reinterpret_cast<uintptr_t>(d_snap) & 15)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return load_on(b, d_snap, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_save_streams(RNNoiseBatch *b, float *snap, const int *streams, int n) {
  return snap_host(b, snap, streams, n, false);
}

extern "C" int rnnoise_batch_load_streams(RNNoiseBatch *b, const float *snap, const int *streams, int n) {
  return snap_host(b, const_cast<float *>(snap), streams, n, true);
}

// ---- FIFO records of the chunk calls (include/rnnoise_amd.h: rnnoise_batch_save_chunk_fifos) ----
// What a snapshot leaves behind of a stream that is fed in chunks: its two sample FIFOs and their fill.  One launch of the state
// kernels' chunk form per call (chunk_fifo.h: rn_chunk_rec_save / rn_chunk_rec_load), n workgroups, list and argument rules as the
// snapshots above.  A save reads whatever the batch has -- restarted FIFOs where it has none --, a load allocates them first.
static_assert(RNNOISE_AMD_CHUNK_REC_FLOATS == RN_CHUNK_REC && RNNOISE_AMD_CHUNK_MAGIC == RN_CHUNK_MAGIC && RN_CHUNK_MAGIC != RN_SNAP_MAGIC,
              "one FIFO record for the kernels and the API");
namespace {
int fifo_rec_on(RNNoiseBatch *b, float *d_rec, const int *d_list, int n, bool load, hipStream_t st) {
  if (load && batch_chunk_fifos_ready(b, st)) return -1;
  RnChunkDev ck = batch_chunk_fifos(b, 0);
  ck.M = batch_frame_samples(b);
  ck.N = n;
  ck.list = d_list;
  ck.S = b->n;
  ck.op = load ? RN_CHUNK_OP_LOAD : RN_CHUNK_OP_SAVE;
  ck.rec = d_rec;
  if (load) HIP_OK(rn_launch_state_scatter(&b->g, RN_REC_CHUNK, nullptr, nullptr, n, 0, nullptr, &ck, st));
  else HIP_OK(rn_launch_state_gather(&b->g, RN_REC_CHUNK, nullptr, nullptr, n, 0, nullptr, &ck, st));
  return 0;
}
constexpr int FIFO_REC_CHUNK = 8192;  // rows of the host forms' staging buffer (32 MB)

int fifo_rec_host(RNNoiseBatch *b, float *rec, const int *streams, int n, bool load) {
  if (!snap_args_ok(b, rec, streams, n)) return -1;
  if (n == 0) return 0;
  const int M = batch_frame_samples(b);
  if (!host_list_ok(b, streams, n, load)) return -1;  // (a save may name a stream twice)
  std::vector<int> list((size_t)n);
  for (int i = 0; i < n; i++) {
    if (load) {
      int hdr[3];  // fill, M, magic
      memcpy(hdr, rec + (size_t)i * RN_CHUNK_REC + RN_CHUNK_OFF_FILL, sizeof hdr);
      if (!rn_chunk_rec_ok(hdr[2], hdr[1], hdr[0], M)) return -1;
    }
    list[i] = streams ? streams[i] : i;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  const size_t chunk = n < FIFO_REC_CHUNK ? n : FIFO_REC_CHUNK, row_bytes = RN_CHUNK_REC * sizeof(float);
  DevScratch d;
  const size_t o_rec = d.carve(chunk * row_bytes), o_list = d.carve(chunk * sizeof(int));
  if (d.alloc()) return -1;
  float *d_rec = d.at<float>(o_rec);
  int *d_list = d.at<int>(o_list);
  for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk) {
    const int rows = (int)std::min(chunk, (size_t)n - r0);
    float *h = rec + r0 * RN_CHUNK_REC;
    HIP_OK(hipMemcpy(d_list, list.data() + r0, rows * sizeof(int), hipMemcpyHostToDevice));
    if (load) HIP_OK(hipMemcpy(d_rec, h, rows * row_bytes, hipMemcpyHostToDevice));
    if (fifo_rec_on(b, d_rec, d_list, rows, load, nullptr)) return -1;
    HIP_OK(hipStreamSynchronize(nullptr));
    if (!load) HIP_OK(hipMemcpy(h, d_rec, rows * row_bytes, hipMemcpyDeviceToHost));
  }
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_save_chunk_fifos_device(RNNoiseBatch *b, float *d_rec, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_rec, d_streams, n)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return fifo_rec_on(b, d_rec, d_streams, n, false, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_load_chunk_fifos_device(RNNoiseBatch *b, const float *d_rec, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_rec, d_streams, n)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return fifo_rec_on(b, const_cast<float *>(d_rec), d_streams, n, true, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_save_chunk_fifos(RNNoiseBatch *b, float *rec, const int *streams, int n) {
  return fifo_rec_host(b, rec, streams, n, false);
}

extern "C" int rnnoise_batch_load_chunk_fifos(RNNoiseBatch *b, const float *rec, const int *streams, int n) {
  return fifo_rec_host(b, const_cast<float *>(rec), streams, n, true);
}
