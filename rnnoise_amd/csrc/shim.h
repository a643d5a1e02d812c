// shim.h -- what the host-side translation units of librnnoise_amd.so share: the kernel launchers (one per .hip file), the
// device guard and error macros, the host-side types behind the opaque handles of include/rnnoise.h and include/rnnoise_amd.h,
// and the few functions that cross file boundaries.  Internal: nothing here is exported (-fvisibility=hidden, exports.map).
//
//   model.cpp    "DNNw" blob reader, "RNPK" pack, GPU re-layout of the model, rnnoise_model_* entry points
//   tables.cpp   static tables by formula, the rcpps profile
//   batch.cpp         rnnoise_batch_*: N streams on one GPU -- create, destroy, reset, training features, timing, debug taps
//   batch_step.cpp    the frame step as a pipeline over HIP streams (batch_step.h: its stages), its host-buffer form, the plain, masked
//                     and list calls
//   batch_chunks.cpp  the chunk calls: any number of samples per stream through device FIFOs
//   batch_eval.cpp    the feature calls: the network alone on features that exist, training records scored with the trainer's loss
//   batch_split.cpp   the split calls: analysis and synthesis as calls of their own around a network of the caller's -- the two halves
//                     of the step and their host-buffer forms, the pending frames
//   batch_tables.cpp  a batch's configuration: PCM rate, strides, channels, the per-stream tables (rates, formats, models, controls)
//   batch_state.cpp   single streams of a batch: per-stream reset, state export / import, stream snapshots
//   train_mix.hip     training sequences: levels, Viterbi VAD and mix of src/dump_features.c:408-465, host code and kernels
//   train_rir.hip     training sequences: the RIR filtering of src/dump_features.c:51-144, :449-465, host code and kernels
//   train_common.h    what those two share: the upload into a batch-owned buffer, argument tests, the device clip-and-quantise
//   host_io.cpp  host-fed calls: the pinned frame ring, the bounce chunks of pageable callers
//   dropin.cpp   the reference's own API (include/rnnoise.h): state pools, the combiner of concurrent one-frame calls
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rnnoise_amd.h"
#include "rn_dev.h"
#if RN_INSTRUMENT
#include "../../include/rnnoise_amd_debug.h"
#endif
#include "rcp_profiles.h"
#include "dispatch.h"
#include "chunk_plan.h"

// the launchers of a frame step take the form the step's plan chose (dispatch.h: rn_plan)
extern "C" hipError_t rn_launch_hp(const RnGroupDev *, const void *, int in_s16, int, RnHpForm, hipStream_t, hipEvent_t, hipEvent_t);
extern "C" hipError_t rn_launch_analysis(const RnGroupDev *, const RnTablesDev *, int, int, RnK1Form, hipStream_t, hipEvent_t, hipEvent_t);
extern "C" hipError_t rn_launch_synthesis(const RnGroupDev *, const RnTablesDev *, void *, int out_s16, int, int, RnK3Form, hipStream_t,
                                          hipEvent_t, hipEvent_t);
extern "C" hipError_t rn_launch_train_features(const RnGroupDev *, const RnTablesDev *, const float *, int, int,
                                               const RnTrainArgs *, hipStream_t);
extern "C" hipError_t rn_launch_eval_step(const RnGroupDev *, const RnTablesDev *, const RnEvalStep *, hipStream_t);
extern "C" hipError_t rn_launch_split_step(const RnGroupDev *, const RnTablesDev *, const RnSplitStep *, int mode, hipStream_t);
// the score walk (rn_dev.h: RnScoreStep): the record step's launcher in its fourth mode, one wave per row of the caller's, one launch for
// the call's frames
inline hipError_t rn_launch_score_rows(const RnGroupDev *g, const RnTablesDev *tb, const RnScoreStep *score, int n_rows, hipStream_t st) {
  RnEvalStep step{};
  step.on = RN_STEP_SCORE;
  step.score = score;
  step.score_rows = n_rows;
  return rn_launch_eval_step(g, tb, &step, st);
}
extern "C" hipError_t rn_launch_nn_vector(const RnGroupDev *, const RnModelDev *, const RnTablesDev *, hipStream_t, hipEvent_t,
                                          hipEvent_t);
// (lds_opt_in: the batch's answer to the kernel's large-LDS opt-in, RNNoiseBatch::lds_one / lds_gru, returned instead of a launch)
extern "C" hipError_t rn_launch_nn_one(const RnGroupDev *, const RnModelDev *, const RnTablesDev *, hipError_t lds_opt_in, hipStream_t,
                                       hipEvent_t, hipEvent_t);
extern "C" hipError_t rn_launch_nn_mfma(const RnGroupDev *, const RnModelDev *, const RnTablesDev *, RnNnForm, hipStream_t, hipEvent_t,
                                        hipEvent_t);
extern "C" hipError_t rn_launch_nn_layers(const RnGroupDev *, const RnModelDev *, const RnTablesDev *, RnGruForm,
                                          const hipError_t lds_opt_in[2], hipStream_t, hipEvent_t[5][2]);
extern "C" hipError_t rn_launch_nn_requant(const RnGroupDev *, hipStream_t, const int *list = nullptr, int n = 0);
extern "C" hipError_t rn_nn_one_opt_in(void);             // nn_kernels.hip, on the current device
extern "C" void rn_nn_gru_opt_in(hipError_t out[2]);      // nn_layers.hip, both forms (RnGruForm order), on the current device
extern "C" hipError_t rn_launch_release_store(void *, long long, hipStream_t);
#if RN_INSTRUMENT
extern "C" hipError_t rn_launch_log_energy(const float *, unsigned, float *, unsigned, const double *, hipStream_t);
extern "C" hipError_t rn_launch_vad_libm(int, unsigned, unsigned, double *, unsigned, hipStream_t);
extern "C" hipError_t rn_launch_fft_probe(int, const float *, float *, unsigned long long *, int, int, const RnTablesDev *, hipStream_t);
extern "C" hipError_t rn_launch_xlane_probe(int *, hipStream_t);
#endif
// (state_kernels.hip: `rows` records of `kind`, record i <-> stream list[i] of the view, at frame phase p or at the per-stream
//  phases `phase`; and the zero state for the listed streams of the view, or for all of them.  ck: the sample FIFOs of the view's
//  streams (chunk_plan.h; batch_chunk_fifos below), which every scatter restarts -- null where the group has none -- and, with
//  RN_REC_CHUNK, the chunk call the launch is a staging step of -- full-size or on a stream list -- or the FIFO records it saves /
//  loads: `rows` is then ck->N, the rows of the call or of the records.  out_Ls: the batch's out-rate table for the snapshot
//  launches, RNNoiseBatch::out_Ls -- null: none, and on every other launch)
extern "C" hipError_t rn_launch_state_gather(const RnGroupDev *, RnRecKind kind, float *rec, const int *list, int rows, int p,
                                             const int *phase, const RnChunkDev *ck, hipStream_t, const uint8_t *out_Ls = nullptr);
extern "C" hipError_t rn_launch_state_scatter(const RnGroupDev *, RnRecKind kind, const float *rec, const int *list, int rows, int p,
                                              const int *phase, const RnChunkDev *ck, hipStream_t, const uint8_t *out_Ls = nullptr);
extern "C" hipError_t rn_launch_state_zero(const RnGroupDev *, const int *list, int n, const RnChunkDev *ck, hipStream_t);

extern "C" hipError_t rn_launch_hp_rows(const RnGroupDev *, const RnRows *, hipStream_t);
extern "C" hipError_t rn_launch_analysis_rows(const RnGroupDev *, const RnTablesDev *, const RnRows *, hipStream_t);
extern "C" hipError_t rn_launch_nn_rows(const RnGroupDev *, const RnModelDev *, const RnTablesDev *, const RnRows *, hipError_t lds_opt_in,
                                        hipStream_t);
extern "C" hipError_t rn_launch_synthesis_rows(const RnGroupDev *, const RnTablesDev *, const RnRows *, hipStream_t);

// Every entry point works on the batch's device and leaves the calling thread's current device as it found it
// (a host thread may be driving another GPU: torch on cuda:0 beside a batch on device 1).
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (prev == device) || hipSetDevice(device) == hipSuccess;
    if (prev == device) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define ON_DEVICE(dev)                                                                                 \
  DeviceGuard guard_(dev);                                                                             \
  if (!guard_.ok) {                                                                                    \
    fprintf(stderr, "[rnnoise_amd] cannot select HIP device %d (%s:%d)\n", (dev), __FILE__, __LINE__);  \
    return -1;                                                                                         \
  }

#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      fprintf(stderr, "[rnnoise_amd] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                                       \
    }                                                                                                  \
  } while (0)

inline size_t rn_align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }
// The staging buffer of a host-buffer convenience call: its pieces are carved first (offsets), then allocated as one, and freed when
// the call's scope ends -- whichever way it ends.
struct DevScratch {
  uint8_t *dev = nullptr;
  size_t bytes = 0;
  DevScratch() = default;
  DevScratch(const DevScratch &) = delete;
  ~DevScratch() { if (dev) hipFree(dev); }
  size_t carve(size_t n) { const size_t off = bytes; bytes += rn_align256(n); return off; }
  int alloc() { HIP_OK(hipMalloc((void **)&dev, bytes)); return 0; }
  template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(dev + off); }
};

// Host view of one layer (pointers alias the blob, like the reference's LinearLayer)
struct HostLinear {
  const float *bias = nullptr, *subias = nullptr, *fw = nullptr, *diag = nullptr, *scale = nullptr;
  const int8_t *w = nullptr;
  const int32_t *idx = nullptr;
  int idx_words = 0, nblocks = 0, nin = 0, nout = 0;
  bool is_int8() const { return w != nullptr; }
};

struct HostModel {
  HostLinear conv1, conv2, gru_in[3], gru_rec[3], dense_out, vad_dense;
};

// device arena: one allocation, 256-byte aligned carve-outs
struct Staging {
  std::vector<uint8_t> bytes;
  size_t add(const void *src, size_t n) {
    size_t off = (bytes.size() + 255) & ~size_t(255);
    bytes.resize(off + n);
    if (src) memcpy(bytes.data() + off, src, n);
    else memset(bytes.data() + off, 0, n);
    return off;
  }
};

struct DevLinearOffsets {
  size_t bias = 0, fw = 0, scale = 0, diag = 0, w = 0, wmf = 0, rowsum = 0, grp = 0, cols = 0;  // (float layers: wmf = MFMA-ordered copy)
  bool has_fw = false, has_diag = false, has_cols = false, is_int8 = false;
};

struct DeviceModel {
  int device = -1;
  void *mem = nullptr, *mem_rows = nullptr;  // the staged model; the row-major int8 copies of the vector path
  RnModelDev dev{};
};

// =============================================================================================
// public types
// =============================================================================================
struct StatePool;
struct StagedModel;  // model.cpp
struct RNNModel {
  const void *const_blob = nullptr;  // borrowed (rnnoise_model_from_buffer)
  void *blob = nullptr;              // owned (rnnoise_model_from_file)
  int blob_len = 0;
  FILE *file = nullptr;
  std::mutex mu;
  int parsed = 0;  // 0 not yet, 1 ok, -1 rejected
  HostModel host;                  // layer views into a "DNNw" blob (unused for a packed model)
  StagedModel *staged = nullptr;   // device layout of every layer, built from the blob or taken from an "RNPK" pack
  long weight_bytes = 0;           // SURVEY 8d "W"
  std::vector<DeviceModel> dev;
  std::vector<StatePool *> pools;  // device-resident one-stream states behind rnnoise_create / rnnoise_process_frame
  const void *bytes() const { return blob ? blob : const_blob; }
};

struct RNNoiseBatch {
  RNNModel *model = nullptr;
  int device = 0, n = 0, nn_path = 0;
  // facts about the device, resolved once by rnnoise_batch_create: its compute units (dispatch.h: RnStepShape::cus) and the
  // large-LDS opt-ins of rn_nn_one_kernel and the two GRU forms (RnGruForm order) -- a launch of a form whose opt-in failed returns it
  int cus = 256;
  hipError_t lds_one = hipSuccess, lds_gru[2] = {hipSuccess, hipSuccess};
  bool img_valid = false;  // g.act_q[1..3] mirror gru_state (rn_dev.h); cleared by whatever else writes the state
  int schedule = 0;  // 0: default (3-stream frame pipeline in multi-frame calls); 9: one stream; 1: only the high-pass aside
  int parity = 0;  // spectra slot (mod RN_SPEC_SLOTS) the next frame writes; the previous one holds the delayed spectra
  long frame_no = 0;  // selects the per-step scratch copy (features / silence / pitch are double-buffered)
  float *features2[2] = {nullptr, nullptr};
  int *silence2[2] = {nullptr, nullptr}, *pitch2[2] = {nullptr, nullptr};
  int ring_slot = 0;  // pitch-ring slot the next frame is written to
  // per-stream frame phase (include/rnnoise_amd.h: masked calls): from the first masked call until rnnoise_batch_reset the kernels
  // take each stream's ring and spectra slots from phase_buf (rn_dev.h: RnGroupDev::phase) instead of ring_slot / parity
  bool per_stream = false;
  int *phase_buf = nullptr;  // [N] in the arena
  // PCM rate of the calls (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate).  rs_buf: the resampler histories (rn_dev.h:
  // RnGroupDev::rs_hist); g.rs_hist / g.rs_L are set only while the rate is away from 48 kHz or a rate table is set.  This buffer and
  // the four tables below are allocated on first use (batch_tables.cpp: table_alloc) and live until the batch ends
  int pcm_rate = 48000;
  float *rs_buf = nullptr;
  // per-stream rates (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates): rate_map, the [N] divisor bytes K0 / K3 and the snapshot
  // kernels read (rn_dev.h: RnGroupDev::rs_Ls); g.rs_Ls points at it while a table is set, and g.rs_L / g.rs_hist are then set at
  // 48 kHz too (batch_tables.cpp: rs_point)
  uint8_t *rate_map = nullptr;
  // per-stream PCM formats (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats): fmt_map, the [N] format bytes K0 / K3 read in
  // the int16 calls (rn_dev.h: RnGroupDev::pcm_fmt); g.pcm_fmt points at it while a table is set.  Configuration, not state: no reset,
  // import, load or rate change touches it
  uint8_t *fmt_map = nullptr;
  // per-stream OUTPUT rates and formats (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates, _out_formats): out_rate_map and
  // out_fmt_map, [N] bytes each; out_Ls / out_fmt point at them while a table is set.  b->g never carries them: K0 and K1 get the
  // batch's group, with the input tables, and the step points K3's copy at these (shim.h: batch_k3_group) -- and gives that copy
  // the resampler fields where the batch's group has none (48 kHz inputs without a rate table: batch_rs_48k).  The state kernels get
  // out_Ls beside a group with those fields (batch_state_group).  Dropped with the rate table by rnnoise_batch_set_pcm_rate
  uint8_t *out_rate_map = nullptr, *out_fmt_map = nullptr;
  const uint8_t *out_Ls = nullptr, *out_fmt = nullptr;
  // caller-defined PCM strides (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout), in samples; both 0: the default layout.  The
  // process calls hand row_stride to K0 / K3 (rn_dev.h: RnGroupDev::pcm_pitch) and step their frame pointers by frame_stride; b->g
  // itself never carries a pitch.  Configuration, not state
  long frame_stride = 0, row_stride = 0;
  // interleaved channels (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels): the PCM rows of every process call are taken
  // `channels` at a time; 1: none.  The process calls hand it to K0 / K3 (rn_dev.h: RnGroupDev::pcm_chan, 0 for 1); b->g itself
  // never carries it.  Configuration, not state
  int channels = 1;
  // linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link): the rows of every process call are taken `link` at a time and
  // K3 gives each group one set of band gains and one VAD for the gate; 1: none.  The step hands it to K3 alone (rn_dev.h:
  // RnGroupDev::link, 0 for 1); b->g itself never carries it.  Configuration, not state
  int link = 1;
  // per-stream models (include/rnnoise_amd.h: rnnoise_batch_add_model): slot k's model and its device copy (slot 0's: model / m),
  // and model_map, the [N] slot bytes the network launches read (rn_dev.h: RnGroupDev::model_of), there from the first add_model on;
  // g.model_of / g.n_models are set from then on
  int n_models = 1;
  RNNModel *models[RNNOISE_AMD_MAX_MODELS] = {};
  RnModelDev slot_m[RNNOISE_AMD_MAX_MODELS] = {};
  uint8_t *model_map = nullptr;
  // per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls): [N][RN_CTL_FLOATS] table, then the [N]
  // counters; g.ctl / g.gate_c point into it while a table is set
  float *ctl_buf = nullptr;
  // the [N] RNNoiseTrainMix table of the last training-mix call (train_mix.hip), allocated on first use
  void *train_mix_buf = nullptr;
  // train_rir.hip, both allocated on first use: the 65,536 twiddles followed by one transform of scratch for the RIR loader; the [N]
  // RNNoiseTrainRir records of the last filter call followed by its list of filtered sequences
  void *train_rir_tw = nullptr, *train_rir_buf = nullptr;
  // side stream + events: in multi-frame calls the (latency-bound, 1 lane per stream) high-pass of frame
  // f+1 runs beside analysis/network/synthesis of frame f
  hipStream_t side = nullptr, side_hp = nullptr;
  // ordering events of the pipelined schedule: own_* are the batch's persistent events, cur_* the handle that marks the
  // completion of hp / analysis / synthesis of frame f & 7 (an own_* event, or the stop event of a timed launch)
  hipEvent_t ev_begin = nullptr, own_hp[8] = {}, own_k1[8] = {}, own_k3[8] = {};
  hipEvent_t cur_hp[8] = {}, cur_k1[8] = {}, cur_k3[8] = {};
  void *arena = nullptr;
  size_t arena_bytes = 0;
  RnGroupDev g{};
  RnModelDev m{};
  RnTablesDev tb{};
  float *scratch_gains = nullptr, *scratch_vad = nullptr;
  float *debug_buf = nullptr;
  float *state_stage = nullptr;  // one flat state in HBM: export / import go through the gather / scatter kernels
  // chunk calls (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks; batch_chunks.cpp).  chunk_fifo: the streams' sample FIFOs, from
  // the first chunk call to the batch's end -- [N] records of RN_CHUNK_REC floats (chunk_plan.h; batch_chunk_fifos).  chunk_stage: the frames and the mask of the masked call inside a chunk call, [F][rows][M] floats then, F x rows
  // frames of RN_FRAME_SIZE floats in, [F][rows] bytes -- rows = N, or a list call's n_rows; chunk_stage_bytes of it, which grow when
  // a call needs more
  float *chunk_fifo = nullptr;
  void *chunk_stage = nullptr;
  size_t chunk_stage_bytes = 0;
  // split calls (include/rnnoise_amd.h: rnnoise_batch_analyze_device; batch_split.cpp).  split_pending: frames analysed and not yet
  // synthesised; split_parity: the spectra slot the first of them was analysed at.  split_store: split_cap entries of
  // rnnoise_amd_split_frame_bytes(n) each -- X | P | Ex Ep Exp | silence words (batch_split_entry) --, grown when a call needs more.
  // Pending frame f of T keeps its silence words in entry f and, unless it is the last, its spectra too; the last frame's spectra lie
  // in the batch's own slot, and where that slot is the one synthesis of frame 0 reads as "delayed" (T a multiple of RN_SPEC_SLOTS)
  // entry T - 1 holds a copy of the delayed spectra, made in front of the last K1 (split_prev_kept)
  int split_pending = 0, split_parity = 0, split_cap = 0;
  bool split_prev_kept = false;
  void *split_store = nullptr;
  // host-fed path (rnnoise_batch_process, host_io.cpp).  `run` carries the kernels and `down` the downloads of both kinds of caller
  struct HostIo {
    hipStream_t up = nullptr, run = nullptr, down = nullptr;
    // pageable callers, the chunk loop: two chunks in flight -- H2D of chunk i+1 (on `up`) and D2H of chunk i-1 overlap the kernels of
    // chunk i -- between device staging d_* and pinned bounce buffers h_*
    hipEvent_t up_done[2] = {}, run_done[2] = {}, down_done[2] = {};
    float *d_in[2] = {}, *d_out[2] = {}, *d_vad[2] = {}, *d_gains[2] = {};
    float *h_in[2] = {}, *h_out[2] = {}, *h_vad[2] = {}, *h_gains[2] = {};
    int chunk_frames = 0;
    size_t pcm_floats = 0;  // capacity of d_in / d_out and h_in / h_out of one chunk
    // pinned callers: a ring of RING frame slots, filled and drained frame by frame beside the kernels of one device call
    static constexpr int RING = 6;
    char *ring_mem = nullptr;
    hipEvent_t r_k3[RING] = {}, r_down[RING] = {}, r_up[RING] = {}, r_hp[RING] = {};
    struct Sdma *sdma = nullptr;  // copy mode "sdma" (host_io.cpp): explicit copy engines underneath HIP, created on first use
  } io;
  // timing
  bool timing = false;
  struct Ev { hipEvent_t a, b; int kind; };
  std::vector<Ev> pending, pool;
  double ms_sum[4] = {0, 0, 0, 0};  // analysis, network, synthesis, high-pass
  long launches = 0;
};

struct PooledRef;
// The combiner of a pool (dropin.cpp): concurrent rnnoise_process_frame calls on states of one pool are gathered into launch
// groups -- ONE set of the four latency kernels over a row list (rn_dev.h: RnRows) per group, a few groups in flight on streams
// of their own.
struct CombMember {
  PooledRef *ref;  // dereferenced only while the request is queued or being launched (its caller is blocked then); afterwards an identity
  int slot;        // the state's row: its request / sleeping / done words are the pool's (StatePool::req ...), valid whatever the state does
  uint32_t seq;    // the request of `ref` this entry stands for (a state that has its frame may be back with the next one
                   // before the group's owner has retired the old entry)
};
struct Combiner {
  static constexpr int MAXG = 8;
  std::mutex mu;
  int n_streams = 0;                       // streams created so far (at most $RNNOISE_AMD_COMBINE_STREAMS)
  hipStream_t stream[MAXG] = {};
  bool busy[MAXG] = {};                    // a group is in flight on the stream
  std::vector<CombMember> members[MAXG];   // ... these requests
  std::vector<CombMember> queue;           // submitted, not launched yet
  bool gathering = false;                  // a caller holds a free stream back for the callers that have just got their frames
  std::atomic<int> pending_returns{0};     // callers that have just got their frame and have not come back with the next one yet
  std::atomic<uint64_t> t_complete_ns{0};  // ... when the last of them left
  std::atomic<int> active{0};              // threads inside rnnoise_process_frame on this pool right now (spin or sleep?)
  std::atomic<uint64_t> group_ns{0};       // running estimate of a group's launch -> frames-out time (followers sleep through most of it)
};

// A pool of device-resident one-stream states of one model on one device: the arrays of a POOL_SLOTS-stream batch, of
// which every rnnoise_create() owns one row, and one block of pinned host memory per row through which the row's frames
// travel (the kernels address it directly: no copy commands).
struct StatePool {
  // rows of a pool: $RNNOISE_AMD_POOL_ROWS (default and maximum RN_POOL_ROWS_MAX = 1024, at least 64; 27 KB of HBM and 3.9 KB of
  // pinned host memory per row).  Round 4 had 64 = one launch group's worth, so the 65th state opened a second pool with a combiner
  // and three streams of its own -- 64 threads over 256 / 1,024 states: 152 k / 30 k frames/s against 304 k / 132 k with 256 rows.
  int rows = 0;
  RNNoiseBatch *batch = nullptr;   // owns the arena; never processed as a whole
  static constexpr int FLAT_ROWS = 64;  // staged states (rnnoise_init states borrow rows 0 .. 63 only)
  float *h_io = nullptr;                // pinned [rows][RN_ROW_IO]: in[480] | pad[4] | out[480] | vad | pad[2] | done (rn_dev.h: RnRows)
  float *d_flat = nullptr;              // [FLAT_ROWS][RN_STATE_PITCH] staging of self-contained states (rnnoise_init path)
  std::mutex mu;
  std::vector<unsigned long long> used;  // bit per row
  // combiner words of the rows' requests.  They live HERE, not in the state (PooledRef), because a group's owner touches a
  // member's words after the member may have taken its frame and been destroyed: pool memory outlives every state of the pool
  int *req = nullptr;        // [rows] (sequence number << 4 | state) of the row's request in flight (atomic access; futex word)
  int *sleeping = nullptr;   // [rows] the row's caller sleeps on req[row] (atomic access)
  Combiner comb;
};

// What a DenoiseState holds when it came from rnnoise_create(): a row of a StatePool plus the host-side frame
// bookkeeping of that row.  (A member of a union with the self-contained state: plain data only.)
struct PooledRef {
  StatePool *pool;
  int slot;
  int parity, ring_slot;
  float *h_io;        // the row's block of the pool's pinned frame memory
  std::mutex *mu;     // one frame at a time per state (the reference's states are not re-entrant either)
  int grp;            // combiner: stream slot of the group the request went into
  uint32_t seq;       // combiner: sequence number of the request (never 0); the last kernel stores it into the row's `done` word
  uint32_t req_no;    // combiner: requests made so far, failed ones included (the sequence numbers come from here, so that a retried
                      //           frame is never mistaken for the failed request)
  int poisoned;       // a launch group this state was in failed part of the way: its pitch ring may already hold the frame.  The
                      //           next call restarts the state from zero (as rnnoise_init would) instead of running one slot off
};

struct DenoiseState {
  uint32_t magic;
  uint32_t pad;
  RNNModel *model;
  union {
    float state[RN_STATE_FLOATS];  // rnnoise_init() on caller memory: self-contained POD, no library-owned resource (SURVEY 8b "Types")
    PooledRef ref;                 // rnnoise_create(): device-resident, released by rnnoise_destroy()
  };
};
static const uint32_t kStateMagic = 0x524e4e41u;   // "RNNA": self-contained state
static const uint32_t kPooledMagic = 0x524e4e50u;  // "RNNP": row of a StatePool

// The copy back end of a host-fed call (host_io.cpp): the frame buffers of the call are then a ring of `ring` frame slots in HBM
// (frame f lives in slot f % ring) that uploads fill and downloads drain while the kernels run; each hook is called on the host
// right where the named kernel of frame f is enqueued, with the stream it goes to.
struct FrameIo {
  int ring = 0;
  virtual int before_hp(int f, hipStream_t sc) = 0;
  virtual int after_hp(int f, hipStream_t sc) = 0;
  virtual int before_nn(int f, hipStream_t st) = 0;
  virtual int after_k3(int f, hipStream_t st) = 0;
 protected:
  ~FrameIo() = default;
};

// ---- functions that cross file boundaries ----
int tables_for_device(int device, RnTablesDev &out);                 // tables.cpp
int model_parse_locked(RNNModel *m);                                 // model.cpp (caller holds m->mu)
int model_on_device(RNNModel *m, int device, RnModelDev &out);       // model.cpp
RNNModel *default_model();                                           // model.cpp: the blob behind model == NULL
void pools_free(RNNModel *model);                                    // dropin.cpp: the state pools of a model (rnnoise_model_free)
RnGroupDev group_view(const RnGroupDev &g, int first, int count);    // batch.cpp
const RnKnobs &rn_knobs();                                           // batch.cpp: the dispatch switches, read once per process
void host_io_release(RNNoiseBatch *b);                               // host_io.cpp
// One process call of a batch: what the entry points of include/rnnoise_amd.h hand to the step (batch_step.cpp: batch_process_device_impl, device
// memory, asynchronous on `stream`) or to its host-buffer form (batch_process_staged: host memory through one device allocation,
// synchronous; stream, hooks and packed are not read).
struct ProcessCall {
  void *out = nullptr;  // PCM frames: float, or int16 with s16 set
  const void *in = nullptr;
  float *vad = nullptr, *gains = nullptr;  // optional
  int n_frames = 0;
  void *stream = nullptr;  // a hipStream_t, as the API hands it over
  bool s16 = false;
  const uint8_t *active = nullptr;  // the presence mask of a masked call ([n_frames][rows] bytes, include/rnnoise_amd.h), or null
  // the streams of a stream-list call (n_rows int32, include/rnnoise_amd.h), or null; the buffers and `active` then have n_rows rows
  // per frame (rn_dev.h: RnGroupDev::list)
  const int *list = nullptr;
  int n_rows = 0;
  FrameIo *hooks = nullptr;  // the pinned ring of the host-fed path (host_io.cpp)
  bool packed = false;  // the buffers are the library's own, in the default layout whatever the batch's (batch_process_staged)
};
// One split call (include/rnnoise_amd.h: rnnoise_batch_analyze_device, rnnoise_batch_synthesize_device; batch_split.cpp): the caller's
// rows in place of what the other half of the step would have read or written.  Strides in floats, resolved (never 0).
struct SplitCall {
  float *features = nullptr;  // analyze: 65 floats per stream and frame
  long feat_fs = 0, feat_rs = 0;
  int *silence = nullptr;     // analyze: [n_frames][N] or null
  const float *gains = nullptr, *vad = nullptr;  // synthesize: 32 floats / 1 float per stream and frame
  long gains_fs = 0, gains_rs = 0, vad_fs = 0, vad_rs = 0;
};
// the arrays of entry k of a batch's pending store, and the bytes of an entry for n streams (= rnnoise_amd_split_frame_bytes)
struct SplitEntry {
  float *X, *P, *E;
  int *silence;
};
inline size_t batch_split_spec_bytes(int n) { return rn_align256((size_t)n * RN_SPEC_STRIDE * 4); }
inline size_t batch_split_entry_bytes(int n) {
  return 2 * batch_split_spec_bytes(n) + rn_align256((size_t)n * RN_SPEC_E_ROW * 4) + rn_align256((size_t)n * 4);
}
inline SplitEntry batch_split_entry(const RNNoiseBatch *b, int k) {
  const size_t spec = batch_split_spec_bytes(b->n), e = rn_align256((size_t)b->n * RN_SPEC_E_ROW * 4);
  uint8_t *p = static_cast<uint8_t *>(b->split_store) + (size_t)k * batch_split_entry_bytes(b->n);
  return {reinterpret_cast<float *>(p), reinterpret_cast<float *>(p + spec), reinterpret_cast<float *>(p + 2 * spec),
          reinterpret_cast<int *>(p + 2 * spec + e)};
}
// Whether a call that is refused while frames are pending (include/rnnoise_amd.h: "Split calls") has to return -1: every PCM, chunk
// and training call, state export / import / save / load and every setter start with it
inline bool batch_split_busy(const RNNoiseBatch *b) { return b && b->split_pending > 0; }
int batch_process_device_impl(RNNoiseBatch *b, const ProcessCall &c);  // batch_step.cpp: the whole step
int batch_process_staged(RNNoiseBatch *b, const ProcessCall &c);       // batch_step.cpp: ... on host buffers
// batch_step.cpp: the network of one frame on group g, once per model slot, timed as kind 1
int batch_network_step(RNNoiseBatch *b, RnGroupDev &g, const RnPlan &plan, bool listed, hipStream_t st);
int batch_chunk_restart_all(RNNoiseBatch *b);                          // batch_chunks.cpp: every stream's sample FIFOs as after create
int batch_chunk_fifos_ready(RNNoiseBatch *b, hipStream_t st);          // batch_chunks.cpp: ... allocated where the batch has none yet
// batch.cpp: whether the n entries of a HOST stream list all lie inside the batch and, with `unique`, name no stream twice; a null
// list stands for stream i in row i
bool host_list_ok(const RNNoiseBatch *b, const int *list, int n, bool unique);
// samples per row and frame at the batch's PCM rate
inline int batch_frame_samples(const RNNoiseBatch *b) { return b->g.rs_L ? b->g.rs_pitch : RN_FRAME_SIZE; }
// the sample FIFOs of streams first, first + 1, ... of a batch as the state kernels take them (chunk_plan.h: RnChunkDev, the call's
// fields null), at the batch's current frame length; all null before the first chunk call
inline RnChunkDev batch_chunk_fifos(const RNNoiseBatch *b, int first) {
  RnChunkDev c{};
  if (!b->chunk_fifo) return c;
  c.fifo = b->chunk_fifo + (size_t)first * RN_CHUNK_REC;
  c.M = batch_frame_samples(b);
  return c;
}
// whether a host call takes the staged path instead of the pinned ring / bounce chunks of host_io.cpp: at a PCM rate other than 48 kHz
// or with a rate table or an out-rate table, with a PCM layout, with interleaved channels, and the int16 calls of a batch with a
// format table, the input one or the output one
inline bool batch_host_call_staged(const RNNoiseBatch *b, bool s16) {
  return b->g.rs_L || b->out_Ls || b->row_stride || b->channels > 1 || b->link > 1 || (s16 && (b->g.pcm_fmt || b->out_fmt));
}
// the resampler fields of a 48 kHz batch (batch_tables.cpp: rs_point with a table) on a copy of the group of a batch that has an
// out-rate table and no resampling on its input side; rs_buf is there from the first out-rate table on
inline void batch_rs_48k(const RNNoiseBatch *b, RnGroupDev &g) {
  const size_t N = b->n;
  g.rs_L = 1;
  g.rs_pitch = RN_FRAME_SIZE;
  g.rs_hist = b->rs_buf;
  g.rs_up = b->rs_buf + N * RN_RS_HIST;
  g.rs_dn = b->rs_buf + N * (RN_RS_HIST + RN_FRAME_SIZE);
}
// K3's copy of a step's group: the effective output tables in the place of the input ones (rn_dev.h: RnGroupDev::rs_Ls, ::pcm_fmt).
// Without output tables: g as it is
inline RnGroupDev batch_k3_group(const RNNoiseBatch *b, RnGroupDev g) {
  if (b->out_Ls) {
    if (!g.rs_L) batch_rs_48k(b, g);
    g.rs_Ls = b->out_Ls;
  }
  if (b->out_fmt) g.pcm_fmt = b->out_fmt;
  return g;
}
// the batch's group as the state kernels take it: with the histories of a batch whose only resampling is on its output side
inline RnGroupDev batch_state_group(const RNNoiseBatch *b) {
  RnGroupDev g = b->g;
  if (b->out_Ls && !g.rs_L) batch_rs_48k(b, g);
  return g;
}
