// dispatch.h -- which form of each kernel a frame step runs, as pure functions of the step's shape and the dispatch switches
// (no HIP in here, so that tests/test_dispatch_cpu.py can run the rules at every boundary without a GPU).  All forms of a stage give
// the same bits; the rules only pick the fastest.  batch.cpp builds one plan per call (batch_process_device_impl); the launchers take
// the chosen form and make no size decision of their own.  (Drop-in frames take no plan: they run the row-list kernels, dropin.cpp.)
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// The dispatch switches ("Environment variables"; A/B runs and tests), read once per process by rn_knobs()
// (batch.cpp) through rn_knobs_from_env().
struct RnKnobs {
  int nn_layers_min;  // $RNNOISE_AMD_NN_LAYERS_MIN: MFMA path from this many streams layer by layer
  int nn_one_max;     // $RNNOISE_AMD_NN_ONE_MAX: vector path up to this many streams as rn_nn_one_kernel (0 = never)
  int hp_one_max;     // $RNNOISE_AMD_HP_ONE_MAX: K0 one wave per stream up to this many streams (a negative value: the default)
  int k1_spw;         // $RNNOISE_AMD_K1_SPW: 0 by size, 1 one stream per analysis workgroup, any other value four
  int tile_waves;     // $RNNOISE_AMD_TILE_WAVES: 8 | 16 forces the tile kernel's form, anything else by size
  int gru;            // $RNNOISE_AMD_GRU_VARIANT: 0 by size, 4 | 8 forced, -1 an unknown name (the layer-wise network fails)
  int pipe;           // $RNNOISE_AMD_PIPE: the frame schedule when the batch has none of its own (rn_schedule)
};

static inline RnKnobs rn_knobs_from_env() {
  auto num = [](const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
  };
  RnKnobs k;
  k.nn_layers_min = num("RNNOISE_AMD_NN_LAYERS_MIN", 10240);
  k.nn_one_max = num("RNNOISE_AMD_NN_ONE_MAX", 512);
  k.hp_one_max = num("RNNOISE_AMD_HP_ONE_MAX", -1);
  if (k.hp_one_max < 0) k.hp_one_max = 2048;
  k.k1_spw = num("RNNOISE_AMD_K1_SPW", 0);
  k.tile_waves = num("RNNOISE_AMD_TILE_WAVES", 0);
  k.pipe = num("RNNOISE_AMD_PIPE", 0);
  k.gru = 0;
  if (const char *e = getenv("RNNOISE_AMD_GRU_VARIANT"); e && *e) {
    if (!strcmp(e, "w4")) k.gru = 4;
    else if (!strcmp(e, "w8")) k.gru = 8;
    else {
      fprintf(stderr, "[rnnoise_amd] RNNOISE_AMD_GRU_VARIANT=%s: no such form of the layer kernel in this build (w4 | w8)\n", e);
      k.gru = -1;
    }
  }
  return k;
}

// ---- the forms ----
enum RnHpForm { RN_HP_ONE_WAVE, RN_HP_LANES };                                         // rn_hp_one_kernel | rn_hp_kernel
enum RnK1Form { RN_K1_SINGLE, RN_K1_FOUR };                                            // rn_analysis_single_kernel | rn_analysis_kernel
enum RnNnForm { RN_NN_ONE, RN_NN_VECTOR, RN_NN_TILE8, RN_NN_TILE16, RN_NN_LAYERS };    // rn_nn_one / _vector / _mfma / _mfma16 / layers
enum RnGruForm { RN_GRU_W4, RN_GRU_W8, RN_GRU_UNKNOWN };                               // rn_nn_gru_kernel | rn_nn_gru_w8_kernel
enum RnK3Form { RN_K3_FEW, RN_K3_WIDE };                                               // rn_synthesis_few_kernel | rn_synthesis_kernel

// What the rules look at in one step of one group of streams
struct RnStepShape {
  int n;           // streams of the group
  bool whole;      // the group is the whole batch and its state planes fit the layer kernels' 32-bit byte offsets
  int cus;         // compute units of the batch's device
  int nn_path;     // the batch's network path (rnnoise_batch_set_nn_path): 0 vector, 1 MFMA, 2 layer-wise
  bool pipelined;  // the step is a frame of a pipelined multi-frame call (rn_schedule): other frames' kernels run beside it
  bool per_stream; // per-stream frame phase (rn_dev.h: RnGroupDev::phase)
  bool low_rate;   // PCM below 48 kHz, or a per-stream rate table (rn_shape_low_rate; rn_dev.h: RnGroupDev::rs_L, ::rs_Ls)
  bool listed = false;  // a stream-list call (rn_dev.h: RnGroupDev::list): n counts its listed rows, never the batch
  bool companded = false;  // an int16 call of a batch with a per-stream format table (rn_dev.h: RnGroupDev::pcm_fmt)
  int channels = 1;        // interleaved channels of the call's PCM rows (rn_dev.h: RnGroupDev::pcm_chan); 1: none
  // The batch has an output table (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates, _out_formats): low_rate and companded
  // above then describe the INPUT side alone -- what K0 reads --, and the two below the OUTPUT side -- what K3 writes.  false: one
  // description serves both sides and the two below are not read (every plan is the one of a batch without output tables).
  bool split = false;
  bool out_low_rate = false;   // K3 runs its resampling epilogue: PCM below 48 kHz, a rate table, or an out-rate table
  bool out_companded = false;  // an int16 call whose output rows follow a format table, the input one or the output one
};

// RnStepShape::low_rate of a batch: its calls run the resampling prologue / epilogue -- at a PCM rate below 48 kHz, and at any rate
// once the batch carries a rate table (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates), whose streams may be at any of them
static inline bool rn_shape_low_rate(int pcm_rate, bool rate_table) { return pcm_rate != 48000 || rate_table; }

struct RnPlan {
  RnHpForm hp;
  RnK1Form k1;
  RnNnForm nn;
  RnGruForm gru;  // (RN_NN_LAYERS only)
  RnK3Form k3;
  bool k3_rs;  // K3 is launched with its resampling epilogue (dsp_kernels.hip: bit 9 of parity_arg): the output side's low_rate
};

static inline RnPlan rn_plan(const RnKnobs &k, const RnStepShape &s) {
  RnPlan p;
  // K0.  Up to 2,048 streams one wave per stream is the faster form.  With the lane = stream kernel's block loop waiting properly
  // (profiles/r6_hp_specialised.txt) that kernel is one wave's latency chain of ~36 us whatever the batch, from 1,024 to 5,120 streams,
  // and the one-wave form 25 / 35 / 45 / 55 / 65 us at 1,024 / 2,048 / 3,072 / 4,096 / 5,120: the switch sits at 2,048 -- alone on the
  // machine (one frame per call: 0.258 -> 0.239 ms per step at 4,096 streams) and inside pipelined calls (3,072 streams: 20.8 -> 21.1 M
  // frames/s; at 2,048 the one-wave form is the better one by 6 %).  Rounds 5-6 until then: 5,120 / 3,072.
  // Low-rate rows take the wave-per-stream form at every batch size.  (An upsampling prologue in the lane = stream kernel, one stream
  // after the other per wave, took that kernel from 50 to 61-64 SGPRs in every arrangement tried; the 48 kHz kernels keep their
  // registers instead.  The cost at large batches: DESIGN.md 4.10, profiles/resample_rate_bench.txt)  A batch with a rate table
  // plans the same way: its low-rate streams need the prologue, and one wave serves one stream, so each takes its own L.
  // A list call: the one-wave form at every size (the lane = stream kernel has no list path).
  // An int16 call of a batch with a format table (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats): the one-wave form at every
  // size too -- one wave serves one stream, so the row's format is wave-uniform and a wave reads either bytes or int16, and the lane =
  // stream kernel, where 64 neighbours of different formats would share a wave, keeps its registers.
  // Interleaved channels (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels): the one-wave form at every size as well.  A wave
  // of it reads its row with lane-consecutive samples, each cache line of the group slot once; a lane of the lane = stream kernel
  // would walk its row 4 C samples at a time beside 63 lanes of other slots, and its block loop has no registers to spare for the
  // addressing.  No other stage looks at the caller's PCM: K1, the network and K3's form do not depend on it.
  // Output tables (RnStepShape::split): K0 never reads them, so low_rate and companded are then the input side's alone, and a batch
  // whose inputs are all 48 kHz linear keeps the lane = stream kernel above hp_one_max whatever its outputs are.
  p.hp = s.listed || s.low_rate || s.companded || s.channels > 1 || s.n <= k.hp_one_max ? RN_HP_ONE_WAVE : RN_HP_LANES;
  // K1.  From 2,560 streams four streams share a workgroup (rn_analysis_kernel).  6,144 until round 6's last day; since the narrow
  // phases and the follower are shared by the four streams of a workgroup (round 6) that form is ahead from 3,072 streams -- 23.3
  // against 20.8 M frames/s there, 26.4 against 24.5 at 4,096 (one frame per call 0.201 against 0.231 ms), 27.8 against 26.0 at
  // 5,120 -- and level at 2,048 (profiles/r6_late_ab.txt).  Per-stream frame phase: the one-stream form at every size (the four
  // streams of rn_analysis_kernel share their narrow phases).
  p.k1 = s.listed || s.per_stream || k.k1_spw == 1 || (k.k1_spw == 0 && s.n < 2560) ? RN_K1_SINGLE : RN_K1_FOUR;
  // K2.  Path 1 runs the network layer by layer (nn_layers.hip: 64 streams per GRU workgroup) from 10,240 streams; below it the five
  // launches and the smaller grids cost more than the weight reuse gains.  The tile kernel holds out while a CU has at most two tiles
  // (8,192 streams on 256 CUs: 25.9 against 24.2 M frames/s); with a third its K2 jumps (0.139 -> 0.193 ms at 10,240 streams) and the
  // layer-wise network is ahead -- 27.5 against 25.8 M frames/s at 10,240, 29.5 against 26.2 at 12,288, one frame per call 24.8
  // against 23.0 M at 10,240 (profiles/r6_late_ab.txt; rounds 3-6 had the switch at 16,384).  The layer images are indexed by tile of
  // the whole batch: a part of a batch takes the tile kernel on paths 1 and 2 alike.
  // The tile kernel: sixteen waves per tile in a call that runs nothing beside the network while every tile has a CU to itself, eight
  // otherwise (nn_mfma.hip: rn_nn_mfma16_kernel has the measurements).
  // Path 0: up to 512 streams the latency-oriented kernel (nn_kernels.hip: rn_nn_one_kernel, one 14-wave workgroup with 125 KB of LDS
  // per stream, one per CU) finishes first -- measured K2 at 64 / 256 / 512 / 768 streams: 36 / 42 / 83 / 120 us against 82 / 101 /
  // 105 / 105 us for MFMA tiles of 16 streams; the vector kernel above.
  // A list call: never layer by layer (its tiles are tiles of listed rows, the layer images tiles of the batch) -- the tile kernel on
  // paths 1 and 2, the one-stream kernel on path 0 whatever the number of rows.
  const int tiles = (s.n + 15) / 16;
  const RnNnForm tile = k.tile_waves == 16 || (k.tile_waves != 8 && !s.pipelined && tiles <= s.cus) ? RN_NN_TILE16 : RN_NN_TILE8;
  if (s.listed) p.nn = s.nn_path == 0 ? RN_NN_ONE : tile;
  else if (s.whole && (s.nn_path == 2 || (s.nn_path == 1 && s.n >= k.nn_layers_min))) p.nn = RN_NN_LAYERS;
  else if (s.nn_path >= 1) p.nn = tile;
  else p.nn = s.n <= k.nn_one_max ? RN_NN_ONE : RN_NN_VECTOR;
  // The GRU layer kernel: the four-wave form (two workgroups per CU: 1-3 % under the eight-wave one stand-alone in every A/B of
  // profiles/r5_gru_bound.txt) once there are more 64-stream groups than CUs; the eight-wave form while every group has a CU to itself
  // (a four-wave workgroup would then leave each SIMD with ONE wave: 16,384 streams 0.200 against 0.174 ms for the three layers +
  // front + dense).  A forced name that is not a form fails the layer-wise network, not silently a default.
  const int groups = (tiles + 3) / 4;
  p.gru = k.gru == 4 ? RN_GRU_W4 : k.gru == 8 ? RN_GRU_W8 : k.gru ? RN_GRU_UNKNOWN : groups > s.cus ? RN_GRU_W4 : RN_GRU_W8;
  // K3.  Up to 256 streams the form that requests every operand up front (one frame: 10.4 -> 9.6 us).
  p.k3 = s.n <= 256 ? RN_K3_FEW : RN_K3_WIDE;
  // ... and its resampling epilogue from the side K3 writes: the output side of a batch with output tables, else the one description
  p.k3_rs = s.split ? s.out_low_rate : s.low_rate;
  return p;
}

// The frame schedule of a call (batch.cpp: batch_process_device_impl).  Multi-frame calls are pipelined over three streams: K0 on
// one side stream, K1 on another, network + synthesis on the caller's.  A forced schedule -- the batch's own
// (rnnoise_batch_set_schedule), else $RNNOISE_AMD_PIPE -- of 9 keeps every kernel on the caller's stream, 1 puts only K0 aside.
// Measured after the fence-free events: the 3-stream schedule is the best or within noise of the best from 1 K to 64 K streams
// (65,536: 20.2 M frames/s vs 20.0 M on one stream, 19.6 M with only K0 aside), so it is the only default.
struct RnSchedule {
  bool pipelined;  // K0 (and K1) of later frames on side streams
  bool side_k1;    // K1 on a side stream of its own
};
static inline RnSchedule rn_schedule(const RnKnobs &k, int n_frames, int batch_schedule) {
  const int force = batch_schedule ? batch_schedule : k.pipe;
  const bool pipelined = n_frames > 1 && force != 9;
  return {pipelined, pipelined && force != 1};
}

// The network path of a new batch: the MFMA tiles above rn_nn_one_kernel's range (and from one whole tile up), the vector path below.
static inline int rn_default_nn_path(const RnKnobs &k, int n) { return n > k.nn_one_max && n >= 16 ? 1 : 0; }

// ---- caller-defined PCM strides (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout) ----
// what the setter accepts: the default (0, 0), or two positive multiples of 4 samples (the row stride an int: the kernels' row pitch)
static inline bool rn_pcm_layout_ok(long frame_stride, long row_stride) {
  if (frame_stride == 0 && row_stride == 0) return true;
  return frame_stride > 0 && row_stride > 0 && frame_stride % 4 == 0 && row_stride % 4 == 0 && row_stride <= 2147483647L;
}
// whether the frame slots of a call -- n_frames x n_rows slots of M samples, slot (f, r) at f * frame_stride + r * row_stride -- are
// disjoint: rows inside a frame (row-major) or frames inside a row (stream-contiguous).  A call with no slot fits.
static inline bool rn_pcm_layout_fits(long frame_stride, long row_stride, int M, int n_rows, int n_frames) {
  if (M <= 0 || n_rows < 0 || n_frames < 0 || frame_stride <= 0 || row_stride <= 0) return false;
  if (n_rows == 0 || n_frames == 0) return true;
  typedef long long ll;
  const bool row_major = row_stride >= M && (ll)frame_stride >= (ll)n_rows * row_stride;
  const bool stream_contiguous = frame_stride >= M && (ll)row_stride >= (ll)n_frames * frame_stride;
  return row_major || stream_contiguous;
}

// ---- interleaved channels (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels) ----
#define RN_MAX_CHANNELS 8  // = RNNOISE_AMD_MAX_CHANNELS
// what the setter accepts for a batch of n streams
static inline bool rn_pcm_channels_ok(int channels, int n_streams) {
  return channels >= 1 && channels <= RN_MAX_CHANNELS && n_streams % channels == 0;
}
// whether a call's group slots -- n_frames x n_rows / channels slots of M * channels samples, slot (f, g) at f * frame_stride +
// g * row_stride -- are disjoint: rn_pcm_layout_fits with the slot as the row.  Rows that do not fill whole groups never fit.
static inline bool rn_pcm_channels_fit(long frame_stride, long row_stride, int M, int channels, int n_rows, int n_frames) {
  if (channels < 1 || channels > RN_MAX_CHANNELS || M <= 0 || n_rows < 0 || n_rows % channels) return false;
  return rn_pcm_layout_fits(frame_stride, row_stride, M * channels, n_rows / channels, n_frames);
}
