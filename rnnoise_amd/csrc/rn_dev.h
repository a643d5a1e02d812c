// rn_dev.h -- device-side data model shared by the HIP kernels and the host shim.
//
// Layout in HBM (one RnGroupDev per group of N streams on one GPU):
//   every per-stream field is its own dense [N][len] fp32 array, so a wavefront that
//   owns one stream-frame reads and writes contiguous, coalesced rows, and the batched
//   network kernel sees (streams x features) row-major matrices.
//   The spectra that the reference copies into delayed_* every frame
//   (src/denoise.c:498-502) rotate through RN_SPEC_SLOTS = 3 slots instead: the analysis
//   kernel of frame t writes slot t%3, the synthesis kernel of frame t reads slot (t-1)%3
//   as "delayed" -- no copy -- and the third slot lets analysis(t+1) overlap synthesis(t).
//   analysis_mem (src/denoise.c:73) is not stored: it always equals the last 480 samples
//   of the previous pitch_buf (both are the previous high-passed frame), which sit in
//   the pitch ring (RN_RING_SLOTS = 6 slots of 480 samples = 2880 floats per stream).
#pragma once
#include <stdint.h>
// 1: the instrumented build (librnnoise_amd_instr.so) -- stage taps and shader-clock probes compiled into the kernels, probe
// kernels and the rnnoise_amd_debug.h entry points present.  0: the product library.
#ifndef RN_INSTRUMENT
#define RN_INSTRUMENT 0
#endif
#include "../../include/rn_layout.h"
#include "g711.h"
#include <stdlib.h>
// The environment variables this library reads come in two classes:
//   getenv("RNNOISE_AMD_...")   product knobs: configuration, and dispatch thresholds that select between kernels with the
//                               same bits.  Every one of them is listed in INTEGRATION.md ("Environment variables");
//                               tests/test_product_surface_cpu.py compares the names found in the product .so with that list.
//   RN_LAB_ENV("...")           read by the INSTRUMENTED build only: TEST_FAIL_GROUP (fault injection, dropin.cpp) and K1_STOP
//                               (section prefix runs, dsp_kernels.hip).  In the product the macro is a null constant -- the name is
//                               not even in the binary, and no environment can steer a drop-in librnnoise.so.0 onto them.
#if RN_INSTRUMENT
#define RN_LAB_ENV(name) getenv("RNNOISE_AMD_" name)
#else
#define RN_LAB_ENV(name) (static_cast<const char *>(nullptr))
#endif

// floats of one band-product array in LDS (the layout of RnTablesDev::band_q, tables.cpp: tables_for_device); the analysis
// kernel forms two band vectors at once from two arrays this far apart
#define RN_BAND_QSTRIDE 1044
#define RN_SPEC_STRIDE 964  // 481 complex = 962 floats, padded to a 16-byte multiple
// the other row lengths of the per-stream arrays (RN_GROUP_ARRAYS below) that no constant of rn_layout.h names
#define RN_SPEC_E_ROW 96    // Ex | Ep | Exp, RN_NB_BANDS each
#define RN_CONV1_ROW 130    // conv1_state: two frames of RN_CONV1_IN inputs
#define RN_CONV2_ROW 256    // conv2_state: two frames of RN_CONV2_IN inputs
#define RN_FEAT_ROW 68      // RN_NB_FEATURES = 65 used
#define RN_LPC2_ROW 8       // 5 used
// floats between the portable states of an array of them on the device (state_kernels.hip): rows stay 16-byte aligned, which
// RN_STATE_FLOATS * 4 = 25,128 bytes would not give every other row
#define RN_STATE_PITCH ((RN_STATE_FLOATS + 3) & ~3)
// spectra slots: frame t writes slot t%3, synthesis of frame t reads slots t%3 (Ex) and (t-1)%3 (the
// reference's delayed_*); the third slot lets the analysis of frame t+1 run beside synthesis of frame t
#define RN_SPEC_SLOTS 3
// pitch ring: the 1728-sample pitch_buf (3.6 frames) lives in a ring of 480-sample slots and is never
// shifted.  Six slots rather than four: the analysis of frame t reads slots t-3..t, so the high-pass
// kernel may run up to two frames ahead (it writes slot t+1 or t+2) without touching what is being read.
#define RN_RING_SLOTS 6
#define RN_RING_SIZE (RN_RING_SLOTS * RN_FRAME_SIZE)
// ... and beside it the same ring 2x DECIMATED (src/pitch.c:155-160: x_lp[i] = .5 (.5 (x[2i-1] + x[2i+1]) + x[2i])): 240 samples per slot.
// pitch_buf[0] always sits at an even ring position, so a decimated sample is a function of three neighbouring ring samples whichever
// frame asks for it -- except x_lp[0], which has no left neighbour and is formed by its reader.  The high-pass kernel that writes a
// slot of the ring writes the slot's 240 decimated samples too (it has the filtered frame in registers); its autocorrelation pass and
// the analysis kernel then read 864 floats per frame instead of decimating 1728 again each: 3.4 KB per stream and frame less, in each.
// Derived data: rebuilt by the state scatter kernel after an import, zero after a reset (as the ring).
#define RN_XRING_SLOT (RN_FRAME_SIZE / 2)
#define RN_XRING_SIZE (RN_RING_SLOTS * RN_XRING_SLOT)
// ring position of pitch_buf[0] when the newest frame sits in `slot` (its last sample = pitch_buf[1727])
#define RN_RING0(slot) (((slot) * RN_FRAME_SIZE + RN_RING_SIZE - (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE)) % RN_RING_SIZE)

struct RnTablesDev {
  const float *half_window;   // [480]   src/rnnoise_tables.c:570 (by formula)
  const float *dct;           // [32*32] src/rnnoise_tables.c:669
  const float *twiddles;      // [960*2] src/rnnoise_tables.c:77
  const float *band_frac;     // [400]   (float)j/band_size of each bin (src/denoise.c:100)
  const uint16_t *bitrev;     // [960]   digit reversal of the 5.3.4.4.4 FFT (src/rnnoise_tables.c:10, by formula), padded position
  const uint8_t *band_of_bin; // [400]   band index i with eband[i] <= bin < eband[i+1]
  const uint16_t *rcp16;      // [4096]  x86 rcpps stand-in of the active host profile (rcp_profiles.h, oracle/rcp_capture.c):
                              //         entry i = (bits(rcp(1 + i/4096)) - 0x3f000000) >> 11; see rn_rcp_bits()
  const float *fft_tw;        // [16][64][2] per-lane twiddles of the register-resident FFT (fft_reg.h: RN_FTW_*)
  const uint32_t *band_q;     // [400]  per bin: LDS slot of its (1-frac) term | slot of its frac term << 11 | band << 22
  const uint32_t *band_chain; // [34]   per band accumulator: first slot (16-byte aligned) | number of terms << 16
  const uint16_t *band_pad;   // [64]   the floats behind an accumulator's last term up to the end of its last 16-byte slot
                              //        (48 of them; the table repeats the last): they hold +0.0f while the sums are formed
  const double *log_tab;      // [128][2] {1/c, log c}: the table of the host libm's log() (log10_glibc.h) -- the feature stage then evaluates
                              //         log10 operation for operation as the reference's host does; null: the device library's log10
                              //         ($RNNOISE_AMD_LOG10=ocml, or a host whose libm is not the modelled one; tables.cpp)
  double dct_scale;           // sqrt(2./22), src/denoise.c:168
};

// one linear layer of the network, repacked for the GPU (model.cpp: stage_linear)
struct RnLinearDev {
  const float *bias;      // float layers: bias; int8 layers: subias (x86 profile, nnet_arch.h:145-147)
  const float *fw;        // float weights, column-major W[j*N + i]
  const float *fwm;       // the same in v_mfma_f32_16x16x4_f32 operand order [row tile][step/4][lane][step%4] (nout % 16 == 0), or null
  const float *scale;     // per-output scale (already /127, c_export/common.py:248)
  const float *diag;      // recurrent diagonal [3*M] or null
  const int8_t *w;        // int8 blocks, 32 bytes each = [8 rows][4 cols]
  const int8_t *wmf;      // same weights zero-filled to dense, in MFMA A-fragment order
                          //   [row tile][k tile][lane][16 B]: row = 16*rt + (lane&15), k = 64*kt + 16*(lane>>4) + byte
  const int *rowsum128;   // 128 * sum_j w[i][j]  (offset that turns s8 x s8 dots into s8 x u8)
  const int *grp_start;   // [nout/8 + 1] first block of each 8-row group
  const uint16_t *cols;   // [nblocks] first input column of each block
  // the same int8 weights once more, row-major for the vector path (model.cpp: model_on_device): a row's bytes of FOUR
  // consecutive blocks of its group are one 16-byte chunk, a group's list padded with zero blocks to a multiple of four --
  //   wrow [(((grp4[g] + c) * 8 + (row & 7)) * 4 .. + 3]       chunk c of a row of group g (grp4[g+1] - grp4[g] chunks; the eight
  //                                                            rows' chunks c are one 128-byte line)
  //   cq   [grp4[g] + c]                                       input dword (column / 4) of the chunk's four blocks, one byte each
  // so a lane fetches four blocks per load instruction instead of one (the texture addresser spends as long on a 4-byte
  // load as on a 16-byte one: it, not the cache, paced the row products)
  const int *wrow;
  const uint32_t *cq;
  const int *grp4;        // [nout/8 + 1]
  const float *fw4;       // dense_out only: the float weights as [input / 4][output][input % 4] -- a lane of the one-stream
                          //   kernel's chain wave reads the weights of four consecutive steps of ITS output as one 16-byte LDS read
  int nin, nout;
};

struct RnModelDev {
  RnLinearDev conv1, conv2, gru_in[3], gru_rec[3], dense_out, vad_dense;
};

struct RnGroupDev {
  int n_streams;   // streams this launch works on (rows 0..n_streams-1 of every array below)
  int n_stride;    // streams the arrays were laid out for: plane stride of gru_state / lpc2.  A kernel may be pointed at a
                   // sub-range of a batch (the pooled one-stream states behind rnnoise_create): every pointer advanced by
                   // first_stream * row length, n_streams = count, n_stride = the batch's size
  // persistent per-stream state
  float *mem_hp;       // [N][2]
  float *pitch_ring;   // [N][RN_RING_SIZE = 2880] ring of high-passed frames; pitch_buf (src/denoise.c:76) = its latest 1728 samples
  float *xlp_ring;     // [N][RN_XRING_SIZE = 1440] the same ring 2x decimated (derived: see RN_XRING_SLOT)
  float *synth_mem;    // [N][480]
  float *last_gain;    // [N]
  int *last_period;    // [N]
  float *lastg;        // [N][32]
  float *conv1_state;  // [N][RN_CONV1_ROW = 130]
  float *conv2_state;  // [N][RN_CONV2_ROW = 256]
  float *gru_state;    // [3][N][384]
  float *spec_X[RN_SPEC_SLOTS];  // [N][RN_SPEC_STRIDE]  rotating: current, delayed, (free for the next frame)
  float *spec_P[RN_SPEC_SLOTS];  // [N][RN_SPEC_STRIDE]
  float *spec_E[RN_SPEC_SLOTS];  // [N][RN_SPEC_E_ROW = 96] = Ex | Ep | Exp
  // per-step scratch
  float *features;     // [N][RN_FEAT_ROW = 68] (65 used)
  int *silence;        // [N]
  int *pitch;          // [N]   final period (debug/tests)
  float *features_b;   // second copy of the three per-step arrays above (the host alternates them per frame
  int *silence_b;      //   so that the analysis of frame t+1 may overlap network/synthesis of frame t)
  int *pitch_b;
  float *gains;        // [N][32] raw network gains of the current step
  float *vad;          // [N]
  float *lpc2;         // [RN_RING_SLOTS][N][RN_LPC2_ROW = 8] (5 used) FIR taps of rnn_pitch_downsample, produced by K0, consumed by K1
  float *nn_act;       // [N][384] conv2 output in f32 (MFMA path: input of dense_out)
  int8_t *act_q[4];    // [ceil(N/16)][6144] layer-wise network: u8-quantised activations per 16-stream tile, B-fragment order:
                       //   [0] conv2 output (scratch of the step), [1 + k] GRU state k -- at once the input of layer k + 1 and
                       //   the recurrent operand of layer k at the NEXT frame, so the layer kernels never re-quantise the
                       //   f32 state.  Derived data: valid only while every state change went through the layer kernels
                       //   (RNNoiseBatch::img_valid; rn_launch_nn_requant rebuilds them).  Whole batches only, never offset by views.
  float *train_clean_mem;  // [N][480] analysis memory of the clean stream (training-feature extraction only)
  float *debug;        // [N][RN_DBG_FLOATS] pitch stage taps, or null (tests only)
  // per-stream frame phase (include/rnnoise_amd.h: masked calls).  Null `phase` on every lock-step launch: the kernels then take the
  // ring and spectra slots from their launch arguments.  Set, stream s is at frame phase p = phase[s] + (frames of s present in
  // 0 .. call_frame - 1) of the call: ring slot p % RN_RING_SLOTS, spectra slot p % RN_SPEC_SLOTS (rn_stream_phase).  The K0 / K1 / K3
  // forms that own one stream per workgroup or lane honour it; the synthesis kernel of the call's last frame advances phase[s].
  int *phase;                  // [N] frame phase of each stream at the start of the call, mod RN_RING_SLOTS
  const uint8_t *active;       // [call_frames][n_stride] nonzero = the stream has this frame; null = every stream present
                               //   ([call_frames][list_n], by row, in a list call)
  int call_frame, call_frames; // frame of the call this launch works on; frames in the call
  // Stream-list calls (include/rnnoise_amd.h: rnnoise_batch_process_device_list).  Null `list` on every other launch.  Set, the launch
  // works on list_n ROWS: workgroup (or tile row) i is stream list[i] (rn_stream_at: RnStreamAt::i, ::s).  The caller's buffers -- the
  // PCM rows the launchers hand K0 and K3, the mask `active`, list_vad, list_gains -- are indexed by row, every per-stream array by
  // stream; an entry outside [0, n_stride) is an absent row that touches nothing.  `vad` / `gains` then point at the per-stream
  // scratch (the network writes them by stream as in every call) and K3 copies row i out to list_vad / list_gains, zeros for an absent
  // row.  Grids are sized by list_n (rn_launch_rows).
  const int *list;             // [list_n] int32, or null
  int list_n;
  float *list_vad;             // [list_n] or null
  float *list_gains;           // [list_n][32] or null
  // PCM rate of the batch's calls as its code rs_L (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate): the divisor 48000 / R, or
  // RN_RATE_32K for 32 kHz, which divides nothing (2:3; rn_rate_samples: the frame of a code).  0 / null at 48 kHz: every
  // launch is today's.  Otherwise K0 upsamples the caller's rows and K3 downsamples its output (rs_coeffs.h: the filters), and
  // rs_hist[s] holds stream s's filter histories: [0, RN_RS_UP_HIST) the last low-rate input samples, [RN_RS_DOWN0, RN_RS_DOWN0 +
  // RN_RS_DOWN_HIST(L)) the last 48 kHz output samples (RN_RS_DOWN_HIST_32K at 32 kHz), oldest first.  Zeroed by reset, reset_streams,
  // import and a rate change.
  float *rs_hist;              // [N][RN_RS_HIST]
  float *rs_up, *rs_dn;        // [N][480] each: the frame at 48 kHz as K0 formed it from the low-rate row / as K3's body formed it
  void *rs_out;                // K3 only: the caller's low-rate output (float or int16)
  int rs_L;
  // Per-stream PCM rates (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates).  Null rs_Ls: every stream runs at the batch's rate
  // (every launch is today's).  Set, rs_L is the BATCH's rate code Lb (1 at 48 kHz: the batch then has rs_hist / rs_up / rs_dn too) and
  // stream s runs at code rs_Ls[s] -- anything that is no code, or whose frame is longer than the batch's, reads as Lb (rn_stream_L).
  // Indexed by batch stream, also in a list call.  rs_pitch: samples between the caller's PCM rows, the M of Lb (rn_rate_samples), set
  // whenever rs_L is; a stream uses the first M_s samples of its row.  L_s = 1 (only where Lb = 1, so its row is a whole 48 kHz frame):
  // K0's body reads the row and K3's body writes it in place, no filter runs and the stream's history is not touched.
  const uint8_t *rs_Ls;        // [N] or null
  int rs_pitch;
  // Caller-defined PCM layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout).  0: the caller's rows are the form's own constant
  // apart -- RN_FRAME_SIZE samples, or rs_pitch on a resampling launch (every launch is today's).  Otherwise the samples (of the call's
  // type: float or int16; a companded row keeps its int16 pitch) between the caller's rows i and i + 1 of `in` and `out`, a multiple
  // of 4 (rn_pcm_pitch).  Only K0 and K3 look at it, and only where they address the caller's buffers: the scratch rows rs_up / rs_dn
  // stay RN_FRAME_SIZE apart.  The frame pitch is the host's: the launchers get each frame's base pointer (batch.cpp).
  int pcm_pitch;
  // Interleaved channels (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels).  0: one row per slot (every launch is today's).
  // C = 2 .. 8: the caller's rows are taken C at a time -- row r = C g + c is channel c of group g, its sample i at
  //     g * pitch + c + i * C      (pitch: pcm_pitch, or C times the form's own constant without a layout)
  // of `in` and `out`, a companded row's BYTE i at byte g * pitch * sizeof(short) + c + i * C (rn_pcm_row).  K0 and K3 only, and only
  // in their one-wave-per-stream forms (dispatch.h: the lane = stream K0 is never planned for such a call); r is the list position in
  // a list call.  K3 stores single elements: the siblings' samples in between belong to other workgroups, maybe of other launches.
  int pcm_chan;
  // Linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link).  0: every row keeps its own gains and VAD (every launch is
  // today's).  K = 2 .. 8: the rows of the launch are taken K at a time -- rows K j .. K j + K - 1 are a link group, a row being the
  // stream index or the list position -- and K3 (synthesis_body) folds the raw gains and the VADs of the group's PARTICIPANTS, the rows
  // whose silence word of this frame is 0, in ascending row order: per band the smallest gain, and the largest VAD.  A participant
  // shapes its spectrum with the folded gains; every present row decides its gate with the folded VAD.  Set only on the copies the
  // step hands K3 (batch.cpp); b->g never carries it.  K3 reads what the network and K1 of this frame wrote for the siblings --
  // gains, vad, silence -- and nothing a sibling's K3 workgroup writes.  (The int fills the padding in front of pcm_fmt: no
  // kernel's arguments move.)
  int link;
  // Per-stream PCM formats (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats).  Null pcm_fmt: every row of an int16 call holds
  // int16 samples (every launch is today's).  Set, stream s's rows of the int16 calls hold pcm_fmt[s]: RN_PCM_ULAW / RN_PCM_ALAW
  // (g711.h) one byte per sample in the FIRST 480 / L_s bytes of the row -- K0 expands them where it reads the row (hp_one_body,
  // rs_up_stream), K3 compresses its truncated int16 value where it stores it (synthesis_body, rs_down_stream) --, anything else
  // int16 (rn_stream_fmt).  Rows keep their pitch.  Indexed by batch stream, also in a list call.  Float calls never look at it.
  const uint8_t *pcm_fmt;      // [N] or null
  // Per-stream models (include/rnnoise_amd.h: rnnoise_batch_add_model).  Null model_of: every row belongs to the launch (a batch with
  // one model).  Set, the network launch of slot model_sel owns row s when (model_of[s] < n_models ? model_of[s] : 0) == model_sel
  // (rn_owns): only owned rows get stores -- state, state images, gains, vad -- and a workgroup with no owned row returns at once.
  const uint8_t *model_of;     // [N] slot of every stream, or null
  int model_sel, n_models;
  // Per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls).  Null ctl / gate_c: every launch is
  // today's (every drop-in pool, and a batch without a table).  Set, K3 (synthesis_body) reads stream s's record ctl[s] = {floor, thr,
  // hold} -- NaN as 0, each value clamped into its range, hold truncated -- and its counter gate_c[s], the frames since its last voice
  // frame (RN_CTL_NONE: none yet).  On every frame the stream has: c = (thr == 0 || vad >= thr) ? 0 : min(c + 1, RN_CTL_NONE); the
  // band gains that shape the spectrum are floored at `floor` (after the decay cap and the lastg update, which see the raw gain); the
  // spectrum is zero when thr > 0 && c > hold.  gate_c[s] = RN_CTL_NONE after reset, reset_streams and import (the scatter kernel)
  // and when a table is set after none.
  const float *ctl;            // [N][RN_CTL_FLOATS] or null
  int *gate_c;                 // [N] or null
};
// The per-stream arrays of RnGroupDev, once, in the order the arena holds them: batch_layout carves them and group_view advances
// them from this list (batch.cpp).
//   ROWS(member, type, row, planes)   [planes][N][row]: carved whole, a view advances it by `row` per stream; the planes of gru_state
//                                     and lpc2 stay n_stride rows apart
//   TILES(member, type, tile)         `tile` elements per 16 streams: whole batches only, never offset by a view
//   OPT(member, row)                  [N][row], not in the arena: null until its feature sets it, advanced only when set (ctl and
//                                     gate_c are set together, and so are rs_hist, rs_up and rs_dn)
// Slot k of the three spectra sets lies together, and so the four images of act_q.
#define RN_EACH(k, n, ...) \
  for (int k = 0; k < (n); k++) { __VA_ARGS__ }
#define RN_GROUP_ARRAYS(ROWS, TILES, OPT)                        \
  ROWS(mem_hp, float, 2, 1)                                      \
  ROWS(pitch_ring, float, RN_RING_SIZE, 1)                       \
  ROWS(xlp_ring, float, RN_XRING_SIZE, 1)                        \
  ROWS(synth_mem, float, RN_FRAME_SIZE, 1)                       \
  ROWS(last_gain, float, 1, 1)                                   \
  ROWS(last_period, int, 1, 1)                                   \
  ROWS(lastg, float, RN_NB_BANDS, 1)                             \
  ROWS(conv1_state, float, RN_CONV1_ROW, 1)                      \
  ROWS(conv2_state, float, RN_CONV2_ROW, 1)                      \
  ROWS(gru_state, float, RN_GRU, 3)                              \
  RN_EACH(k, RN_SPEC_SLOTS,                                      \
          ROWS(spec_X[k], float, RN_SPEC_STRIDE, 1)              \
          ROWS(spec_P[k], float, RN_SPEC_STRIDE, 1)              \
          ROWS(spec_E[k], float, RN_SPEC_E_ROW, 1))              \
  ROWS(features, float, RN_FEAT_ROW, 1)                          \
  ROWS(silence, int, 1, 1)                                       \
  ROWS(pitch, int, 1, 1)                                         \
  ROWS(features_b, float, RN_FEAT_ROW, 1)                        \
  ROWS(silence_b, int, 1, 1)                                     \
  ROWS(pitch_b, int, 1, 1)                                       \
  ROWS(gains, float, RN_NB_BANDS, 1)                             \
  ROWS(vad, float, 1, 1)                                         \
  ROWS(nn_act, float, RN_GRU, 1)                                 \
  RN_EACH(k, 4, TILES(act_q[k], int8_t, 6144))                   \
  ROWS(lpc2, float, RN_LPC2_ROW, RN_RING_SLOTS)                  \
  ROWS(train_clean_mem, float, RN_FRAME_SIZE, 1)                 \
  OPT(debug, RN_DBG_FLOATS)                                      \
  OPT(phase, 1)                                                  \
  OPT(active, 1) /* (rows of the mask keep the stride n_stride) */ \
  OPT(model_of, 1)                                               \
  OPT(ctl, RN_CTL_FLOATS)                                        \
  OPT(gate_c, 1)                                                 \
  OPT(rs_Ls, 1)                                                  \
  OPT(pcm_fmt, 1)                                                \
  OPT(rs_hist, RN_RS_HIST)                                       \
  OPT(rs_up, RN_FRAME_SIZE)                                      \
  OPT(rs_dn, RN_FRAME_SIZE)
// what the records of a state gather / scatter launch are (state_kernels.hip): portable states, RN_STATE_PITCH floats apart, or
// snapshot records (include/rn_layout.h: RN_SNAP_*), or the caller's PCM rows of a chunk call (chunk_plan.h: RnChunkDev -- no `rec`)
enum RnRecKind { RN_REC_STATE, RN_REC_SNAP, RN_REC_CHUNK };
#define RN_CTL_FLOATS 3      // = RNNOISE_AMD_CTL_FLOATS: floor, thr, hold
#define RN_CTL_NONE 65536    // counter of a stream with no voice frame yet
#define RN_RS_TAPS 48                           // taps per phase of the up filter; the down filter has RN_RS_TAPS * L
#define RN_RS_UP_HIST (RN_RS_TAPS - 1)          // 47 low-rate samples
#define RN_RS_DOWN_HIST(L) ((RN_RS_TAPS - 1) * (L))  // N - L 48 kHz samples
#define RN_RS_DOWN0 48
#define RN_RS_HIST (RN_RS_DOWN0 + RN_RS_DOWN_HIST(6) + 6)  // 336 floats (1,344 B) per stream
#define RN_RATE_32K 32                          // = RNNOISE_AMD_RATE_32K: the code of 32 kHz where the other rates have their divisor
#define RN_RATE_32K_SAMPLES 320                 // its frame: the longest below 48 kHz
#define RN_RS_DOWN_TAPS_32K 72                  // taps per phase of its down filter (rs_coeffs.h: rn_rs_hd32), and what they reach back
#define RN_RS_DOWN_HIST_32K (RN_RS_DOWN_TAPS_32K - 2)
#define RN_RS_XS (RN_RS_UP_HIST + RN_RATE_32K_SAMPLES)      // LDS floats of one staged low-rate row: history + frame, at most 367
// samples per frame at the rate of code L (1, 2, 3, 6 or RN_RATE_32K): the one place that knows 320 is no 480 / L.  Selects, no
// division: the kernels call it with a run-time L
static inline
#ifdef __HIPCC__
__host__ __device__
#endif
int rn_rate_samples(int L) {
  return L == RN_RATE_32K ? RN_RATE_32K_SAMPLES : L == 2 ? RN_FRAME_SIZE / 2 : L == 3 ? RN_FRAME_SIZE / 3 : L == 6 ? RN_FRAME_SIZE / 6 : RN_FRAME_SIZE;
}

// Row list of the one-frame API (dropin.cpp: the combiner behind rnnoise_process_frame).  Concurrent rnnoise_process_frame calls on
// states of one pool are gathered into ONE launch group: block b of the latency kernels (rn_hp_one_kernel,
// rn_analysis_rows_kernel, rn_nn_one_kernel, rn_synthesis_few_kernel) then works on pool row RN_ROW_OF(e[b]) at that row's own
// frame phase -- ring slot RN_ROW_RING(e[b]), spectra slot RN_ROW_SPEC(e[b]) -- and exchanges the frame through the row's block
// of the pool's pinned host memory: io + row * RN_ROW_IO = in[480] | pad[4] | out[480] | vad | pad[2] | done (RN_ROW_IN ...), where
// the last kernel of the group stores the request's sequence number RN_ROW_SEQ(e[b]) into `done` once frame and VAD are out.  n == 0:
// no list -- block b is stream b of the group and the launch's own arguments apply (every batched call).  Passed by value: the list
// rides in the kernel arguments, so a group costs no copy and no extra memory round trip.
// A list has at most RN_ROWS_MAX entries; a pool has up to RN_POOL_ROWS_MAX rows (round 5: 1024 instead of 64, so that a thousand
// states share ONE combiner and its three streams instead of opening a pool -- and three streams -- per 64).
#define RN_ROWS_MAX 64
#define RN_POOL_ROWS_MAX 1024
#define RN_ROW_ENTRY(row, ring, spec, seq) ((uint32_t)(row) | (uint32_t)(ring) << 10 | (uint32_t)(spec) << 13 | (uint32_t)(seq) << 16)
#define RN_ROW_OF(e) ((int)((e) & 1023u))
#define RN_ROW_RING(e) ((int)(((e) >> 10) & 7u))
#define RN_ROW_SPEC(e) ((int)(((e) >> 13) & 3u))
#define RN_ROW_SEQ(e) ((e) >> 16)
#define RN_ROW_IO 968                          // floats of a row's block
#define RN_ROW_IN 0                            // the frame in
#define RN_ROW_OUT (RN_FRAME_SIZE + 4)         // the frame out (16-byte aligned)
#define RN_ROW_VAD (2 * RN_FRAME_SIZE + 4)     // its VAD probability
#define RN_ROW_DONE (RN_ROW_IO - 1)            // the sequence number of the last request whose frame and VAD are out
struct RnRows {
  float *io;
  int n;
  uint32_t e[RN_ROWS_MAX];
};

// The record step of the feature calls (include/rnnoise_amd.h: rnnoise_batch_process_features_device, rnnoise_batch_eval_records_device;
// batch_eval.cpp), the second mode of rn_train_features_kernel: one launch between the network of step t and the network of step
// t + 1, one wave per stream s.  It scores what the network of step t wrote -- gains[s][32], vad[s] -- against the record whose row
// s is target + s * row_stride (record t - 1: the reference network looks one frame ahead) into sums[s], and stages the row
// stage + s * row_stride (the features of step t + 1) into g.features[s] with its three pad floats zero and g.silence[s] = 0.
// target null: nothing is scored (and gains, vad, sums are not read); stage null: nothing is staged (the call's last launch).
// Rows are read float by float: any 4-byte aligned pointer and stride.
#define RN_EVAL_SUMS 4  // = RNNOISE_AMD_EVAL_SUMS: doubles per stream {sum of gain terms, sum of vad terms, frames scored, 0}
// Two further modes of the same launch serve the split calls (include/rnnoise_amd.h: rnnoise_batch_analyze_device,
// rnnoise_batch_synthesize_device; batch_split.cpp), one wave per stream s, lane = element, single-float accesses:
//   RN_STEP_EXPORT  behind K1 of a frame, on K1's stream: the 65 features K1 left in g.features[s] go to feat + s * feat_stride, its
//                   silence word g.silence[s] to sil_keep[s] (the pending frame's, which K3 will read) and to sil_out[s] (the
//                   caller's, or null)
//   RN_STEP_IMPORT  in front of K3 of a pending frame: gains + s * gains_stride (32 floats) and vad[s * vad_stride] go to g.gains[s]
//                   and g.vad[s] -- the batch's scratch, where K3 looks for them -- as they are; where sil[s] != 0 the caller's rows
//                   are not read and zeros go there, which is what the network writes on a silent frame
// A fourth mode scores predictions of the caller's (include/rnnoise_amd.h: rnnoise_batch_score_records_device; batch_eval.cpp):
//   RN_STEP_SCORE   the scoring of the record step with the network taken out, ONE launch for a whole call: one wave per row s walks
//                   its n frames in order -- frame f's record at rec + f * rec_frame_stride + s * rec_row_stride, its predictions
//                   at gains + f * gain_frame_stride + s * gain_row_stride and vad + f * vad_frame_stride + s * vad_row_stride -- with
//                   the record step's own terms and additions (eval_frame_terms), the three sums and the band's sum in registers
//                   between frames, the next frame's floats requested before the current frame's f64 calls.  No batch state is read.
enum { RN_STEP_EVAL = 1, RN_STEP_EXPORT = 2, RN_STEP_IMPORT = 3, RN_STEP_SCORE = 4 };
struct RnScoreStep {
  const float *rec;        // the record of the first scored step, row 0 (features[65] | gain targets[32] | vad target)
  long long rec_frame_stride, rec_row_stride;
  const float *gains;      // the gains of the first scored step, row 0
  long long gain_frame_stride, gain_row_stride;
  const float *vad;        // its vad
  long long vad_frame_stride, vad_row_stride;
  double *sums;            // [rows][RN_EVAL_SUMS], added to
  double *band_sums;       // [rows][32], added to, or null
  double gamma;            // the perceptual exponent of the gain term
  int n;                   // scored steps, > 0
};
struct RnSplitStep {
  float *feat;             // export: the caller's feature rows of this frame
  long long feat_stride;
  int *sil_keep, *sil_out; // export: [N] each; sil_out may be null
  const int *sil;          // import: [N] the pending frame's silence words
  const float *gains;      // import: the caller's gain rows of this frame
  long long gains_stride;
  const float *vad;        // import: the caller's vad row of this frame
  long long vad_stride;
};
struct RnEvalStep {
  int on;                  // 0: the extraction launch -- nothing below is read; RN_STEP_EVAL: the fields below; RN_STEP_EXPORT /
                           // RN_STEP_IMPORT: RnTrainArgs::split alone; RN_STEP_SCORE: RnTrainArgs::score alone
  const float *stage;      // features of the next step, or null
  const float *target;     // record to score against (features[65] | gain targets[32] | vad target), or null
  long long row_stride;    // floats between the rows of two streams, in `stage` and in `target`
  const float *gains;      // [N][32] the network's output of this step
  const float *vad;        // [N]
  double *sums;            // [N][RN_EVAL_SUMS], added to
  double gamma;            // the perceptual exponent of the gain term
  const struct RnScoreStep *score;  // HOST side only, on = RN_STEP_SCORE: what rn_launch_eval_step copies into RnTrainArgs::score (the
  int score_rows;                   // kernel sees null) and the rows it launches -- shim.h: rn_launch_score_rows
};

// per-step arguments of the training-feature extraction kernel (src/dump_features.c:466-491)
struct RnTrainArgs {
  const float *clean;      // [N][480] clean target frames (already filtered/scaled by the caller's mixer)
  float *clean_mem;        // [N][480] analysis memory of the clean stream (the `st` state of dump_features)
  const float *vad;        // [N] VAD targets, passed through to the record
  const int *lowpass;      // [N] first zeroed bin (denoise.c:340-343); 481 = none
  const int *band_lp;      // [N] bands above this get target -1 (dump_features.c:475); 32 = none
  const int *noise_free;   // [N] noise_gain==0 && fgnoise_gain==0 (dump_features.c:477)
  float *rec;              // [N][98] out: features[65] | gain targets[32] | vad
  RnEvalStep step;         // step.on: the launch is a record step of the feature calls instead, and nothing above is read
  RnSplitStep split;       // ... or a staging step of the split calls (step.on = RN_STEP_EXPORT / RN_STEP_IMPORT)
  RnScoreStep score;       // ... or the scoring of a whole call on predictions of the caller's (step.on = RN_STEP_SCORE)
};

// bits(rcpps(x)) for a positive normal x with bits b, from the 16-bit table entry v = rcp16[(b >> 11) & 0xfff]:
//   (v << 11) + 0x3f000000 - ((b & 0x7f800000) - 0x3f800000)
#define RN_RCP_K 0x7e800000u
#ifdef __HIPCC__
__device__ __forceinline__ float rn_rcp_x86(float x, const uint16_t *lut16) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t v = lut16[(b >> 11) & 0xfff];
  return __uint_as_float((v << 11) + (RN_RCP_K - (b & 0x7f800000u)));
}
// The 5 FIR taps of rnn_pitch_downsample from the 5 raw autocorrelation lags (src/pitch.c:176-199: lag window, order-4
// Levinson of src/celt_lpc.c:38-89, bandwidth expansion, the c1 = .8 zero): one body for the high-pass kernels, which
// compute the lags lane- or wave-per-stream, and for the one-row analysis workgroup, which computes them on a spare wave.
__device__ __forceinline__ void rn_fir_taps_from_ac(float (&ac)[5], float (&o)[5]) {
  ac[0] *= 1.0001f;
#pragma unroll
  for (int i = 1; i <= 4; i++) ac[i] -= ac[i] * (.008f * i) * (.008f * i);
  float lpc[4] = {0, 0, 0, 0};
  if (ac[0] != 0) {
    float error = ac[0];
    bool done = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (!done) {
        float rr = 0;
#pragma unroll
        for (int j = 0; j < i; j++) rr += lpc[j] * ac[i - j];
        rr += ac[i + 1];
        const float r = -rr / error;
        lpc[i] = r;
#pragma unroll
        for (int j = 0; j < (i + 1) >> 1; j++) {
          const float t1 = lpc[j], t2 = lpc[i - 1 - j];
          lpc[j] = t1 + r * t2;
          lpc[i - 1 - j] = t2 + r * t1;
        }
        error = error - (r * r) * error;
        if (error < .001f * ac[0]) done = true;  // `break` (celt_lpc.c:81-82)
      }
    }
  }
  float tmp = 1.f;
  const float c1 = .8f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    tmp = .9f * tmp;
    lpc[i] = lpc[i] * tmp;
  }
  o[0] = lpc[0] + .8f;
  o[1] = lpc[1] + c1 * lpc[0];
  o[2] = lpc[2] + c1 * lpc[1];
  o[3] = lpc[3] + c1 * lpc[2];
  o[4] = c1 * lpc[3];
}
// Frame phase of stream s (caller row i: column i of the mask) at frame g.call_frame of a call in per-stream mode (g.phase set;
// rn_dev.h: RnGroupDev) and whether the stream has that frame.  At most call_frame + 1 byte loads, down the row's column of the mask.
__device__ __forceinline__ int rn_stream_phase(const RnGroupDev &g, int s, int i, bool &present) {
  typedef __attribute__((address_space(1))) const uint8_t gu8;
  int p = *(__attribute__((address_space(1))) const int *)(g.phase + s);
  present = true;
  if (g.active) {
    gu8 *a = (gu8 *)(g.active + i);
    const size_t stride = g.list ? g.list_n : g.n_stride;
    for (int f = 0; f < g.call_frame; f++) p += a[(size_t)f * stride] != 0;
    present = a[(size_t)g.call_frame * stride] != 0;
  } else {
    p += g.call_frame;
  }
  return p;
}
// PCM-rate code of stream s in a launch with resampling on (g.rs_L != 0; rn_dev.h: RnGroupDev::rs_Ls): a byte of the table that is a
// code and whose frame fits the batch's row (g.rs_pitch), else the batch's.  s is the workgroup's one stream: the result is wave-uniform
__device__ __forceinline__ int rn_stream_L(const RnGroupDev &g, int s) {
  if (!g.rs_Ls) return g.rs_L;
  const int v = __builtin_amdgcn_readfirstlane((int)*(__attribute__((address_space(1))) const uint8_t *)(g.rs_Ls + s));
  return ((v == 1 || v == 2 || v == 3 || v == 6 || v == RN_RATE_32K) && rn_rate_samples(v) <= g.rs_pitch) ? v : g.rs_L;
}
// Samples between the caller's PCM rows (rn_dev.h: RnGroupDev::pcm_pitch): the layout's, or `own` -- the form's constant -- without one
__device__ __forceinline__ size_t rn_pcm_pitch(const RnGroupDev &g, int own) { return (size_t)(g.pcm_pitch ? g.pcm_pitch : own); }
// The caller's PCM row `row` (rn_dev.h: RnGroupDev::pcm_pitch, ::pcm_chan): its sample i lies at  slot + c + i * step  samples of the
// call's type, a companded row's byte i at byte  slot * sizeof(short) + c + i * step.  Without channels: c = 0, step = 1, slot =
// row * pitch -- what the kernels computed before there were channels.  row is wave-uniform (RnStreamAt::i), and so is the result
struct RnPcmRow {
  size_t slot;
  int c, step;
};
__device__ __forceinline__ RnPcmRow rn_pcm_row(const RnGroupDev &g, int row, int own) {
  if (!g.pcm_chan) return {(size_t)row * rn_pcm_pitch(g, own), 0, 1};
  const unsigned grp = (unsigned)row / (unsigned)g.pcm_chan;
  return {(size_t)grp * rn_pcm_pitch(g, own * g.pcm_chan), (int)((unsigned)row - grp * (unsigned)g.pcm_chan), g.pcm_chan};
}
// PCM format of stream s's rows in an int16 call (rn_dev.h: RnGroupDev::pcm_fmt): RN_PCM_ULAW, RN_PCM_ALAW, or 0 for int16 rows -- no
// table, or a byte that names neither law.  s is the workgroup's one stream: the result is wave-uniform
__device__ __forceinline__ int rn_stream_fmt(const RnGroupDev &g, int s) {
  if (!g.pcm_fmt) return 0;
  const int v = __builtin_amdgcn_readfirstlane((int)*(__attribute__((address_space(1))) const uint8_t *)(g.pcm_fmt + s));
  return (v == RN_PCM_ULAW || v == RN_PCM_ALAW) ? v : 0;
}
// Whether the network launch of g.model_sel owns stream s (rn_dev.h: RnGroupDev::model_of); an entry naming no slot reads as slot 0
__device__ __forceinline__ bool rn_owns(const RnGroupDev &g, int s) {
  if (!g.model_of) return true;
  const int k = *(__attribute__((address_space(1))) const uint8_t *)(g.model_of + s);
  return (k < g.n_models ? k : 0) == g.model_sel;
}
// Stream of list row r of a list call (rn_dev.h: RnGroupDev::list), or stream 0 for an entry naming none: an address to load from,
// never to store to (the 16-stream tile kernels)
__device__ __forceinline__ int rn_list_stream_or0(const RnGroupDev &g, int r) {
  const int e = *(__attribute__((address_space(1))) const int *)(g.list + r);
  return (unsigned)e < (unsigned)g.n_stride ? e : 0;
}
// Which stream a workgroup-per-stream kernel works on, and at which frame phase -- resolved once at its top (rn_stream_at):
// from its row list entry (listed), from the stream's own phase (g.phase set), or from the launch's arguments (lock-step).
// Every field is wave-uniform.
struct RnStreamAt {
  int s;           // the stream's row in the group's arrays (-1: a list entry naming no stream -- present is false)
  int i;           // the caller's row: the row of its in / out / vad / gains / mask (= s except in a list call)
  int ring;        // pitch-ring slot of this frame
  int spec, prev;  // spectra slot of this frame, and the one before it (the reference's delayed_*)
  bool present;    // the stream has this frame (false only for a masked-out stream of a per-stream call)
  bool listed;     // block b works on row list entry e ...
  uint32_t e;
  float *io;       // ... and exchanges the frame through this block of pinned memory (rn_dev.h: RnRows)
};
// rows: the kernel's row list, or null for the kernels that have none; ring / spec / prev: the launch's lock-step arguments
__device__ __forceinline__ RnStreamAt rn_stream_at(const RnGroupDev &g, const RnRows *rows, int ring, int spec, int prev) {
  RnStreamAt a;
  a.listed = rows && rows->n > 0;
  a.present = true;
  if (a.listed) {
    a.e = rows->e[blockIdx.x];
    a.s = RN_ROW_OF(a.e);
    a.ring = RN_ROW_RING(a.e);
    a.spec = RN_ROW_SPEC(a.e);
    a.prev = (a.spec + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
    a.io = rows->io + (size_t)a.s * RN_ROW_IO;
    a.i = a.s;
    return a;
  }
  a.e = 0;
  a.io = nullptr;
  a.i = (int)blockIdx.x;
  a.s = a.i;
  a.ring = ring;
  a.spec = spec;
  a.prev = prev;
  if (g.list) {  // a list call (rn_dev.h: RnGroupDev::list): row i is stream list[i]
    a.s = __builtin_amdgcn_readfirstlane(*(__attribute__((address_space(1))) const int *)(g.list + a.i));
    if ((unsigned)a.s >= (unsigned)g.n_stride) {
      a.s = -1;
      a.present = false;
      return a;
    }
  }
  if (g.phase) {
    const int p = __builtin_amdgcn_readfirstlane(rn_stream_phase(g, a.s, a.i, a.present));  // (the workgroup's one stream: uniform)
    a.ring = p % RN_RING_SLOTS;
    a.spec = p % RN_SPEC_SLOTS;
    a.prev = (p + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
  }
  return a;
}
#endif
// Stream of member j of the link group that row `row` belongs to (rn_dev.h: RnGroupDev::link = k): row k * (row / k) + j of the launch
// -- the stream of that index, or that list entry's in a list call, range-checked as rn_stream_at checks its own.  -1: a list entry
// naming no stream.  row is wave-uniform (RnStreamAt::i) and so is the result.  Host code compiles it too (tests/csrc)
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int rn_link_stream(const RnGroupDev &g, int row, int k, int j) {
  const int r = (int)((unsigned)row / (unsigned)k * (unsigned)k) + j;
  if (!g.list) return r;
  const int e = g.list[r];
  return (unsigned)e < (unsigned)g.n_stride ? e : -1;
}
// rows a launch of g works on: one workgroup (or tile row) per stream, or per list entry in a list call
static inline int rn_launch_rows(const RnGroupDev *g) { return g->list ? g->list_n : g->n_streams; }
#ifdef __HIPCC__
#include <hip/hip_ext.h>
// Launch with optional start / stop events: they are bound to the dispatch packet itself (hipExtLaunchKernel), so
// timing a kernel or publishing its completion to another stream adds no packets to the queue.
#define RN_LAUNCH(kernel, grid, block, shmem, st, e0, e1, ...)                                          \
  do {                                                                                                  \
    if ((e0) || (e1)) hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, e0, e1, 0, __VA_ARGS__);              \
    else hipLaunchKernelGGL(kernel, grid, block, shmem, st, __VA_ARGS__);                                \
  } while (0)
#endif
