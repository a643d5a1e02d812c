// batch_split.cpp -- the split calls (include/rnnoise_amd.h): the two DSP halves of the frame step as calls of their own,
// around a network that is the caller's.
//   analyze      K0 and K1 of n_frames frames, with the plan, the groups, the PCM addressing and the schedule of the whole step (the
//                stages of batch_step.h, which batch_step.cpp: batch_process_device_impl drives too), and behind every K1 an export
//                step (rn_dev.h: RnSplitStep) that copies the frame's 65 features and silence words out.  The frames stay PENDING: their spectra and silence words
//                wait in the batch's store (shim.h: RNNoiseBatch::split_store), the last frame's spectra in the batch's own slot.
//   synthesize   per pending frame an import step -- the caller's gains and vad into the scratch the network would have written,
//                zeros on a silent frame -- and K3, pointed at the frame's spectra and silence words.
// This file has the two halves, their host-buffer forms, and the bookkeeping: the store, the pending count, the row layouts, and what
// is refused.
#include "batch_step.h"

namespace {
// the strides a call runs with: NULL or {0, 0} is [frame][n_streams][row_floats]
bool split_rows(const RNNoiseRows *r, int row_floats, int n_streams, int n_frames, long &fs, long &rs) {
  if (row_floats < 1 || n_streams < 1 || n_frames < 0) return false;
  fs = r ? r->frame_stride : 0;
  rs = r ? r->row_stride : 0;
  if (fs == 0 && rs == 0) {
    rs = row_floats;
    fs = (long)n_streams * row_floats;
    return true;
  }
  return rn_pcm_layout_fits(fs, rs, row_floats, n_streams, n_frames);
}

// room for max_frames pending frames; growing drains the device first (the old store may be in use by a call in flight)
int store_ready(RNNoiseBatch *b, int max_frames) {
  if (max_frames <= b->split_cap) return 0;
  if (b->split_store) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(b->split_store));
    b->split_store = nullptr;
    b->split_cap = 0;
  }
  HIP_OK(hipMalloc(&b->split_store, (size_t)max_frames * batch_split_entry_bytes(b->n)));
  b->split_cap = max_frames;
  return 0;
}

struct Half {
  void *out = nullptr;
  const void *in = nullptr;
  int n_frames = 0;
  bool s16 = false, host = false;
  void *stream = nullptr;
};

// The analysis half: K1 in frame order on the caller's stream, with its export step behind it, and K0 three frames ahead on the side
// stream where the call is pipelined.  c: the call's `in`, frames, stream and sample type
int analysis_half(RNNoiseBatch *b, const ProcessCall &c, const SplitCall &sp) {
  Step s;
  if (s.begin(b, c, {.side_k1 = false, .k0 = true, .k3 = false})) return -1;
  const int n_frames = c.n_frames;
  for (int f = 0; s.pipelined && f < 3 && f < n_frames; f++)
    if (s.highpass(f)) return -1;
  for (int f = 0; f < n_frames; f++) {
    if (!s.pipelined && s.highpass(f)) return -1;
    RnGroupDev g = s.frame_group(f);
    const int slot = (b->parity + f) % RN_SPEC_SLOTS;
    const SplitEntry e = batch_split_entry(b, f);
    if (f + 1 < n_frames) {  // a pending frame's spectra go to its entry of the store; the call's last to the batch's own slot
      g.spec_X[slot] = e.X, g.spec_P[slot] = e.P, g.spec_E[slot] = e.E;
    } else if (b->split_prev_kept) {
      // ... which, in a call of a multiple of RN_SPEC_SLOTS frames, still holds what synthesis of frame 0 reads as the delayed
      // spectra: they move to the store's last entry first, on K1's stream
      const size_t N = b->n;
      HIP_OK(hipMemcpyAsync(e.X, b->g.spec_X[slot], N * RN_SPEC_STRIDE * 4, hipMemcpyDeviceToDevice, s.sb));
      HIP_OK(hipMemcpyAsync(e.P, b->g.spec_P[slot], N * RN_SPEC_STRIDE * 4, hipMemcpyDeviceToDevice, s.sb));
      HIP_OK(hipMemcpyAsync(e.E, b->g.spec_E[slot], N * RN_SPEC_E_ROW * 4, hipMemcpyDeviceToDevice, s.sb));
    }
    if (s.analysis(f, g)) return -1;
    RnSplitStep x{};  // the frame's features and silence words out of the per-step scratch, behind K1 on K1's stream
    x.feat = sp.features + (size_t)f * sp.feat_fs;
    x.feat_stride = sp.feat_rs;
    x.sil_keep = e.silence;
    x.sil_out = sp.silence ? sp.silence + (size_t)f * b->n : nullptr;
    HIP_OK(rn_launch_split_step(&g, &b->tb, &x, RN_STEP_EXPORT, s.sb));
    if (s.pipelined && f + 3 < n_frames && s.highpass(f + 3)) return -1;  // (a timed pair counts its frames once, in the synthesis half)
  }
  return s.finish();  // (the frame counters move here: the synthesis half runs at the slots the frames were analysed at)
}

// The synthesis half: per pending frame an import step and K3, at the slots the frame was analysed at (the batch's have moved on).
// K3's copy of the group gets the frame's spectra and silence words in the place of the batch's slots (shim.h:
// RNNoiseBatch::split_store), and the caller's gains and vad -- zeros on a silent frame -- go into the scratch K3 reads, where the
// network would have left its own.  The analysis half has moved the frame counters.  c: the call's `out`, frames, stream and sample type
int synthesis_half(RNNoiseBatch *b, const ProcessCall &c, const SplitCall &sp) {
  Step s;
  if (s.begin(b, c, {.side_k1 = false, .k0 = false, .k3 = true})) return -1;
  const int n_frames = c.n_frames;
  for (int f = 0; f < n_frames; f++) {
    RnGroupDev g = s.frame_group(f);
    const int cur = (b->split_parity + f) % RN_SPEC_SLOTS, prev = (cur + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
    if (f + 1 < n_frames) {
      const SplitEntry e = batch_split_entry(b, f);
      g.spec_X[cur] = e.X, g.spec_P[cur] = e.P, g.spec_E[cur] = e.E;
    }
    if (f > 0 || b->split_prev_kept) {
      const SplitEntry e = batch_split_entry(b, f > 0 ? f - 1 : n_frames - 1);
      g.spec_X[prev] = e.X, g.spec_P[prev] = e.P, g.spec_E[prev] = e.E;
    }
    g.silence = batch_split_entry(b, f).silence;
    RnSplitStep x{};
    x.sil = g.silence;
    x.gains = sp.gains + (size_t)f * sp.gains_fs;
    x.gains_stride = sp.gains_rs;
    x.vad = sp.vad + (size_t)f * sp.vad_fs;
    x.vad_stride = sp.vad_rs;
    HIP_OK(rn_launch_split_step(&g, &b->tb, &x, RN_STEP_IMPORT, s.st));
    if (s.synthesis(f, g, cur, prev)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  return 0;
}

// The halves on host buffers (batch_step.cpp: batch_process_staged has the whole step's): the caller's rows are host memory too, under
// the caller's strides, and travel as [frame][stream][row] through the staging buffer -- which keeps the whole step's order of pieces
// (in, out, vad, gains, mask), so a half leaves the other half's pieces empty
int analysis_staged(RNNoiseBatch *b, const ProcessCall &c, const SplitCall &sp) {
  StagedCall s;
  if (staged_begin(s, b, c)) return -1;
  ON_DEVICE(b->device);
  DevScratch d;
  const size_t o_in = d.carve(s.pcm), o_mask = d.carve(s.fs), o_feat = d.carve(s.fs * RN_NB_FEATURES * 4), o_sil = d.carve(s.fs * 4);
  (void)o_mask;
  if (d.alloc()) return -1;
  SplitCall dsp;
  dsp.features = d.at<float>(o_feat), dsp.feat_fs = (long)s.rows * RN_NB_FEATURES, dsp.feat_rs = RN_NB_FEATURES;
  dsp.silence = d.at<int>(o_sil);
  if (s.pcm_copy(d.at<char>(o_in), c.in, true)) return -1;
  if (analysis_half(b, {.in = d.at<char>(o_in), .n_frames = c.n_frames, .s16 = c.s16, .packed = true}, dsp)) return -1;
  HIP_OK(hipDeviceSynchronize());
  // the features to the caller's rows, 65 floats each and nothing around them; the silence words as they lie
  std::vector<float> tight(s.fs * RN_NB_FEATURES);
  HIP_OK(hipMemcpy(tight.data(), dsp.features, s.fs * RN_NB_FEATURES * 4, hipMemcpyDeviceToHost));
  for (size_t f = 0; f < (size_t)c.n_frames; f++)
    for (size_t r = 0; r < s.rows; r++)
      memcpy(sp.features + f * sp.feat_fs + r * sp.feat_rs, &tight[(f * s.rows + r) * RN_NB_FEATURES], RN_NB_FEATURES * 4);
  if (sp.silence) HIP_OK(hipMemcpy(sp.silence, dsp.silence, s.fs * 4, hipMemcpyDeviceToHost));
  return 0;
}

int synthesis_staged(RNNoiseBatch *b, const ProcessCall &c, const SplitCall &sp) {
  StagedCall s;
  if (staged_begin(s, b, c)) return -1;
  ON_DEVICE(b->device);
  DevScratch d;
  const size_t o_out = d.carve(s.pcm), o_vad = d.carve(s.fs * 4), o_gains = d.carve(s.fs * RN_NB_BANDS * 4), o_mask = d.carve(s.fs);
  (void)o_mask;
  if (d.alloc()) return -1;
  SplitCall dsp;
  dsp.gains = d.at<float>(o_gains), dsp.gains_fs = (long)s.rows * RN_NB_BANDS, dsp.gains_rs = RN_NB_BANDS;
  dsp.vad = d.at<float>(o_vad), dsp.vad_fs = (long)s.rows, dsp.vad_rs = 1;
  // (rows of a silent frame go up with the others; the device does not read them)
  std::vector<float> tight(s.fs * RN_NB_BANDS);
  for (size_t f = 0; f < (size_t)c.n_frames; f++)
    for (size_t r = 0; r < s.rows; r++)
      memcpy(&tight[(f * s.rows + r) * RN_NB_BANDS], sp.gains + f * sp.gains_fs + r * sp.gains_rs, RN_NB_BANDS * 4);
  HIP_OK(hipMemcpy(d.at<char>(o_gains), tight.data(), s.fs * RN_NB_BANDS * 4, hipMemcpyHostToDevice));
  for (size_t f = 0; f < (size_t)c.n_frames; f++)
    for (size_t r = 0; r < s.rows; r++) tight[f * s.rows + r] = sp.vad[f * sp.vad_fs + r * sp.vad_rs];
  HIP_OK(hipMemcpy(d.at<char>(o_vad), tight.data(), s.fs * 4, hipMemcpyHostToDevice));
  if (s.out_up(d.at<char>(o_out), c)) return -1;
  if (synthesis_half(b, {.out = d.at<char>(o_out), .n_frames = c.n_frames, .s16 = c.s16, .packed = true}, dsp)) return -1;
  HIP_OK(hipDeviceSynchronize());
  return s.pcm_copy(c.out, d.at<char>(o_out), false);
}

int analyze(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence, const Half &h) {
  if (!b || !features || !h.in || h.n_frames < 0 || b->per_stream || b->split_pending) return -1;
  SplitCall sp;
  sp.features = features;
  sp.silence = silence;
  if (!split_rows(feat_rows, RN_NB_FEATURES, b->n, h.n_frames, sp.feat_fs, sp.feat_rs)) return -1;
  if (h.n_frames == 0) return 0;
  ON_DEVICE(b->device);
  if (store_ready(b, h.n_frames)) return -1;
  b->split_parity = b->parity;
  // (the batch's slot of the last frame is the one frame 0 is synthesised against: analysis_half keeps a copy)
  b->split_prev_kept = h.n_frames % RN_SPEC_SLOTS == 0;
  const ProcessCall c{.in = h.in, .n_frames = h.n_frames, .stream = h.stream, .s16 = h.s16};
  if (h.host ? analysis_staged(b, c, sp) : analysis_half(b, c, sp)) return -1;
  b->split_pending = h.n_frames;
  return 0;
}

int synthesize(RNNoiseBatch *b, const float *gains, const RNNoiseRows *gain_rows, const float *vad, const RNNoiseRows *vad_rows,
               const Half &h) {
  if (!b || !h.out || !gains || !vad || h.n_frames < 0 || b->per_stream || h.n_frames != b->split_pending) return -1;
  SplitCall sp;
  sp.gains = gains;
  sp.vad = vad;
  if (!split_rows(gain_rows, RN_NB_BANDS, b->n, h.n_frames, sp.gains_fs, sp.gains_rs) ||
      !split_rows(vad_rows, 1, b->n, h.n_frames, sp.vad_fs, sp.vad_rs))
    return -1;
  if (h.n_frames == 0) return 0;
  const ProcessCall c{.out = h.out, .n_frames = h.n_frames, .stream = h.stream, .s16 = h.s16};
  if (h.host ? synthesis_staged(b, c, sp) : synthesis_half(b, c, sp)) return -1;
  b->split_pending = 0;
  return 0;
}
}  // namespace

extern "C" long rnnoise_amd_split_frame_bytes(int n_streams) {
  return n_streams > 0 ? (long)batch_split_entry_bytes(n_streams) : -1;
}

extern "C" int rnnoise_amd_split_rows_check(const RNNoiseRows *r, int row_floats, int n_streams, int n_frames) {
  long fs, rs;
  return split_rows(r, row_floats, n_streams, n_frames, fs, rs) ? 1 : 0;
}

extern "C" int rnnoise_batch_split_reserve(RNNoiseBatch *b, int max_frames) {
  if (!b || max_frames < 0 || b->split_pending) return -1;
  ON_DEVICE(b->device);
  return store_ready(b, max_frames);
}

extern "C" int rnnoise_batch_split_pending(const RNNoiseBatch *b) { return b ? b->split_pending : -1; }

extern "C" int rnnoise_batch_analyze_device(RNNoiseBatch *b, float *d_features, const RNNoiseRows *feat_rows, int *d_silence,
                                            const float *d_in, int n_frames, void *hip_stream) {
  return analyze(b, d_features, feat_rows, d_silence, {.in = d_in, .n_frames = n_frames, .stream = hip_stream});
}
extern "C" int rnnoise_batch_analyze_device_s16(RNNoiseBatch *b, float *d_features, const RNNoiseRows *feat_rows, int *d_silence,
                                                const short *d_in, int n_frames, void *hip_stream) {
  return analyze(b, d_features, feat_rows, d_silence, {.in = d_in, .n_frames = n_frames, .s16 = true, .stream = hip_stream});
}
extern "C" int rnnoise_batch_analyze(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence, const float *in,
                                     int n_frames) {
  return analyze(b, features, feat_rows, silence, {.in = in, .n_frames = n_frames, .host = true});
}
extern "C" int rnnoise_batch_analyze_s16(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence, const short *in,
                                         int n_frames) {
  return analyze(b, features, feat_rows, silence, {.in = in, .n_frames = n_frames, .s16 = true, .host = true});
}

extern "C" int rnnoise_batch_synthesize_device(RNNoiseBatch *b, float *d_out, const float *d_gains, const RNNoiseRows *gain_rows,
                                               const float *d_vad, const RNNoiseRows *vad_rows, int n_frames, void *hip_stream) {
  return synthesize(b, d_gains, gain_rows, d_vad, vad_rows, {.out = d_out, .n_frames = n_frames, .stream = hip_stream});
}
extern "C" int rnnoise_batch_synthesize_device_s16(RNNoiseBatch *b, short *d_out, const float *d_gains, const RNNoiseRows *gain_rows,
                                                   const float *d_vad, const RNNoiseRows *vad_rows, int n_frames, void *hip_stream) {
  return synthesize(b, d_gains, gain_rows, d_vad, vad_rows, {.out = d_out, .n_frames = n_frames, .s16 = true, .stream = hip_stream});
}
extern "C" int rnnoise_batch_synthesize(RNNoiseBatch *b, float *out, const float *gains, const RNNoiseRows *gain_rows, const float *vad,
                                        const RNNoiseRows *vad_rows, int n_frames) {
  return synthesize(b, gains, gain_rows, vad, vad_rows, {.out = out, .n_frames = n_frames, .host = true});
}
extern "C" int rnnoise_batch_synthesize_s16(RNNoiseBatch *b, short *out, const float *gains, const RNNoiseRows *gain_rows,
                                            const float *vad, const RNNoiseRows *vad_rows, int n_frames) {
  return synthesize(b, gains, gain_rows, vad, vad_rows, {.out = out, .n_frames = n_frames, .s16 = true, .host = true});
}
