// batch_split.cpp -- the split calls (include/rnnoise_amd.h): the two DSP halves of the frame step as calls of their own,
// around a network that is the caller's.
//   analyze      K0 and K1 of n_frames frames, with the plan and the schedule of the whole step (batch.cpp: batch_process_device_impl,
//                which runs either half when its call names one), and behind every K1 an export step (rn_dev.h: RnSplitStep) that
//                copies the frame's 65 features and silence words out.  The frames stay PENDING: their spectra and silence words
//                wait in the batch's store (shim.h: RNNoiseBatch::split_store), the last frame's spectra in the batch's own slot.
//   synthesize   per pending frame an import step -- the caller's gains and vad into the scratch the network would have written,
//                zeros on a silent frame -- and K3, pointed at the frame's spectra and silence words.
// This file has the bookkeeping: the store, the pending count, the row layouts, and what is refused.
#include "shim.h"

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

int analyze(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence, const Half &h) {
  if (!b || !features || !h.in || h.n_frames < 0 || b->per_stream || b->split_pending) return -1;
  SplitCall sp;
  sp.analyze = true;
  sp.features = features;
  sp.silence = silence;
  if (!split_rows(feat_rows, RN_NB_FEATURES, b->n, h.n_frames, sp.feat_fs, sp.feat_rs)) return -1;
  if (h.n_frames == 0) return 0;
  ON_DEVICE(b->device);
  if (store_ready(b, h.n_frames)) return -1;
  b->split_parity = b->parity;
  // (the batch's slot of the last frame is the one frame 0 is synthesised against: batch.cpp keeps a copy)
  b->split_prev_kept = h.n_frames % RN_SPEC_SLOTS == 0;
  const ProcessCall c{.in = h.in, .n_frames = h.n_frames, .stream = h.stream, .s16 = h.s16, .split = &sp};
  if (h.host ? batch_process_staged(b, c) : batch_process_device_impl(b, c)) return -1;
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
  const ProcessCall c{.out = h.out, .n_frames = h.n_frames, .stream = h.stream, .s16 = h.s16, .split = &sp};
  if (h.host ? batch_process_staged(b, c) : batch_process_device_impl(b, c)) return -1;
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
