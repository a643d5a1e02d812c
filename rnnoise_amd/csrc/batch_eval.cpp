// batch_eval.cpp -- the feature calls (include/rnnoise_amd.h): the network alone on features that already exist
// (rnnoise_batch_process_features*), and the same walk over 98-float training records scored with the reference trainer's loss
// (rnnoise_batch_eval_records*).  A call is n_frames + 1 record steps (rn_dev.h: RnEvalStep, the second mode of
// rn_train_features_kernel) with the network of frame t between step t and step t + 1, everything on the caller's stream:
//   step 0          stages the features of frame t0
//   network t       reads the staged row and silence = 0, writes the frame's gains and VAD where the caller asked for them, or
//                   into the batch's scratch
//   step t + 1      scores them against record t - 1 into the stream's sums, stages the features of frame t + 1
// Only the network state moves: conv histories, GRU states, the layer images under img_valid.
#include "shim.h"

#include <limits.h>

#include <cmath>

namespace {
struct EvalConfig {
  double gamma;
  int first;
};
// the configuration a call runs with: NULL or a zeroed struct is the trainer's; anything else is taken as it stands
bool eval_config(const RNNoiseEvalConfig *cfg, EvalConfig &out) {
  out = {0.25, 4};
  if (!cfg || (cfg->gamma == 0.f && cfg->first == 0)) return true;
  if (!(cfg->gamma > 0.f) || !std::isfinite(cfg->gamma) || cfg->first < 0) return false;
  out = {(double)cfg->gamma, cfg->first};
  return true;
}
// the strides a call runs with: 0, 0 is [frame][n][row_floats]
void eval_strides(long &frame_stride, long &row_stride, int row_floats, int n_streams) {
  if (frame_stride == 0 && row_stride == 0) {
    row_stride = row_floats;
    frame_stride = (long)n_streams * row_floats;
  }
}
bool eval_layout_fits(long frame_stride, long row_stride, int row_floats, int n_streams, int t0, int n_frames) {
  if (row_floats < 1 || n_streams < 1 || t0 < 0 || n_frames < 0 || (long long)t0 + n_frames > INT_MAX) return false;
  if ((frame_stride == 0) != (row_stride == 0)) return false;
  eval_strides(frame_stride, row_stride, row_floats, n_streams);
  return rn_pcm_layout_fits(frame_stride, row_stride, row_floats, n_streams, t0 + n_frames);
}

struct EvalCall {
  float *gains = nullptr, *vad = nullptr;  // [n_frames][N][32], [n_frames][N], or null
  const float *rows = nullptr;             // frame t, stream s at t * frame_stride + s * row_stride
  long frame_stride = 0, row_stride = 0;
  int row_floats = RN_NB_FEATURES;
  int t0 = 0, n_frames = 0;
  double *sums = nullptr;                  // [N][RN_EVAL_SUMS]: the call scores (rows are records), or null
  const RNNoiseEvalConfig *cfg = nullptr;
  void *stream = nullptr;
};

// floats from `rows` to the end of the last slot the call may read (frames 0 .. t0 + n_frames - 1)
size_t eval_extent(const EvalCall &c, int n) {
  const size_t T = (size_t)c.t0 + c.n_frames;
  return T && n ? (T - 1) * (size_t)c.frame_stride + (size_t)(n - 1) * (size_t)c.row_stride + c.row_floats : 0;
}

int eval_device(RNNoiseBatch *b, EvalCall c) {
  if (!b || !c.rows) return -1;
  EvalConfig cfg;
  if (!eval_config(c.cfg, cfg) || !eval_layout_fits(c.frame_stride, c.row_stride, c.row_floats, b->n, c.t0, c.n_frames)) return -1;
  if (c.n_frames == 0) return 0;
  eval_strides(c.frame_stride, c.row_stride, c.row_floats, b->n);
  const hipStream_t st = static_cast<hipStream_t>(c.stream);
  ON_DEVICE(b->device);
  const size_t N = b->n;
  // the plan of a whole batch in a call that runs nothing beside the network (dispatch.h: rn_plan)
  const bool whole = b->g.n_streams == b->g.n_stride && N * RN_GRU * 4 < (1ull << 32);
  const RnStepShape shape{(int)N, whole, b->cus, b->nn_path, false, false, false};
  const RnPlan plan = rn_plan(rn_knobs(), shape);
  // the batch's group in lock-step form: no phase, mask or list, the first copy of the per-step scratch
  RnGroupDev g = b->g;
  g.features = b->features2[0];
  g.silence = b->silence2[0];
  g.pitch = b->pitch2[0];
  RnEvalStep step{};
  step.row_stride = c.row_stride;
  step.sums = c.sums;
  step.gamma = cfg.gamma;
  auto frame_rows = [&](long long t) { return c.rows + t * c.frame_stride; };
  for (int f = 0; f <= c.n_frames; f++) {
    // the step in front of network t0 + f: scores network t0 + f - 1 (whose outputs step.gains / step.vad still name), stages the next
    const long long t = (long long)c.t0 + f;
    step.stage = f < c.n_frames ? frame_rows(t) : nullptr;
    // record t - 2 belongs to step t - 1, which is scored from `first` on; step 0 has no record
    step.target = c.sums && f > 0 && t - 1 >= std::max(cfg.first, 1) ? frame_rows(t - 2) : nullptr;
    HIP_OK(rn_launch_eval_step(&g, &b->tb, &step, st));
    if (f == c.n_frames) break;
    g.gains = c.gains ? c.gains + (size_t)f * N * RN_NB_BANDS : b->scratch_gains;
    g.vad = c.vad ? c.vad + (size_t)f * N : b->scratch_vad;
    step.gains = g.gains;
    step.vad = g.vad;
    if (batch_network_step(b, g, plan, false, st)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  return 0;
}

// the host forms: the caller's rows go up as they lie (one copy of everything from `rows` to the last slot), the outputs come back
int eval_host(RNNoiseBatch *b, EvalCall c, double *sums) {
  if (!b || !c.rows || (c.row_floats == 98 && !sums)) return -1;
  EvalConfig cfg;
  if (!eval_config(c.cfg, cfg) || !eval_layout_fits(c.frame_stride, c.row_stride, c.row_floats, b->n, c.t0, c.n_frames)) return -1;
  if (c.n_frames == 0) return 0;
  eval_strides(c.frame_stride, c.row_stride, c.row_floats, b->n);
  ON_DEVICE(b->device);
  const size_t N = b->n, fs = (size_t)c.n_frames * N, ext = eval_extent(c, b->n);
  DevScratch d;
  const size_t o_rows = d.carve(ext * 4), o_gains = d.carve(fs * RN_NB_BANDS * 4), o_vad = d.carve(fs * 4),
               o_sums = d.carve(N * RN_EVAL_SUMS * sizeof(double));
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_rows), c.rows, ext * 4, hipMemcpyHostToDevice));
  if (sums) HIP_OK(hipMemcpy(d.at<char>(o_sums), sums, N * RN_EVAL_SUMS * sizeof(double), hipMemcpyHostToDevice));
  EvalCall dc = c;
  dc.rows = d.at<float>(o_rows);
  dc.gains = c.gains ? d.at<float>(o_gains) : nullptr;
  dc.vad = c.vad ? d.at<float>(o_vad) : nullptr;
  dc.sums = sums ? d.at<double>(o_sums) : nullptr;
  dc.stream = nullptr;
  if (eval_device(b, dc)) return -1;
  HIP_OK(hipDeviceSynchronize());
  if (c.gains) HIP_OK(hipMemcpy(c.gains, dc.gains, fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost));
  if (c.vad) HIP_OK(hipMemcpy(c.vad, dc.vad, fs * 4, hipMemcpyDeviceToHost));
  if (sums) HIP_OK(hipMemcpy(sums, dc.sums, N * RN_EVAL_SUMS * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- the score calls: the trainer's loss on predictions of the caller's (RN_STEP_SCORE, one launch) ----
struct ScoreCall {
  double *sums = nullptr, *band_sums = nullptr;  // [n_rows][RN_EVAL_SUMS], [n_rows][32] or null
  const float *gains = nullptr, *vad = nullptr;  // step t0 + f, row s at f * frame_stride + s * row_stride
  long gain_fs = 0, gain_rs = 0, vad_fs = 0, vad_rs = 0;
  const float *rec = nullptr;                    // record t, row s at t * rec_fs + s * rec_rs
  long rec_fs = 0, rec_rs = 0;
  int n_rows = 0, t0 = 0, n_frames = 0;
  const RNNoiseEvalConfig *cfg = nullptr;
  void *stream = nullptr;
};
bool score_layout_fits(const ScoreCall &c) {
  return eval_layout_fits(c.rec_fs, c.rec_rs, 98, c.n_rows, c.t0, c.n_frames) &&
         eval_layout_fits(c.gain_fs, c.gain_rs, RN_NB_BANDS, c.n_rows, 0, c.n_frames) &&
         eval_layout_fits(c.vad_fs, c.vad_rs, 1, c.n_rows, 0, c.n_frames);
}
void score_strides(ScoreCall &c) {
  eval_strides(c.rec_fs, c.rec_rs, 98, c.n_rows);
  eval_strides(c.gain_fs, c.gain_rs, RN_NB_BANDS, c.n_rows);
  eval_strides(c.vad_fs, c.vad_rs, 1, c.n_rows);
}
// the first scored step of a call, and how many follow it: step t against record t - 1 for t >= max(first, 1)
void score_range(const ScoreCall &c, const EvalConfig &cfg, long long &t_first, int &n) {
  t_first = std::max<long long>(c.t0, std::max(cfg.first, 1));
  const long long left = (long long)c.t0 + c.n_frames - t_first;
  n = left > 0 ? (int)left : 0;
}

int score_device(RNNoiseBatch *b, ScoreCall c) {
  if (!b || !c.rec || !c.gains || !c.vad || !c.sums) return -1;
  EvalConfig cfg;
  if (!eval_config(c.cfg, cfg) || !score_layout_fits(c)) return -1;
  score_strides(c);
  long long t_first;
  int n;
  score_range(c, cfg, t_first, n);
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  RnScoreStep x{};
  x.rec = c.rec + (t_first - 1) * c.rec_fs, x.rec_frame_stride = c.rec_fs, x.rec_row_stride = c.rec_rs;
  x.gains = c.gains + (t_first - c.t0) * c.gain_fs, x.gain_frame_stride = c.gain_fs, x.gain_row_stride = c.gain_rs;
  x.vad = c.vad + (t_first - c.t0) * c.vad_fs, x.vad_frame_stride = c.vad_fs, x.vad_row_stride = c.vad_rs;
  x.sums = c.sums, x.band_sums = c.band_sums, x.gamma = cfg.gamma, x.n = n;
  // (the batch names the device; its group and tables ride along as the kernel's arguments and are not read in this mode)
  HIP_OK(rn_launch_score_rows(&b->g, &b->tb, &x, c.n_rows, static_cast<hipStream_t>(c.stream)));
  return 0;
}

// floats from a base to the end of the last of n_rows x T slots
size_t score_extent(long fs, long rs, int row_floats, int n_rows, long long T) {
  return T > 0 ? (size_t)(T - 1) * (size_t)fs + (size_t)(n_rows - 1) * (size_t)rs + row_floats : 0;
}

int score_host(RNNoiseBatch *b, ScoreCall c) {
  if (!b || !c.rec || !c.gains || !c.vad || !c.sums) return -1;
  EvalConfig cfg;
  if (!eval_config(c.cfg, cfg) || !score_layout_fits(c)) return -1;
  score_strides(c);
  long long t_first;
  int n;
  score_range(c, cfg, t_first, n);
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  // records 0 .. t0 + n_frames - 2 (the last step's record is the last one read), the predictions of the call's n_frames steps
  const size_t R = c.n_rows, e_rec = score_extent(c.rec_fs, c.rec_rs, 98, c.n_rows, (long long)c.t0 + c.n_frames - 1),
               e_g = score_extent(c.gain_fs, c.gain_rs, RN_NB_BANDS, c.n_rows, c.n_frames),
               e_v = score_extent(c.vad_fs, c.vad_rs, 1, c.n_rows, c.n_frames);
  DevScratch d;
  const size_t o_rec = d.carve(e_rec * 4), o_g = d.carve(e_g * 4), o_v = d.carve(e_v * 4),
               o_sums = d.carve(R * RN_EVAL_SUMS * sizeof(double)), o_band = d.carve(R * RN_NB_BANDS * sizeof(double));
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_rec), c.rec, e_rec * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_g), c.gains, e_g * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_v), c.vad, e_v * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_sums), c.sums, R * RN_EVAL_SUMS * sizeof(double), hipMemcpyHostToDevice));
  if (c.band_sums) HIP_OK(hipMemcpy(d.at<char>(o_band), c.band_sums, R * RN_NB_BANDS * sizeof(double), hipMemcpyHostToDevice));
  ScoreCall dc = c;
  dc.rec = d.at<float>(o_rec), dc.gains = d.at<float>(o_g), dc.vad = d.at<float>(o_v);
  dc.sums = d.at<double>(o_sums), dc.band_sums = c.band_sums ? d.at<double>(o_band) : nullptr;
  dc.stream = nullptr;
  if (score_device(b, dc)) return -1;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(c.sums, dc.sums, R * RN_EVAL_SUMS * sizeof(double), hipMemcpyDeviceToHost));
  if (c.band_sums) HIP_OK(hipMemcpy(c.band_sums, dc.band_sums, R * RN_NB_BANDS * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

extern "C" int rnnoise_amd_score_records_check(const RNNoiseEvalConfig *cfg, long rec_frame_stride, long rec_row_stride,
                                               long gain_frame_stride, long gain_row_stride, long vad_frame_stride,
                                               long vad_row_stride, int n_rows, int t0, int n_frames) {
  EvalConfig e;
  ScoreCall c;
  c.rec_fs = rec_frame_stride, c.rec_rs = rec_row_stride, c.gain_fs = gain_frame_stride, c.gain_rs = gain_row_stride;
  c.vad_fs = vad_frame_stride, c.vad_rs = vad_row_stride, c.n_rows = n_rows, c.t0 = t0, c.n_frames = n_frames;
  return eval_config(cfg, e) && score_layout_fits(c) ? 1 : 0;
}

extern "C" int rnnoise_batch_score_records_device(RNNoiseBatch *b, double *d_sums, double *d_band_sums, const float *d_gains,
                                                  long gain_frame_stride, long gain_row_stride, const float *d_vad,
                                                  long vad_frame_stride, long vad_row_stride, const float *d_records,
                                                  long rec_frame_stride, long rec_row_stride, int n_rows, int t0, int n_frames,
                                                  const RNNoiseEvalConfig *cfg, void *hip_stream) {
  ScoreCall c;
  c.sums = d_sums, c.band_sums = d_band_sums, c.gains = d_gains, c.gain_fs = gain_frame_stride, c.gain_rs = gain_row_stride;
  c.vad = d_vad, c.vad_fs = vad_frame_stride, c.vad_rs = vad_row_stride, c.rec = d_records, c.rec_fs = rec_frame_stride;
  c.rec_rs = rec_row_stride, c.n_rows = n_rows, c.t0 = t0, c.n_frames = n_frames, c.cfg = cfg, c.stream = hip_stream;
  return score_device(b, c);
}

extern "C" int rnnoise_batch_score_records(RNNoiseBatch *b, double *sums, double *band_sums, const float *gains,
                                           long gain_frame_stride, long gain_row_stride, const float *vad, long vad_frame_stride,
                                           long vad_row_stride, const float *records, long rec_frame_stride, long rec_row_stride,
                                           int n_rows, int t0, int n_frames, const RNNoiseEvalConfig *cfg) {
  ScoreCall c;
  c.sums = sums, c.band_sums = band_sums, c.gains = gains, c.gain_fs = gain_frame_stride, c.gain_rs = gain_row_stride;
  c.vad = vad, c.vad_fs = vad_frame_stride, c.vad_rs = vad_row_stride, c.rec = records, c.rec_fs = rec_frame_stride;
  c.rec_rs = rec_row_stride, c.n_rows = n_rows, c.t0 = t0, c.n_frames = n_frames, c.cfg = cfg;
  return score_host(b, c);
}

extern "C" int rnnoise_amd_eval_records_check(const RNNoiseEvalConfig *cfg, long frame_stride, long row_stride, int row_floats,
                                              int n_streams, int t0, int n_frames) {
  EvalConfig e;
  return eval_config(cfg, e) && eval_layout_fits(frame_stride, row_stride, row_floats, n_streams, t0, n_frames) ? 1 : 0;
}

extern "C" int rnnoise_batch_process_features_device(RNNoiseBatch *b, float *d_gains, float *d_vad, const float *d_features,
                                                     long frame_stride, long row_stride, int n_frames, void *hip_stream) {
  EvalCall c;
  c.gains = d_gains, c.vad = d_vad, c.rows = d_features, c.frame_stride = frame_stride, c.row_stride = row_stride;
  c.n_frames = n_frames, c.stream = hip_stream;
  return eval_device(b, c);
}

extern "C" int rnnoise_batch_process_features(RNNoiseBatch *b, float *gains, float *vad, const float *features, long frame_stride,
                                              long row_stride, int n_frames) {
  EvalCall c;
  c.gains = gains, c.vad = vad, c.rows = features, c.frame_stride = frame_stride, c.row_stride = row_stride, c.n_frames = n_frames;
  return eval_host(b, c, nullptr);
}

extern "C" int rnnoise_batch_eval_records_device(RNNoiseBatch *b, double *d_sums, float *d_gains, float *d_vad, const float *d_records,
                                                 long frame_stride, long row_stride, int t0, int n_frames,
                                                 const RNNoiseEvalConfig *cfg, void *hip_stream) {
  if (!d_sums) return -1;
  EvalCall c;
  c.gains = d_gains, c.vad = d_vad, c.rows = d_records, c.frame_stride = frame_stride, c.row_stride = row_stride, c.row_floats = 98;
  c.t0 = t0, c.n_frames = n_frames, c.sums = d_sums, c.cfg = cfg, c.stream = hip_stream;
  return eval_device(b, c);
}

extern "C" int rnnoise_batch_eval_records(RNNoiseBatch *b, double *sums, float *gains, float *vad, const float *records,
                                          long frame_stride, long row_stride, int t0, int n_frames, const RNNoiseEvalConfig *cfg) {
  EvalCall c;
  c.gains = gains, c.vad = vad, c.rows = records, c.frame_stride = frame_stride, c.row_stride = row_stride, c.row_floats = 98;
  c.t0 = t0, c.n_frames = n_frames, c.cfg = cfg;
  return eval_host(b, c, sums);
}
