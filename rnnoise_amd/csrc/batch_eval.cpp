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
}  // namespace

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
