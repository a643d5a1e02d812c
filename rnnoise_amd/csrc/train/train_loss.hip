// train_loss.hip -- librnnoise_amd_train.so (include/rnnoise_amd_train.h): the trainer's loss with its gradient, two launches.
//
// The terms are not this file's: eval_frame_terms and eval_vad_term (../eval_terms.h) are the text dsp_kernels.hip compiles for the
// product's score calls, under the same flags, so a scored step's two doubles are that call's bit for bit.  What this file adds is the
// gradient -- from the pw and d the terms already hold, so no power is raised twice -- and the shape of the work: the score walk is
// one wave per row, because it keeps a row's sums in registers; a training step scores 128 x 1996 steps, so here a wave takes a step
// at a time out of a grid over (row, block of steps), parks the step's two doubles in the caller's workspace, and a second launch
// adds them up per row in step order.  No atomics, nothing waits on another workgroup, and the order of additions is the walk's.
//
// Everything outside the `#ifndef RN_TL_HOST` blocks is also what tests/csrc/train_loss_main.cpp compiles for the host (behind
// tests/csrc/train_loss_shim.h): there RN_TL_LANES is 64, a "wave" is a loop over the lanes, and the shim runs eval_frame_terms for
// the 64 lanes of a step with the wave's exchanges replayed.  On the device RN_TL_LANES is 1 and every such loop is one pass.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <cmath>
#include "rnnoise_amd_train.h"
#define WAVE 64
#define RN_NB_BANDS RNNOISE_AMD_TRAIN_BANDS
#ifndef RN_TL_HOST
#include <hip/hip_runtime.h>
#include <stdio.h>
#define RN_TL_LANES 1
#define RN_TL_FN __device__ __forceinline__
#endif
#include "../eval_terms.h"
#define RN_SIDE_LIB "rnnoise_amd_train"
#include "../side_host.h"

#define RN_TL_REC RNNOISE_AMD_TRAIN_RECORD
#define RN_TL_TARGETS (RN_TL_REC - RN_NB_BANDS - 1)  // the first gain target of a record
#define RN_TL_SUMS RNNOISE_AMD_TRAIN_SUMS
#define RN_TL_FB RNNOISE_AMD_TRAIN_FRAME_BLOCK

struct RnTlArgs {
  const float *rec, *gains, *vad;  // record 0 of row 0; the predictions of step t0 of row 0
  long long rec_fs, rec_rs, gain_fs, gain_rs, vad_fs, vad_rs;
  float *grad_gains, *grad_vad;  // both or neither
  double *terms;                 // [n_rows][n_frames][2]
  double *sums;                  // [n_rows][RN_TL_SUMS]
  double gamma, w_gain, w_vad;
  int n_rows, t0, n_frames;
  int f_first;  // the first scored step of the call, counted from t0: steps f_first .. n_frames - 1 are scored
};
// what one lane holds of one step: its band's target and prediction, the frame's VAD target and prediction
struct RnTlIn {
  float gt, v, p, q;
};

#ifndef RN_TL_HOST
static RN_TL_FN void rn_tl_terms(const RnTlIn (&in)[RN_TL_LANES], double gamma, int lane0, EvalTerms (&k)[RN_TL_LANES]) {
  k[0] = eval_frame_terms(in[0].gt, in[0].v, in[0].p, in[0].q, gamma, lane0);
}
#endif

// a lane's part of a scored step once the wave has its terms: lane 0 parks the two doubles, lanes 0 .. 31 write their band's
// gradient, lane 0 the VAD's
static RN_TL_FN void rn_tl_finish(const RnTlArgs &a, int row, int f, int lane, const RnTlIn &in, const EvalTerms &k) {
  const double v = (double)in.v;
  if (lane == 0) {
    double *const ft = a.terms + ((long long)row * a.n_frames + f) * 2;
    ft[0] = k.term;
    ft[1] = eval_vad_term(in.v, k);
  }
  if (!a.grad_gains) return;
  if (lane < RN_NB_BANDS) {
    const double gt = (double)in.gt, p = (double)in.p;
    const double m = gt + 1.0 > 1.0 ? 1.0 : gt + 1.0;
    double g = 0.0;  // p <= 0 (or a NaN): the header's rule
    if (p > 0.0) g = (a.w_gain * 2.0) * ((1.0 + 5.0 * v) * m) * k.d * a.gamma * k.pw / p;
    a.grad_gains[(long long)f * a.gain_fs + (long long)row * a.gain_rs + lane] = (float)g;
  }
  if (lane == 0) {
    const double q = (double)in.q;
    const double g = a.w_vad * fabs(2.0 * v - 1.0) * (-v / (.01 + q) + (1.0 - v) / (1.01 - q));
    a.grad_vad[(long long)f * a.vad_fs + (long long)row * a.vad_rs] = (float)g;
  }
}

// step f of a row by one wave; lane0: this thread's lane on the device, 0 on the host (which passes through all 64)
static RN_TL_FN void rn_tl_step(const RnTlArgs &a, int row, int f, int lane0) {
  if (f < a.f_first) {  // (wave-uniform) not scored: zeros where gradients are asked for, nothing else
    if (a.grad_gains)
      for (int l = 0; l < RN_TL_LANES; l++) {
        const int lane = lane0 + l;
        if (lane < RN_NB_BANDS) a.grad_gains[(long long)f * a.gain_fs + (long long)row * a.gain_rs + lane] = 0.f;
        if (lane == 0) a.grad_vad[(long long)f * a.vad_fs + (long long)row * a.vad_rs] = 0.f;
      }
    return;
  }
  // step t0 + f is scored against record t0 + f - 1 (f >= f_first: that is record 0 at the least)
  const float *const rec = a.rec + ((long long)a.t0 + f - 1) * a.rec_fs + (long long)row * a.rec_rs + RN_TL_TARGETS;
  const float *const pg = a.gains + (long long)f * a.gain_fs + (long long)row * a.gain_rs;
  const float *const pq = a.vad + (long long)f * a.vad_fs + (long long)row * a.vad_rs;
  RnTlIn in[RN_TL_LANES];
  for (int l = 0; l < RN_TL_LANES; l++) {
    const int band = (lane0 + l) & (RN_NB_BANDS - 1);
    in[l].gt = rec[band], in[l].v = rec[RN_NB_BANDS], in[l].p = pg[band], in[l].q = pq[0];
  }
  EvalTerms k[RN_TL_LANES];
  rn_tl_terms(in, a.gamma, lane0, k);
  for (int l = 0; l < RN_TL_LANES; l++) rn_tl_finish(a, row, f, lane0 + l, in[l], k[l]);
}

// a row's frame terms added to its sums in step order: the additions of the score walk
static RN_TL_FN void rn_tl_row_sums(const RnTlArgs &a, int row) {
  double *const sum = a.sums + (long long)row * RN_TL_SUMS;
  const double *ft = a.terms + ((long long)row * a.n_frames + a.f_first) * 2;
  double a0 = sum[0], a1 = sum[1], a2 = sum[2];
  for (int f = a.f_first; f < a.n_frames; f++, ft += 2) {
    a0 += ft[0];
    a1 += ft[1];
    a2 += 1.0;
  }
  sum[0] = a0, sum[1] = a1, sum[2] = a2;
}

namespace {
bool call_ok(const RNNoiseTrainLoss *c) {
  if (!c || !c->records || !c->gains || !c->vad) return false;
  if (c->n_rows < 1 || c->t0 < 0 || c->n_frames < 0 || c->first < 0) return false;
  const long long T = (long long)c->t0 + c->n_frames;
  if (T > INT_MAX) return false;
  if (!(c->gamma > 0.0) || !std::isfinite(c->gamma) || !std::isfinite(c->w_gain) || !std::isfinite(c->w_vad)) return false;
  if ((c->grad_gains == nullptr) != (c->grad_vad == nullptr)) return false;
  return slots_fit(c->rec_frame_stride, c->rec_row_stride, RN_TL_REC, c->n_rows, T - 1, 1) &&
         slots_fit(c->gain_frame_stride, c->gain_row_stride, RN_NB_BANDS, c->n_rows, c->n_frames, 1) &&
         slots_fit(c->vad_frame_stride, c->vad_row_stride, 1, c->n_rows, c->n_frames, 1);
}
}  // namespace

extern "C" int rnnoise_amd_train_loss_check(const RNNoiseTrainLoss *call) { return call_ok(call) ? 0 : -1; }

// The kernels' arguments for a call whose buffers lie where the call says (the device form; the host program of the tests).
// 1: run them, 0: no step in the call, -1: refused.
static int rn_tl_plan(const RNNoiseTrainLoss *call, double *sums, double *frame_terms, RnTlArgs &a) {
  if (!call_ok(call) || !sums || !frame_terms) return -1;
  const RNNoiseTrainLoss &c = *call;
  a = RnTlArgs{};
  if (c.n_frames == 0) return 0;
  a.rec = c.records, a.rec_fs = c.rec_frame_stride, a.rec_rs = c.rec_row_stride;
  a.gains = c.gains, a.gain_fs = c.gain_frame_stride, a.gain_rs = c.gain_row_stride;
  a.vad = c.vad, a.vad_fs = c.vad_frame_stride, a.vad_rs = c.vad_row_stride;
  a.grad_gains = c.grad_gains, a.grad_vad = c.grad_vad;
  a.terms = frame_terms, a.sums = sums;
  a.gamma = c.gamma, a.w_gain = c.w_gain, a.w_vad = c.w_vad;
  a.n_rows = c.n_rows, a.t0 = c.t0, a.n_frames = c.n_frames;
  const long long t_first = c.first > 1 ? c.first : 1, ff = t_first - c.t0;
  a.f_first = ff <= 0 ? 0 : ff >= c.n_frames ? c.n_frames : (int)ff;
  return 1;
}

#ifndef RN_TL_HOST
#define RN_TL_WAVES 4  // waves of a workgroup of the first launch: each takes every fourth step of the block
extern "C" __global__ __launch_bounds__(RN_TL_WAVES * WAVE) void rn_train_loss_kernel(RnTlArgs a) {
  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = (int)(threadIdx.x & (WAVE - 1));
  const long long f0 = (long long)blockIdx.x * RN_TL_FB;
  for (int row = (int)blockIdx.y; row < a.n_rows; row += (int)gridDim.y)
    for (int i = wave; i < RN_TL_FB && f0 + i < a.n_frames; i += RN_TL_WAVES) rn_tl_step(a, row, (int)(f0 + i), lane);
}

extern "C" __global__ __launch_bounds__(WAVE) void rn_train_loss_sums_kernel(RnTlArgs a) {
  const long long row = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (row < a.n_rows) rn_tl_row_sums(a, (int)row);
}

namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

int launch(const RnTlArgs &a, hipStream_t st) {
  const bool scored = a.f_first < a.n_frames;
  if (scored || a.grad_gains) {
    const unsigned blocks = (unsigned)(((long long)a.n_frames + RN_TL_FB - 1) / RN_TL_FB), rows = a.n_rows < 65535 ? a.n_rows : 65535;
    hipLaunchKernelGGL(rn_train_loss_kernel, dim3(blocks, rows), dim3(RN_TL_WAVES * WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  if (scored) {
    hipLaunchKernelGGL(rn_train_loss_sums_kernel, dim3((unsigned)(((long long)a.n_rows + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// floats from a base to the end of the last of n_rows x T slots of M floats
size_t extent(long long fs, long long rs, int M, int n_rows, long long T) {
  return T > 0 ? (size_t)(T - 1) * (size_t)fs + (size_t)(n_rows - 1) * (size_t)rs + M : 0;
}
}  // namespace

extern "C" int rnnoise_amd_train_loss_device(int device, double *d_sums, double *d_frame_terms, const RNNoiseTrainLoss *call,
                                             void *hip_stream) {
  RnTlArgs a;
  const int plan = rn_tl_plan(call, d_sums, d_frame_terms, a);
  if (plan <= 0) return plan;
  ON_DEVICE(device);
  return launch(a, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_amd_train_loss(int device, double *sums, double *frame_terms, const RNNoiseTrainLoss *call) {
  if (!call_ok(call) || !sums) return -1;
  const RNNoiseTrainLoss &c = *call;
  if (c.n_frames == 0) return 0;
  ON_DEVICE(device);
  const size_t R = c.n_rows, e_rec = extent(c.rec_frame_stride, c.rec_row_stride, RN_TL_REC, c.n_rows, (long long)c.t0 + c.n_frames - 1),
               e_g = extent(c.gain_frame_stride, c.gain_row_stride, RN_NB_BANDS, c.n_rows, c.n_frames),
               e_v = extent(c.vad_frame_stride, c.vad_row_stride, 1, c.n_rows, c.n_frames),
               n_terms = R * (size_t)c.n_frames * 2;
  DevBuf rec, g, v, gg, gv, dsums, dterms;
  HIP_OK(hipMalloc(&rec.p, (e_rec ? e_rec : 1) * 4));
  HIP_OK(hipMalloc(&g.p, e_g * 4));
  HIP_OK(hipMalloc(&v.p, e_v * 4));
  HIP_OK(hipMalloc(&dsums.p, R * RN_TL_SUMS * sizeof(double)));
  HIP_OK(hipMalloc(&dterms.p, n_terms * sizeof(double)));
  if (e_rec) HIP_OK(hipMemcpy(rec.p, c.records, e_rec * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(g.p, c.gains, e_g * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(v.p, c.vad, e_v * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dsums.p, sums, R * RN_TL_SUMS * sizeof(double), hipMemcpyHostToDevice));
  // (the untouched records of unscored steps and the gaps of padded gradient rows come back as they went up)
  if (frame_terms) HIP_OK(hipMemcpy(dterms.p, frame_terms, n_terms * sizeof(double), hipMemcpyHostToDevice));
  if (c.grad_gains) {
    HIP_OK(hipMalloc(&gg.p, e_g * 4));
    HIP_OK(hipMalloc(&gv.p, e_v * 4));
    HIP_OK(hipMemcpy(gg.p, c.grad_gains, e_g * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(gv.p, c.grad_vad, e_v * 4, hipMemcpyHostToDevice));
  }
  RNNoiseTrainLoss dc = c;
  dc.records = static_cast<const float *>(rec.p), dc.gains = static_cast<const float *>(g.p), dc.vad = static_cast<const float *>(v.p);
  dc.grad_gains = static_cast<float *>(gg.p), dc.grad_vad = static_cast<float *>(gv.p);
  RnTlArgs a;
  if (rn_tl_plan(&dc, static_cast<double *>(dsums.p), static_cast<double *>(dterms.p), a) != 1) return -1;
  if (launch(a, nullptr)) return -1;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(sums, dsums.p, R * RN_TL_SUMS * sizeof(double), hipMemcpyDeviceToHost));
  if (frame_terms) HIP_OK(hipMemcpy(frame_terms, dterms.p, n_terms * sizeof(double), hipMemcpyDeviceToHost));
  if (c.grad_gains) {
    HIP_OK(hipMemcpy(c.grad_gains, gg.p, e_g * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(c.grad_vad, gv.p, e_v * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}
#endif
