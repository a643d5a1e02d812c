// audio_score.hip -- librnnoise_amd_score.so (include/rnnoise_amd_score.h): three PCM planes in, eight double sums per row out.
//
// The interface fixes the order of every addition (the header's ORDER), so the kernel has no freedom in its arithmetic; what it
// chooses is how the bytes arrive.  One wave per row.  A frame is 120 float4 granules; lane l owns granules l and l + 64, so one
// global_load_dwordx4 per plane reads 1 KiB of a frame and a second one its last 896 bytes (lanes 56..63 read their first granule again).  ref / in are read
// at the output index minus the delay: with delay % 4 == 0 a granule stays one aligned float4 (frames are 480 = 4 * 120 samples, strides
// multiples of 4), else it is four dword loads -- same values into the same registers, so the sums do not know the difference.  The loads
// of frame t + 1 are issued before frame t is reduced.  The 64 lanes combine with the wave's own exchange (__shfl_xor: ds_bpermute, no
// LDS memory); the row's totals stay in registers from the first frame to the last.
//
// Everything outside the `#ifndef RN_AS_HOST` blocks is also what tests/csrc/audio_score_main.cpp compiles for the host (with -DRN_AS_HOST,
// behind tests/csrc/audio_score_shim.h): there RN_AS_LANES is 64, a "wave" is a loop over the lanes, and the exchange works on the
// array of their accumulators.  On the device RN_AS_LANES is 1 and every such loop is one pass.
#include <limits.h>
#include <stddef.h>
#include "rnnoise_amd_score.h"
#ifndef RN_AS_HOST
#include <hip/hip_runtime.h>
#include <stdio.h>
#define RN_AS_LANES 1
#define RN_AS_FN __device__ __forceinline__
// nothing is scheduled across this point: the loads in front of it are issued before the arithmetic behind it starts
#define RN_AS_ISSUED() __builtin_amdgcn_sched_barrier(0)
// acc = acc + acc[lane ^ m], all eight slots
static RN_AS_FN void rn_as_exchange(double (&acc)[RN_AS_LANES][RNNOISE_AMD_SCORE_SLOTS], int m) {
#pragma unroll
  for (int k = 0; k < RNNOISE_AMD_SCORE_SLOTS; k++) acc[0][k] = acc[0][k] + __shfl_xor(acc[0][k], m, 64);
}
#endif

#define RN_SIDE_LIB "rnnoise_amd_score"
#include "../side_host.h"

#define RN_AS_FRAME RNNOISE_AMD_SCORE_FRAME
#define RN_AS_SLOTS RNNOISE_AMD_SCORE_SLOTS
#define RN_AS_WAVE 64
#define RN_AS_FULL_LANES 56  // lanes with a second granule: 120 granules = 64 + 56

struct alignas(16) RnAsGranule {
  float v[4];
};
// what one lane holds of one frame: its two granules of each plane
struct RnAsFrame {
  RnAsGranule y[2], r[2], x[2];
};
struct RnAsArgs {
  const float *ref, *in, *out;  // each at frame f0 of row 0
  long long ref_fs, ref_rs, in_fs, in_rs, out_fs, out_rs;
  double *sums;    // [n_rows][8]
  double *terms;   // or null: row s, frame t at terms + s * terms_rs + (t - terms_t0) * 8
  long long terms_rs;
  int terms_t0;
  int f0;          // the frame the plane pointers stand at (0 in the device form; the first staged frame in the host form)
  int n_rows;
  int t_first, n;  // the scored frames: t_first .. t_first + n - 1
  int dq, dr;      // delay = dq * 480 + dr, 0 <= dr < 480
};

// samples i .. i + 3 of output frame t, delayed: ref / in sample (t * 480 + i + e) - delay lies in frame t - dq, or the one before.
// ALIGNED (delay % 4 == 0): the granule is one aligned float4 of one frame
template <bool ALIGNED>
static RN_AS_FN void rn_as_load_delayed(const RnAsArgs &a, const float *p, long long fs, long long rs, int row, int t, int i, RnAsGranule &g) {
  if (ALIGNED) {
    int j = i - a.dr, tt = t - a.dq;
    if (j < 0) j += RN_AS_FRAME, tt -= 1;
    g = *reinterpret_cast<const RnAsGranule *>(p + (long long)(tt - a.f0) * fs + (long long)row * rs + j);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; e++) {
    int j = i + e - a.dr, tt = t - a.dq;
    if (j < 0) j += RN_AS_FRAME, tt -= 1;
    g.v[e] = p[(long long)(tt - a.f0) * fs + (long long)row * rs + j];
  }
}

// Lanes 56..63 have no second granule: they read their first one again (a cache hit, never used), so that the loads of a frame are
// the same straight-line sequence in every lane and the wait in front of the arithmetic can count them.
template <bool ALIGNED>
static RN_AS_FN void rn_as_load(const RnAsArgs &a, int row, int t, int lane, RnAsFrame &f) {
#pragma unroll
  for (int g = 0; g < 2; g++) {
    const int i = 4 * lane + (g == 1 && lane < RN_AS_FULL_LANES ? 4 * RN_AS_WAVE : 0);
    f.y[g] = *reinterpret_cast<const RnAsGranule *>(a.out + (long long)(t - a.f0) * a.out_fs + (long long)row * a.out_rs + i);
    rn_as_load_delayed<ALIGNED>(a, a.ref, a.ref_fs, a.ref_rs, row, t, i, f.r[g]);
    rn_as_load_delayed<ALIGNED>(a, a.in, a.in_fs, a.in_rs, row, t, i, f.x[g]);
  }
}

// one lane's share of a frame record: its samples in ascending i, every accumulator from 0.0, one rounding per operation
// (-ffp-contract=off: no multiply is fused into an add)
static RN_AS_FN void rn_as_terms(const RnAsFrame &f, int lane, double (&acc)[RN_AS_SLOTS]) {
#pragma unroll
  for (int k = 0; k < RN_AS_SLOTS; k++) acc[k] = 0.0;
#pragma unroll
  for (int g = 0; g < 2; g++) {
    if (g == 1 && lane >= RN_AS_FULL_LANES) break;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const double r = (double)f.r[g].v[e], x = (double)f.x[g].v[e], y = (double)f.y[g].v[e];
      const double xr = x - r, yr = y - r;
      acc[0] = acc[0] + r * r;
      acc[1] = acc[1] + x * x;
      acc[2] = acc[2] + y * y;
      acc[3] = acc[3] + x * r;
      acc[4] = acc[4] + y * r;
      acc[5] = acc[5] + xr * xr;
      acc[6] = acc[6] + yr * yr;
      acc[7] = acc[7] + 1.0;
    }
  }
}

// frame t of a row, as the lanes hold it in cur: the frame record, added to the totals and, where asked for, written out
static RN_AS_FN void rn_as_frame(const RnAsArgs &a, int row, int t, int lane0, const RnAsFrame (&cur)[RN_AS_LANES], double (&total)[RN_AS_SLOTS]) {
  double acc[RN_AS_LANES][RN_AS_SLOTS];
  for (int l = 0; l < RN_AS_LANES; l++) rn_as_terms(cur[l], lane0 + l, acc[l]);
#pragma unroll
  for (int m = RN_AS_WAVE / 2; m >= 1; m >>= 1) rn_as_exchange(acc, m);
#pragma unroll
  for (int k = 0; k < RN_AS_SLOTS; k++) total[k] = total[k] + acc[0][k];
  if (a.terms && lane0 == 0) {
    double *const rec = a.terms + (long long)row * a.terms_rs + (long long)(t - a.terms_t0) * RN_AS_SLOTS;
#pragma unroll
    for (int k = 0; k < RN_AS_SLOTS; k++) rec[k] = acc[0][k];
  }
}

// the walk of one row by one wave; lane0: this thread's lane on the device, 0 on the host (which passes through all 64).  The last
// frame stands outside the loop so that inside it the loads of frame t + 1 are unconditional: the wait in front of frame t's
// arithmetic then leaves exactly those in flight.
template <bool ALIGNED>
static RN_AS_FN void rn_as_row(const RnAsArgs &a, int row, int lane0) {
  RnAsFrame cur[RN_AS_LANES], nxt[RN_AS_LANES];
  double total[RN_AS_SLOTS];
  double *const sums = a.sums + (long long)row * RN_AS_SLOTS;
#pragma unroll
  for (int k = 0; k < RN_AS_SLOTS; k++) total[k] = sums[k];
  for (int l = 0; l < RN_AS_LANES; l++) rn_as_load<ALIGNED>(a, row, a.t_first, lane0 + l, cur[l]);
  const int t_last = a.t_first + a.n - 1;
  for (int t = a.t_first; t < t_last; t++) {
    for (int l = 0; l < RN_AS_LANES; l++) rn_as_load<ALIGNED>(a, row, t + 1, lane0 + l, nxt[l]);
    RN_AS_ISSUED();
    rn_as_frame(a, row, t, lane0, cur, total);
    for (int l = 0; l < RN_AS_LANES; l++) cur[l] = nxt[l];
  }
  rn_as_frame(a, row, t_last, lane0, cur, total);
  if (lane0 == 0) {
#pragma unroll
    for (int k = 0; k < RN_AS_SLOTS; k++) sums[k] = total[k];
  }
}

static RN_AS_FN void rn_as_wave(const RnAsArgs &a, int row, int lane0) {
  if ((a.dr & 3) == 0)  // (the same for every wave of a launch)
    rn_as_row<true>(a, row, lane0);
  else
    rn_as_row<false>(a, row, lane0);
}

namespace {
// last float of a plane that a call over frames [0, T) of n_rows rows may name, or false where that is beyond LONG_MAX
bool plane_ok(const RNNoiseAudioPlane &p, int n_rows, long long T) {
  if (!p.p || !aligned16(p.p)) return false;
  if (p.frame_stride < RN_AS_FRAME || p.row_stride < RN_AS_FRAME || (p.frame_stride & 3) || (p.row_stride & 3)) return false;
  const __int128 end = (__int128)(T > 0 ? T - 1 : 0) * p.frame_stride + (__int128)(n_rows - 1) * p.row_stride + RN_AS_FRAME;
  return end <= (__int128)LONG_MAX;
}

bool call_ok(const RNNoiseAudioScore *c) {
  if (!c || c->n_rows < 1 || c->t0 < 0 || c->n_frames < 0 || c->first < 0 || c->delay < 0) return false;
  const long long T = (long long)c->t0 + c->n_frames;
  if (T > INT_MAX || (long long)c->first * RN_AS_FRAME < c->delay) return false;
  return plane_ok(c->ref, c->n_rows, T) && plane_ok(c->in, c->n_rows, T) && plane_ok(c->out, c->n_rows, T);
}

// the scored frames of a call: false when there is none
bool scored_range(const RNNoiseAudioScore &c, int &t_first, int &n) {
  t_first = c.t0 > c.first ? c.t0 : c.first;
  const long long left = (long long)c.t0 + c.n_frames - t_first;
  n = left > 0 ? (int)left : 0;
  return n > 0;
}
}  // namespace

extern "C" int rnnoise_amd_audio_score_check(const RNNoiseAudioScore *call) { return call_ok(call) ? 0 : -1; }

static void rn_as_set_delay(RnAsArgs &a, int delay) { a.dq = delay / RN_AS_FRAME, a.dr = delay % RN_AS_FRAME; }

// The kernel's arguments for a call whose planes, sums and records lie where the call says (the device form; the host program of the
// tests).  1: run them, 0: no frame to score, -1: refused.
static int rn_as_plan(const RNNoiseAudioScore *call, double *sums, double *frame_terms, RnAsArgs &a) {
  if (!call_ok(call) || !sums) return -1;
  const RNNoiseAudioScore &c = *call;
  if (frame_terms && c.terms_frames < (long long)c.t0 + c.n_frames) return -1;
  a = RnAsArgs{};
  if (!scored_range(c, a.t_first, a.n)) return 0;
  a.ref = c.ref.p, a.ref_fs = c.ref.frame_stride, a.ref_rs = c.ref.row_stride;
  a.in = c.in.p, a.in_fs = c.in.frame_stride, a.in_rs = c.in.row_stride;
  a.out = c.out.p, a.out_fs = c.out.frame_stride, a.out_rs = c.out.row_stride;
  a.sums = sums, a.terms = frame_terms, a.terms_rs = (long long)c.terms_frames * RN_AS_SLOTS, a.terms_t0 = 0, a.f0 = 0;
  a.n_rows = c.n_rows;
  rn_as_set_delay(a, c.delay);
  return 1;
}

#ifndef RN_AS_HOST
#define RN_AS_WAVES 4  // rows of a workgroup
extern "C" __global__ __launch_bounds__(RN_AS_WAVES * RN_AS_WAVE) void rn_audio_score_kernel(RnAsArgs a) {
  const int row = (int)blockIdx.x * RN_AS_WAVES + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  rn_as_wave(a, row, threadIdx.x & (RN_AS_WAVE - 1));
}

namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

int launch(const RnAsArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(rn_audio_score_kernel, dim3((unsigned)((a.n_rows + RN_AS_WAVES - 1) / RN_AS_WAVES)), dim3(RN_AS_WAVES * RN_AS_WAVE), 0, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rnnoise_amd_audio_score_device(int device, double *d_sums, double *d_frame_terms, const RNNoiseAudioScore *call,
                                              void *hip_stream) {
  RnAsArgs a;
  const int plan = rn_as_plan(call, d_sums, d_frame_terms, a);
  if (plan <= 0) return plan;
  ON_DEVICE(device);
  return launch(a, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_amd_audio_score(int device, double *sums, double *frame_terms, const RNNoiseAudioScore *call) {
  if (!call_ok(call) || !sums) return -1;
  const RNNoiseAudioScore &c = *call;
  if (frame_terms && c.terms_frames < (long long)c.t0 + c.n_frames) return -1;
  int t_first, n;
  if (!scored_range(c, t_first, n)) return 0;
  ON_DEVICE(device);
  // the frames the call reads: out t_first .., ref / in from the frame of sample t_first * 480 - delay; staged as [rows][Tn][480]
  const int tA = (int)(((long long)t_first * RN_AS_FRAME - c.delay) / RN_AS_FRAME), Tn = t_first + n - tA;
  const size_t row_floats = (size_t)Tn * RN_AS_FRAME, row_bytes = row_floats * sizeof(float);
  size_t R = ((size_t)48 << 20) / (3 * row_bytes);
  R = R < 1 ? 1 : R > (size_t)c.n_rows ? (size_t)c.n_rows : R;
  DevBuf pcm, dsums, dterms;
  HIP_OK(hipMalloc(&pcm.p, 3 * R * row_bytes));
  HIP_OK(hipMalloc(&dsums.p, R * RN_AS_SLOTS * sizeof(double)));
  if (frame_terms) HIP_OK(hipMalloc(&dterms.p, R * (size_t)n * RN_AS_SLOTS * sizeof(double)));
  float *const d_ref = static_cast<float *>(pcm.p), *const d_in = d_ref + R * row_floats, *const d_out = d_in + R * row_floats;
  RnAsArgs a{};
  a.ref = d_ref, a.in = d_in, a.out = d_out;
  a.ref_fs = a.in_fs = a.out_fs = RN_AS_FRAME, a.ref_rs = a.in_rs = a.out_rs = (long long)row_floats;
  a.sums = static_cast<double *>(dsums.p), a.terms = static_cast<double *>(dterms.p);
  a.terms_rs = (long long)n * RN_AS_SLOTS, a.terms_t0 = t_first, a.f0 = tA, a.t_first = t_first, a.n = n;
  rn_as_set_delay(a, c.delay);
  // frames [from, t_first + n) of `rows` rows of a host plane into their staged slots
  auto up = [&](float *dst, const RNNoiseAudioPlane &p, size_t r0, size_t rows, int from) -> int {
    for (size_t r = 0; r < rows; r++)
      HIP_OK(hipMemcpy2D(dst + r * row_floats + (size_t)(from - tA) * RN_AS_FRAME, RN_AS_FRAME * sizeof(float),
                         p.p + (long long)from * p.frame_stride + (long long)(r0 + r) * p.row_stride, (size_t)p.frame_stride * sizeof(float),
                         RN_AS_FRAME * sizeof(float), (size_t)(t_first + n - from), hipMemcpyHostToDevice));
    return 0;
  };
  for (size_t r0 = 0; r0 < (size_t)c.n_rows; r0 += R) {
    const size_t rows = (size_t)c.n_rows - r0 < R ? (size_t)c.n_rows - r0 : R;
    if (up(d_ref, c.ref, r0, rows, tA) || up(d_in, c.in, r0, rows, tA) || up(d_out, c.out, r0, rows, t_first)) return -1;
    HIP_OK(hipMemcpy(dsums.p, sums + r0 * RN_AS_SLOTS, rows * RN_AS_SLOTS * sizeof(double), hipMemcpyHostToDevice));
    a.n_rows = (int)rows;
    if (launch(a, nullptr)) return -1;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(sums + r0 * RN_AS_SLOTS, dsums.p, rows * RN_AS_SLOTS * sizeof(double), hipMemcpyDeviceToHost));
    if (frame_terms)  // a row's scored records are one run on both sides
      HIP_OK(hipMemcpy2D(frame_terms + (r0 * (size_t)c.terms_frames + (size_t)t_first) * RN_AS_SLOTS,
                         (size_t)c.terms_frames * RN_AS_SLOTS * sizeof(double), dterms.p, (size_t)n * RN_AS_SLOTS * sizeof(double),
                         (size_t)n * RN_AS_SLOTS * sizeof(double), rows, hipMemcpyDeviceToHost));
  }
  return 0;
}
#endif
