// gru_seq.hip -- librnnoise_amd_gru.so (include/rnnoise_amd_gru.h): the recurrence of a float GRU over a sequence, one launch per step.
//
// The cell is ../gru_cell.h's (the workgroup's shape, the order of every sum, the gate math): the forward kernel is the cell of a layer
// that is given its gi, the backward kernel the cell of a layer that neither takes nor leaves a dx.  This file has the argument blocks,
// the two kernels and the host loops.
//
// Forward: y[t-1] is read from the slot before -- another slot than the one written, so no hazard.  Backward: the result
// w_hh^T dgh + dh z goes to the OTHER dh buffer: every workgroup of a row tile reads all of dh while the others write their slices.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include "rnnoise_amd_gru.h"
#ifdef RN_GRU_HOST  // the host half alone as plain C++ (tests/csrc/gru_stack_main.cpp): no kernels, every launch handed to the test
#include "gru_stack_shim.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdio.h>
#include "../gru_cell.h"
#define RN_SIDE_LIB "rnnoise_amd_gru"
#include "../side_host.h"

static_assert(RNNOISE_AMD_GRU_TILE == RN_CELL_TILE, "the header's tile is the cell's");

struct RnGruStep {  // the forward step t
  const float *gi;    // slot (t, 0)
  const float *w_hh, *b_hh;
  const float *prev;  // y[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  float *y;           // slot (t, 0)
  float *saved;       // [n_rows][4H] of step t
  long long in_rs, prev_rs, y_rs;  // in_rs: the row stride of gi
  int n_rows, H;
};

struct RnGruGradStep {  // the backward step t
  const float *saved;   // [n_rows][4H] of step t
  const float *dy;      // slot (t, 0)
  const float *prev;    // y[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  const float *dh_in;   // [n_rows][H]: dh after step t + 1 (dhT at t = T - 1), or NULL: zeros
  const float *w_hh;
  float *dgi;           // slot (t, 0)
  float *dgh;           // [n_rows][3H] of step t
  float *dh_out;        // [n_rows][H]: never dh_in
  long long dy_rs, prev_rs, dgi_rs;
  int n_rows, H;
};

#ifndef RN_GRU_HOST
extern "C" __global__ __launch_bounds__(RN_CELL_WAVES * RN_CELL_WAVE) void rn_gru_step_kernel(RnGruStep a) {
  __shared__ RnCellFwdLds<false> lds;
  rn_cell_forward<false>(a, a.n_rows, a.H, (int)blockIdx.x * RN_CELL_TILE, lds);
}

extern "C" __global__ __launch_bounds__(RN_CELL_WAVES * RN_CELL_WAVE) void rn_gru_step_grad_kernel(RnGruGradStep a) {
  __shared__ RnCellBwdLds<false> lds;
  rn_cell_backward<false, false>(a, a.n_rows, a.H, (int)blockIdx.x * RN_CELL_TILE, lds);
}
#endif  // RN_GRU_HOST

namespace {
bool counts_ok(int n_rows, int n_frames, int hidden) {
  if (n_rows < 1 || n_rows > RNNOISE_AMD_GRU_MAX_ROWS || n_frames < 0) return false;
  if (hidden < RNNOISE_AMD_GRU_MIN_HIDDEN || hidden > RNNOISE_AMD_GRU_MAX_HIDDEN || hidden % RN_CELL_TILE) return false;
  return (__int128)n_frames * n_rows * 4 * hidden <= (__int128)LONG_MAX;
}

bool seq_ok(const RNNoiseGruSeq *c) {
  if (!c || !c->gi || !c->w_hh || !c->b_hh || !c->y) return false;
  if (!counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  if (!aligned16(c->gi) || !aligned16(c->w_hh) || !aligned16(c->y) || !aligned16(c->h0) || !aligned4(c->b_hh)) return false;
  return slots_fit(c->gi_frame_stride, c->gi_row_stride, 3L * c->hidden, c->n_rows, c->n_frames, 4) &&
         slots_fit(c->y_frame_stride, c->y_row_stride, c->hidden, c->n_rows, c->n_frames, 4);
}

bool grad_ok(const RNNoiseGruSeqGrad *c) {
  if (!c || !c->dy || !c->y || !c->w_hh || !c->dgi || !c->dgh || !c->dh0) return false;
  if (!counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  if (!aligned16(c->dy) || !aligned16(c->y) || !aligned16(c->w_hh) || !aligned16(c->h0) || !aligned16(c->dhT) || !aligned16(c->dgi) ||
      !aligned16(c->dgh) || !aligned16(c->dh0))
    return false;
  if (c->dhT && !buffers_apart(c->dhT, c->dh0, (uintptr_t)c->n_rows * c->hidden * sizeof(float))) return false;  // both [N][H]
  return slots_fit(c->dy_frame_stride, c->dy_row_stride, c->hidden, c->n_rows, c->n_frames, 4) &&
         slots_fit(c->y_frame_stride, c->y_row_stride, c->hidden, c->n_rows, c->n_frames, 4) &&
         slots_fit(c->dgi_frame_stride, c->dgi_row_stride, 3L * c->hidden, c->n_rows, c->n_frames, 4);
}

dim3 grid_of(int n_rows, int hidden) { return dim3((unsigned)(hidden / RN_CELL_TILE), (unsigned)((n_rows + RN_CELL_TILE - 1) / RN_CELL_TILE)); }
}  // namespace

extern "C" int rnnoise_amd_gru_check(const RNNoiseGruSeq *call) { return seq_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_grad_check(const RNNoiseGruSeqGrad *call) { return grad_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_workspace(const RNNoiseGruSeq *call, size_t *saved_floats, size_t *scratch_floats) {
  if (!call || !counts_ok(call->n_rows, call->n_frames, call->hidden)) return -1;
  if (saved_floats) *saved_floats = (size_t)call->n_frames * (size_t)call->n_rows * 4 * (size_t)call->hidden;
  if (scratch_floats) *scratch_floats = 2 * (size_t)call->n_rows * (size_t)call->hidden;
  return 0;
}

extern "C" int rnnoise_amd_gru_forward_device(int device, const RNNoiseGruSeq *call, float *d_saved, void *hip_stream) {
  if (!seq_ok(call) || !d_saved || !aligned16(d_saved)) return -1;
  const RNNoiseGruSeq &c = *call;
  if (c.n_frames == 0) return 0;
  ON_DEVICE(device);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const dim3 grid = grid_of(c.n_rows, c.hidden);
  RnGruStep a{};
  a.w_hh = c.w_hh, a.b_hh = c.b_hh, a.in_rs = c.gi_row_stride, a.y_rs = c.y_row_stride, a.n_rows = c.n_rows, a.H = c.hidden;
  const long long slot = (long long)c.n_rows * 4 * c.hidden;
  for (int t = 0; t < c.n_frames; t++) {
    a.gi = c.gi + (long long)t * c.gi_frame_stride;
    a.y = c.y + (long long)t * c.y_frame_stride;
    a.saved = d_saved + t * slot;
    if (t == 0)
      a.prev = c.h0, a.prev_rs = c.hidden;
    else
      a.prev = c.y + (long long)(t - 1) * c.y_frame_stride, a.prev_rs = c.y_row_stride;
    hipLaunchKernelGGL(rn_gru_step_kernel, grid, dim3(RN_CELL_WAVES * RN_CELL_WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

extern "C" int rnnoise_amd_gru_backward_device(int device, const RNNoiseGruSeqGrad *call, const float *d_saved, float *d_scratch,
                                               void *hip_stream) {
  if (!grad_ok(call) || !d_saved || !d_scratch || !aligned16(d_saved) || !aligned16(d_scratch)) return -1;
  const RNNoiseGruSeqGrad &c = *call;
  if (c.n_frames == 0) return 0;
  ON_DEVICE(device);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const dim3 grid = grid_of(c.n_rows, c.hidden);
  RnGruGradStep a{};
  a.w_hh = c.w_hh, a.dy_rs = c.dy_row_stride, a.dgi_rs = c.dgi_row_stride, a.n_rows = c.n_rows, a.H = c.hidden;
  const long long slot = (long long)c.n_rows * c.hidden;
  float *const half[2] = {d_scratch, d_scratch + slot};
  const float *dh = c.dhT;
  int which = 0;
  for (int t = c.n_frames - 1; t >= 0; t--) {
    a.saved = d_saved + t * slot * 4;
    a.dy = c.dy + (long long)t * c.dy_frame_stride;
    a.dgi = c.dgi + (long long)t * c.dgi_frame_stride;
    a.dgh = c.dgh + t * slot * 3;
    if (t == 0)
      a.prev = c.h0, a.prev_rs = c.hidden;
    else
      a.prev = c.y + (long long)(t - 1) * c.y_frame_stride, a.prev_rs = c.y_row_stride;
    a.dh_in = dh;
    a.dh_out = t == 0 ? c.dh0 : half[which];  // the half the step before did not write; the last step writes dh0
    hipLaunchKernelGGL(rn_gru_step_grad_kernel, grid, dim3(RN_CELL_WAVES * RN_CELL_WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
    dh = a.dh_out;
    which ^= 1;
  }
  return 0;
}
