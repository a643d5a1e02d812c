// gru_stack.hip -- librnnoise_amd_gru_stack.so (include/rnnoise_amd_gru_stack.h): three chained float GRU layers over a sequence, one
// diagonal launch per step: layer l runs step s - l in launch s (backward: the mirror image), so a launch holds up to three layers.
//
// The cell is ../gru_cell.h's (the workgroup's shape, the order of every sum, the gate math).  A workgroup owns 16 hidden units x 16
// rows of ONE layer: blockIdx.x / (H/16) picks it among the layers that have a step in this launch, uniform per workgroup, and the
// kernels call the cell in the form that layer has.  Forward, layer 0 is given its gi; layers 1 and 2 project their own from
// y_{l-1}[t], written by the launch before.  Backward, layers 0 and 1 add the dx of the layer above to dy, and layers 1 and 2 leave a
// dx in the half the layer below reads one launch later.  This file has the argument blocks, the two kernels and the host loops.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include "rnnoise_amd_gru_stack.h"
#ifdef RN_STK_HOST  // the host half alone as plain C++ (tests/csrc/gru_stack_main.cpp): no kernels, every launch handed to the test
#include "gru_stack_shim.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdio.h>
#include "../gru_cell.h"
#define RN_SIDE_LIB "rnnoise_amd_gru_stack"
#include "../side_host.h"

#define RN_STK_LAYERS RNNOISE_AMD_GRU_STACK_LAYERS
static_assert(RNNOISE_AMD_GRU_STACK_TILE == RN_CELL_TILE, "the header's tile is the cell's");

struct RnStackLayerStep {  // one layer's forward step of a launch
  const float *gi;    // layer 0: gi0's slot (t, 0); NULL for the layers that project their own
  const float *x;     // layers 1, 2: y_{l-1}[t] of row 0
  const float *w_ih, *b_ih;
  const float *w_hh, *b_hh;
  const float *prev;  // y_l[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  float *y;           // slot (t, 0)
  float *saved;       // [n_rows][4H] of layer l, step t
  long long in_rs, prev_rs, y_rs;  // in_rs: the row stride of gi or of x
};

struct RnStackStep {
  RnStackLayerStep L[RN_STK_LAYERS];  // the layers of this launch, the first live one at [0]
  int n_rows, H, tiles;               // tiles: H / 16, the workgroups of a layer per row tile
};

struct RnStackLayerGrad {  // one layer's backward step of a launch
  const float *saved;   // [n_rows][4H] of layer l, step t
  const float *dy;      // slot (t, 0)
  const float *dx_in;   // [n_rows][H]: dx_{l+1}[t], written by the launch before; NULL for the top layer
  const float *prev;    // y_l[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  const float *dh_in;   // [n_rows][H]: dh after step t + 1 (dhT at t = T - 1), or NULL: zeros
  const float *w_hh;
  const float *w_ih;    // layers 1, 2; NULL for layer 0
  float *dgi;           // slot (t, 0)
  float *dgh;           // [n_rows][3H] of step t
  float *dh_out;        // [n_rows][H]: never dh_in
  float *dx_out;        // [n_rows][H]: dx_l[t], the half the layer below does not read in this launch; NULL for layer 0
  long long dy_rs, prev_rs, dgi_rs;
};

struct RnStackGradStep {
  RnStackLayerGrad L[RN_STK_LAYERS];
  int n_rows, H, tiles;
};

#ifndef RN_STK_HOST
extern "C" __global__ __launch_bounds__(RN_CELL_WAVES * RN_CELL_WAVE) void rn_gru_stack_kernel(RnStackStep a) {
  __shared__ RnCellFwdLds<true> lds;  // (layer 0 uses three of the four sets)
  const int li = (int)blockIdx.x / a.tiles;  // (uniform) which of the launch's layers
  const RnStackLayerStep &p = a.L[li];
  const int u0 = ((int)blockIdx.x - li * a.tiles) * RN_CELL_TILE;
  if (p.gi == nullptr)  // layers 1, 2
    rn_cell_forward<true>(p, a.n_rows, a.H, u0, lds);
  else
    rn_cell_forward<false>(p, a.n_rows, a.H, u0, reinterpret_cast<RnCellFwdLds<false> &>(lds));
}

extern "C" __global__ __launch_bounds__(RN_CELL_WAVES * RN_CELL_WAVE) void rn_gru_stack_grad_kernel(RnStackGradStep a) {
  __shared__ RnCellBwdLds<true> lds;  // (layer 0 uses one of the two sets)
  const int li = (int)blockIdx.x / a.tiles;  // (uniform) which of the launch's layers
  const RnStackLayerGrad &p = a.L[li];
  const int c0 = ((int)blockIdx.x - li * a.tiles) * RN_CELL_TILE;
  if (p.dx_out == nullptr)  // layer 0
    rn_cell_backward<true, false>(p, a.n_rows, a.H, c0, reinterpret_cast<RnCellBwdLds<false> &>(lds));
  else if (p.dx_in != nullptr)  // layer 1
    rn_cell_backward<true, true>(p, a.n_rows, a.H, c0, lds);
  else  // layer 2
    rn_cell_backward<false, true>(p, a.n_rows, a.H, c0, lds);
}
#endif  // RN_STK_HOST

namespace {
bool stack_counts_ok(int n_rows, int n_frames, int hidden) {
  if (n_rows < 1 || n_rows > RNNOISE_AMD_GRU_STACK_MAX_ROWS || n_frames < 0) return false;
  if (hidden < RNNOISE_AMD_GRU_STACK_MIN_HIDDEN || hidden > RNNOISE_AMD_GRU_STACK_MAX_HIDDEN || hidden % RN_CELL_TILE) return false;
  return (__int128)RN_STK_LAYERS * n_frames * n_rows * 4 * hidden <= (__int128)LONG_MAX;
}

bool stack_ok(const RNNoiseGruStack *c) {
  if (!c || !c->gi0 || !aligned16(c->gi0)) return false;
  if (!stack_counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++) {
    if (!c->w_hh[l] || !c->b_hh[l] || !c->y[l]) return false;
    if (!aligned16(c->w_hh[l]) || !aligned4(c->b_hh[l]) || !aligned16(c->y[l]) || !aligned16(c->h0[l])) return false;
    if (l > 0 && (!c->w_ih[l] || !c->b_ih[l] || !aligned16(c->w_ih[l]) || !aligned4(c->b_ih[l]))) return false;
    if (!slots_fit(c->y_frame_stride[l], c->y_row_stride[l], c->hidden, c->n_rows, c->n_frames, 4)) return false;
  }
  if (!slots_fit(c->gi0_frame_stride, c->gi0_row_stride, 3L * c->hidden, c->n_rows, c->n_frames, 4)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++)
    for (int k = l + 1; k < RN_STK_LAYERS; k++)
      if (!slots_apart(c->y[l], c->y_frame_stride[l], c->y_row_stride[l], c->y[k], c->y_frame_stride[k], c->y_row_stride[k], c->hidden,
                       c->n_rows, c->n_frames))
        return false;
  return true;
}

bool grad_ok(const RNNoiseGruStackGrad *c) {
  if (!c || !stack_counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++) {
    if (!c->dy[l] || !c->y[l] || !c->w_hh[l] || !c->dgi[l] || !c->dgh[l] || !c->dh0[l]) return false;
    if (!aligned16(c->dy[l]) || !aligned16(c->y[l]) || !aligned16(c->w_hh[l]) || !aligned16(c->h0[l]) || !aligned16(c->dhT[l]) ||
        !aligned16(c->dgi[l]) || !aligned16(c->dgh[l]) || !aligned16(c->dh0[l]))
      return false;
    if (l > 0 && (!c->w_ih[l] || !aligned16(c->w_ih[l]))) return false;
    if (c->dhT[l] && !buffers_apart(c->dhT[l], c->dh0[l], (uintptr_t)c->n_rows * c->hidden * sizeof(float))) return false;  // both [N][H]
    if (!slots_fit(c->dy_frame_stride[l], c->dy_row_stride[l], c->hidden, c->n_rows, c->n_frames, 4) ||
        !slots_fit(c->y_frame_stride[l], c->y_row_stride[l], c->hidden, c->n_rows, c->n_frames, 4))
      return false;
  }
  return slots_fit(c->dgi0_frame_stride, c->dgi0_row_stride, 3L * c->hidden, c->n_rows, c->n_frames, 4);
}

// the grid of a launch that holds `layers` layers
dim3 grid_of(int layers, int n_rows, int hidden) {
  return dim3((unsigned)(layers * (hidden / RN_CELL_TILE)), (unsigned)((n_rows + RN_CELL_TILE - 1) / RN_CELL_TILE));
}
}  // namespace

extern "C" int rnnoise_amd_gru_stack_check(const RNNoiseGruStack *call) { return stack_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_stack_grad_check(const RNNoiseGruStackGrad *call) { return grad_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_stack_workspace(const RNNoiseGruStack *call, size_t *saved_floats, size_t *scratch_floats) {
  if (!call || !stack_counts_ok(call->n_rows, call->n_frames, call->hidden)) return -1;
  if (saved_floats) *saved_floats = (size_t)RN_STK_LAYERS * (size_t)call->n_frames * (size_t)call->n_rows * 4 * (size_t)call->hidden;
  if (scratch_floats) *scratch_floats = (size_t)(RN_STK_LAYERS + RN_STK_LAYERS - 1) * 2 * (size_t)call->n_rows * (size_t)call->hidden;
  return 0;
}

extern "C" int rnnoise_amd_gru_stack_forward_device(int device, const RNNoiseGruStack *call, float *d_saved, void *hip_stream) {
  if (!stack_ok(call) || !d_saved || !aligned16(d_saved)) return -1;
  const RNNoiseGruStack &c = *call;
  if (c.n_frames == 0) return 0;
  ON_DEVICE(device);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int T = c.n_frames;
  const long long slot = (long long)c.n_rows * 4 * c.hidden;
  RnStackStep a{};
  a.n_rows = c.n_rows, a.H = c.hidden, a.tiles = c.hidden / RN_CELL_TILE;
  for (int s = 0; s < T + RN_STK_LAYERS - 1; s++) {
    // launch s: layer l at step s - l, for the layers lo .. hi that have one
    const int lo = s - (T - 1) > 0 ? s - (T - 1) : 0, hi = s < RN_STK_LAYERS - 1 ? s : RN_STK_LAYERS - 1;
    for (int l = lo; l <= hi; l++) {
      const int t = s - l;
      RnStackLayerStep &p = a.L[l - lo];
      p = RnStackLayerStep{};
      if (l == 0)
        p.gi = c.gi0 + (long long)t * c.gi0_frame_stride, p.in_rs = c.gi0_row_stride;
      else
        p.x = c.y[l - 1] + (long long)t * c.y_frame_stride[l - 1], p.in_rs = c.y_row_stride[l - 1], p.w_ih = c.w_ih[l], p.b_ih = c.b_ih[l];
      p.w_hh = c.w_hh[l], p.b_hh = c.b_hh[l];
      p.y = c.y[l] + (long long)t * c.y_frame_stride[l], p.y_rs = c.y_row_stride[l];
      p.saved = d_saved + ((long long)l * T + t) * slot;
      if (t == 0)
        p.prev = c.h0[l], p.prev_rs = c.hidden;
      else
        p.prev = c.y[l] + (long long)(t - 1) * c.y_frame_stride[l], p.prev_rs = c.y_row_stride[l];
    }
    hipLaunchKernelGGL(rn_gru_stack_kernel, grid_of(hi - lo + 1, c.n_rows, c.hidden), dim3(RN_CELL_WAVES * RN_CELL_WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

extern "C" int rnnoise_amd_gru_stack_backward_device(int device, const RNNoiseGruStackGrad *call, const float *d_saved, float *d_scratch,
                                                     void *hip_stream) {
  if (!grad_ok(call) || !d_saved || !d_scratch || !aligned16(d_saved) || !aligned16(d_scratch)) return -1;
  const RNNoiseGruStackGrad &c = *call;
  if (c.n_frames == 0) return 0;
  ON_DEVICE(device);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int T = c.n_frames, top = RN_STK_LAYERS - 1;
  const long long slot = (long long)c.n_rows * c.hidden;
  // the scratch: the dh pair of layer l at 2 l, the dx pair of layer l >= 1 at 2 (3 + l - 1)
  const float *dh[RN_STK_LAYERS];
  for (int l = 0; l < RN_STK_LAYERS; l++) dh[l] = c.dhT[l];
  RnStackGradStep a{};
  a.n_rows = c.n_rows, a.H = c.hidden, a.tiles = c.hidden / RN_CELL_TILE;
  for (int s = 0; s < T + RN_STK_LAYERS - 1; s++) {
    // launch s: layer l at step T - 1 - s + (2 - l), for the layers lo .. hi that have one
    const int lo = top - s > 0 ? top - s : 0, hi = T + 1 - s < top ? T + 1 - s : top;
    const int half = s & 1;  // what this launch writes of every pair; it reads the other one
    for (int l = lo; l <= hi; l++) {
      const int t = T - 1 - s + (top - l);
      RnStackLayerGrad &p = a.L[l - lo];
      p = RnStackLayerGrad{};
      p.saved = d_saved + ((long long)l * T + t) * slot * 4;
      p.dy = c.dy[l] + (long long)t * c.dy_frame_stride[l], p.dy_rs = c.dy_row_stride[l];
      if (l == 0)
        p.dgi = c.dgi[0] + (long long)t * c.dgi0_frame_stride, p.dgi_rs = c.dgi0_row_stride;
      else
        p.dgi = c.dgi[l] + t * slot * 3, p.dgi_rs = 3LL * c.hidden;
      p.dgh = c.dgh[l] + t * slot * 3;
      if (t == 0)
        p.prev = c.h0[l], p.prev_rs = c.hidden;
      else
        p.prev = c.y[l] + (long long)(t - 1) * c.y_frame_stride[l], p.prev_rs = c.y_row_stride[l];
      p.w_hh = c.w_hh[l], p.w_ih = l > 0 ? c.w_ih[l] : nullptr;
      p.dh_in = dh[l];
      p.dh_out = t == 0 ? c.dh0[l] : d_scratch + (2 * l + half) * slot;  // the last step writes dh0
      dh[l] = p.dh_out;
      p.dx_in = l < top ? d_scratch + (2 * (RN_STK_LAYERS + l) + (half ^ 1)) * slot : nullptr;  // layer l + 1's, of the launch before
      p.dx_out = l > 0 ? d_scratch + (2 * (RN_STK_LAYERS + l - 1) + half) * slot : nullptr;
    }
    hipLaunchKernelGGL(rn_gru_stack_grad_kernel, grid_of(hi - lo + 1, c.n_rows, c.hidden), dim3(RN_CELL_WAVES * RN_CELL_WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  return 0;
}
