// gru_stack.hip -- librnnoise_amd_gru_stack.so (include/rnnoise_amd_gru_stack.h): three chained float GRU layers over a sequence, one
// diagonal launch per step: layer l runs step s - l in launch s (backward: the mirror image), so a launch holds up to three layers.
//
// The workgroup is the gru library's.  Four waves own 16 hidden units x 16 rows of ONE layer (blockIdx.x / (H/16) picks it among the
// layers that have a step in this launch, uniform per workgroup); wave w takes the w-th quarter of every sum with
// v_mfma_f32_16x16x4_f32 (exact float32), A = weights, B = the rows' vectors, so a row is a column of B and of the result and never
// meets another row.  The quarters go through LDS and thread e of the 256 adds them up in wave order for unit e & 15 of row e >> 4,
// does the gate math and stores with ordinary vector-memory stores.  Where a quarter holds 16 k or more, lane group q = lane >> 4
// loads the four consecutive k 16 c' + 4 q .. + 3 as one 16-byte read and issue c of the chunk takes element c of every group; what
// is left of a quarter (H = 16, 48) goes one k per lane group and issue.
//
// Forward, layers 1 and 2: K = 2H -- w_hh over y_l[t-1] and w_ih over y_{l-1}[t], both written by the launch before; the reads of
// both halves of a block of chunks are issued together.  The r and z sums of the two halves meet per wave (P^hh_w + P^ih_w); the n
// gate keeps hn and gi_n as sums of their own.  Backward, layers 1 and 2 carry a second accumulator set: from the gate gradients a
// lane computes anyway, dx = w_ih^T dgi beside w_hh^T dgh, stored into the dx half the layer below reads one launch later.
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

#define WAVE 64
#define RN_STK_LAYERS RNNOISE_AMD_GRU_STACK_LAYERS
#define RN_STK_TILE RNNOISE_AMD_GRU_STACK_TILE
#define RN_STK_WAVES 4
#define RN_STK_PAD 68  // floats of a register's row of partial sums: 64 lanes + 4, so the transposed read of the last stage hits 64 banks

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
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

static __device__ __forceinline__ float rn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// Chunks of 16 k whose reads a wave issues together before the first of their matrix instructions (a step is short and every read is a
// trip to L2 or HBM).  Forward: 6 chunks of one half (layer 0; H = 384: the whole quarter) or 3 of both halves (24 reads of 16 bytes
// either way); backward: 3 for layer 0 as in the gru library, 2 where the second weight matrix is read too.
#define RN_STK_FWD_CH 6
#define RN_STK_FWD2_CH 3
#define RN_STK_BWD_CH 3
#define RN_STK_BWD2_CH 2

// what a lane of the forward step reads: the row's vector and the three gates' weight rows of unit u0 + (lane & 15), from the
// wave's first k on
struct RnStackFwdHalf {
  const float *pb, *pa0, *pa1, *pa2;
};

// CH chunks of the forward sums from k offset kk on: every read first (both halves), then the issues in k order, each half a chain of
// its own (the order does not depend on CH)
template <int CH, bool HH, bool IH>
static __device__ __forceinline__ void rn_stack_fwd_chunks(const RnStackFwdHalf &h, const RnStackFwdHalf &x, int kk, bool live,
                                                           f32x4 (&hh)[3], f32x4 (&ih)[3]) {
  f32x4 hb[CH], h0[CH], h1[CH], h2[CH], xb[CH], x0[CH], x1[CH], x2[CH];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int o = kk + 16 * i;
    if (HH) {
      hb[i] = *reinterpret_cast<const f32x4 *>(h.pb + o);
      h0[i] = *reinterpret_cast<const f32x4 *>(h.pa0 + o);
      h1[i] = *reinterpret_cast<const f32x4 *>(h.pa1 + o);
      h2[i] = *reinterpret_cast<const f32x4 *>(h.pa2 + o);
    }
    if (IH) {
      xb[i] = *reinterpret_cast<const f32x4 *>(x.pb + o);
      x0[i] = *reinterpret_cast<const f32x4 *>(x.pa0 + o);
      x1[i] = *reinterpret_cast<const f32x4 *>(x.pa1 + o);
      x2[i] = *reinterpret_cast<const f32x4 *>(x.pa2 + o);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the reads stay together above
#pragma unroll
  for (int i = 0; i < CH; i++) {
    if (!live) hb[i] = f32x4{0.f, 0.f, 0.f, 0.f}, xb[i] = f32x4{0.f, 0.f, 0.f, 0.f};  // rows beyond the last read as zeros (the read went to row 0)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (HH) {
        hh[0] = RN_MFMA(h0[i][c], hb[i][c], hh[0]);
        hh[1] = RN_MFMA(h1[i][c], hb[i][c], hh[1]);
        hh[2] = RN_MFMA(h2[i][c], hb[i][c], hh[2]);
      }
      if (IH) {
        ih[0] = RN_MFMA(x0[i][c], xb[i][c], ih[0]);
        ih[1] = RN_MFMA(x1[i][c], xb[i][c], ih[1]);
        ih[2] = RN_MFMA(x2[i][c], xb[i][c], ih[2]);
      }
    }
  }
}

// a wave's quarter of the forward sums: L k from the halves' first on
template <int CH, bool HH, bool IH>
static __device__ __forceinline__ void rn_stack_fwd_quarter(const RnStackFwdHalf &h, const RnStackFwdHalf &x, int L, int q, bool live,
                                                            f32x4 (&hh)[3], f32x4 (&ih)[3]) {
  int k = 0;
  for (; k + 16 * CH <= L; k += 16 * CH) rn_stack_fwd_chunks<CH, HH, IH>(h, x, k + 4 * q, live, hh, ih);
  for (; k + 16 <= L; k += 16) rn_stack_fwd_chunks<1, HH, IH>(h, x, k + 4 * q, live, hh, ih);
  for (; k < L; k += 4) {  // what is left of a quarter: one k per lane group and issue
    const int kk = k + q;
    if (HH) {
      const float b = live ? h.pb[kk] : 0.f;
      hh[0] = RN_MFMA(h.pa0[kk], b, hh[0]);
      hh[1] = RN_MFMA(h.pa1[kk], b, hh[1]);
      hh[2] = RN_MFMA(h.pa2[kk], b, hh[2]);
    }
    if (IH) {
      const float b = live ? x.pb[kk] : 0.f;
      ih[0] = RN_MFMA(x.pa0[kk], b, ih[0]);
      ih[1] = RN_MFMA(x.pa1[kk], b, ih[1]);
      ih[2] = RN_MFMA(x.pa2[kk], b, ih[2]);
    }
  }
}

extern "C" __global__ __launch_bounds__(RN_STK_WAVES * WAVE) void rn_gru_stack_kernel(RnStackStep a) {
  __shared__ float part[RN_STK_WAVES][4][4][RN_STK_PAD];  // sets: r, z, hn, gi_n (the last for layers 1, 2 only)
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1), q = lane >> 4, m = lane & 15;
  const int li = (int)blockIdx.x / a.tiles;  // (uniform) which of the launch's layers
  const RnStackLayerStep &p = a.L[li];
  const int H = a.H, u0 = ((int)blockIdx.x - li * a.tiles) * RN_STK_TILE, s0 = (int)blockIdx.y * RN_STK_TILE;
  const int L = H >> 2, k0 = wave * L;  // this wave's k: k0 .. k0 + L - 1
  const bool own_gi = p.gi == nullptr;  // (uniform) layers 1, 2
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = u0 + fi;
  const bool flive = frow < a.n_rows;
  const long long fr = flive ? frow : 0;
  float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f;
  if (own_gi) {
    gi_r = p.b_ih[fu], gi_z = p.b_ih[H + fu], gi_n = p.b_ih[2 * H + fu];
  } else {
    const float *const gi = p.gi + fr * p.in_rs;
    gi_r = gi[fu], gi_z = gi[H + fu], gi_n = gi[2 * H + fu];
  }
  const float b_r = p.b_hh[fu], b_z = p.b_hh[H + fu], b_n = p.b_hh[2 * H + fu];
  const float hp = p.prev != nullptr ? p.prev[fr * p.prev_rs + fu] : 0.f;
  f32x4 hh[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 ih[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  {
    const int row = s0 + m;
    const bool live = row < a.n_rows;
    const long long lrow = live ? row : 0, wo = (long long)(u0 + m) * H + k0, HH2 = (long long)H * H;
    RnStackFwdHalf h{}, x{};
    if (p.prev != nullptr) h.pb = p.prev + lrow * p.prev_rs + k0, h.pa0 = p.w_hh + wo, h.pa1 = h.pa0 + HH2, h.pa2 = h.pa1 + HH2;
    if (own_gi) x.pb = p.x + lrow * p.in_rs + k0, x.pa0 = p.w_ih + wo, x.pa1 = x.pa0 + HH2, x.pa2 = x.pa1 + HH2;
    if (own_gi) {  // (all uniform) zeros before: that half's sums stay zero
      if (p.prev != nullptr)
        rn_stack_fwd_quarter<RN_STK_FWD2_CH, true, true>(h, x, L, q, live, hh, ih);
      else
        rn_stack_fwd_quarter<RN_STK_FWD_CH, false, true>(h, x, L, q, live, hh, ih);
    } else if (p.prev != nullptr) {
      rn_stack_fwd_quarter<RN_STK_FWD_CH, true, false>(h, x, L, q, live, hh, ih);
    }
  }
  // the result's map: lane holds row (column) lane & 15, units 4 (lane >> 4) + register
#pragma unroll
  for (int r = 0; r < 4; r++) {
    part[wave][0][r][lane] = own_gi ? hh[0][r] + ih[0][r] : hh[0][r];
    part[wave][1][r][lane] = own_gi ? hh[1][r] + ih[1][r] : hh[1][r];
    part[wave][2][r][lane] = hh[2][r];
    part[wave][3][r][lane] = ih[2][r];
  }
  __syncthreads();
  if (!flive) return;  // rows that do not exist are not stored
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  float S[4];
#pragma unroll
  for (int g = 0; g < 4; g++) S[g] = ((part[0][g][reg][src] + part[1][g][reg][src]) + part[2][g][reg][src]) + part[3][g][reg][src];
  float r, z, n;
  const float hn = S[2] + b_n;
  if (own_gi) {
    r = rn_sigmoid(S[0] + (gi_r + b_r)), z = rn_sigmoid(S[1] + (gi_z + b_z));
    n = tanhf((S[3] + gi_n) + r * hn);
  } else {
    r = rn_sigmoid(gi_r + (S[0] + b_r)), z = rn_sigmoid(gi_z + (S[1] + b_z));
    n = tanhf(gi_n + r * hn);
  }
  p.y[(long long)frow * p.y_rs + fu] = (1.f - z) * n + z * hp;
  float *const sv = p.saved + (long long)frow * 4 * H + fu;
  sv[0] = r, sv[H] = z, sv[2 * H] = n, sv[3 * H] = hn;
}

// dgh of one unit of one row from what the forward step saved: -> a_r, a_z, a_n (dgi) and a_n r (dgh's third)
static __device__ __forceinline__ void rn_stack_gate_grads(float r, float z, float n, float hn, float dh, float hp, float &a_r, float &a_z,
                                                           float &a_n, float &b_n) {
  a_n = dh * (1.f - z) * (1.f - n * n);
  a_z = dh * (hp - n) * z * (1.f - z);
  a_r = a_n * hn * r * (1.f - r);
  b_n = a_n * r;
}

// what a lane of the backward step reads and writes of its row (row 0 where the row does not exist: read, zeroed, never stored)
struct RnStackGradLane {
  const float *sv, *dy, *dxi, *dhi, *hp;  // saved[t], dy[t], dx_{l+1}[t] (DX_IN), dh before (HAS_DH), y[t-1] (HAS_PREV) of the row
  float *dgi, *dgh;
  const float *pa0, *pa1, *pa2;  // w_hh's column c0 + (lane & 15) in the three gates' rows
  const float *pv0, *pv1, *pv2;  // w_ih's likewise (DX_OUT)
  bool live, store;
};

// CH chunks of 16 units of the backward sums from unit u on: every read first, then per chunk the gate gradients, their stores (unit
// tile 0 only) and the issues
template <bool HAS_DH, bool HAS_PREV, bool DX_IN, bool DX_OUT, int CH>
static __device__ __forceinline__ void rn_stack_bwd_chunks(const RnStackGradLane &p, int H, int u, f32x4 (&acc)[3], f32x4 (&acx)[3]) {
  f32x4 r[CH], z[CH], n[CH], hn[CH], dh[CH], dx[CH], di[CH], h[CH];
  float w0[CH][4], w1[CH][4], w2[CH][4], v0[CH][4], v1[CH][4], v2[CH][4];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    r[i] = *reinterpret_cast<const f32x4 *>(p.sv + v), z[i] = *reinterpret_cast<const f32x4 *>(p.sv + H + v);
    n[i] = *reinterpret_cast<const f32x4 *>(p.sv + 2 * H + v), hn[i] = *reinterpret_cast<const f32x4 *>(p.sv + 3 * H + v);
    dh[i] = *reinterpret_cast<const f32x4 *>(p.dy + v);
    if (DX_IN) dx[i] = *reinterpret_cast<const f32x4 *>(p.dxi + v);
    if (HAS_DH) di[i] = *reinterpret_cast<const f32x4 *>(p.dhi + v);
    h[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (HAS_PREV) h[i] = *reinterpret_cast<const f32x4 *>(p.hp + v);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const long long o = (long long)(v + c) * H;
      w0[i][c] = p.pa0[o], w1[i][c] = p.pa1[o], w2[i][c] = p.pa2[o];
      if (DX_OUT) v0[i][c] = p.pv0[o], v1[i][c] = p.pv1[o], v2[i][c] = p.pv2[o];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (as in the forward step)
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    if (DX_IN) dh[i] = dh[i] + dx[i];
    if (HAS_DH) dh[i] = di[i] + dh[i];
    f32x4 a_r, a_z, a_n, b_n;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float xr, xz, xn, xb;
      rn_stack_gate_grads(r[i][c], z[i][c], n[i][c], hn[i][c], dh[i][c], h[i][c], xr, xz, xn, xb);
      a_r[c] = p.live ? xr : 0.f, a_z[c] = p.live ? xz : 0.f, a_n[c] = p.live ? xn : 0.f, b_n[c] = p.live ? xb : 0.f;
    }
    if (p.store && p.live) {
      *reinterpret_cast<f32x4 *>(p.dgi + v) = a_r, *reinterpret_cast<f32x4 *>(p.dgi + H + v) = a_z;
      *reinterpret_cast<f32x4 *>(p.dgi + 2 * H + v) = a_n;
      *reinterpret_cast<f32x4 *>(p.dgh + v) = a_r, *reinterpret_cast<f32x4 *>(p.dgh + H + v) = a_z;
      *reinterpret_cast<f32x4 *>(p.dgh + 2 * H + v) = b_n;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      acc[0] = RN_MFMA(w0[i][c], a_r[c], acc[0]);
      acc[1] = RN_MFMA(w1[i][c], a_z[c], acc[1]);
      acc[2] = RN_MFMA(w2[i][c], b_n[c], acc[2]);
      if (DX_OUT) {
        acx[0] = RN_MFMA(v0[i][c], a_r[c], acx[0]);
        acx[1] = RN_MFMA(v1[i][c], a_z[c], acx[1]);
        acx[2] = RN_MFMA(v2[i][c], a_n[c], acx[2]);
      }
    }
  }
}

// one layer's backward step; HAS_DH: there is a dh from the step after, HAS_PREV: there is a y[t-1], DX_IN: the layer above adds its
// dx to dy (layers 0, 1), DX_OUT: this layer leaves a dx (layers 1, 2) -- uniform over the workgroup, so the reads of the usual step
// stand unconditionally
template <bool HAS_DH, bool HAS_PREV, bool DX_IN, bool DX_OUT>
static __device__ __forceinline__ void rn_stack_grad_step(const RnStackLayerGrad &a, int n_rows, int H, int c0,
                                                          float (&part)[RN_STK_WAVES][2][4][RN_STK_PAD]) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1), q = lane >> 4, m = lane & 15;
  const int s0 = (int)blockIdx.y * RN_STK_TILE;
  const int L = H >> 2, ub = wave * L;  // this wave's units ub .. ub + L - 1, each with its three gates
  constexpr int CH = DX_OUT ? RN_STK_BWD2_CH : RN_STK_BWD_CH;
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = c0 + fi;
  const bool flive = frow < n_rows;
  const long long fr = flive ? frow : 0;
  float f_dh = a.dy[fr * a.dy_rs + fu];
  const float f_z = a.saved[fr * 4 * H + H + fu];
  if (DX_IN) f_dh = f_dh + a.dx_in[fr * H + fu];
  if (HAS_DH) f_dh = a.dh_in[fr * H + fu] + f_dh;
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 acx[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  {
    const int row = s0 + m;
    RnStackGradLane p;
    p.live = row < n_rows, p.store = c0 == 0;  // (store: uniform) one workgroup of a layer's row tile stores dgi and dgh
    const long long lrow = p.live ? row : 0, HH2 = (long long)H * H;
    p.sv = a.saved + lrow * 4 * H, p.dy = a.dy + lrow * a.dy_rs;
    p.dxi = DX_IN ? a.dx_in + lrow * H : nullptr;
    p.dhi = HAS_DH ? a.dh_in + lrow * H : nullptr;
    p.hp = HAS_PREV ? a.prev + lrow * a.prev_rs : nullptr;
    p.dgi = a.dgi + lrow * a.dgi_rs, p.dgh = a.dgh + lrow * 3 * H;
    // A[i][k] = w[gate row k][c0 + i]: lane reads column c0 + (lane & 15) of the gate rows it feeds
    p.pa0 = a.w_hh + c0 + m, p.pa1 = p.pa0 + HH2, p.pa2 = p.pa1 + HH2;
    p.pv0 = DX_OUT ? a.w_ih + c0 + m : nullptr, p.pv1 = DX_OUT ? p.pv0 + HH2 : nullptr, p.pv2 = DX_OUT ? p.pv1 + HH2 : nullptr;
    int k = 0;
    for (; k + 16 * CH <= L; k += 16 * CH) rn_stack_bwd_chunks<HAS_DH, HAS_PREV, DX_IN, DX_OUT, CH>(p, H, ub + k + 4 * q, acc, acx);
    for (; k + 16 <= L; k += 16) rn_stack_bwd_chunks<HAS_DH, HAS_PREV, DX_IN, DX_OUT, 1>(p, H, ub + k + 4 * q, acc, acx);
    for (; k < L; k += 4) {  // what is left of a quarter: one unit per lane group and issue
      const int u = ub + k + q;
      float dh = p.dy[u];
      if (DX_IN) dh = dh + p.dxi[u];
      if (HAS_DH) dh = p.dhi[u] + dh;
      float a_r, a_z, a_n, b_n;
      rn_stack_gate_grads(p.sv[u], p.sv[H + u], p.sv[2 * H + u], p.sv[3 * H + u], dh, HAS_PREV ? p.hp[u] : 0.f, a_r, a_z, a_n, b_n);
      if (!p.live) a_r = 0.f, a_z = 0.f, a_n = 0.f, b_n = 0.f;
      if (p.store && p.live) {
        p.dgi[u] = a_r, p.dgi[H + u] = a_z, p.dgi[2 * H + u] = a_n;
        p.dgh[u] = a_r, p.dgh[H + u] = a_z, p.dgh[2 * H + u] = b_n;
      }
      const long long o = (long long)u * H;
      acc[0] = RN_MFMA(p.pa0[o], a_r, acc[0]);
      acc[1] = RN_MFMA(p.pa1[o], a_z, acc[1]);
      acc[2] = RN_MFMA(p.pa2[o], b_n, acc[2]);
      if (DX_OUT) {
        acx[0] = RN_MFMA(p.pv0[o], a_r, acx[0]);
        acx[1] = RN_MFMA(p.pv1[o], a_z, acx[1]);
        acx[2] = RN_MFMA(p.pv2[o], a_n, acx[2]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    part[wave][0][r][lane] = (acc[0][r] + acc[1][r]) + acc[2][r];
    if (DX_OUT) part[wave][1][r][lane] = (acx[0][r] + acx[1][r]) + acx[2][r];
  }
  __syncthreads();
  if (!flive) return;
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  const float sum = ((part[0][0][reg][src] + part[1][0][reg][src]) + part[2][0][reg][src]) + part[3][0][reg][src];
  a.dh_out[(long long)frow * H + fu] = f_dh * f_z + sum;
  if (DX_OUT) a.dx_out[(long long)frow * H + fu] = ((part[0][1][reg][src] + part[1][1][reg][src]) + part[2][1][reg][src]) + part[3][1][reg][src];
}

template <bool DX_IN, bool DX_OUT>
static __device__ __forceinline__ void rn_stack_grad_layer(const RnStackLayerGrad &p, int n_rows, int H, int c0,
                                                           float (&part)[RN_STK_WAVES][2][4][RN_STK_PAD]) {
  if (p.dh_in != nullptr) {
    if (p.prev != nullptr)
      rn_stack_grad_step<true, true, DX_IN, DX_OUT>(p, n_rows, H, c0, part);
    else
      rn_stack_grad_step<true, false, DX_IN, DX_OUT>(p, n_rows, H, c0, part);
  } else {
    if (p.prev != nullptr)
      rn_stack_grad_step<false, true, DX_IN, DX_OUT>(p, n_rows, H, c0, part);
    else
      rn_stack_grad_step<false, false, DX_IN, DX_OUT>(p, n_rows, H, c0, part);
  }
}

extern "C" __global__ __launch_bounds__(RN_STK_WAVES * WAVE) void rn_gru_stack_grad_kernel(RnStackGradStep a) {
  __shared__ float part[RN_STK_WAVES][2][4][RN_STK_PAD];  // sets: w_hh^T dgh, w_ih^T dgi
  const int li = (int)blockIdx.x / a.tiles;  // (uniform) which of the launch's layers
  const RnStackLayerGrad &p = a.L[li];
  const int c0 = ((int)blockIdx.x - li * a.tiles) * RN_STK_TILE;
  if (p.dx_out == nullptr)  // layer 0
    rn_stack_grad_layer<true, false>(p, a.n_rows, a.H, c0, part);
  else if (p.dx_in != nullptr)  // layer 1
    rn_stack_grad_layer<true, true>(p, a.n_rows, a.H, c0, part);
  else  // layer 2
    rn_stack_grad_layer<false, true>(p, a.n_rows, a.H, c0, part);
}
#endif  // RN_STK_HOST

namespace {
// whether n_frames x n_rows slots of M floats, slot (f, s) at f * frame_stride + s * row_stride, are disjoint in one of the two
// orders, move in whole 16-byte pieces, and end within LONG_MAX floats
bool slots_fit(long frame_stride, long row_stride, long M, int n_rows, long long n_frames) {
  if (frame_stride <= 0 || row_stride <= 0 || frame_stride % 4 || row_stride % 4) return false;
  if (n_frames <= 0) return true;
  const __int128 fs = frame_stride, rs = row_stride;
  if ((n_frames - 1) * fs + (n_rows - 1) * rs + M > (__int128)LONG_MAX) return false;
  const bool rows_in_frame = rs >= M && fs >= n_rows * rs;
  const bool frames_in_row = fs >= M && rs >= n_frames * fs;
  return rows_in_frame || frames_in_row;
}

// whether two sets of slots of M floats (each of which fits) are apart: their extents do not meet, or they have the same strides and
// lie side by side within the smaller stride (every slot pitch is at least that), as slices of a concatenation buffer do
bool slots_apart(const float *a, long afs, long ars, const float *b, long bfs, long brs, long M, int n_rows, long long n_frames) {
  if (n_frames <= 0) return true;
  const __int128 ua = (__int128)reinterpret_cast<uintptr_t>(a), ub = (__int128)reinterpret_cast<uintptr_t>(b);
  const __int128 ea = ((n_frames - 1) * (__int128)afs + (n_rows - 1) * (__int128)ars + M) * 4;
  const __int128 eb = ((n_frames - 1) * (__int128)bfs + (n_rows - 1) * (__int128)brs + M) * 4;
  if (ua + ea <= ub || ub + eb <= ua) return true;
  if (afs != bfs || ars != brs) return false;
  const __int128 d = (ua < ub ? ub - ua : ua - ub) / 4, inner = afs < ars ? afs : ars;
  return d >= M && d + M <= inner;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

bool counts_ok(int n_rows, int n_frames, int hidden) {
  if (n_rows < 1 || n_rows > RNNOISE_AMD_GRU_STACK_MAX_ROWS || n_frames < 0) return false;
  if (hidden < RNNOISE_AMD_GRU_STACK_MIN_HIDDEN || hidden > RNNOISE_AMD_GRU_STACK_MAX_HIDDEN || hidden % RN_STK_TILE) return false;
  return (__int128)RN_STK_LAYERS * n_frames * n_rows * 4 * hidden <= (__int128)LONG_MAX;
}

bool stack_ok(const RNNoiseGruStack *c) {
  if (!c || !c->gi0 || !aligned16(c->gi0)) return false;
  if (!counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++) {
    if (!c->w_hh[l] || !c->b_hh[l] || !c->y[l]) return false;
    if (!aligned16(c->w_hh[l]) || !aligned4(c->b_hh[l]) || !aligned16(c->y[l]) || !aligned16(c->h0[l])) return false;
    if (l > 0 && (!c->w_ih[l] || !c->b_ih[l] || !aligned16(c->w_ih[l]) || !aligned4(c->b_ih[l]))) return false;
    if (!slots_fit(c->y_frame_stride[l], c->y_row_stride[l], c->hidden, c->n_rows, c->n_frames)) return false;
  }
  if (!slots_fit(c->gi0_frame_stride, c->gi0_row_stride, 3L * c->hidden, c->n_rows, c->n_frames)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++)
    for (int k = l + 1; k < RN_STK_LAYERS; k++)
      if (!slots_apart(c->y[l], c->y_frame_stride[l], c->y_row_stride[l], c->y[k], c->y_frame_stride[k], c->y_row_stride[k], c->hidden,
                       c->n_rows, c->n_frames))
        return false;
  return true;
}

bool grad_ok(const RNNoiseGruStackGrad *c) {
  if (!c || !counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  for (int l = 0; l < RN_STK_LAYERS; l++) {
    if (!c->dy[l] || !c->y[l] || !c->w_hh[l] || !c->dgi[l] || !c->dgh[l] || !c->dh0[l]) return false;
    if (!aligned16(c->dy[l]) || !aligned16(c->y[l]) || !aligned16(c->w_hh[l]) || !aligned16(c->h0[l]) || !aligned16(c->dhT[l]) ||
        !aligned16(c->dgi[l]) || !aligned16(c->dgh[l]) || !aligned16(c->dh0[l]))
      return false;
    if (l > 0 && (!c->w_ih[l] || !aligned16(c->w_ih[l]))) return false;
    if (c->dhT[l]) {  // dh0 [N][H] apart from dhT [N][H]
      const uintptr_t a = reinterpret_cast<uintptr_t>(c->dhT[l]), b = reinterpret_cast<uintptr_t>(c->dh0[l]);
      const uintptr_t bytes = (uintptr_t)c->n_rows * c->hidden * sizeof(float);
      if (a < b ? b - a < bytes : a - b < bytes) return false;
    }
    if (!slots_fit(c->dy_frame_stride[l], c->dy_row_stride[l], c->hidden, c->n_rows, c->n_frames) ||
        !slots_fit(c->y_frame_stride[l], c->y_row_stride[l], c->hidden, c->n_rows, c->n_frames))
      return false;
  }
  return slots_fit(c->dgi0_frame_stride, c->dgi0_row_stride, 3L * c->hidden, c->n_rows, c->n_frames);
}

#define HIP_OK(expr)                                                                                                        \
  do {                                                                                                                      \
    hipError_t e_ = (expr);                                                                                                 \
    if (e_ != hipSuccess) {                                                                                                 \
      fprintf(stderr, "[rnnoise_amd_gru_stack] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                                                            \
    }                                                                                                                       \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (prev == device) || hipSetDevice(device) == hipSuccess;
    if (prev == device) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define ON_DEVICE(dev)                                                                                          \
  DeviceGuard guard_(dev);                                                                                      \
  if (!guard_.ok) {                                                                                             \
    fprintf(stderr, "[rnnoise_amd_gru_stack] cannot select HIP device %d (%s:%d)\n", (dev), __FILE__, __LINE__); \
    return -1;                                                                                                  \
  }

// the grid of a launch that holds `layers` layers
dim3 grid_of(int layers, int n_rows, int hidden) {
  return dim3((unsigned)(layers * (hidden / RN_STK_TILE)), (unsigned)((n_rows + RN_STK_TILE - 1) / RN_STK_TILE));
}
}  // namespace

extern "C" int rnnoise_amd_gru_stack_check(const RNNoiseGruStack *call) { return stack_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_stack_grad_check(const RNNoiseGruStackGrad *call) { return grad_ok(call) ? 0 : -1; }

extern "C" int rnnoise_amd_gru_stack_workspace(const RNNoiseGruStack *call, size_t *saved_floats, size_t *scratch_floats) {
  if (!call || !counts_ok(call->n_rows, call->n_frames, call->hidden)) return -1;
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
  a.n_rows = c.n_rows, a.H = c.hidden, a.tiles = c.hidden / RN_STK_TILE;
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
    hipLaunchKernelGGL(rn_gru_stack_kernel, grid_of(hi - lo + 1, c.n_rows, c.hidden), dim3(RN_STK_WAVES * WAVE), 0, st, a);
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
  a.n_rows = c.n_rows, a.H = c.hidden, a.tiles = c.hidden / RN_STK_TILE;
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
    hipLaunchKernelGGL(rn_gru_stack_grad_kernel, grid_of(hi - lo + 1, c.n_rows, c.hidden), dim3(RN_STK_WAVES * WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  return 0;
}
