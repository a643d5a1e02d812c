// gru_seq.hip -- librnnoise_amd_gru.so (include/rnnoise_amd_gru.h): the recurrence of a float GRU over a sequence, one launch per step.
//
// Both kernels have one shape.  A workgroup of four waves owns 16 hidden units x 16 rows; wave w takes the w-th quarter of the sum
// with v_mfma_f32_16x16x4_f32 (exact float32: a k-ordered fmaf chain), A = weights, B = the rows' vectors, so a row is a column of B
// and of the result and never meets another row.  The quarters go through LDS and thread e of the 256 adds them up in wave order for
// unit e & 15 of row e >> 4, does the gate math and stores with ordinary vector-memory stores.
//
// Which k a lane feeds into an issue is free as long as A and B agree, so where a quarter holds 16 k or more, lane group q = lane >> 4
// loads the four consecutive k 16 c' + 4 q .. + 3 as one 16-byte read and issue c of the chunk takes element c of every group; what
// is left of a quarter (H = 16, 48: 4 and 12 k) goes one k per lane group and issue.
//
// Forward: K = H, three accumulators (the gates' rows of w_hh), y[t-1] read from the slot before -- another slot than the one
// written, so no hazard.  Backward: K = 3H as H units x three gates, the wave's lanes compute the dgh they feed (element-wise on
// saved[t], dh, dy[t], y[t-1]) instead of reading it, the workgroups of unit tile 0 also store it (and dgi), and the result
// w_hh^T dgh + dh z goes to the OTHER dh buffer: every workgroup of a row tile reads all of dh while the others write their slices.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include "rnnoise_amd_gru.h"
#include <hip/hip_runtime.h>
#include <stdio.h>

#define WAVE 64
#define RN_GRU_TILE RNNOISE_AMD_GRU_TILE
#define RN_GRU_WAVES 4
#define RN_GRU_PAD 68  // floats of a register's row of partial sums: 64 lanes + 4, so the transposed read of the last stage hits 64 banks

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct RnGruStep {  // the forward step t
  const float *gi;    // slot (t, 0)
  const float *w, *b;
  const float *prev;  // y[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  float *y;           // slot (t, 0)
  float *saved;       // [n_rows][4H] of step t
  long long gi_rs, prev_rs, y_rs;
  int n_rows, H;
};

struct RnGruGradStep {  // the backward step t
  const float *saved;   // [n_rows][4H] of step t
  const float *dy;      // slot (t, 0)
  const float *prev;    // y[t-1] of row 0 (h0 at t = 0), or NULL: zeros
  const float *dh_in;   // [n_rows][H]: dh after step t + 1 (dhT at t = T - 1), or NULL: zeros
  const float *w;
  float *dgi;           // slot (t, 0)
  float *dgh;           // [n_rows][3H] of step t
  float *dh_out;        // [n_rows][H]: never dh_in
  long long dy_rs, prev_rs, dgi_rs;
  int n_rows, H;
};

#define RN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

static __device__ __forceinline__ float rn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// Chunks of 16 k whose reads a wave issues together before the first of their matrix instructions: a step is short and every read
// is a trip to L2 or HBM, so the reads of a quarter are put in flight at once instead of chunk after chunk.  Forward: 6 (H = 384: a
// wave's whole quarter, 24 reads of 16 bytes); backward, which reads seven vectors and twelve weights per chunk: 3.
#define RN_GRU_FWD_CH 6
#define RN_GRU_BWD_CH 3

// CH chunks of the forward sum from k offset kk on: every read first, then the issues in k order (the order does not depend on CH)
template <int CH>
static __device__ __forceinline__ void rn_gru_fwd_chunks(const float *pb, const float *pa0, const float *pa1, const float *pa2, int kk,
                                                         bool live, f32x4 (&acc)[3]) {
  f32x4 b[CH], a0[CH], a1[CH], a2[CH];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int o = kk + 16 * i;
    b[i] = *reinterpret_cast<const f32x4 *>(pb + o);
    a0[i] = *reinterpret_cast<const f32x4 *>(pa0 + o);
    a1[i] = *reinterpret_cast<const f32x4 *>(pa1 + o);
    a2[i] = *reinterpret_cast<const f32x4 *>(pa2 + o);
  }
  __builtin_amdgcn_sched_barrier(0);  // the reads stay together above: left alone, the scheduler puts 8 in flight and interleaves the rest
#pragma unroll
  for (int i = 0; i < CH; i++) {
    if (!live) b[i] = f32x4{0.f, 0.f, 0.f, 0.f};  // rows beyond the last read as zeros (the read itself went to row 0)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      acc[0] = RN_MFMA(a0[i][c], b[i][c], acc[0]);
      acc[1] = RN_MFMA(a1[i][c], b[i][c], acc[1]);
      acc[2] = RN_MFMA(a2[i][c], b[i][c], acc[2]);
    }
  }
}

extern "C" __global__ __launch_bounds__(RN_GRU_WAVES * WAVE) void rn_gru_step_kernel(RnGruStep a) {
  __shared__ float part[RN_GRU_WAVES][3][4][RN_GRU_PAD];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1), q = lane >> 4, m = lane & 15;
  const int H = a.H, u0 = (int)blockIdx.x * RN_GRU_TILE, s0 = (int)blockIdx.y * RN_GRU_TILE;
  const int L = H >> 2, k0 = wave * L;  // this wave's k: k0 .. k0 + L - 1
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = u0 + fi;
  const bool flive = frow < a.n_rows;
  const float *const gi = a.gi + (long long)(flive ? frow : 0) * a.gi_rs;
  const float gi_r = gi[fu], gi_z = gi[H + fu], gi_n = gi[2 * H + fu];
  const float b_r = a.b[fu], b_z = a.b[H + fu], b_n = a.b[2 * H + fu];
  float hp = 0.f;
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (a.prev != nullptr) {  // (uniform) zeros before: gh = b_hh
    hp = a.prev[(long long)(flive ? frow : 0) * a.prev_rs + fu];
    const int row = s0 + m;
    const bool live = row < a.n_rows;
    const float *const pb = a.prev + (long long)(live ? row : 0) * a.prev_rs + k0;
    const float *const pa0 = a.w + (long long)(u0 + m) * H + k0, *const pa1 = pa0 + (long long)H * H, *const pa2 = pa1 + (long long)H * H;
    int k = 0;
    for (; k + 16 * RN_GRU_FWD_CH <= L; k += 16 * RN_GRU_FWD_CH) rn_gru_fwd_chunks<RN_GRU_FWD_CH>(pb, pa0, pa1, pa2, k + 4 * q, live, acc);
    for (; k + 16 <= L; k += 16) rn_gru_fwd_chunks<1>(pb, pa0, pa1, pa2, k + 4 * q, live, acc);
    for (; k < L; k += 4) {  // what is left of a quarter: one k per lane group and issue
      const int kk = k + q;
      const float b = live ? pb[kk] : 0.f;
      acc[0] = RN_MFMA(pa0[kk], b, acc[0]);
      acc[1] = RN_MFMA(pa1[kk], b, acc[1]);
      acc[2] = RN_MFMA(pa2[kk], b, acc[2]);
    }
  }
  // the result's map: lane holds row (column) lane & 15, units 4 (lane >> 4) + register
#pragma unroll
  for (int g = 0; g < 3; g++)
#pragma unroll
    for (int r = 0; r < 4; r++) part[wave][g][r][lane] = acc[g][r];
  __syncthreads();
  if (!flive) return;  // rows that do not exist are not stored
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  float gh[3];
#pragma unroll
  for (int g = 0; g < 3; g++) gh[g] = ((part[0][g][reg][src] + part[1][g][reg][src]) + part[2][g][reg][src]) + part[3][g][reg][src];
  const float r = rn_sigmoid(gi_r + (gh[0] + b_r)), z = rn_sigmoid(gi_z + (gh[1] + b_z)), hn = gh[2] + b_n;
  const float n = tanhf(gi_n + r * hn);
  a.y[(long long)frow * a.y_rs + fu] = (1.f - z) * n + z * hp;
  float *const sv = a.saved + (long long)frow * 4 * H + fu;
  sv[0] = r, sv[H] = z, sv[2 * H] = n, sv[3 * H] = hn;
}

// dgh of one unit of one row from what the forward step saved: -> a_r, a_z, a_n (dgi) and a_n r (dgh's third)
static __device__ __forceinline__ void rn_gru_gate_grads(float r, float z, float n, float hn, float dh, float hp, float &a_r, float &a_z,
                                                         float &a_n, float &b_n) {
  a_n = dh * (1.f - z) * (1.f - n * n);
  a_z = dh * (hp - n) * z * (1.f - z);
  a_r = a_n * hn * r * (1.f - r);
  b_n = a_n * r;
}

// what a lane of the backward step reads and writes of its row (row 0 where the row does not exist: read, zeroed, never stored)
struct RnGruGradLane {
  const float *sv, *dy, *dhi, *hp;  // saved[t], dy[t], dh before (HAS_DH), y[t-1] (HAS_PREV) of the row
  float *dgi, *dgh;
  const float *pa0, *pa1, *pa2;  // w_hh's column c0 + (lane & 15) in the three gates' rows
  bool live, store;
};

// CH chunks of 16 units of the backward sum from unit u on: every read first, then per chunk the gate gradients, their stores (unit
// tile 0 only) and the issues
template <bool HAS_DH, bool HAS_PREV, int CH>
static __device__ __forceinline__ void rn_gru_bwd_chunks(const RnGruGradLane &p, int H, int u, f32x4 (&acc)[3]) {
  f32x4 r[CH], z[CH], n[CH], hn[CH], dh[CH], di[CH], h[CH];
  float w0[CH][4], w1[CH][4], w2[CH][4];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    r[i] = *reinterpret_cast<const f32x4 *>(p.sv + v), z[i] = *reinterpret_cast<const f32x4 *>(p.sv + H + v);
    n[i] = *reinterpret_cast<const f32x4 *>(p.sv + 2 * H + v), hn[i] = *reinterpret_cast<const f32x4 *>(p.sv + 3 * H + v);
    dh[i] = *reinterpret_cast<const f32x4 *>(p.dy + v);
    if (HAS_DH) di[i] = *reinterpret_cast<const f32x4 *>(p.dhi + v);
    h[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (HAS_PREV) h[i] = *reinterpret_cast<const f32x4 *>(p.hp + v);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const long long o = (long long)(v + c) * H;
      w0[i][c] = p.pa0[o], w1[i][c] = p.pa1[o], w2[i][c] = p.pa2[o];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (as in the forward step)
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    if (HAS_DH) dh[i] = di[i] + dh[i];
    f32x4 a_r, a_z, a_n, b_n;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float xr, xz, xn, xb;
      rn_gru_gate_grads(r[i][c], z[i][c], n[i][c], hn[i][c], dh[i][c], h[i][c], xr, xz, xn, xb);
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
    }
  }
}

// the backward step; HAS_DH: there is a dh from the step after (not at the last step of a call without dhT), HAS_PREV: there is a
// y[t-1] (not at step 0 of a call without h0) -- uniform over the launch, so the reads of the usual step stand unconditionally
template <bool HAS_DH, bool HAS_PREV>
static __device__ __forceinline__ void rn_gru_grad_step(const RnGruGradStep &a, float (&part)[RN_GRU_WAVES][4][RN_GRU_PAD]) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1), q = lane >> 4, m = lane & 15;
  const int H = a.H, c0 = (int)blockIdx.x * RN_GRU_TILE, s0 = (int)blockIdx.y * RN_GRU_TILE;
  const int L = H >> 2, ub = wave * L;  // this wave's units ub .. ub + L - 1, each with its three gates
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = c0 + fi;
  const bool flive = frow < a.n_rows;
  const long long fr = flive ? frow : 0;
  float f_dh = a.dy[fr * a.dy_rs + fu];
  const float f_z = a.saved[fr * 4 * H + H + fu];
  if (HAS_DH) f_dh = a.dh_in[fr * H + fu] + f_dh;
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  {
    const int row = s0 + m;
    RnGruGradLane p;
    p.live = row < a.n_rows, p.store = blockIdx.x == 0;  // (store: uniform) one workgroup of a row tile stores dgi and dgh
    const long long lrow = p.live ? row : 0;
    p.sv = a.saved + lrow * 4 * H, p.dy = a.dy + lrow * a.dy_rs;
    p.dhi = HAS_DH ? a.dh_in + lrow * H : nullptr;
    p.hp = HAS_PREV ? a.prev + lrow * a.prev_rs : nullptr;
    p.dgi = a.dgi + lrow * a.dgi_rs, p.dgh = a.dgh + lrow * 3 * H;
    // A[i][k] = w_hh[gate row k][c0 + i]: lane reads column c0 + (lane & 15) of the gate rows it feeds
    p.pa0 = a.w + c0 + m, p.pa1 = p.pa0 + (long long)H * H, p.pa2 = p.pa1 + (long long)H * H;
    int k = 0;
    for (; k + 16 * RN_GRU_BWD_CH <= L; k += 16 * RN_GRU_BWD_CH) rn_gru_bwd_chunks<HAS_DH, HAS_PREV, RN_GRU_BWD_CH>(p, H, ub + k + 4 * q, acc);
    for (; k + 16 <= L; k += 16) rn_gru_bwd_chunks<HAS_DH, HAS_PREV, 1>(p, H, ub + k + 4 * q, acc);
    for (; k < L; k += 4) {  // what is left of a quarter: one unit per lane group and issue
      const int u = ub + k + q;
      float dh = p.dy[u];
      if (HAS_DH) dh = p.dhi[u] + dh;
      float a_r, a_z, a_n, b_n;
      rn_gru_gate_grads(p.sv[u], p.sv[H + u], p.sv[2 * H + u], p.sv[3 * H + u], dh, HAS_PREV ? p.hp[u] : 0.f, a_r, a_z, a_n, b_n);
      if (!p.live) a_r = 0.f, a_z = 0.f, a_n = 0.f, b_n = 0.f;
      if (p.store && p.live) {
        p.dgi[u] = a_r, p.dgi[H + u] = a_z, p.dgi[2 * H + u] = a_n;
        p.dgh[u] = a_r, p.dgh[H + u] = a_z, p.dgh[2 * H + u] = b_n;
      }
      const long long o = (long long)u * H;
      acc[0] = RN_MFMA(p.pa0[o], a_r, acc[0]);
      acc[1] = RN_MFMA(p.pa1[o], a_z, acc[1]);
      acc[2] = RN_MFMA(p.pa2[o], b_n, acc[2]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) part[wave][r][lane] = (acc[0][r] + acc[1][r]) + acc[2][r];
  __syncthreads();
  if (!flive) return;
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  const float sum = ((part[0][reg][src] + part[1][reg][src]) + part[2][reg][src]) + part[3][reg][src];
  a.dh_out[(long long)frow * H + fu] = f_dh * f_z + sum;
}

extern "C" __global__ __launch_bounds__(RN_GRU_WAVES * WAVE) void rn_gru_step_grad_kernel(RnGruGradStep a) {
  __shared__ float part[RN_GRU_WAVES][4][RN_GRU_PAD];
  if (a.dh_in != nullptr) {
    if (a.prev != nullptr)
      rn_gru_grad_step<true, true>(a, part);
    else
      rn_gru_grad_step<true, false>(a, part);
  } else {
    if (a.prev != nullptr)
      rn_gru_grad_step<false, true>(a, part);
    else
      rn_gru_grad_step<false, false>(a, part);
  }
}

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

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool counts_ok(int n_rows, int n_frames, int hidden) {
  if (n_rows < 1 || n_rows > RNNOISE_AMD_GRU_MAX_ROWS || n_frames < 0) return false;
  if (hidden < RNNOISE_AMD_GRU_MIN_HIDDEN || hidden > RNNOISE_AMD_GRU_MAX_HIDDEN || hidden % RN_GRU_TILE) return false;
  return (__int128)n_frames * n_rows * 4 * hidden <= (__int128)LONG_MAX;
}

bool seq_ok(const RNNoiseGruSeq *c) {
  if (!c || !c->gi || !c->w_hh || !c->b_hh || !c->y) return false;
  if (!counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  if (!aligned16(c->gi) || !aligned16(c->w_hh) || !aligned16(c->y) || !aligned16(c->h0) || (reinterpret_cast<uintptr_t>(c->b_hh) & 3))
    return false;
  return slots_fit(c->gi_frame_stride, c->gi_row_stride, 3L * c->hidden, c->n_rows, c->n_frames) &&
         slots_fit(c->y_frame_stride, c->y_row_stride, c->hidden, c->n_rows, c->n_frames);
}

bool grad_ok(const RNNoiseGruSeqGrad *c) {
  if (!c || !c->dy || !c->y || !c->w_hh || !c->dgi || !c->dgh || !c->dh0) return false;
  if (!counts_ok(c->n_rows, c->n_frames, c->hidden)) return false;
  if (!aligned16(c->dy) || !aligned16(c->y) || !aligned16(c->w_hh) || !aligned16(c->h0) || !aligned16(c->dhT) || !aligned16(c->dgi) ||
      !aligned16(c->dgh) || !aligned16(c->dh0))
    return false;
  if (c->dhT) {  // dh0 [N][H] apart from dhT [N][H]
    const uintptr_t a = reinterpret_cast<uintptr_t>(c->dhT), b = reinterpret_cast<uintptr_t>(c->dh0);
    const uintptr_t bytes = (uintptr_t)c->n_rows * c->hidden * sizeof(float);
    if (a < b ? b - a < bytes : a - b < bytes) return false;
  }
  return slots_fit(c->dy_frame_stride, c->dy_row_stride, c->hidden, c->n_rows, c->n_frames) &&
         slots_fit(c->y_frame_stride, c->y_row_stride, c->hidden, c->n_rows, c->n_frames) &&
         slots_fit(c->dgi_frame_stride, c->dgi_row_stride, 3L * c->hidden, c->n_rows, c->n_frames);
}

#define HIP_OK(expr)                                                                                                  \
  do {                                                                                                                \
    hipError_t e_ = (expr);                                                                                           \
    if (e_ != hipSuccess) {                                                                                           \
      fprintf(stderr, "[rnnoise_amd_gru] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                                                      \
    }                                                                                                                 \
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
#define ON_DEVICE(dev)                                                                                    \
  DeviceGuard guard_(dev);                                                                                \
  if (!guard_.ok) {                                                                                       \
    fprintf(stderr, "[rnnoise_amd_gru] cannot select HIP device %d (%s:%d)\n", (dev), __FILE__, __LINE__); \
    return -1;                                                                                            \
  }

dim3 grid_of(int n_rows, int hidden) { return dim3((unsigned)(hidden / RN_GRU_TILE), (unsigned)((n_rows + RN_GRU_TILE - 1) / RN_GRU_TILE)); }
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
  a.w = c.w_hh, a.b = c.b_hh, a.gi_rs = c.gi_row_stride, a.y_rs = c.y_row_stride, a.n_rows = c.n_rows, a.H = c.hidden;
  const long long slot = (long long)c.n_rows * 4 * c.hidden;
  for (int t = 0; t < c.n_frames; t++) {
    a.gi = c.gi + (long long)t * c.gi_frame_stride;
    a.y = c.y + (long long)t * c.y_frame_stride;
    a.saved = d_saved + t * slot;
    if (t == 0)
      a.prev = c.h0, a.prev_rs = c.hidden;
    else
      a.prev = c.y + (long long)(t - 1) * c.y_frame_stride, a.prev_rs = c.y_row_stride;
    hipLaunchKernelGGL(rn_gru_step_kernel, grid, dim3(RN_GRU_WAVES * WAVE), 0, st, a);
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
  a.w = c.w_hh, a.dy_rs = c.dy_row_stride, a.dgi_rs = c.dgi_row_stride, a.n_rows = c.n_rows, a.H = c.hidden;
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
    hipLaunchKernelGGL(rn_gru_step_grad_kernel, grid, dim3(RN_GRU_WAVES * WAVE), 0, st, a);
    HIP_OK(hipGetLastError());
    dh = a.dh_out;
    which ^= 1;
  }
  return 0;
}
