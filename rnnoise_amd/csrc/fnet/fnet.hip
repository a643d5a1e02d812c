// fnet.hip -- librnnoise_amd_fnet.so (include/rnnoise_amd_fnet.h): the float network of a trainer checkpoint as a streaming runtime.
//
// A piece of T <= max_frames frames goes through five kinds of launches, listed by fnet_plan.h: gather (one workgroup a row: the
// row's history moves to the front of its feature workspace, the piece's frames behind it), conv1 and conv2 (one wave owns 16
// channels x 16 rows of one frame and adds the whole product in one chain), the GRUs on gru_stack.hip's diagonal schedule with
// ../gru_cell.h's cell in its OWN_GI form for all three layers, and the heads (a wave owns 16 of the 33 + 15 padded outputs x 16 rows
// of one frame; the waves of the piece's last frame also keep the three states).  cat[t][row][4H] = c2 | y_0 | y_1 | y_2 is what the
// GRUs read and write and what the heads read.  A row that is still warming up (fewer than four frames since its reset) gets zeros:
// the GRU workgroup that owns its tile overwrites what the cell stored, the heads select.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include <hip/hip_runtime.h>
#include "rnnoise_amd_fnet.h"
#include "../gru_cell.h"
#define RN_SIDE_LIB "rnnoise_amd_fnet"
#include "fnet_plan.h"

#define RN_FNET_FEAT RNNOISE_AMD_FNET_FEATURES
#define RN_FNET_BANDS RNNOISE_AMD_FNET_BANDS
#define RN_FNET_THREADS (RN_CELL_WAVES * RN_CELL_WAVE)

struct RnFnetReset {
  float *xin, *h;
  long long *start;
  const int *rows;  // NULL: row blockIdx.x
  long long x_rs, now;
  int n_rows, H, hist_at;  // hist_at: floats
};

struct RnFnetGather {
  float *xin;
  const float *feat;
  long long f_fs, f_rs, x_rs;
  int n_frames, hist_at;  // hist_at: floats
};

struct RnFnetDense {  // y[t][row][u] = tanh(b[u] + sum_k w[u][k] x[t][row][k])
  const float *w, *b, *x;
  float *y;
  long long x_fs, x_rs, y_fs, y_rs;
  int n_rows, n_frames, K, k_live, unit_tiles;
};

struct RnFnetLayerStep {  // one layer's step of a GRU launch: what ../gru_cell.h's forward names, and the frame's time
  const float *x, *w_ih, *b_ih, *w_hh, *b_hh, *prev;
  float *y, *saved;
  long long in_rs, prev_rs, y_rs;
  long long at;  // the clock at this frame
};

struct RnFnetStep {
  RnFnetLayerStep L[RN_FNET_LAYERS];  // the layers of this launch, the first live one at [0]
  const long long *start;
  int n_rows, H, tiles;
};

struct RnFnetHeads {
  const float *w, *b, *cat;
  float *gains, *vad, *h;
  const long long *start;
  long long g_fs, g_rs, v_fs, v_rs, now;
  int n_rows, n_frames, H, g0, keep;
};

// whether a row whose last reset was at clock `start` is still warming up at clock `at`
static __device__ __forceinline__ bool rn_fnet_warm(long long at, long long start) { return at - start < RNNOISE_AMD_FNET_LOOKAHEAD; }

// CH steps of a wave's product from k on, every read before the first issue.  VEC: a step is a chunk of 16 k, lane group q reads the
// four k 16 c + 4 q .. + 3 as one 16-byte read; otherwise a step is one issue, one k per lane group, and inputs from k_live on read as
// zero without being read.
template <bool VEC, int CH>
static __device__ __forceinline__ void rn_fnet_dot_steps(const float *pa, const float *pb, int k, int k_live, bool live, f32x4 &acc) {
  if constexpr (VEC) {
    f32x4 a[CH], b[CH];
#pragma unroll
    for (int i = 0; i < CH; i++) {
      a[i] = *reinterpret_cast<const f32x4 *>(pa + k + 16 * i);
      b[i] = *reinterpret_cast<const f32x4 *>(pb + k + 16 * i);
    }
#pragma unroll
    for (int i = 0; i < CH; i++) {
      if (!live) b[i] = f32x4{0.f, 0.f, 0.f, 0.f};  // rows beyond the last read as zeros (the read went to row 0)
#pragma unroll
      for (int c = 0; c < 4; c++) acc = RN_MFMA(a[i][c], b[i][c], acc);
    }
  } else {
    float a[CH], b[CH];
#pragma unroll
    for (int i = 0; i < CH; i++) {
      a[i] = pa[k + 4 * i];
      b[i] = (live && k + 4 * i < k_live) ? pb[k + 4 * i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < CH; i++) acc = RN_MFMA(a[i], b[i], acc);
  }
}

// a wave's product: 16 units (pa: the weight row of unit lane & 15) x 16 rows (pb: the input of row lane & 15) over K, one chain in
// ascending steps (the order does not depend on how many reads are in flight)
template <bool VEC>
static __device__ __forceinline__ f32x4 rn_fnet_dot(const float *pa, const float *pb, int K, int k_live, int q, bool live) {
  constexpr int STEP = VEC ? 16 : 4, CH = VEC ? 4 : 7;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + STEP * CH <= K; k += STEP * CH) rn_fnet_dot_steps<VEC, CH>(pa, pb, k + (VEC ? 4 * q : q), k_live, live, acc);
  for (; k < K; k += STEP) rn_fnet_dot_steps<VEC, 1>(pa, pb, k + (VEC ? 4 * q : q), k_live, live, acc);
  return acc;
}

template <bool VEC>
static __device__ __forceinline__ void rn_fnet_conv(const RnFnetDense &a) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (RN_CELL_WAVE - 1), q = lane >> 4, m = lane & 15;
  const int job = (int)blockIdx.x * RN_CELL_WAVES + wave;  // (frame, unit tile), uniform per wave
  if (job >= a.n_frames * a.unit_tiles) return;
  const int t = job / a.unit_tiles, u0 = (job - t * a.unit_tiles) * RN_CELL_TILE;
  const int row = (int)blockIdx.y * RN_CELL_TILE + m;
  const bool live = row < a.n_rows;
  const long long lrow = live ? row : 0;
  const f32x4 acc = rn_fnet_dot<VEC>(a.w + (long long)(u0 + m) * a.K, a.x + t * a.x_fs + lrow * a.x_rs, a.K, a.k_live, q, live);
  if (!live) return;
  // the result's map: lane holds row lane & 15, units 4 (lane >> 4) + register
  const int u = u0 + 4 * q;
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; r++) o[r] = tanhf(acc[r] + a.b[u + r]);
  *reinterpret_cast<f32x4 *>(a.y + t * a.y_fs + (long long)row * a.y_rs + u) = o;
}

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_reset_kernel(RnFnetReset a) {
  const int row = a.rows ? a.rows[blockIdx.x] : (int)blockIdx.x;
  if (row < 0 || row >= a.n_rows) return;  // (uniform)
  const int tid = (int)threadIdx.x;
  float *const x = a.xin + (long long)row * a.x_rs + a.hist_at;
  for (int i = tid; i < RN_FNET_HIST; i += RN_FNET_THREADS) x[i] = 0.f;
  for (int l = 0; l < RN_FNET_LAYERS; l++) {
    float *const h = a.h + ((long long)l * a.n_rows + row) * a.H;
    for (int i = tid; i < a.H; i += RN_FNET_THREADS) h[i] = 0.f;
  }
  if (tid == 0) a.start[row] = a.now;
}

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_gather_kernel(RnFnetGather a) {
  const int tid = (int)threadIdx.x;
  const long long row = blockIdx.x;
  float *const x = a.xin + row * a.x_rs;
  // the history: 260 floats from where the piece before left them to the front; every read before the first write
  const float h0 = x[a.hist_at + tid];
  const float h1 = tid < RN_FNET_HIST - RN_FNET_THREADS ? x[a.hist_at + RN_FNET_THREADS + tid] : 0.f;
  __syncthreads();
  x[tid] = h0;
  if (tid < RN_FNET_HIST - RN_FNET_THREADS) x[RN_FNET_THREADS + tid] = h1;
  const float *const f = a.feat + row * a.f_rs;
  for (int e = tid; e < a.n_frames * RN_FNET_FEAT; e += RN_FNET_THREADS) {
    const int t = e / RN_FNET_FEAT, ch = e - t * RN_FNET_FEAT;
    x[RN_FNET_HIST + e] = f[t * a.f_fs + ch];
  }
}

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_conv1_kernel(RnFnetDense a) { rn_fnet_conv<false>(a); }

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_conv2_kernel(RnFnetDense a) { rn_fnet_conv<true>(a); }

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_gru_kernel(RnFnetStep a) {
  __shared__ RnCellFwdLds<true> lds;
  const int li = (int)blockIdx.x / a.tiles;  // (uniform) which of the launch's layers
  const RnFnetLayerStep &p = a.L[li];
  const int u0 = ((int)blockIdx.x - li * a.tiles) * RN_CELL_TILE;
  rn_cell_forward<true>(p, a.n_rows, a.H, u0, lds);
  // the cell has no row predicate: the thread that stored unit fu of row frow puts a zero there where the row is warming up
  const int tid = (int)threadIdx.x, frow = (int)blockIdx.y * RN_CELL_TILE + (tid >> 4), fu = u0 + (tid & 15);
  if (frow < a.n_rows && rn_fnet_warm(p.at, a.start[frow])) p.y[(long long)frow * p.y_rs + fu] = 0.f;
}

extern "C" __global__ __launch_bounds__(RN_FNET_THREADS) void rn_fnet_heads_kernel(RnFnetHeads a) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (RN_CELL_WAVE - 1), q = lane >> 4, m = lane & 15;
  constexpr int TILES = RN_FNET_HEAD_ROWS / RN_CELL_TILE;
  const int job = (int)blockIdx.x * RN_CELL_WAVES + wave;  // (frame, unit tile), uniform per wave
  if (job >= a.n_frames * TILES) return;
  const int t = job / TILES, ut = job - t * TILES, u0 = ut * RN_CELL_TILE;
  const int s0 = (int)blockIdx.y * RN_CELL_TILE, row = s0 + m;
  const bool live = row < a.n_rows;
  const long long lrow = live ? row : 0, K = 4LL * a.H;
  const float *const cat = a.cat + (long long)t * a.n_rows * K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t >= a.g0)  // (uniform) before it every row is warming up and the GRUs have not run
    acc = rn_fnet_dot<true>(a.w + (u0 + m) * K, cat + lrow * K, (int)K, (int)K, q, live);
  if (live) {
    const bool warm = rn_fnet_warm(a.now + t, a.start[row]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int o = u0 + 4 * q + r;
      const float v = warm ? 0.f : rn_sigmoid(acc[r] + a.b[o]);
      if (o < RN_FNET_BANDS)
        a.gains[t * a.g_fs + row * a.g_rs + o] = v;
      else if (o == RN_FNET_BANDS)
        a.vad[t * a.v_fs + row * a.v_rs] = v;
    }
  }
  if (a.keep && t == a.n_frames - 1) {  // (uniform) unit tile ut keeps layer ut's state of the tile's rows
    const int H4 = a.H >> 2;
    for (int e = lane; e < RN_CELL_TILE * H4; e += RN_CELL_WAVE) {
      const int rr = e / H4, c = e - rr * H4, srow = s0 + rr;
      if (srow < a.n_rows)
        *reinterpret_cast<f32x4 *>(a.h + ((long long)ut * a.n_rows + srow) * a.H + 4 * c) =
            *reinterpret_cast<const f32x4 *>(cat + srow * K + (long long)(ut + 1) * a.H + 4 * c);
    }
  }
}

struct RNNoiseFnet {
  int device, C, H, N, M;
  float *w1, *b1, *w2, *b2, *w_ih[RN_FNET_LAYERS], *w_hh[RN_FNET_LAYERS], *b_ih[RN_FNET_LAYERS], *b_hh[RN_FNET_LAYERS], *wh, *bh;
  float *xin, *h;
  long long *start;
  float *c1, *cat, *saved;
  int *list;
  RnFnetClock clock;
};

namespace {
bool upload(float **d, const float *src, size_t floats) {
  if (hipMalloc(reinterpret_cast<void **>(d), floats * sizeof(float)) != hipSuccess) return false;
  return src == nullptr || hipMemcpy(*d, src, floats * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
}

void release(RNNoiseFnet *f) {
  float *all[] = {f->w1, f->b1, f->w2, f->b2, f->wh, f->bh, f->xin, f->h, f->c1, f->cat, f->saved};
  for (float *p : all) (void)hipFree(p);
  for (int l = 0; l < RN_FNET_LAYERS; l++) (void)hipFree(f->w_ih[l]), (void)hipFree(f->w_hh[l]), (void)hipFree(f->b_ih[l]), (void)hipFree(f->b_hh[l]);
  (void)hipFree(f->start), (void)hipFree(f->list);
  delete f;
}

bool build(RNNoiseFnet *f, const RNNoiseFnetWeights &w) {
  const size_t C = f->C, H = f->H, N = f->N, M = f->M;
  // conv1: k = 65 tap + ch, the pad's weight a zero; conv2: k = C tap + c
  std::vector<float> p1(C * RN_FNET_K1, 0.f), p2(H * 3 * C), ph(RN_FNET_HEAD_ROWS * 4 * H, 0.f), pb(RN_FNET_HEAD_ROWS, 0.f);
  for (size_t c = 0; c < C; c++)
    for (size_t ch = 0; ch < RN_FNET_FEAT; ch++)
      for (size_t tap = 0; tap < 3; tap++) p1[c * RN_FNET_K1 + tap * RN_FNET_FEAT + ch] = w.conv1_weight[(c * RN_FNET_FEAT + ch) * 3 + tap];
  for (size_t u = 0; u < H; u++)
    for (size_t c = 0; c < C; c++)
      for (size_t tap = 0; tap < 3; tap++) p2[u * 3 * C + tap * C + c] = w.conv2_weight[(u * C + c) * 3 + tap];
  memcpy(ph.data(), w.dense_out_weight, RN_FNET_BANDS * 4 * H * sizeof(float));
  memcpy(ph.data() + RN_FNET_BANDS * 4 * H, w.vad_dense_weight, 4 * H * sizeof(float));
  memcpy(pb.data(), w.dense_out_bias, RN_FNET_BANDS * sizeof(float));
  pb[RN_FNET_BANDS] = w.vad_dense_bias[0];
  if (!upload(&f->w1, p1.data(), p1.size()) || !upload(&f->b1, w.conv1_bias, C) || !upload(&f->w2, p2.data(), p2.size()) ||
      !upload(&f->b2, w.conv2_bias, H) || !upload(&f->wh, ph.data(), ph.size()) || !upload(&f->bh, pb.data(), pb.size()))
    return false;
  for (int l = 0; l < RN_FNET_LAYERS; l++)
    if (!upload(&f->w_ih[l], w.gru_weight_ih[l], 3 * H * H) || !upload(&f->w_hh[l], w.gru_weight_hh[l], 3 * H * H) ||
        !upload(&f->b_ih[l], w.gru_bias_ih[l], 3 * H) || !upload(&f->b_hh[l], w.gru_bias_hh[l], 3 * H))
      return false;
  if (!upload(&f->xin, nullptr, (M + RNNOISE_AMD_FNET_LOOKAHEAD) * RN_FNET_FEAT * N) || !upload(&f->h, nullptr, 3 * N * H) ||
      !upload(&f->c1, nullptr, (M + 2) * N * C) || !upload(&f->cat, nullptr, 4 * M * N * H) || !upload(&f->saved, nullptr, 12 * N * H))
    return false;
  if (hipMalloc(reinterpret_cast<void **>(&f->start), N * sizeof(long long)) != hipSuccess) return false;
  if (hipMalloc(reinterpret_cast<void **>(&f->list), N * sizeof(int)) != hipSuccess) return false;
  return true;
}

int reset_launch(RNNoiseFnet *f, const int *d_rows, int n, hipStream_t st) {
  RnFnetReset a{};
  a.xin = f->xin, a.h = f->h, a.start = f->start, a.rows = d_rows;
  a.x_rs = (long long)(f->M + RNNOISE_AMD_FNET_LOOKAHEAD) * RN_FNET_FEAT, a.now = f->clock.seen;
  a.n_rows = f->N, a.H = f->H, a.hist_at = f->clock.hist_at * RN_FNET_FEAT;
  hipLaunchKernelGGL(rn_fnet_reset_kernel, dim3((unsigned)n), dim3(RN_FNET_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}

dim3 wave_jobs(long long jobs, int n_rows) {
  return dim3((unsigned)((jobs + RN_CELL_WAVES - 1) / RN_CELL_WAVES), (unsigned)((n_rows + RN_CELL_TILE - 1) / RN_CELL_TILE));
}

struct Buffers {
  float *gains, *vad;
  const float *feat;
  long g_fs, g_rs, v_fs, v_rs, f_fs, f_rs;
};

bool buffers_ok(const RNNoiseFnet *f, Buffers &b, const RNNoiseFnetRows *gr, const RNNoiseFnetRows *vr, const RNNoiseFnetRows *fr, int n_frames) {
  if (!b.gains || !b.vad || !b.feat || !aligned4(b.gains) || !aligned4(b.vad) || !aligned4(b.feat)) return false;
  return rn_fnet_rows_ok(gr, RN_FNET_BANDS, f->N, n_frames, &b.g_fs, &b.g_rs) && rn_fnet_rows_ok(vr, 1, f->N, n_frames, &b.v_fs, &b.v_rs) &&
         rn_fnet_rows_ok(fr, RN_FNET_FEAT, f->N, n_frames, &b.f_fs, &b.f_rs);
}

// one launch of the plan
bool launch(RNNoiseFnet *f, const Buffers &b, const RnFnetLaunch &L, hipStream_t st) {
  const long long N = f->N, H = f->H, C = f->C, cat_fs = N * 4 * H;
  const long long x_rs = (long long)(f->M + RNNOISE_AMD_FNET_LOOKAHEAD) * RN_FNET_FEAT, c_rs = (long long)(f->M + 2) * C;
  switch (L.kind) {
    case RN_FNET_GATHER: {
      RnFnetGather a{};
      a.xin = f->xin, a.feat = b.feat + (long long)L.t0 * b.f_fs, a.f_fs = b.f_fs, a.f_rs = b.f_rs, a.x_rs = x_rs;
      a.n_frames = L.T, a.hist_at = L.hist_at * RN_FNET_FEAT;
      hipLaunchKernelGGL(rn_fnet_gather_kernel, dim3((unsigned)N), dim3(RN_FNET_THREADS), 0, st, a);
      break;
    }
    case RN_FNET_CONV1: {  // c1 frames -2 .. T-1 of the piece: index j reads the feature frames j .. j + 2 of the workspace
      RnFnetDense a{};
      a.w = f->w1, a.b = f->b1, a.x = f->xin, a.y = f->c1, a.x_fs = RN_FNET_FEAT, a.x_rs = x_rs, a.y_fs = C, a.y_rs = c_rs;
      a.n_rows = f->N, a.n_frames = L.T + 2, a.K = RN_FNET_K1, a.k_live = RN_FNET_K1_LIVE, a.unit_tiles = f->C / RN_CELL_TILE;
      hipLaunchKernelGGL(rn_fnet_conv1_kernel, wave_jobs((long long)a.n_frames * a.unit_tiles, f->N), dim3(RN_FNET_THREADS), 0, st, a);
      break;
    }
    case RN_FNET_CONV2: {  // frame t reads c1's index t .. t + 2, writes cat[t][.][0 .. H)
      RnFnetDense a{};
      a.w = f->w2, a.b = f->b2, a.x = f->c1, a.y = f->cat, a.x_fs = C, a.x_rs = c_rs, a.y_fs = cat_fs, a.y_rs = 4 * H;
      a.n_rows = f->N, a.n_frames = L.T, a.K = 3 * f->C, a.k_live = a.K, a.unit_tiles = f->H / RN_CELL_TILE;
      hipLaunchKernelGGL(rn_fnet_conv2_kernel, wave_jobs((long long)a.n_frames * a.unit_tiles, f->N), dim3(RN_FNET_THREADS), 0, st, a);
      break;
    }
    case RN_FNET_GRU: {
      RnFnetStep a{};
      a.start = f->start, a.n_rows = f->N, a.H = f->H, a.tiles = f->H / RN_CELL_TILE;
      for (int l = L.lo; l <= L.hi; l++) {
        const int t = L.t[l];
        RnFnetLayerStep &p = a.L[l - L.lo];
        float *const slot = f->cat + t * cat_fs;
        p.x = slot + l * H, p.in_rs = 4 * H;  // c2 for layer 0, y_{l-1} above
        p.w_ih = f->w_ih[l], p.b_ih = f->b_ih[l], p.w_hh = f->w_hh[l], p.b_hh = f->b_hh[l];
        p.y = slot + (l + 1) * H, p.y_rs = 4 * H;
        p.saved = f->saved + l * N * 4 * H;  // the cell's record for a backward step: nobody reads it here
        if (rn_fnet_prev_is_state(L, l))
          p.prev = f->h + l * N * H, p.prev_rs = H;
        else
          p.prev = slot - cat_fs + (l + 1) * H, p.prev_rs = 4 * H;
        p.at = L.seen + t;
      }
      hipLaunchKernelGGL(rn_fnet_gru_kernel, dim3((unsigned)((L.hi - L.lo + 1) * a.tiles), (unsigned)((f->N + RN_CELL_TILE - 1) / RN_CELL_TILE)),
                         dim3(RN_FNET_THREADS), 0, st, a);
      break;
    }
    default: {
      RnFnetHeads a{};
      a.w = f->wh, a.b = f->bh, a.cat = f->cat, a.h = f->h, a.start = f->start;
      a.gains = b.gains + (long long)L.t0 * b.g_fs, a.vad = b.vad + (long long)L.t0 * b.v_fs;
      a.g_fs = b.g_fs, a.g_rs = b.g_rs, a.v_fs = b.v_fs, a.v_rs = b.v_rs, a.now = L.seen;
      a.n_rows = f->N, a.n_frames = L.T, a.H = f->H, a.g0 = L.g0, a.keep = L.g0 < L.T;
      hipLaunchKernelGGL(rn_fnet_heads_kernel, wave_jobs((long long)L.T * (RN_FNET_HEAD_ROWS / RN_CELL_TILE), f->N), dim3(RN_FNET_THREADS), 0,
                         st, a);
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fprintf(stderr, "[" RN_SIDE_LIB "] launch %d failed: %s\n", L.kind, hipGetErrorString(e));
  return e == hipSuccess;
}
}  // namespace

extern "C" int rnnoise_amd_fnet_check(const RNNoiseFnetWeights *w, int n_rows, int max_frames) {
  return rn_fnet_weights_ok(w, n_rows, max_frames) ? 0 : -1;
}

extern "C" int rnnoise_amd_fnet_rows_check(const RNNoiseFnetRows *r, int row_floats, int n_rows, int n_frames) {
  return rn_fnet_rows_ok(r, row_floats, n_rows, n_frames, nullptr, nullptr) ? 1 : 0;
}

extern "C" long long rnnoise_amd_fnet_bytes(int cond_size, int gru_size, int n_rows, int max_frames) {
  return rn_fnet_bytes(cond_size, gru_size, n_rows, max_frames);
}

extern "C" RNNoiseFnet *rnnoise_amd_fnet_create(int device, const RNNoiseFnetWeights *w, int n_rows, int max_frames) {
  if (!rn_fnet_weights_ok(w, n_rows, max_frames)) return nullptr;
  DeviceGuard guard(device);
  if (!guard.ok) {
    fprintf(stderr, "[" RN_SIDE_LIB "] cannot select HIP device %d\n", device);
    return nullptr;
  }
  RNNoiseFnet *f = new (std::nothrow) RNNoiseFnet();
  if (!f) return nullptr;
  f->device = device, f->C = w->cond_size, f->H = w->gru_size, f->N = n_rows, f->M = max_frames;
  if (!build(f, *w) || reset_launch(f, nullptr, n_rows, nullptr) != 0 || hipStreamSynchronize(nullptr) != hipSuccess) {
    fprintf(stderr, "[" RN_SIDE_LIB "] cannot set up a runtime of %lld bytes on device %d\n", rn_fnet_bytes(f->C, f->H, f->N, f->M), device);
    release(f);
    return nullptr;
  }
  return f;
}

extern "C" void rnnoise_amd_fnet_destroy(RNNoiseFnet *f) {
  if (!f) return;
  DeviceGuard guard(f->device);
  if (guard.ok) (void)hipDeviceSynchronize();
  release(f);
}

extern "C" int rnnoise_amd_fnet_reset(RNNoiseFnet *f, void *hip_stream) {
  if (!f) return -1;
  ON_DEVICE(f->device);
  f->clock.seen = 0;
  return reset_launch(f, nullptr, f->N, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_amd_fnet_reset_rows_device(RNNoiseFnet *f, const int *d_rows, int n, void *hip_stream) {
  if (!f || n < 0 || n > f->N || (n > 0 && !d_rows)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(f->device);
  return reset_launch(f, d_rows, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_amd_fnet_reset_rows(RNNoiseFnet *f, const int *rows, int n) {
  if (!f || n < 0 || n > f->N || (n > 0 && !rows)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(f->device);
  HIP_OK(hipMemcpy(f->list, rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  if (reset_launch(f, f->list, n, nullptr) != 0) return -1;
  HIP_OK(hipStreamSynchronize(nullptr));
  return 0;
}

extern "C" int rnnoise_amd_fnet_process_device(RNNoiseFnet *f, float *d_gains, const RNNoiseFnetRows *gain_rows, float *d_vad,
                                               const RNNoiseFnetRows *vad_rows, const float *d_features, const RNNoiseFnetRows *feat_rows,
                                               int n_frames, void *hip_stream) {
  if (!f || n_frames < 0) return -1;
  if (n_frames == 0) return 0;
  Buffers b{d_gains, d_vad, d_features};
  if (!buffers_ok(f, b, gain_rows, vad_rows, feat_rows, n_frames)) return -1;
  ON_DEVICE(f->device);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  return rn_fnet_plan(n_frames, f->M, f->clock, [&](const RnFnetLaunch &L) { return launch(f, b, L, st); }) < 0 ? -1 : 0;
}

extern "C" int rnnoise_amd_fnet_process(RNNoiseFnet *f, float *gains, const RNNoiseFnetRows *gain_rows, float *vad,
                                        const RNNoiseFnetRows *vad_rows, const float *features, const RNNoiseFnetRows *feat_rows, int n_frames) {
  if (!f || n_frames < 0) return -1;
  if (n_frames == 0) return 0;
  Buffers b{gains, vad, features};
  if (!buffers_ok(f, b, gain_rows, vad_rows, feat_rows, n_frames)) return -1;
  ON_DEVICE(f->device);
  const size_t N = f->N, P = n_frames < f->M ? n_frames : f->M;
  float *d_f = nullptr, *d_g = nullptr, *d_v = nullptr;
  int rc = -1;
  if (upload(&d_f, nullptr, P * N * RN_FNET_FEAT) && upload(&d_g, nullptr, P * N * RN_FNET_BANDS) && upload(&d_v, nullptr, P * N)) {
    std::vector<float> h_f(P * N * RN_FNET_FEAT), h_g(P * N * RN_FNET_BANDS), h_v(P * N);
    rc = 0;
    for (int t0 = 0; t0 < n_frames && rc == 0; t0 += (int)P) {
      const size_t T = (size_t)(n_frames - t0) < P ? (size_t)(n_frames - t0) : P;
      for (size_t t = 0; t < T; t++)
        for (size_t s = 0; s < N; s++)
          memcpy(&h_f[(t * N + s) * RN_FNET_FEAT], features + (long long)(t0 + t) * b.f_fs + (long long)s * b.f_rs, RN_FNET_FEAT * sizeof(float));
      if (hipMemcpy(d_f, h_f.data(), T * N * RN_FNET_FEAT * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
          rnnoise_amd_fnet_process_device(f, d_g, nullptr, d_v, nullptr, d_f, nullptr, (int)T, nullptr) != 0 ||
          hipMemcpy(h_g.data(), d_g, T * N * RN_FNET_BANDS * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(h_v.data(), d_v, T * N * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        rc = -1;
        break;
      }
      for (size_t t = 0; t < T; t++)
        for (size_t s = 0; s < N; s++) {
          memcpy(gains + (long long)(t0 + t) * b.g_fs + (long long)s * b.g_rs, &h_g[(t * N + s) * RN_FNET_BANDS], RN_FNET_BANDS * sizeof(float));
          vad[(long long)(t0 + t) * b.v_fs + (long long)s * b.v_rs] = h_v[t * N + s];
        }
    }
  }
  (void)hipFree(d_f), (void)hipFree(d_g), (void)hipFree(d_v);
  return rc;
}
