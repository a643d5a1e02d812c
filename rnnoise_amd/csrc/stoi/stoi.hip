// stoi.hip -- librnnoise_amd_stoi.so (include/rnnoise_amd_stoi.h): three PCM planes in, the STOI and ESTOI sums of every row out.
//
// The header fixes the arithmetic and the order of every sum; what is chosen here is where the values wait between the stages.  Five
// plain launches, the kernel boundary the only ordering between them (no atomics, no workgroup waits for another):
//   rn_stoi_resample_kernel   48 -> 10 kHz.  A workgroup of five waves makes 1,280 outputs of one signal of one row: wave r the phase
//                             m % 5 == r, lane l the four consecutive outputs m = 5 (q0 + 4 l + i) + r of it.  Those four read the same
//                             input sample with taps 24 apart, so a sample is read from LDS once (as float, at a pitch of 97 for the
//                             lanes' 96: no bank conflict) and the taps, the same for every lane of a wave, come through scalar loads.
//   rn_stoi_keep_kernel       one workgroup a row: the norms of ref's frames, their maximum, the kept list by a prefix sum.
//   rn_stoi_bands_kernel      one wave per compacted frame: the frame is put together from kept frames m - 1, m, m + 1 (the compacted
//                             signal is never written), one 256-point complex FFT in LDS per signal (a real frame of 512 as its
//                             even and odd samples), the band envelopes.
//   rn_stoi_segments_kernel   one wave per segment: lane b a band row, then lane c a column.
//   rn_stoi_sum_kernel        one lane a row: the sums over segments in ascending order, and the counts.
#include <limits.h>
#include <stddef.h>
#include <hip/hip_runtime.h>
#include <stdio.h>

#define RN_SIDE_LIB "rnnoise_amd_stoi"
#include "../side_host.h"
#include "stoi_plan.h"
#define RN_STOI_CONST __constant__ const
#include "stoi_tables.h"

#define RN_STOI_EPS 0x1p-52
#define RN_STOI_CLIP 6.623413251903491  // 1 + 10^(15/20)
#define RN_STOI_NFFT 512
#define RN_STOI_UP 5
#define RN_STOI_DOWN 24
#define RN_STOI_PTAPS 461  // taps of a phase
#define RN_STOI_CENTRE 1152

__constant__ const int rn_stoi_band_lo[RN_STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// ---- 1. resampling ----
#define RN_RS_QPL 4                                     // consecutive outputs of a phase per lane
#define RN_RS_TILE (64 * RN_RS_QPL)                     // outputs of a phase per workgroup
#define RN_RS_LANE_IN (RN_STOI_DOWN * RN_RS_QPL)        // 96: input samples from one lane's first output to the next lane's
#define RN_RS_C0 230                                    // c = (24 r + 1152) / 5 of phase 0; phase 4 has 249
#define RN_RS_BACK (RN_STOI_PTAPS - 1 - RN_RS_C0)       // the tile's first input sample lies 230 before 24 q0
#define RN_RS_IN (RN_STOI_DOWN * (RN_RS_TILE - 1) + 249 + RN_RS_BACK + 1)  // 6,600 input samples of a tile
#define RN_RS_LDS (RN_RS_IN + RN_RS_IN / RN_RS_LANE_IN + 4)

// span sample n of a signal: ref and in are read `delay` samples earlier than out
static __device__ __forceinline__ float rn_stoi_sample(const float *p, long long fs, long long rs, int row, int g) {
  const int t = g / RN_STOI_FRAME, i = g - t * RN_STOI_FRAME;
  return p[(long long)t * fs + (long long)row * rs + i];
}

// steps [S0, S1) of a lane's walk down its input samples: step s reads the sample n_hi(output 3) - s, which is tap s - 24 (3 - i) of
// output i; outputs I0 .. I1 - 1 have a tap there
template <int I0, int I1, int S0, int S1>
static __device__ __forceinline__ void rn_rs_steps(const float *sx, const double *h, int lane, int c, double (&acc)[RN_RS_QPL]) {
#pragma unroll 4
  for (int s = S0; s < S1; s++) {
    const int v = 3 * RN_STOI_DOWN + c + RN_RS_BACK - s;  // the sample's place in the tile, less the lane's 96 l
    const double x = (double)sx[(RN_RS_LANE_IN + 1) * lane + v + v / RN_RS_LANE_IN];
#pragma unroll
    for (int i = I0; i < I1; i++) acc[i] = acc[i] + h[s - RN_STOI_DOWN * (RN_RS_QPL - 1 - i)] * x;
  }
}

extern "C" __global__ __launch_bounds__(64 * RN_STOI_UP) void rn_stoi_resample_kernel(RnStoiArgs a) {
  __shared__ float sx[RN_RS_LDS];
  const int tid = threadIdx.x, row = blockIdx.y, sig = blockIdx.z == 1 ? 2 : blockIdx.z == 2 ? 1 : 0;  // z: ref, out, in
  const int q0 = (int)blockIdx.x * RN_RS_TILE, Q = a.L10 / RN_STOI_UP;
  const float *p = sig == 0 ? a.ref : sig == 1 ? a.in : a.out;
  const long long fs = sig == 0 ? a.ref_fs : sig == 1 ? a.in_fs : a.out_fs, rs = sig == 0 ? a.ref_rs : sig == 1 ? a.in_rs : a.out_rs;
  const int g0 = a.first * RN_STOI_FRAME - (sig == 2 ? 0 : a.delay);  // plane sample of span sample 0 (>= 0: the check)
  const int n_lo = RN_STOI_DOWN * q0 - RN_RS_BACK;
  for (int pp = tid; pp < RN_RS_IN; pp += 64 * RN_STOI_UP) {
    const int n = n_lo + pp;
    sx[pp + pp / RN_RS_LANE_IN] = n >= 0 && n < a.L ? rn_stoi_sample(p, fs, rs, row, g0 + n) : 0.f;
  }
  __syncthreads();
  const int r = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  // output m = 5 q + r takes input samples 24 q + c down to 24 q + c - 460 with taps k0, k0 + 5, ...
  const int k0 = (RN_STOI_DOWN * r + RN_STOI_CENTRE) % RN_STOI_UP, c = (RN_STOI_DOWN * r + RN_STOI_CENTRE) / RN_STOI_UP;
  const double *h = rn_stoi_h[k0];
  double acc[RN_RS_QPL] = {0.0, 0.0, 0.0, 0.0};
  // every output takes its 461 taps in ascending order: the first 24, 48, 72 steps belong to the later outputs alone, the last ones
  // to the earlier
  rn_rs_steps<3, 4, 0, 24>(sx, h, lane, c, acc);
  rn_rs_steps<2, 4, 24, 48>(sx, h, lane, c, acc);
  rn_rs_steps<1, 4, 48, 72>(sx, h, lane, c, acc);
  rn_rs_steps<0, 4, 72, RN_STOI_PTAPS>(sx, h, lane, c, acc);
  rn_rs_steps<0, 3, RN_STOI_PTAPS, RN_STOI_PTAPS + 24>(sx, h, lane, c, acc);
  rn_rs_steps<0, 2, RN_STOI_PTAPS + 24, RN_STOI_PTAPS + 48>(sx, h, lane, c, acc);
  rn_rs_steps<0, 1, RN_STOI_PTAPS + 48, RN_STOI_PTAPS + 72>(sx, h, lane, c, acc);
  double *const y = a.y10 + ((long long)row * 3 + sig) * a.C;
#pragma unroll
  for (int i = 0; i < RN_RS_QPL; i++) {
    const int q = q0 + RN_RS_QPL * lane + i;
    if (q < Q) y[RN_STOI_UP * q + r] = 5.0 * acc[i];
  }
}

// ---- 2. frame norms of ref, their maximum, the kept list ----
#define RN_KEEP_THREADS 256
extern "C" __global__ __launch_bounds__(RN_KEEP_THREADS) void rn_stoi_keep_kernel(RnStoiArgs a) {
  __shared__ double s_max[RN_KEEP_THREADS];
  __shared__ int s_nan[RN_KEEP_THREADS], s_scan[RN_KEEP_THREADS];
  const int tid = threadIdx.x, row = blockIdx.x;
  const double *const y = a.y10 + (long long)row * 3 * a.C;
  double *const norm = a.norm + (long long)row * a.G;
  double mx = 0.0;
  int nan = 0;
  for (int j = tid; j < a.F; j += RN_KEEP_THREADS) {
    double acc = 0.0;
    for (int i = 0; i < RN_STOI_WIN; i++) {
      const double t = rn_stoi_w[i] * y[RN_STOI_HOP * j + i];
      acc = acc + t * t;
    }
    const double v = sqrt(acc);
    norm[j] = v;
    if (v != v) nan = 1;
    else mx = v > mx ? v : mx;
  }
  s_max[tid] = mx, s_nan[tid] = nan;
  __syncthreads();
  for (int m = RN_KEEP_THREADS / 2; m >= 1; m >>= 1) {  // (a maximum has no order)
    if (tid < m) {
      s_max[tid] = s_max[tid + m] > s_max[tid] ? s_max[tid + m] : s_max[tid];
      s_nan[tid] |= s_nan[tid + m];
    }
    __syncthreads();
  }
  const double top = s_nan[0] ? __builtin_nan("") : s_max[0];
  const double limit = (top + RN_STOI_EPS) * 0.01;  // NaN: no frame is kept
  __syncthreads();
  int *const idx = a.idx + (long long)row * (a.G + a.G % 2);
  int base = 0;
  for (int j0 = 0; j0 < a.F; j0 += RN_KEEP_THREADS) {
    const int j = j0 + tid;
    const int keep = j < a.F && (norm[j] + RN_STOI_EPS) > limit;  // (norm[j]: this thread's own store)
    s_scan[tid] = keep;
    __syncthreads();
    for (int d = 1; d < RN_KEEP_THREADS; d <<= 1) {
      const int v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    if (keep) idx[base + s_scan[tid] - 1] = j;
    base += s_scan[RN_KEEP_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) a.cnt[2 * row] = base, a.cnt[2 * row + 1] = 0;
}

// ---- 3. compaction, STFT, bands ----
#define RN_STOI_HALF (RN_STOI_NFFT / 2)  // points of the complex transform that carries a real frame of 512
static __device__ __forceinline__ int rn_stoi_brev8(int i) { return (int)(__builtin_bitreverse32((unsigned)i) >> 24); }

// sample i of the windowed compacted frame m of the 10 kHz signal y: the kept frames m - 1 (f_lo, where there is one) and m (f_mid)
// meet in its first half, m and m + 1 (f_hi) in its second; the lower frame's term is the first operand of the sum
static __device__ __forceinline__ double rn_stoi_frame_sample(const double *y, int i, int f_lo, int f_mid, int f_hi, bool has_lo) {
  const bool first_half = i < RN_STOI_HOP;
  const int ia = first_half ? i + RN_STOI_HOP : i, ib = first_half ? i : i - RN_STOI_HOP;  // offsets in the lower and the higher frame
  const long long pa = (long long)RN_STOI_HOP * (first_half ? f_lo : f_mid) + ia, pb = (long long)RN_STOI_HOP * (first_half ? f_mid : f_hi) + ib;
  const double ta = !first_half || has_lo ? rn_stoi_w[ia] * y[pa] : 0.0;
  return rn_stoi_w[i] * (ta + rn_stoi_w[ib] * y[pb]);
}

extern "C" __global__ __launch_bounds__(64) void rn_stoi_bands_kernel(RnStoiArgs a) {
  __shared__ double s_re[3][RN_STOI_HALF], s_im[3][RN_STOI_HALF];
  const int lane = threadIdx.x, m = blockIdx.x, row = blockIdx.y;
  const int K = a.cnt[2 * row];
  if (m >= K - 1) return;  // (the same for the whole workgroup)
  const int *const idx = a.idx + (long long)row * (a.G + a.G % 2);
  const int f_lo = m >= 1 ? idx[m - 1] : 0, f_mid = idx[m], f_hi = idx[m + 1];
  const double *const y0 = a.y10 + (long long)row * 3 * a.C;
  // every signal has a transform of its own -- nothing of one signal reaches another's spectrum, an all-zero frame has an all-zero
  // spectrum --: the 512 real samples (256 of the frame, 256 zeros) go as 256 complex points z[j] = x[2 j] + i x[2 j + 1]
#pragma unroll
  for (int sig = 0; sig < 3; sig++) {
    if (sig == 1 && !a.in) continue;
    const double *const y = y0 + (long long)sig * a.C;
#pragma unroll
    for (int u = 0; u < RN_STOI_HALF / 64; u++) {
      const int j = lane + 64 * u, at = rn_stoi_brev8(j);
      const bool in_frame = 2 * j < RN_STOI_WIN;
      s_re[sig][at] = in_frame ? rn_stoi_frame_sample(y, 2 * j, f_lo, f_mid, f_hi, m >= 1) : 0.0;
      s_im[sig][at] = in_frame ? rn_stoi_frame_sample(y, 2 * j + 1, f_lo, f_mid, f_hi, m >= 1) : 0.0;
    }
  }
  __syncthreads();
  for (int half = 1; half < RN_STOI_HALF; half <<= 1) {  // radix 2, decimation in time, 8 stages
#pragma unroll
    for (int u = 0; u < RN_STOI_HALF / 128; u++) {
      const int b = lane + 64 * u, k = b & (half - 1), lo = ((b - k) << 1) + k, hi = lo + half;
      const int tw = k * (RN_STOI_HALF / half);  // exp(-2 pi i k / (2 half)) in the table of 512
      const double c = rn_stoi_cos[tw], s = rn_stoi_sin[tw];  // W = c - i s
#pragma unroll
      for (int sig = 0; sig < 3; sig++) {
        if (sig == 1 && !a.in) continue;
        const double br = s_re[sig][hi], bi = s_im[sig][hi], ar = s_re[sig][lo], ai = s_im[sig][lo];
        const double tr = br * c + bi * s, ti = bi * c - br * s;
        s_re[sig][lo] = ar + tr, s_im[sig][lo] = ai + ti;
        s_re[sig][hi] = ar - tr, s_im[sig][hi] = ai - ti;
      }
    }
    __syncthreads();
  }
  // bin k of the real frame: X[k] = E[k] + W^k O[k], E and O the transforms of the even and the odd samples, separated by the
  // conjugate symmetry of a real signal's spectrum; lane b a band, its bins in ascending order
  if (lane < RN_STOI_BANDS) {
#pragma unroll
    for (int sig = 0; sig < 3; sig++) {
      if (sig == 1 && !a.in) continue;
      double acc = 0.0;
      for (int k = rn_stoi_band_lo[lane]; k < rn_stoi_band_lo[lane + 1]; k++) {
        const double zr = s_re[sig][k], zi = s_im[sig][k], nr = s_re[sig][RN_STOI_HALF - k], ni = s_im[sig][RN_STOI_HALF - k];
        const double er = 0.5 * (zr + nr), ei = 0.5 * (zi - ni), pr = 0.5 * (zi + ni), pi = 0.5 * (nr - zr);
        const double c = rn_stoi_cos[k], s = rn_stoi_sin[k];
        const double xr = er + (pr * c + pi * s), xi = ei + (pi * c - pr * s);
        acc = acc + (xr * xr + xi * xi);
      }
      a.env[(((long long)row * 3 + sig) * a.G + m) * RN_STOI_BANDS + lane] = sqrt(acc);
    }
  }
}

// ---- 4. segments ----
// (the compiler unrolls the 30-column and 15-band loops fully, 253 VGPRs: measured faster than the rolled loops' 55, DESIGN.md 4.35 --
// 15 and then 30 lanes work, and the unrolled loops are their instruction-level parallelism)
#define RN_SEG_N (RN_STOI_BANDS * RN_STOI_SEG)
extern "C" __global__ __launch_bounds__(64) void rn_stoi_segments_kernel(RnStoiArgs a) {
  __shared__ double sx[RN_SEG_N], sy[RN_SEG_N], sxn[RN_SEG_N], syn[RN_SEG_N], s_d[RN_STOI_SEG];  // [column][band]
  const int lane = threadIdx.x, sg = blockIdx.x, row = blockIdx.y;
  const int K = a.cnt[2 * row];
  if (sg >= K - RN_STOI_SEG) return;  // (the same for the whole workgroup)
  for (int pair = a.in ? 0 : 1; pair < 2; pair++) {
    const double *const ex = a.env + ((long long)row * 3 * a.G + sg) * RN_STOI_BANDS;  // columns sg .. sg + 29 of ref
    const double *const ey = ex + (long long)(pair + 1) * a.G * RN_STOI_BANDS;     // ... of in or out
    for (int i = lane; i < RN_SEG_N; i += 64) sx[i] = ex[i], sy[i] = ey[i];
    __syncthreads();
    if (lane < RN_STOI_BANDS) {  // a band row
      const int b = lane;
      double xx = 0.0, yy = 0.0, xs = 0.0, ys = 0.0;
      for (int c = 0; c < RN_STOI_SEG; c++) {
        const double x = sx[c * RN_STOI_BANDS + b], y = sy[c * RN_STOI_BANDS + b];
        xx = xx + x * x, yy = yy + y * y, xs = xs + x, ys = ys + y;
      }
      const double alpha = sqrt(xx) / (sqrt(yy) + RN_STOI_EPS);
      double ps = 0.0;
      for (int c = 0; c < RN_STOI_SEG; c++) {
        const double x = sx[c * RN_STOI_BANDS + b], ya = alpha * sy[c * RN_STOI_BANDS + b], cl = x * RN_STOI_CLIP;
        const double yp = (ya != ya || ya < cl) ? ya : cl;  // min; a NaN goes through
        syn[c * RN_STOI_BANDS + b] = yp;  // (for now: the clipped row)
        ps = ps + yp;
      }
      const double xm = xs / RN_STOI_SEG, ym = ys / RN_STOI_SEG, pm = ps / RN_STOI_SEG;
      double xv = 0.0, yv = 0.0, pv = 0.0;
      for (int c = 0; c < RN_STOI_SEG; c++) {
        const double x = sx[c * RN_STOI_BANDS + b] - xm, y = sy[c * RN_STOI_BANDS + b] - ym, p = syn[c * RN_STOI_BANDS + b] - pm;
        xv = xv + x * x, yv = yv + y * y, pv = pv + p * p;
      }
      const double xd = sqrt(xv) + RN_STOI_EPS, yd = sqrt(yv) + RN_STOI_EPS, pd = sqrt(pv) + RN_STOI_EPS;
      double d = 0.0;
      for (int c = 0; c < RN_STOI_SEG; c++) {
        const double xn = (sx[c * RN_STOI_BANDS + b] - xm) / xd, pn = (syn[c * RN_STOI_BANDS + b] - pm) / pd;
        d = d + xn * pn;
        sxn[c * RN_STOI_BANDS + b] = xn;
        syn[c * RN_STOI_BANDS + b] = (sy[c * RN_STOI_BANDS + b] - ym) / yd;  // ESTOI's rows: the unclipped y
      }
      s_d[b] = d;
    }
    __syncthreads();
    double *const out = a.seg + ((long long)row * a.G + sg) * 4 + 2 * pair;
    if (lane == 0) {
      double d = 0.0;
      for (int b = 0; b < RN_STOI_BANDS; b++) d = d + s_d[b];
      out[0] = d / RN_STOI_BANDS;
    }
    __syncthreads();
    if (lane < RN_STOI_SEG) {  // a column
      const double *const x = sxn + lane * RN_STOI_BANDS, *const y = syn + lane * RN_STOI_BANDS;
      double xs = 0.0, ys = 0.0;
      for (int b = 0; b < RN_STOI_BANDS; b++) xs = xs + x[b], ys = ys + y[b];
      const double xm = xs / RN_STOI_BANDS, ym = ys / RN_STOI_BANDS;
      double xv = 0.0, yv = 0.0;
      for (int b = 0; b < RN_STOI_BANDS; b++) {
        const double p = x[b] - xm, q = y[b] - ym;
        xv = xv + p * p, yv = yv + q * q;
      }
      const double xd = sqrt(xv) + RN_STOI_EPS, yd = sqrt(yv) + RN_STOI_EPS;
      double d = 0.0;
      for (int b = 0; b < RN_STOI_BANDS; b++) d = d + ((x[b] - xm) / xd) * ((y[b] - ym) / yd);
      s_d[lane] = d;
    }
    __syncthreads();
    if (lane == 0) {
      double d = 0.0;
      for (int c = 0; c < RN_STOI_SEG; c++) d = d + s_d[c];
      out[1] = d / RN_STOI_SEG;
    }
    __syncthreads();
  }
}

// ---- 5. the sums over segments ----
extern "C" __global__ __launch_bounds__(64) void rn_stoi_sum_kernel(RnStoiArgs a) {
  const int row = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (row >= a.n_rows) return;
  const int K = a.cnt[2 * row], n = K > RN_STOI_SEG ? K - RN_STOI_SEG : 0;
  const double *const seg = a.seg + (long long)row * a.G * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int sg = 0; sg < n; sg++) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k >= 2 || a.in) s[k] = s[k] + seg[4 * sg + k];
  }
  double *const r = a.results + (long long)row * RN_STOI_SLOTS;
  r[0] = s[0], r[1] = s[1], r[2] = a.in ? (double)n : 0.0, r[3] = a.in ? (double)K : 0.0;
  r[4] = s[2], r[5] = s[3], r[6] = (double)n, r[7] = (double)K;
}

extern "C" int rnnoise_amd_stoi_check(const RNNoiseStoi *call) { return stoi_call_ok(call) ? 0 : -1; }

extern "C" long long rnnoise_amd_stoi_workspace(int n_rows, int n_frames) { return stoi_workspace(n_rows, n_frames); }

namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// at most five launches; a stage without work (a sequence too short for a frame, for two, for a segment) is left out
int launch(const RnStoiArgs &a, hipStream_t st) {
  const unsigned rows = (unsigned)a.n_rows;
  const int Q = a.L10 / RN_STOI_UP;
  if (Q > 0) {
    hipLaunchKernelGGL(rn_stoi_resample_kernel, dim3((unsigned)((Q + RN_RS_TILE - 1) / RN_RS_TILE), rows, a.in ? 3 : 2), dim3(64 * RN_STOI_UP), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(rn_stoi_keep_kernel, dim3(rows), dim3(RN_KEEP_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
  if (a.F > 1) {
    hipLaunchKernelGGL(rn_stoi_bands_kernel, dim3((unsigned)(a.F - 1), rows), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  if (a.F > RN_STOI_SEG) {
    hipLaunchKernelGGL(rn_stoi_segments_kernel, dim3((unsigned)(a.F - RN_STOI_SEG), rows), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(rn_stoi_sum_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int rnnoise_amd_stoi_device(int device, double *d_results, void *d_scratch, long long scratch_bytes, const RNNoiseStoi *call,
                                       void *hip_stream) {
  RnStoiArgs a;
  if (!stoi_plan(call, d_results, d_scratch, scratch_bytes, a)) return -1;
  ON_DEVICE(device);
  return launch(a, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_amd_stoi(int device, double *results, const RNNoiseStoi *call) {
  if (!stoi_call_ok(call) || !results) return -1;
  const RNNoiseStoi &c = *call;
  ON_DEVICE(device);
  // staged as [rows][T][480]; a piece's PCM and scratch within 256 MiB, one row at least
  const size_t T = (size_t)c.n_frames, row_floats = T * RN_STOI_FRAME, row_bytes = row_floats * sizeof(float);
  const int n_planes = c.in.p ? 3 : 2;
  const size_t per_row = n_planes * row_bytes + (size_t)stoi_workspace(1, c.n_frames) + RN_STOI_SLOTS * sizeof(double);
  size_t R = ((size_t)256 << 20) / per_row;
  R = R < 1 ? 1 : R > (size_t)c.n_rows ? (size_t)c.n_rows : R;
  const long long scratch_bytes = stoi_workspace((int)R, c.n_frames);
  DevBuf pcm, scratch, dres;
  HIP_OK(hipMalloc(&pcm.p, n_planes * R * row_bytes + 16));
  HIP_OK(hipMalloc(&scratch.p, (size_t)scratch_bytes));
  HIP_OK(hipMalloc(&dres.p, R * RN_STOI_SLOTS * sizeof(double)));
  float *const d_ref = static_cast<float *>(pcm.p), *const d_out = d_ref + R * row_floats;
  float *const d_in = c.in.p ? d_out + R * row_floats : nullptr;  // (allocated only beside a noisy plane)
  auto staged = [&](float *p) { return RNNoiseStoiPlane{p, RN_STOI_FRAME, row_floats ? (long)row_floats : RN_STOI_FRAME}; };
  auto up = [&](float *dst, const RNNoiseStoiPlane &p, size_t r0, size_t rows) -> int {
    for (size_t r = 0; r < rows && T; r++)
      HIP_OK(hipMemcpy2D(dst + r * row_floats, RN_STOI_FRAME * sizeof(float), p.p + (long long)(r0 + r) * p.row_stride,
                         (size_t)p.frame_stride * sizeof(float), RN_STOI_FRAME * sizeof(float), T, hipMemcpyHostToDevice));
    return 0;
  };
  for (size_t r0 = 0; r0 < (size_t)c.n_rows; r0 += R) {
    const size_t rows = (size_t)c.n_rows - r0 < R ? (size_t)c.n_rows - r0 : R;
    if (up(d_ref, c.ref, r0, rows) || up(d_out, c.out, r0, rows) || (c.in.p && up(d_in, c.in, r0, rows))) return -1;
    RNNoiseStoi piece = c;
    piece.n_rows = (int)rows;
    piece.ref = staged(d_ref), piece.out = staged(d_out), piece.in = c.in.p ? staged(d_in) : RNNoiseStoiPlane{nullptr, 0, 0};
    RnStoiArgs a;
    if (!stoi_plan(&piece, static_cast<double *>(dres.p), scratch.p, scratch_bytes, a)) return -1;
    if (launch(a, nullptr)) return -1;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(results + r0 * RN_STOI_SLOTS, dres.p, rows * RN_STOI_SLOTS * sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}
