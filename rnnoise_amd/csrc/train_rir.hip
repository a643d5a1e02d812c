// train_rir.hip -- room impulse responses for training sequences (include/rnnoise_amd.h: RNNoiseTrainRir; the reference's
// src/dump_features.c:51-144 and :449-465): rnnoise_amd_train_rir_check, rnnoise_amd_train_rir_work_bytes,
// rnnoise_batch_train_rir_load_device, rnnoise_batch_train_rir_device and their five kernels.  DESIGN.md section 4.21.
//
// The reference filters a sequence by overlap-save with 65,536-point kiss_fft transforms (factors 4^8): per block of 32,768 samples
// x = [previous block | this block], X = fft(x), X *= Y * 65536 / 2, y = ifft(X), the block's output is the real second half of y.
// The transform is restated to the bit: every butterfly keeps kf_bfly4's operation order (src/kiss_fft.c:112-131 for m = 1, :139-166
// for the rest), the twiddles are the host libm's.
//
// 65,536 points are two passes of 256 x 256.  With i = 256 k + q the input index, the bit-reversal puts element i at p = 256 r + c with
// c = rev4(k), r = rev4(q) (rev4: the four base-4 digits reversed), so
//   pass 1  (stages m = 1, 4, 16, 64) works inside the run r: the 256 inputs of one residue class q, placed at c = rev4(k);
//   pass 2  (stages m = 256 ... 16384) works on the 256 elements r of one column c, placed at r = rev4(q); twiddles depend on c.
// A workgroup holds 16 neighbouring columns of either pass in LDS as [point][16 columns]; the tile between the passes is stored as
// T[c / 16][q][c % 16], which both sides move in 128-byte pieces.  The product with the RIR's spectrum, the conjugation and the inverse
// transform's bit-reversal need exactly the elements a pass-2 workgroup holds (the inverse's pass 1 for residue class c), so one unit
// -- one (sequence, signal, block) -- takes three launches:
//   rn_rir_fwd1  gather from the frame layout * 1/65536, pass 1                  -> T
//   rn_rir_mid   pass 2, * Y * 65536 / 2, conjugate, permute, pass 1             -> T2
//   rn_rir_inv2  pass 2, real part of the second half, clip, quantise            -> the frame layout
// rn_rir_spec is the pass 2 that ends load_rir (natural order out), rn_rir_finish clips and quantises the unfiltered sequences.
//
// tests/csrc/hip_emul compiles THIS FILE as host C++ against a stand-in for shim.h (tests/test_train_rir_cpu.py, under the address
// sanitizer): a HIP call, a builtin or a member of RNNoiseBatch that this file starts to use needs its counterpart there.
#include "train_common.h"

#include <limits.h>

namespace {
constexpr int NFFT = 65536, HALF = NFFT / 2;        // RIR_FFT_SIZE, the block of overlap-save
constexpr int RUN = 256;                            // points of one pass
constexpr int COLS = 16;                            // columns of a workgroup
constexpr int THREADS = 256;                        // 16 columns x 16: a thread does 4 of the 64 butterflies of its column per stage
constexpr int TILES = RUN / COLS;
constexpr int ROWS = RUN + RUN / 4;                 // LDS rows: point p sits in row p + p / 4 (lds_row)
constexpr int RIR_MAX = HALF;                       // RIR_MAX_DURATION
constexpr size_t UNIT_BYTES = 2 * (size_t)NFFT * sizeof(float2);  // T and T2 of one unit

struct RirLds {
  float re[ROWS * COLS], im[ROWS * COLS];
};

struct RirArgs {
  const float2 *tw;             // [65536] the twiddles of rnn_fft_alloc_twiddles(65536)
  float2 *work;                 // [units of the launch][2][65536]
  // filter
  const RNNoiseTrainRir *rec;   // [n_seq] (the batch's device copy)
  const int *fseq;              // [n_filtered] the sequences with rir_id >= 0, ascending
  const float2 *spectra;        // [n_rirs][2][65536]
  float *clean, *noisy;         // [n_frames][n_seq][480]
  int n_seq, n_frames, n_filtered, n_blocks, unit0;
  // load
  const float *rir;             // one row of d_rir
  float2 *spec_out;             // one [65536] spectrum
  int len, early;
};

struct Cpx {
  float r, i;
};

// C_MUL (src/_kiss_fft_guts.h): four products, two sums, each rounded
__device__ __forceinline__ Cpx c_mul(Cpx a, Cpx b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }

__device__ __forceinline__ int rev4(int k) { return (k & 3) << 6 | (k & 12) << 2 | (k & 48) >> 2 | (k & 192) >> 6; }
// Row of point p: with 16 columns of 4 bytes a row is a quarter of the 64 banks, and the four rows a wave touches at once in any stage
// (four neighbouring butterflies, the same leg) differ mod 4 under this map -- no bank conflict in the butterflies.
__device__ __forceinline__ int lds_row(int p) { return p + (p >> 2); }
// The 16 points a thread moves between global memory and LDS: its wave's four 16-lane groups take points 64 apart, whose rev4 differ
// in the lowest digit (distinct rows mod 4).
__device__ __forceinline__ int move_point(int it) { return ((threadIdx.x >> 4) & 3) * 64 + (threadIdx.x >> 6) * 16 + it; }

// unit u of a filter call: blocks in DESCENDING order (block b reads the original samples of blocks b - 1 and b and overwrites b),
// inside a block the filtered sequences, clean then noisy
struct Unit {
  int seq, sig, blk;
};
__device__ __forceinline__ Unit unit_of(const RirArgs &a, int local) {
  const int u = a.unit0 + local, per = 2 * a.n_filtered;
  const int rem = u % per;
  return {a.fseq[rem >> 1], rem & 1, a.n_blocks - 1 - u / per};
}

// One radix-4 stage over the 256 points of each column: m = 1, 4, 16, 64 is the distance of a butterfly's legs.  t1: the index of the
// first twiddle of butterfly position j inside m (the second and third are 2 t1 and 3 t1); pass 1 at m = 1 is the twiddle-free form.
template <bool HIGH>
__device__ __forceinline__ void stage(RirLds &s, const float2 *tw, int m, int c) {
  const int col = threadIdx.x & 15;
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const int bf = (threadIdx.x >> 4) + 16 * it;
    const int j = bf & (m - 1), p0 = ((bf - j) << 2) + j;
    const int i0 = lds_row(p0) * COLS + col, i1 = lds_row(p0 + m) * COLS + col, i2 = lds_row(p0 + 2 * m) * COLS + col,
              i3 = lds_row(p0 + 3 * m) * COLS + col;
    Cpx f0{s.re[i0], s.im[i0]}, s0{s.re[i1], s.im[i1]}, s1{s.re[i2], s.im[i2]}, s2{s.re[i3], s.im[i3]};
    if (HIGH || m != 1) {
      // pass 1: fstride = 65536 / (4 m); pass 2: the stage is 256 m wide, position j * 256 + c, fstride = 64 / m
      const int t1 = HIGH ? (j * RUN + c) * (64 / m) : j * (NFFT / 4 / m);
      const float2 w1 = tw[t1], w2 = tw[2 * t1], w3 = tw[3 * t1];
      s0 = c_mul(s0, {w1.x, w1.y});
      s1 = c_mul(s1, {w2.x, w2.y});
      s2 = c_mul(s2, {w3.x, w3.y});
    }
    // kf_bfly4, both forms: the same sums in the same order
    const Cpx s5{f0.r - s1.r, f0.i - s1.i};
    f0 = {f0.r + s1.r, f0.i + s1.i};
    const Cpx s3{s0.r + s2.r, s0.i + s2.i}, s4{s0.r - s2.r, s0.i - s2.i};
    s.re[i2] = f0.r - s3.r;
    s.im[i2] = f0.i - s3.i;
    s.re[i0] = f0.r + s3.r;
    s.im[i0] = f0.i + s3.i;
    s.re[i1] = s5.r + s4.i;
    s.im[i1] = s5.i - s4.r;
    s.re[i3] = s5.r - s4.i;
    s.im[i3] = s5.i + s4.r;
  }
  __syncthreads();
}

// the four stages of a pass on the tile in LDS (a barrier before and after); c0: the tile's first column (pass 2)
template <bool HIGH>
__device__ __forceinline__ void pass(RirLds &s, const float2 *tw, int c0) {
  __syncthreads();
  const int c = c0 + (threadIdx.x & 15);
  stage<HIGH>(s, tw, 1, c);
  stage<HIGH>(s, tw, 4, c);
  stage<HIGH>(s, tw, 16, c);
  stage<HIGH>(s, tw, 64, c);
}

// after pass 1 of residue classes q0 .. q0 + 15: LDS [c][q - q0] -> T[c / 16][q][c % 16]
__device__ __forceinline__ void store_tile(const RirLds &s, float2 *T, int q0) {
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4;
  for (int ct = 0; ct < TILES; ct++) {
    const int i = lds_row(ct * COLS + cl) * COLS + q;
    T[((size_t)ct * RUN + q0 + q) * COLS + cl] = make_float2(s.re[i], s.im[i]);
  }
}

// before pass 2 of columns 16 ct .. 16 ct + 15: T[ct][q][c % 16] -> LDS [rev4(q)][c % 16]
__device__ __forceinline__ void load_tile(RirLds &s, const float2 *T, int ct) {
  const int col = threadIdx.x & 15;
  for (int it = 0; it < 16; it++) {
    const int q = move_point(it);
    const float2 v = T[((size_t)ct * RUN + q) * COLS + col];
    const int i = lds_row(rev4(q)) * COLS + col;
    s.re[i] = v.x;
    s.im[i] = v.y;
  }
}

// sample s of a (sequence, signal) in the frame layout; 0 outside the sequence
__device__ __forceinline__ size_t frame_at(const RirArgs &a, int seq, unsigned s) {
  const unsigned f = s / RN_FRAME_SIZE;
  return ((size_t)f * a.n_seq + seq) * RN_FRAME_SIZE + (s - f * RN_FRAME_SIZE);
}
}  // namespace

// (tests/test_product_surface_cpu.py and tests/test_kernel_budgets_cpu.py pin the kernels of this file by name)
// grid: units * 16; LOAD: one RIR in one form (load_rir, :63-88), else a unit's [previous block | block]
extern "C" __global__ __launch_bounds__(THREADS) void rn_rir_fwd1(RirArgs a) {
  __shared__ RirLds s;
  const int local = blockIdx.x / TILES, q0 = (blockIdx.x % TILES) * COLS, col = threadIdx.x & 15;
  const float scale = 1.f / NFFT;
  const bool load = a.rir != nullptr;
  Unit u{};
  const float *audio = nullptr;
  if (!load) {
    u = unit_of(a, local);
    audio = u.sig ? a.noisy : a.clean;
  }
  const int total = a.n_frames * RN_FRAME_SIZE;
  for (int it = 0; it < 16; it++) {
    const int k = move_point(it), i = k * RUN + q0 + col;
    float v = 0.f;
    if (load) {
      if (i < a.len) {
        v = a.rir[i];
        if (a.early) {
          if (i >= 720) v = 0.f;
          else if (i >= 480) v *= (1 - (i - 480) / 240.f);
        }
      }
    } else {
      const int at = (u.blk - 1) * HALF + i;  // x = [previous block | this block]: one run of the signal
      if (at >= 0 && at < total) v = audio[frame_at(a, u.seq, (unsigned)at)];
    }
    const int at = lds_row(rev4(k)) * COLS + col;
    s.re[at] = scale * v;
    s.im[at] = scale * 0.f;
  }
  pass<false>(s, a.tw, 0);
  store_tile(s, a.work + (size_t)local * 2 * NFFT, q0);
}

// grid: 16; the second pass of load_rir's transform, natural order out
extern "C" __global__ __launch_bounds__(THREADS) void rn_rir_spec(RirArgs a) {
  __shared__ RirLds s;
  const int c0 = blockIdx.x * COLS, col = threadIdx.x & 15;
  load_tile(s, a.work, blockIdx.x);
  pass<true>(s, a.tw, c0);
  for (int it = 0; it < 16; it++) {
    const int r = (threadIdx.x >> 4) + 16 * it, i = lds_row(r) * COLS + col;
    a.spec_out[r * RUN + c0 + col] = make_float2(s.re[i], s.im[i]);
  }
}

// grid: units * 16
extern "C" __global__ __launch_bounds__(THREADS) void rn_rir_mid(RirArgs a) {
  __shared__ RirLds s;
  const int local = blockIdx.x / TILES, ct = blockIdx.x % TILES, c0 = ct * COLS, col = threadIdx.x & 15;
  const Unit u = unit_of(a, local);
  float2 *T = a.work + (size_t)local * 2 * NFFT;
  // (:449-452: the early response on the clean signal, the whole one on the noisy signal)
  const float2 *Y = a.spectra + ((size_t)a.rec[u.seq].rir_id * 2 + (u.sig ? 0 : 1)) * NFFT;
  load_tile(s, T, ct);
  pass<true>(s, a.tw, c0);
  // X[p] * Y[p] * 65536 / 2 at p = 256 r + c (:134-139); rnn_ifft_c: to bitrev[p], which is point rev4(r) of residue class c, .i negated
  Cpx x[16];
  for (int it = 0; it < 16; it++) {
    const int r = move_point(it), i = lds_row(r) * COLS + col;
    const float2 y = Y[r * RUN + c0 + col];
    const Cpx t = c_mul({s.re[i], s.im[i]}, {y.x, y.y});
    x[it] = {t.r * (float)NFFT / 2, -(t.i * (float)NFFT / 2)};
  }
  __syncthreads();
  for (int it = 0; it < 16; it++) {
    const int i = lds_row(rev4(move_point(it))) * COLS + col;
    s.re[i] = x[it].r;
    s.im[i] = x[it].i;
  }
  pass<false>(s, a.tw, 0);
  store_tile(s, T + NFFT, c0);
}

// grid: units * 16
extern "C" __global__ __launch_bounds__(THREADS) void rn_rir_inv2(RirArgs a) {
  __shared__ RirLds s;
  const int local = blockIdx.x / TILES, ct = blockIdx.x % TILES, c0 = ct * COLS, col = threadIdx.x & 15;
  const Unit u = unit_of(a, local);
  load_tile(s, a.work + (size_t)local * 2 * NFFT + NFFT, ct);
  pass<true>(s, a.tw, c0);
  // audio[i + j] = y[32768 + j].r (:141; the last negation of .i does not reach it), then :457 and :463 on the noisy signal
  const int clip = u.sig ? a.rec[u.seq].clip : 0, quantize = u.sig ? a.rec[u.seq].quantize : 0;
  float *audio = u.sig ? a.noisy : a.clean;
  const int total = a.n_frames * RN_FRAME_SIZE;
  for (int it = 0; it < 8; it++) {
    const int r = RUN / 2 + (threadIdx.x >> 4) + 16 * it;
    const int at = u.blk * HALF + (r - RUN / 2) * RUN + c0 + col;
    if (at < total) audio[frame_at(a, u.seq, (unsigned)at)] = clip_quantize(s.re[lds_row(r) * COLS + col], clip, quantize);
  }
}

// grid: n_frames * n_seq, 128 threads: :457 and :463 on the noisy signal of the sequences that are not filtered
extern "C" __global__ __launch_bounds__(128) void rn_rir_finish(RirArgs a) {
  const RNNoiseTrainRir rec = a.rec[blockIdx.x % a.n_seq];
  if (rec.rir_id >= 0 || !(rec.clip | rec.quantize) || threadIdx.x >= RN_FRAME_SIZE / 4) return;
  float4 *p = reinterpret_cast<float4 *>(a.noisy + (size_t)blockIdx.x * RN_FRAME_SIZE) + threadIdx.x;
  const float4 v = *p;
  *p = make_float4(clip_quantize(v.x, rec.clip, rec.quantize), clip_quantize(v.y, rec.clip, rec.quantize),
                   clip_quantize(v.z, rec.clip, rec.quantize), clip_quantize(v.w, rec.clip, rec.quantize));
}

// ---- host ----
extern "C" int rnnoise_amd_train_rir_check(const RNNoiseTrainRir *rir, int n_seq, int n_rirs) {
  if (!rir || n_seq < 1 || n_rirs < 0) return 0;
  for (int s = 0; s < n_seq; s++) {
    const RNNoiseTrainRir &p = rir[s];
    if (p.rir_id < -1 || p.rir_id >= n_rirs) return 0;
    if (!train_flag01(p.clip) || !train_flag01(p.quantize)) return 0;
  }
  return 1;
}

extern "C" long long rnnoise_amd_train_rir_work_bytes(long long n_units) { return n_units < 1 ? 0 : n_units * (long long)UNIT_BYTES; }

namespace {
// The batch's twiddle table, followed by one transform of scratch for rnnoise_batch_train_rir_load_device: built on first use.
// compute_twiddles (src/kiss_fft.c:406-421): the phase in double with the reference's literal of pi, cos and sin of the host's libm.
int twiddles(RNNoiseBatch *b, hipStream_t st) {
  if (b->train_rir_tw) return 0;
  std::vector<float> tw(2 * (size_t)NFFT);
  for (int i = 0; i < NFFT; i++) {
    const double pi = 3.14159265358979323846264338327;
    const double phase = (-2 * pi / NFFT) * i;
    tw[2 * i] = (float)cos(phase);
    tw[2 * i + 1] = (float)sin(phase);
  }
  return train_upload(&b->train_rir_tw, 2 * (size_t)NFFT * sizeof(float2), tw.data(), (size_t)NFFT * sizeof(float2), st);
}

// What both device calls do around their launches: on the batch's device and the caller's stream, the twiddles in place and in `a`.
template <typename Launches>
int rir_call(RNNoiseBatch *b, void *hip_stream, Launches launches) {
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  if (twiddles(b, st)) return -1;
  RirArgs a{};
  a.tw = static_cast<const float2 *>(b->train_rir_tw);
  if (launches(a, st)) return -1;
  HIP_OK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_train_rir_load_device(RNNoiseBatch *b, float *d_spectra, const float *d_rir, const int *lens, int n_rirs,
                                                   void *hip_stream) {
  if (!b || !d_spectra || !d_rir || !lens || n_rirs < 1) return -1;
  if (train_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!aligned16(d_spectra) || !aligned16(d_rir)) return -1;
  for (int r = 0; r < n_rirs; r++)
    if (lens[r] < 1 || lens[r] > RIR_MAX) return -1;
  return rir_call(b, hip_stream, [&](RirArgs &a, hipStream_t st) {
    a.work = static_cast<float2 *>(b->train_rir_tw) + NFFT;  // (one transform at a time: the launches of a stream run in order)
    for (int r = 0; r < n_rirs; r++)
      for (int early = 0; early < 2; early++) {
        a.rir = d_rir + (size_t)r * RIR_MAX;
        a.len = lens[r];
        a.early = early;
        a.spec_out = reinterpret_cast<float2 *>(d_spectra) + ((size_t)r * 2 + early) * NFFT;
        hipLaunchKernelGGL(rn_rir_fwd1, dim3(TILES), dim3(THREADS), 0, st, a);
        hipLaunchKernelGGL(rn_rir_spec, dim3(TILES), dim3(THREADS), 0, st, a);
      }
    return 0;
  });
}

extern "C" int rnnoise_batch_train_rir_device(RNNoiseBatch *b, float *d_clean, float *d_noisy, const float *d_spectra, int n_rirs,
                                              const RNNoiseTrainRir *rir, void *d_work, long long work_bytes, int n_frames,
                                              void *hip_stream) {
  if (!b || !d_clean || !d_noisy || !d_spectra || !rir || !d_work) return -1;
  if (train_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (n_frames < 1 || n_frames > (INT_MAX - NFFT) / RN_FRAME_SIZE || work_bytes < (long long)UNIT_BYTES) return -1;
  if (!aligned16(d_clean) || !aligned16(d_noisy) || !aligned16(d_spectra) || !aligned16(d_work)) return -1;
  if (!rnnoise_amd_train_rir_check(rir, b->n, n_rirs)) return -1;
  // the records and the list of filtered sequences, in one buffer of the batch and one copy
  const int n = b->n;
  std::vector<int> table(4 * (size_t)n);
  memcpy(table.data(), rir, sizeof(RNNoiseTrainRir) * n);
  int n_filtered = 0, finish = 0;
  for (int s = 0; s < n; s++) {
    if (rir[s].rir_id >= 0) table[3 * (size_t)n + n_filtered++] = s;
    else finish |= rir[s].clip | rir[s].quantize;
  }
  const int n_blocks = (int)(((long long)n_frames * RN_FRAME_SIZE + HALF - 1) / HALF);
  const long long units = (long long)n_blocks * 2 * n_filtered;
  if (units > INT_MAX || (long long)n_frames * n > INT_MAX) return -1;  // (a unit index and the grid of rn_rir_finish are ints)
  return rir_call(b, hip_stream, [&](RirArgs &a, hipStream_t st) {
    const size_t bytes = table.size() * sizeof(int);
    if (train_upload(&b->train_rir_buf, bytes, table.data(), bytes, st)) return -1;
    a.work = static_cast<float2 *>(d_work);
    a.rec = static_cast<const RNNoiseTrainRir *>(b->train_rir_buf);
    a.fseq = static_cast<const int *>(b->train_rir_buf) + 3 * (size_t)n;
    a.spectra = reinterpret_cast<const float2 *>(d_spectra);
    a.clean = d_clean;
    a.noisy = d_noisy;
    a.n_seq = n;
    a.n_frames = n_frames;
    a.n_filtered = n_filtered;
    a.n_blocks = n_blocks;
    if (finish) hipLaunchKernelGGL(rn_rir_finish, dim3((unsigned)n_frames * n), dim3(128), 0, st, a);
    // Slabs of as many units as the workspace holds, blocks descending: a slab's loads (fwd1) all precede its stores (inv2), and a
    // later slab reads only blocks that no earlier one wrote for the same signal.
    const long long slab = std::min<long long>(work_bytes / (long long)UNIT_BYTES, INT_MAX / TILES);
    for (long long u0 = 0; u0 < units; u0 += slab) {
      const unsigned grid = (unsigned)(std::min(slab, units - u0) * TILES);
      a.unit0 = (int)u0;
      hipLaunchKernelGGL(rn_rir_fwd1, dim3(grid), dim3(THREADS), 0, st, a);
      hipLaunchKernelGGL(rn_rir_mid, dim3(grid), dim3(THREADS), 0, st, a);
      hipLaunchKernelGGL(rn_rir_inv2, dim3(grid), dim3(THREADS), 0, st, a);
    }
    return 0;
  });
}
