// state_kernels.hip -- portable per-stream state (include/rn_layout.h: the 25,128 live bytes of the reference's
// DenoiseState, src/denoise.c:68-88) <-> the batch's structure-of-arrays layout (rn_dev.h), on the device.
// One launch moves `g.n_streams` states (a 1024-thread workgroup each: the per-word field dispatch is latency, 17 us with 256
// threads); the host side needs one memcpy per direction instead of one per field.  The same two kernels have a bulk form for
// snapshots of many streams (rows > 0), which is a copy loop per field.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rn_dev.h"

// ---- the bulk forms: snapshots (include/rn_layout.h: RN_SNAP_*) of many streams, by list, at each stream's own frame phase ----
// rnnoise_batch_save_streams / load_streams move 26.5 KB per stream for up to 65,536 streams, so their body is a copy, not a
// dispatch: every field is one contiguous run in the record and one in the batch's arrays (the pitch ring: at most two on each side
// of its wrap, and RN_RING0 is a multiple of 96 floats), and a run moves at the widest access both of its ends are aligned for.
// Record rows are 16-byte aligned (RN_SNAP_FLOATS % 4 == 0), but the portable layout puts conv2_state (word 2854), the GRU states
// (3110), delayed_X (4262) and the band energies (6186) on 8-byte boundaries only, and conv1_state rows (130 floats) alternate: the
// width is chosen per run, 16, 8 or 4 bytes per lane.  One workgroup of RN_SNAP_THREADS lanes per row, RN_SNAP_GRID_CAP workgroups
// at the most (DESIGN 4.14 has the measurements behind the two).
#ifndef RN_SNAP_THREADS
#define RN_SNAP_THREADS 256
#endif
#ifndef RN_SNAP_GRID_CAP
#define RN_SNAP_GRID_CAP 65536
#endif
static_assert(RN_SNAP_HIST_FLOATS == RN_RS_HIST && RN_SNAP_GATE_NONE == RN_CTL_NONE, "the record and the kernels agree");
static_assert(RN_SNAP_FLOATS % 4 == 0 && RN_SNAP_OFF_HIST % 4 == 0 && RN_OFF_PITCH_BUF % 4 == 0, "16-byte rows and runs");
static_assert(RN_RING0(1) % 4 == 0 && RN_FRAME_SIZE % 4 == 0 && RN_PITCH_BUF_SIZE % 4 == 0, "ring runs are 16-byte aligned");
namespace {
// n floats, src -> dst, by the workgroup (both pointers uniform)
__device__ __forceinline__ void move_run(float *__restrict__ dst, const float *__restrict__ src, int n) {
  const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src));
  const int t = threadIdx.x, nt = blockDim.x;
  if (!(a & 15)) {
    for (int i = t; i < (n >> 2); i += nt) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
    for (int i = (n & ~3) + t; i < n; i += nt) dst[i] = src[i];
  } else if (!(a & 7)) {
    for (int i = t; i < (n >> 1); i += nt) reinterpret_cast<float2 *>(dst)[i] = reinterpret_cast<const float2 *>(src)[i];
    for (int i = (n & ~1) + t; i < n; i += nt) dst[i] = src[i];
  } else {
    for (int i = t; i < n; i += nt) dst[i] = src[i];
  }
}
__device__ __forceinline__ void zero_run(float *__restrict__ dst, int n) {
  const int t = threadIdx.x, nt = blockDim.x;
  if (!(reinterpret_cast<uintptr_t>(dst) & 15)) {
    for (int i = t; i < (n >> 2); i += nt) reinterpret_cast<float4 *>(dst)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = (n & ~3) + t; i < n; i += nt) dst[i] = 0.f;
  } else {
    for (int i = t; i < n; i += nt) dst[i] = 0.f;
  }
}
// slot k of a rotating plane set (a select, not an indexed read of the kernel's arguments)
__device__ __forceinline__ float *slot3(float *const (&a)[RN_SPEC_SLOTS], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : a[2]; }
// the slots that hold stream s's latest frame: from its own phase (per-stream mode) or from the launch (lock-step)
__device__ __forceinline__ void latest_slots(const int *__restrict__ phase, int s, int &newest_slot, int &last) {
  if (!phase) return;
  const unsigned p = (unsigned)phase[s] % RN_RING_SLOTS;
  newest_slot = (p + RN_RING_SLOTS - 1) % RN_RING_SLOTS;
  last = (p + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
}

// the divisor stream s's resampler history belongs to: the batch's (1 at 48 kHz), or the stream's own where the batch has a rate table
// (rn_dev.h: RnGroupDev::rs_Ls)
__device__ __forceinline__ int stream_L(const RnGroupDev &g, int s) { return g.rs_L ? rn_stream_L(g, s) : 1; }

// snap[row][RN_SNAP_FLOATS] <- stream list[row] (row, without a list); an entry outside the view leaves an empty record (magic 0)
__device__ __forceinline__ void gather_rows(const RnGroupDev &g, float *__restrict__ snap, int newest_arg, int last_arg,
                                            const int *__restrict__ list, const int *__restrict__ phase, int rows) {
  const size_t N = g.n_stride;
  const int t = threadIdx.x;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    float *f = snap + (size_t)row * RN_SNAP_FLOATS;
    const int sl = list ? list[row] : row;
    if (sl < 0 || sl >= g.n_streams) {
      if (t == 0) f[RN_SNAP_OFF_MAGIC] = __int_as_float(0);
      continue;
    }
    const size_t s = sl;
    int newest_slot = newest_arg, last = last_arg;
    latest_slots(phase, sl, newest_slot, last);
    const float *ring = g.pitch_ring + s * RN_RING_SIZE;
    const int ring0 = RN_RING0(newest_slot), n1 = min(RN_PITCH_BUF_SIZE, RN_RING_SIZE - ring0);
    move_run(f + RN_OFF_ANALYSIS, ring + newest_slot * RN_FRAME_SIZE, RN_FRAME_SIZE);  // analysis_mem = tail of pitch_buf = the newest slot
    move_run(f + RN_OFF_SYNTHESIS, g.synth_mem + s * RN_FRAME_SIZE, RN_FRAME_SIZE);
    move_run(f + RN_OFF_PITCH_BUF, ring + ring0, n1);
    if (n1 < RN_PITCH_BUF_SIZE) move_run(f + RN_OFF_PITCH_BUF + n1, ring, RN_PITCH_BUF_SIZE - n1);
    if (t == 0) f[RN_OFF_LAST_GAIN] = g.last_gain[s];
    if (t == 1) f[RN_OFF_LAST_PERIOD] = __int_as_float(g.last_period[s]);
    if (t >= 2 && t < 4) f[RN_OFF_MEM_HP + t - 2] = g.mem_hp[2 * s + t - 2];
    move_run(f + RN_OFF_LASTG, g.lastg + s * RN_NB_BANDS, RN_NB_BANDS);
    move_run(f + RN_OFF_CONV1, g.conv1_state + s * 130, 130);
    move_run(f + RN_OFF_CONV2, g.conv2_state + s * 256, 256);
    for (int k = 0; k < 3; k++) move_run(f + RN_OFF_GRU1 + k * RN_GRU, g.gru_state + (k * N + s) * RN_GRU, RN_GRU);
    move_run(f + RN_OFF_DELAYED_X, slot3(g.spec_X, last) + s * RN_SPEC_STRIDE, RN_OFF_DELAYED_P - RN_OFF_DELAYED_X);
    move_run(f + RN_OFF_DELAYED_P, slot3(g.spec_P, last) + s * RN_SPEC_STRIDE, RN_OFF_DELAYED_EX - RN_OFF_DELAYED_P);
    move_run(f + RN_OFF_DELAYED_EX, slot3(g.spec_E, last) + s * 96, 96);
    if (t >= 64 && t < 70) {  // the header: magic, L, counter, three reserved zeros
      const int w = t - 64;
      const int v = w == 0 ? RN_SNAP_MAGIC : w == 1 ? stream_L(g, sl) : w == 2 ? (g.gate_c ? g.gate_c[s] : RN_CTL_NONE) : 0;
      f[RN_SNAP_OFF_MAGIC + w] = __int_as_float(v);
    }
    if (g.rs_hist) move_run(f + RN_SNAP_OFF_HIST, g.rs_hist + s * RN_RS_HIST, RN_RS_HIST);
    else zero_run(f + RN_SNAP_OFF_HIST, RN_RS_HIST);
  }
}

// stream list[row] <- snap[row][RN_SNAP_FLOATS]: what the one-state form below writes, at the stream's own phase, then the
// resampler history (when the record's L is the stream's current one; zeros otherwise) and the gate counter (when the view has one).  A row with
// another magic word, or an entry outside the view, touches nothing.
__device__ __forceinline__ void scatter_rows(const RnGroupDev &g, const float *__restrict__ snap, int newest_arg, int last_arg,
                                             const int *__restrict__ list, const int *__restrict__ phase, int rows) {
  const size_t N = g.n_stride;
  const int t = threadIdx.x, nt = blockDim.x;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const float *f = snap + (size_t)row * RN_SNAP_FLOATS;
    const int sl = list ? list[row] : row;
    if (sl < 0 || sl >= g.n_streams || __float_as_int(f[RN_SNAP_OFF_MAGIC]) != RN_SNAP_MAGIC) continue;
    const size_t s = sl;
    int newest_slot = newest_arg, last = last_arg;
    latest_slots(phase, sl, newest_slot, last);
    float *ring = g.pitch_ring + s * RN_RING_SIZE;
    const float *pb = f + RN_OFF_PITCH_BUF;
    // pitch_buf at ring0 (two runs where it wraps); the RN_RING_SIZE - RN_PITCH_BUF_SIZE positions behind it are zeroed
    const int ring0 = RN_RING0(newest_slot), n1 = min(RN_PITCH_BUF_SIZE, RN_RING_SIZE - ring0);
    move_run(ring + ring0, pb, n1);
    if (n1 < RN_PITCH_BUF_SIZE) move_run(ring, pb + n1, RN_PITCH_BUF_SIZE - n1);
    const int z0 = (ring0 + RN_PITCH_BUF_SIZE) % RN_RING_SIZE, nz = RN_RING_SIZE - RN_PITCH_BUF_SIZE, z1 = min(nz, RN_RING_SIZE - z0);
    zero_run(ring + z0, z1);
    if (z1 < nz) zero_run(ring, nz - z1);
    // the decimated ring (rn_dev.h: RN_XRING_SLOT), two samples per lane from the RECORD's pitch_buf: ring position 2q is pitch_buf
    // index j = 2q - ring0 (mod the ring), a multiple of 4 for even q, so j .. j+3 is one aligned float4 that lies wholly inside
    // pitch_buf or wholly in the zeroed part; j - 1 is the one word outside it
    float *xring = g.xlp_ring + s * RN_XRING_SIZE;
    for (int q = 2 * t; q < RN_XRING_SIZE; q += 2 * nt) {
      int j = 2 * q - ring0;
      j += j < 0 ? RN_RING_SIZE : 0;
      const int jm = j ? j - 1 : RN_RING_SIZE - 1;
      const float4 v = j < RN_PITCH_BUF_SIZE ? *reinterpret_cast<const float4 *>(pb + j) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float m = jm < RN_PITCH_BUF_SIZE ? pb[jm] : 0.f;
      // (the word after the float4, j + 4, belongs to sample q + 2: not needed here)
      float2 o;
      o.x = .5f * (.5f * (m + v.y) + v.x);
      o.y = .5f * (.5f * (v.y + v.w) + v.z);
      *reinterpret_cast<float2 *>(xring + q) = o;
    }
    move_run(g.synth_mem + s * RN_FRAME_SIZE, f + RN_OFF_SYNTHESIS, RN_FRAME_SIZE);
    if (t == 0) g.last_gain[s] = f[RN_OFF_LAST_GAIN];
    if (t == 1) g.last_period[s] = __float_as_int(f[RN_OFF_LAST_PERIOD]);
    if (t >= 2 && t < 4) g.mem_hp[2 * s + t - 2] = f[RN_OFF_MEM_HP + t - 2];
    move_run(g.lastg + s * RN_NB_BANDS, f + RN_OFF_LASTG, RN_NB_BANDS);
    move_run(g.conv1_state + s * 130, f + RN_OFF_CONV1, 130);
    move_run(g.conv2_state + s * 256, f + RN_OFF_CONV2, 256);
    for (int k = 0; k < 3; k++) move_run(g.gru_state + (k * N + s) * RN_GRU, f + RN_OFF_GRU1 + k * RN_GRU, RN_GRU);
    move_run(slot3(g.spec_X, last) + s * RN_SPEC_STRIDE, f + RN_OFF_DELAYED_X, RN_OFF_DELAYED_P - RN_OFF_DELAYED_X);
    move_run(slot3(g.spec_P, last) + s * RN_SPEC_STRIDE, f + RN_OFF_DELAYED_P, RN_OFF_DELAYED_EX - RN_OFF_DELAYED_P);
    move_run(slot3(g.spec_E, last) + s * 96, f + RN_OFF_DELAYED_EX, 96);
    if (g.rs_hist) {
      if (__float_as_int(f[RN_SNAP_OFF_L]) == stream_L(g, sl)) move_run(g.rs_hist + s * RN_RS_HIST, f + RN_SNAP_OFF_HIST, RN_RS_HIST);
      else zero_run(g.rs_hist + s * RN_RS_HIST, RN_RS_HIST);
    }
    if (g.gate_c && t == 64) g.gate_c[s] = min(max(__float_as_int(f[RN_SNAP_OFF_GATE]), 0), RN_CTL_NONE);
  }
}
}  // namespace

// flat[s][RN_STATE_FLOATS] <- stream s of the view.  newest_slot = pitch-ring slot of the latest frame,
// last = spectra slot of the latest frame (the reference's delayed_*).
extern "C" __global__ void __launch_bounds__(1024)
rn_state_gather_kernel(RnGroupDev g, float *__restrict__ flat, int newest_slot, int last, const int *__restrict__ list,
                       const int *__restrict__ phase, int rows) {
  // rows > 0: the bulk form -- flat is [rows][RN_SNAP_FLOATS], row i is stream list[i] (stream i without a list) at the frame phase
  // phase[stream] (the launch's slots without `phase`)
  if (rows > 0) return gather_rows(g, flat, newest_slot, last, list, phase, rows);
  const size_t s = blockIdx.x, N = g.n_stride;
  float *f = flat + s * RN_STATE_FLOATS;
  const int ring0 = RN_RING0(newest_slot);
  const float *ring = g.pitch_ring + s * RN_RING_SIZE;
  for (int w = threadIdx.x; w < RN_STATE_FLOATS; w += blockDim.x) {
    float v;
    if (w < RN_OFF_SYNTHESIS) v = ring[(ring0 + (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE) + w) % RN_RING_SIZE];  // analysis_mem = tail of pitch_buf
    else if (w < RN_OFF_PITCH_BUF) v = g.synth_mem[s * RN_FRAME_SIZE + (w - RN_OFF_SYNTHESIS)];
    else if (w < RN_OFF_LAST_GAIN) v = ring[(ring0 + (w - RN_OFF_PITCH_BUF)) % RN_RING_SIZE];
    else if (w == RN_OFF_LAST_GAIN) v = g.last_gain[s];
    else if (w == RN_OFF_LAST_PERIOD) v = __int_as_float(g.last_period[s]);
    else if (w < RN_OFF_LASTG) v = g.mem_hp[2 * s + (w - RN_OFF_MEM_HP)];
    else if (w < RN_OFF_CONV1) v = g.lastg[s * RN_NB_BANDS + (w - RN_OFF_LASTG)];
    else if (w < RN_OFF_CONV2) v = g.conv1_state[s * 130 + (w - RN_OFF_CONV1)];
    else if (w < RN_OFF_GRU1) v = g.conv2_state[s * 256 + (w - RN_OFF_CONV2)];
    else if (w < RN_OFF_DELAYED_X) {
      const int k = (w - RN_OFF_GRU1) / RN_GRU, i = (w - RN_OFF_GRU1) % RN_GRU;
      v = g.gru_state[(k * N + s) * RN_GRU + i];
    } else if (w < RN_OFF_DELAYED_P) v = g.spec_X[last][s * RN_SPEC_STRIDE + (w - RN_OFF_DELAYED_X)];
    else if (w < RN_OFF_DELAYED_EX) v = g.spec_P[last][s * RN_SPEC_STRIDE + (w - RN_OFF_DELAYED_P)];
    else v = g.spec_E[last][s * 96 + (w - RN_OFF_DELAYED_EX)];
    f[w] = v;
  }
}

// stream s of the view <- flat[s][RN_STATE_FLOATS] (analysis_mem is implied by pitch_buf and not stored).
// g.rs_hist set: the stream's resampler histories are zeroed too; g.gate_c set: the stream's counter restarts at RN_CTL_NONE.
// list (optional): block b works on stream list[b] instead of stream b; entries outside the view are ignored.  flat == null: the zero
// state of rnnoise_init() -- every slot of the two rings and of the spectra, whatever the stream's frame phase.
// rows > 0: the bulk form -- flat is [rows][RN_SNAP_FLOATS] (scatter_rows above).
extern "C" __global__ void __launch_bounds__(1024)
rn_state_scatter_kernel(RnGroupDev g, const float *__restrict__ flat, int newest_slot, int last, const int *__restrict__ list,
                        const int *__restrict__ phase, int rows) {
  if (rows > 0) return scatter_rows(g, flat, newest_slot, last, list, phase, rows);
  const int sl = list ? list[blockIdx.x] : (int)blockIdx.x;
  if (sl < 0 || sl >= g.n_streams) return;
  const size_t s = sl, N = g.n_stride;
  // the resampler histories (rn_dev.h: rs_hist) restart from zero on a reset and on an import: the portable state carries none
  if (g.rs_hist)
    for (int i = threadIdx.x; i < RN_RS_HIST; i += blockDim.x) g.rs_hist[s * RN_RS_HIST + i] = 0.f;
  // ... and so does the counter of the suppression controls (rn_dev.h: gate_c): no voice frame yet
  if (g.gate_c && threadIdx.x == 0) g.gate_c[s] = RN_CTL_NONE;
  if (!flat) {
    auto zero = [](float *p, int n) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0.f;
    };
    zero(g.pitch_ring + s * RN_RING_SIZE, RN_RING_SIZE);
    zero(g.xlp_ring + s * RN_XRING_SIZE, RN_XRING_SIZE);
    zero(g.synth_mem + s * RN_FRAME_SIZE, RN_FRAME_SIZE);
    zero(g.mem_hp + 2 * s, 2);
    zero(g.lastg + s * RN_NB_BANDS, RN_NB_BANDS);
    zero(g.last_gain + s, 1);
    zero(g.conv1_state + s * 130, 130);
    zero(g.conv2_state + s * 256, 256);
    for (int k = 0; k < 3; k++) zero(g.gru_state + (k * N + s) * RN_GRU, RN_GRU);
    for (int k = 0; k < RN_SPEC_SLOTS; k++) {
      zero(g.spec_X[k] + s * RN_SPEC_STRIDE, RN_SPEC_STRIDE);
      zero(g.spec_P[k] + s * RN_SPEC_STRIDE, RN_SPEC_STRIDE);
      zero(g.spec_E[k] + s * 96, 96);
    }
    if (threadIdx.x == 0) g.last_period[s] = 0;
    return;
  }
  const float *f = flat + s * RN_STATE_FLOATS;
  const int ring0 = RN_RING0(newest_slot);
  float *ring = g.pitch_ring + s * RN_RING_SIZE;
  for (int p = threadIdx.x; p < RN_RING_SIZE; p += blockDim.x) {  // the 1152 ring positions outside pitch_buf are zeroed
    const int i = (p - ring0 + RN_RING_SIZE) % RN_RING_SIZE;
    ring[p] = i < RN_PITCH_BUF_SIZE ? f[RN_OFF_PITCH_BUF + i] : 0.f;
  }
  // the decimated ring is derived data (rn_dev.h: RN_XRING_SLOT): sample q = the high-pass kernel's expression over ring positions
  // 2q-1, 2q, 2q+1 as just written (zeros outside pitch_buf)
  float *xring = g.xlp_ring + s * RN_XRING_SIZE;
  auto at = [&](int p) {
    const int i = (p - ring0 + 2 * RN_RING_SIZE) % RN_RING_SIZE;
    return i < RN_PITCH_BUF_SIZE ? f[RN_OFF_PITCH_BUF + i] : 0.f;
  };
  for (int q = threadIdx.x; q < RN_XRING_SIZE; q += blockDim.x) xring[q] = .5f * (.5f * (at(2 * q - 1) + at(2 * q + 1)) + at(2 * q));
  for (int w = RN_OFF_SYNTHESIS + threadIdx.x; w < RN_STATE_FLOATS; w += blockDim.x) {
    const float v = f[w];
    if (w < RN_OFF_PITCH_BUF) g.synth_mem[s * RN_FRAME_SIZE + (w - RN_OFF_SYNTHESIS)] = v;
    else if (w < RN_OFF_LAST_GAIN) continue;
    else if (w == RN_OFF_LAST_GAIN) g.last_gain[s] = v;
    else if (w == RN_OFF_LAST_PERIOD) g.last_period[s] = __float_as_int(v);
    else if (w < RN_OFF_LASTG) g.mem_hp[2 * s + (w - RN_OFF_MEM_HP)] = v;
    else if (w < RN_OFF_CONV1) g.lastg[s * RN_NB_BANDS + (w - RN_OFF_LASTG)] = v;
    else if (w < RN_OFF_CONV2) g.conv1_state[s * 130 + (w - RN_OFF_CONV1)] = v;
    else if (w < RN_OFF_GRU1) g.conv2_state[s * 256 + (w - RN_OFF_CONV2)] = v;
    else if (w < RN_OFF_DELAYED_X) {
      const int k = (w - RN_OFF_GRU1) / RN_GRU, i = (w - RN_OFF_GRU1) % RN_GRU;
      g.gru_state[(k * N + s) * RN_GRU + i] = v;
    } else if (w < RN_OFF_DELAYED_P) g.spec_X[last][s * RN_SPEC_STRIDE + (w - RN_OFF_DELAYED_X)] = v;
    else if (w < RN_OFF_DELAYED_EX) g.spec_P[last][s * RN_SPEC_STRIDE + (w - RN_OFF_DELAYED_P)] = v;
    else g.spec_E[last][s * 96 + (w - RN_OFF_DELAYED_EX)] = v;
  }
}

extern "C" hipError_t rn_launch_state_gather(const RnGroupDev *g, float *flat, int newest_slot, int last, hipStream_t st) {
  hipLaunchKernelGGL(rn_state_gather_kernel, dim3(g->n_streams), dim3(1024), 0, st, *g, flat, newest_slot, last, nullptr, nullptr, 0);
  return hipGetLastError();
}
extern "C" hipError_t rn_launch_state_scatter(const RnGroupDev *g, const float *flat, int newest_slot, int last, hipStream_t st,
                                              const int *list, int n) {
  // (list: n stream indices of the view, one block each; otherwise one block per stream of the view)
  if (list && n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rn_state_scatter_kernel, dim3(list ? n : g->n_streams), dim3(1024), 0, st, *g, flat, newest_slot, last, list,
                     nullptr, 0);
  return hipGetLastError();
}
// The bulk forms: `rows` snapshot records, row i <-> stream list[i] (stream i when list is null).  p: the frame phase of a lock-step
// batch (the ring slot its next frame writes); phase: the per-stream phases on the device, which then take p's place.
extern "C" hipError_t rn_launch_state_save(const RnGroupDev *g, float *snap, const int *list, int rows, int p, const int *phase,
                                           hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(rn_state_gather_kernel, dim3(rows < RN_SNAP_GRID_CAP ? rows : RN_SNAP_GRID_CAP), dim3(RN_SNAP_THREADS), 0, st, *g,
                     snap, (p + RN_RING_SLOTS - 1) % RN_RING_SLOTS, (p + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS, list, phase, rows);
  return hipGetLastError();
}
extern "C" hipError_t rn_launch_state_load(const RnGroupDev *g, const float *snap, const int *list, int rows, int p, const int *phase,
                                           hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(rn_state_scatter_kernel, dim3(rows < RN_SNAP_GRID_CAP ? rows : RN_SNAP_GRID_CAP), dim3(RN_SNAP_THREADS), 0, st, *g,
                     snap, (p + RN_RING_SLOTS - 1) % RN_RING_SLOTS, (p + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS, list, phase, rows);
  return hipGetLastError();
}

// One 64-bit store with system-scope release: how a HIP stream releases an explicit SDMA-engine copy that lists an HSA signal as its
// dependency (host_io.cpp, copy mode "sdma": p = the value word of the signal; everything the stream's earlier kernels wrote is
// visible to the copy engine that sees the 0).
extern "C" __global__ void rn_release_store_kernel(long long *p, long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
extern "C" hipError_t rn_launch_release_store(void *p, long long v, hipStream_t st) {
  hipLaunchKernelGGL(rn_release_store_kernel, dim3(1), dim3(1), 0, st, static_cast<long long *>(p), v);
  return hipGetLastError();
}
