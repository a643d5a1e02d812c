// state_kernels.hip -- portable per-stream state (include/rn_layout.h: the 25,128 live bytes of the reference's
// DenoiseState, src/denoise.c:68-88) <-> the batch's structure-of-arrays layout (rn_dev.h), on the device.
// Two kernels, one per direction, and one copy body per direction (gather_state / scatter_state) behind every caller:
//   rows == 0   one portable state per stream of the view (export / import, the caller-memory frames of the drop-in API);
//   rows > 0    snapshot records (include/rn_layout.h: RN_SNAP_*) of many streams: the same body, then the record's tail;
//   no record   (scatter only) the zero state of rnnoise_init().
// A third record kind moves no state: the caller's PCM rows of a chunk call <-> the streams' sample FIFOs (chunk_fifo.h), scatter
// in front of the call's frames and gather behind them.
// The host side needs one memcpy per direction instead of one per field.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rn_dev.h"
#include "chunk_fifo.h"

// rnnoise_batch_save_streams / load_streams move 26.5 KB per stream for up to 65,536 streams, so the body is a copy, not a
// dispatch: every field is one contiguous run in the record and one in the batch's arrays (the pitch ring: at most two on each side
// of its wrap, and RN_RING0 is a multiple of 96 floats), and a run moves at the widest access both of its ends are aligned for.
// Record rows are 16-byte aligned (RN_SNAP_FLOATS and RN_STATE_PITCH are multiples of 4), but the portable layout puts conv2_state
// (word 2854), the GRU states (3110), delayed_X (4262) and the band energies (6186) on 8-byte boundaries only, and conv1_state rows
// (130 floats) alternate: the width is chosen per run, 16, 8 or 4 bytes per lane.  One workgroup per record: RN_SNAP_THREADS lanes
// and at most RN_SNAP_GRID_CAP workgroups where many records share the device; RN_STATE_THREADS lanes for a single state, whose
// latency is the caller's (DESIGN 4.14 has the measurements behind the three).
#ifndef RN_SNAP_THREADS
#define RN_SNAP_THREADS 256
#endif
#ifndef RN_SNAP_GRID_CAP
#define RN_SNAP_GRID_CAP 65536
#endif
#ifndef RN_STATE_THREADS
#define RN_STATE_THREADS 1024
#endif
static_assert(RN_SNAP_HIST_FLOATS == RN_RS_HIST && RN_SNAP_GATE_NONE == RN_CTL_NONE, "the record and the kernels agree");
static_assert(RN_SNAP_FLOATS % 4 == 0 && RN_STATE_PITCH % 4 == 0 && RN_SNAP_OFF_HIST % 4 == 0 && RN_OFF_PITCH_BUF % 4 == 0,
              "16-byte rows and runs");
static_assert(RN_RS_DOWN0 % 4 == 0 && RN_RS_HIST % 4 == 0, "both halves of a history are whole float4s");
static_assert(RN_SNAP_THREADS > 128, "a snapshot's header words are written by lanes 64 .. 69 and 128");
static_assert(RN_RING0(1) % 4 == 0 && RN_FRAME_SIZE % 4 == 0 && RN_PITCH_BUF_SIZE % 4 == 0, "ring runs are 16-byte aligned");
static_assert(RN_OFF_LAST_PERIOD == RN_OFF_LAST_GAIN + 1 && RN_OFF_MEM_HP == RN_OFF_LAST_GAIN + 2, "the four scalar words are consecutive");
static_assert(!(RN_SNAP_THREADS & (RN_SNAP_THREADS - 1)) && !(RN_STATE_THREADS & (RN_STATE_THREADS - 1)), "move_run rotates lanes by a mask");
static_assert(RN_CHUNK_FIFO_ROW == RN_FRAME_SIZE, "a FIFO row holds the longest frame");
static_assert(RN_RING_SLOTS % RN_SPEC_SLOTS == 0, "one frame phase, mod RN_RING_SLOTS, gives the ring slot and the spectra slot");
enum { RN_CHUNK_PITCH_MORE = 0 };  // `pitch` of a chunk launch that is not the full-size call's
namespace {
// n floats, src -> dst, by the workgroup (both pointers uniform), lane `lane0` (mod the workgroup, a power of two) taking the first
// access: a record's runs start on the lane their record offset names, so that they spread over the waves and a wave that has
// no part in one run is already waiting for the loads of the next
__device__ __forceinline__ void move_run(float *__restrict__ dst, const float *__restrict__ src, int n, unsigned lane0 = 0) {
  const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src));
  const int nt = blockDim.x, t = (threadIdx.x - lane0) & (nt - 1);
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
// the slots that hold stream s's latest frame, from its frame phase (the slots its NEXT frame writes): its own phase[s] in
// per-stream mode, the launch's p in lock-step
struct Latest {
  int ring, spec;  // pitch-ring slot; spectra slot (the reference's delayed_*)
};
__device__ __forceinline__ Latest latest_slots(int p, const int *__restrict__ phase, int s) {
  const unsigned q = (unsigned)(phase ? phase[s] : p) % RN_RING_SLOTS;
  return {(int)((q + RN_RING_SLOTS - 1) % RN_RING_SLOTS), (int)((q + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS)};
}

// the divisor stream s's resampler history belongs to: the batch's (1 at 48 kHz), or the stream's own where the batch has a rate table
// (rn_dev.h: RnGroupDev::rs_Ls)
__device__ __forceinline__ int stream_L(const RnGroupDev &g, int s) { return g.rs_L ? rn_stream_L(g, s) : 1; }
// ... and the code its DOWN half belongs to: the stream's own code `in_L`, or its byte of the out-rate table where the batch has one
// (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates; the view then has its resampler fields), read as K3 reads its copy of
// the table (rn_dev.h: rn_stream_L)
__device__ __forceinline__ int stream_out_L(const RnGroupDev &g, const uint8_t *out_Ls, int s, int in_L) {
  if (!out_Ls) return in_L;
  const int v = __builtin_amdgcn_readfirstlane((int)*(__attribute__((address_space(1))) const uint8_t *)(out_Ls + s));
  return ((v == 1 || v == 2 || v == 3 || v == 6 || v == RN_RATE_32K) && rn_rate_samples(v) <= g.rs_pitch) ? v : g.rs_L;
}

// The fields that are one run on either side, once for both directions and for the zero state: (array row, record offset, floats)
enum Dir { TO_RECORD, TO_STREAM, TO_ZERO };
template <Dir D>
__device__ __forceinline__ void run(float *row, float *f, int off, int n) {
  if (D == TO_RECORD) move_run(f + off, row, n, off / 4);
  else if (D == TO_STREAM) move_run(row, f + off, n, off / 4);
  else zero_run(row, n);
}
template <Dir D>
__device__ __forceinline__ void plain_fields(const RnGroupDev &g, size_t s, float *f) {
  const size_t N = g.n_stride;
  run<D>(g.synth_mem + s * RN_FRAME_SIZE, f, RN_OFF_SYNTHESIS, RN_FRAME_SIZE);
  if (threadIdx.x < 4) {  // last_gain, last_period (an int32, moved as its bit pattern), mem_hp[2]: four words of the record, a lane each
    const int w = threadIdx.x;
    float *a = w == 0 ? g.last_gain + s : w == 1 ? reinterpret_cast<float *>(g.last_period) + s : g.mem_hp + 2 * s + (w - 2);
    if (D == TO_RECORD) f[RN_OFF_LAST_GAIN + w] = *a;
    else *a = D == TO_STREAM ? f[RN_OFF_LAST_GAIN + w] : 0.f;
  }
  run<D>(g.lastg + s * RN_NB_BANDS, f, RN_OFF_LASTG, RN_NB_BANDS);
  run<D>(g.conv1_state + s * RN_CONV1_ROW, f, RN_OFF_CONV1, RN_CONV1_ROW);
  run<D>(g.conv2_state + s * RN_CONV2_ROW, f, RN_OFF_CONV2, RN_CONV2_ROW);
  for (int k = 0; k < 3; k++) run<D>(g.gru_state + (k * N + s) * RN_GRU, f, RN_OFF_GRU1 + k * RN_GRU, RN_GRU);
}
// ... and the delayed spectra, in slot `slot` of their rotating sets (962 of a row's RN_SPEC_STRIDE floats are the spectrum)
template <Dir D>
__device__ __forceinline__ void spectra(const RnGroupDev &g, size_t s, float *f, int slot) {
  run<D>(slot3(g.spec_X, slot) + s * RN_SPEC_STRIDE, f, RN_OFF_DELAYED_X, RN_OFF_DELAYED_P - RN_OFF_DELAYED_X);
  run<D>(slot3(g.spec_P, slot) + s * RN_SPEC_STRIDE, f, RN_OFF_DELAYED_P, RN_OFF_DELAYED_EX - RN_OFF_DELAYED_P);
  run<D>(slot3(g.spec_E, slot) + s * RN_SPEC_E_ROW, f, RN_OFF_DELAYED_EX, RN_SPEC_E_ROW);
}

// f[0, RN_STATE_FLOATS) <- stream s, whose latest frame sits in the slots `at`
__device__ __forceinline__ void gather_state(const RnGroupDev &g, size_t s, float *__restrict__ f, Latest at) {
  const float *ring = g.pitch_ring + s * RN_RING_SIZE;
  const int ring0 = RN_RING0(at.ring), n1 = min(RN_PITCH_BUF_SIZE, RN_RING_SIZE - ring0);
  move_run(f + RN_OFF_ANALYSIS, ring + at.ring * RN_FRAME_SIZE, RN_FRAME_SIZE);  // analysis_mem = tail of pitch_buf = the newest slot
  move_run(f + RN_OFF_PITCH_BUF, ring + ring0, n1, RN_OFF_PITCH_BUF / 4);
  if (n1 < RN_PITCH_BUF_SIZE) move_run(f + RN_OFF_PITCH_BUF + n1, ring, RN_PITCH_BUF_SIZE - n1, (RN_OFF_PITCH_BUF + n1) / 4);
  plain_fields<TO_RECORD>(g, s, f);
  spectra<TO_RECORD>(g, s, f, at.spec);
}

// stream s <- f[0, RN_STATE_FLOATS), f 16-byte aligned, with the stream's latest frame in the slots `at` (analysis_mem is implied by
// pitch_buf and not stored)
__device__ __forceinline__ void scatter_state(const RnGroupDev &g, size_t s, const float *__restrict__ f, Latest at) {
  const int t = threadIdx.x, nt = blockDim.x;
  float *ring = g.pitch_ring + s * RN_RING_SIZE;
  const float *pb = f + RN_OFF_PITCH_BUF;
  // pitch_buf at ring0 (two runs where it wraps); the RN_RING_SIZE - RN_PITCH_BUF_SIZE positions behind it are zeroed
  const int ring0 = RN_RING0(at.ring), n1 = min(RN_PITCH_BUF_SIZE, RN_RING_SIZE - ring0);
  move_run(ring + ring0, pb, n1, RN_OFF_PITCH_BUF / 4);
  if (n1 < RN_PITCH_BUF_SIZE) move_run(ring, pb + n1, RN_PITCH_BUF_SIZE - n1, (RN_OFF_PITCH_BUF + n1) / 4);
  const int z0 = (ring0 + RN_PITCH_BUF_SIZE) % RN_RING_SIZE, nz = RN_RING_SIZE - RN_PITCH_BUF_SIZE, z1 = min(nz, RN_RING_SIZE - z0);
  zero_run(ring + z0, z1);
  if (z1 < nz) zero_run(ring, nz - z1);
  // the decimated ring is derived data (rn_dev.h: RN_XRING_SLOT): sample q = the high-pass kernel's expression over ring positions
  // 2q-1, 2q, 2q+1 (zeros outside pitch_buf).  Two samples per lane from the RECORD's pitch_buf: ring position 2q is pitch_buf
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
  plain_fields<TO_STREAM>(g, s, const_cast<float *>(f));  // (TO_STREAM only reads the record)
  spectra<TO_STREAM>(g, s, const_cast<float *>(f), at.spec);
}

// stream s <- the zero state of rnnoise_init(): every slot of the two rings and of the spectra, whatever the stream's frame phase
__device__ __forceinline__ void zero_state(const RnGroupDev &g, size_t s) {
  zero_run(g.pitch_ring + s * RN_RING_SIZE, RN_RING_SIZE);
  zero_run(g.xlp_ring + s * RN_XRING_SIZE, RN_XRING_SIZE);
  plain_fields<TO_ZERO>(g, s, nullptr);
  for (int k = 0; k < RN_SPEC_SLOTS; k++) {
    zero_run(slot3(g.spec_X, k) + s * RN_SPEC_STRIDE, RN_SPEC_STRIDE);
    zero_run(slot3(g.spec_P, k) + s * RN_SPEC_STRIDE, RN_SPEC_STRIDE);
    zero_run(slot3(g.spec_E, k) + s * RN_SPEC_E_ROW, RN_SPEC_E_ROW);
  }
}
// what a stream of a batch has beside its portable state restarts with a state that carries none of it: the resampler histories
// (rn_dev.h: rs_hist) zeroed, the counter of the suppression controls (gate_c) at "no voice frame yet", the sample FIFOs of the chunk
// calls (chunk_plan.h: RnChunkDev) empty in and M zeros out
__device__ __forceinline__ void restart_extras(const RnGroupDev &g, size_t s, const RnChunkDev &ck) {
  if (g.rs_hist) zero_run(g.rs_hist + s * RN_RS_HIST, RN_RS_HIST);
  if (g.gate_c && threadIdx.x == 0) g.gate_c[s] = RN_CTL_NONE;
  rn_chunk_restart(ck, s, threadIdx.x, blockDim.x);
}
}  // namespace

// Both kernels: record `row` <-> stream list[row] of the view (stream `row` without a list), at the frame phase phase[stream] (the
// launch's p without `phase`).  rows > 0: `rows` snapshot records of RN_SNAP_FLOATS, the workgroups striding over them.  rows == 0:
// one workgroup per record, portable states `pitch` floats apart.  An entry outside the view moves nothing.
// rows < 0: a chunk launch (RN_REC_CHUNK; ck carries the call), workgroup b = stream b of the group and nothing of the above; the two
// halves of its body (chunk_fifo.h) on either side of the workgroup's barrier.  (The sign of `rows`, not a field of ck: a state
// launch decides from the arguments it read before there was a ck, and never waits for ck's end of the argument block.)  Further
// cases of the chunk launch, told apart by ck's last fields: with ck.list, workgroup b = row b of a list call's buffers and stream
// ck.list[b]; with ck.op, no call at all -- row b of ck.rec <-> that stream's FIFOs (gather saves, scatter loads).  `pitch`,
// which a chunk launch has no other use for, says whether there is any such field to look at (RN_CHUNK_PITCH_MORE): the full-size
// call's launch reads what it read before there were any.  (Told by a second value of `rows` instead, the scatter kernel reserved
// 20 bytes of scratch; told by the fields alone, the full-size call with few streams pushing lost 0.3 to 0.5 %: DESIGN 4.26.)

// rec[row] <- stream.  A snapshot's tail: the header (magic, L, the gate counter or RN_CTL_NONE, the code of the down history where
// the batch has an out-rate table -- out_Ls, read by snapshot launches alone, behind the state's copy -- or zero, two zeros) and the
// resampler history or zeros; an entry outside the view leaves an empty record (magic 0).
extern "C" __global__ void __launch_bounds__(1024)
rn_state_gather_kernel(RnGroupDev g, float *__restrict__ rec, int p, const int *__restrict__ list, const int *__restrict__ phase, int rows,
                       int pitch, RnChunkDev ck, const uint8_t *__restrict__ out_Ls) {
  if (rows < 0) {  // out[s] <- the stream's output FIFO ++ its staged frames; what is left is the FIFO
    extern __shared__ float kept[];  // (RN_CHUNK_FIFO_ROW floats, on chunk launches only: a state launch keeps its LDS-free dispatch)
    if (blockIdx.x >= (unsigned)ck.N) return;
    if (pitch == RN_CHUNK_PITCH_MORE) {  // (the full-size launch never waits for ck's last fields either)
      if (ck.op == RN_CHUNK_OP_SAVE) return rn_chunk_rec_save(ck, blockIdx.x, threadIdx.x, blockDim.x);  // rec[row] <- the stream's FIFOs
      // the same on a stream list: workgroup b = row b of the call, stream list[b]
      const int row = blockIdx.x, ls = rn_chunk_row_stream(ck, row);
      const RnChunkHead lh = rn_chunk_list_gather_head(ck, row, ls);
      rn_chunk_list_gather_pop(ck, row, ls, lh, kept, threadIdx.x, blockDim.x);
      __syncthreads();
      return rn_chunk_list_gather_keep(ck, row, ls, lh, kept, threadIdx.x, blockDim.x);
    }
    const size_t s = blockIdx.x;
    const RnChunkHead h = rn_chunk_gather_head(ck, s);
    rn_chunk_gather_pop(ck, s, h, kept, threadIdx.x, blockDim.x);
    __syncthreads();
    return rn_chunk_gather_keep(ck, s, h, kept, threadIdx.x, blockDim.x);
  }
  const bool snap = rows > 0;
  const int n = snap ? rows : (int)gridDim.x, t = threadIdx.x;
  const size_t stride = snap ? RN_SNAP_FLOATS : pitch;
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    float *f = rec + row * stride;
    const int s = list ? list[row] : row;
    if (s < 0 || s >= g.n_streams) {
      if (snap && t == 0) f[RN_SNAP_OFF_MAGIC] = __int_as_float(0);
      continue;
    }
    gather_state(g, s, f, latest_slots(p, phase, s));
    if (!snap) continue;
    if (t >= 64 && t < 70 && !(out_Ls && t == 64 + RN_SNAP_OFF_OUT_L - RN_SNAP_OFF_MAGIC)) {
      const int w = t - 64;
      const int v = w == 0 ? RN_SNAP_MAGIC : w == 1 ? stream_L(g, s) : w == 2 ? (g.gate_c ? g.gate_c[s] : RN_CTL_NONE) : 0;
      f[RN_SNAP_OFF_MAGIC + w] = __int_as_float(v);
    }
    // (the out-rate table's code in the place of its zero, by a lane of another wave, where there is a table)
    if (out_Ls && t == 128) f[RN_SNAP_OFF_OUT_L] = __int_as_float(stream_out_L(g, out_Ls, s, g.rs_L));
    if (g.rs_hist) move_run(f + RN_SNAP_OFF_HIST, g.rs_hist + (size_t)s * RN_RS_HIST, RN_RS_HIST);
    else zero_run(f + RN_SNAP_OFF_HIST, RN_RS_HIST);
  }
}

// stream <- rec[row] (16-byte aligned records), then what the portable state does not carry, where the view has it (g.rs_hist,
// g.gate_c).  A snapshot brings both: the resampler history, each half when the code it was saved under is the stream's current one --
// the up half under the record's L against the stream's own code, the down half under the record's output code (0: its L) against the
// stream's output code (stream_out_L) -- and zeros otherwise, and the gate counter, clamped; a record with another magic word touches
// nothing.  A portable state restarts them (restart_extras).
// No `rec`: stream <- the zero state, one workgroup per stream, and the extras restart as well (ck: the FIFOs among them).
extern "C" __global__ void __launch_bounds__(1024)
rn_state_scatter_kernel(RnGroupDev g, const float *__restrict__ rec, int p, const int *__restrict__ list, const int *__restrict__ phase,
                        int rows, int pitch, RnChunkDev ck, const uint8_t *__restrict__ out_Ls) {
  if (rows < 0) {  // the stream's pending samples ++ in[s] -> its frames of the call and their mask; the tail is left pending
    if (blockIdx.x >= (unsigned)ck.N) return;
    if (pitch == RN_CHUNK_PITCH_MORE) {
      if (ck.op == RN_CHUNK_OP_LOAD) return rn_chunk_rec_load(ck, blockIdx.x, threadIdx.x, blockDim.x);  // the stream's FIFOs <- rec[row]
      const int row = blockIdx.x, ls = rn_chunk_row_stream(ck, row);
      const RnChunkHead lh = rn_chunk_list_scatter_head(ck, row, ls);
      rn_chunk_list_scatter_frames(ck, row, ls, lh, threadIdx.x, blockDim.x);
      __syncthreads();
      return rn_chunk_list_scatter_tail(ck, row, ls, lh, threadIdx.x, blockDim.x);
    }
    const size_t s = blockIdx.x;
    const RnChunkHead h = rn_chunk_scatter_head(ck, s);
    rn_chunk_scatter_frames(ck, s, h, threadIdx.x, blockDim.x);
    __syncthreads();
    return rn_chunk_scatter_tail(ck, s, h, threadIdx.x, blockDim.x);
  }
  const bool snap = rows > 0;
  const int n = snap ? rows : (int)gridDim.x, t = threadIdx.x;
  if (!rec) {
    const int s = list ? list[blockIdx.x] : (int)blockIdx.x;
    if (s < 0 || s >= g.n_streams) return;
    zero_state(g, s);
    return restart_extras(g, s, ck);
  }
  const size_t stride = snap ? RN_SNAP_FLOATS : pitch;
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    const float *f = rec + row * stride;
    const int s = list ? list[row] : row;
    if (s < 0 || s >= g.n_streams || (snap && __float_as_int(f[RN_SNAP_OFF_MAGIC]) != RN_SNAP_MAGIC)) continue;
    scatter_state(g, s, f, latest_slots(p, phase, s));
    if (!snap) {
      restart_extras(g, s, ck);
      continue;
    }
    if (g.rs_hist) {
      float *hist = g.rs_hist + (size_t)s * RN_RS_HIST;
      const int rec_L = __float_as_int(f[RN_SNAP_OFF_L]), rec_out = __float_as_int(f[RN_SNAP_OFF_OUT_L]), L = stream_L(g, s);
      const bool up = rec_L == L, down = (rec_out ? rec_out : rec_L) == stream_out_L(g, out_Ls, s, L);
      // (one pass over the row's float4s, each from the record or zero by its half: RN_RS_DOWN0 is a multiple of 4)
      for (int i = t; i < RN_RS_HIST / 4; i += blockDim.x)
        reinterpret_cast<float4 *>(hist)[i] = (i < RN_RS_DOWN0 / 4 ? up : down) ? reinterpret_cast<const float4 *>(f + RN_SNAP_OFF_HIST)[i]
                                                                                : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (g.gate_c && t == 64) g.gate_c[s] = min(max(__float_as_int(f[RN_SNAP_OFF_GATE]), 0), RN_CTL_NONE);
    rn_chunk_restart(ck, s, t, blockDim.x);  // (a record carries no FIFO contents)
  }
}

// The launchers, one per direction: `rows` records of `kind`, record i <-> stream list[i] of the view (stream i when list is null).
// p: the frame phase of a lock-step batch (the ring slot its next frame writes); phase: the per-stream phases on the device, indexed
// as the view's rows, which then take p's place.  Scattered records are 16-byte aligned (both pitches are multiples of 4 floats).
// ck: the FIFOs of the view's streams, which a scatter restarts (null: the group has none), and with kind RN_REC_CHUNK the chunk
// call -- `rows` streams, one workgroup of RN_SNAP_THREADS lanes each, no record and no list among the arguments: a list call's
// list and a FIFO record launch's records travel in ck, with as many workgroups as they have rows.
// out_Ls: the batch's out-rate table (shim.h: RNNoiseBatch::out_Ls), indexed as the view's rows, for the snapshot launches; null: none.
namespace {
template <typename Kernel, typename Rec>
hipError_t launch_state(Kernel kernel, const RnGroupDev *g, RnRecKind kind, Rec rec, const int *list, int rows, int p, const int *phase,
                        const RnChunkDev *ck, hipStream_t st, const uint8_t *out_Ls) {
  if (rows <= 0) return hipSuccess;
  const bool snap = kind == RN_REC_SNAP;
  RnChunkDev c = ck ? *ck : RnChunkDev{};
  if (kind == RN_REC_CHUNK) {
    if (!ck || rows != ck->N || rec) return hipErrorInvalidValue;
    if (ck->op == RN_CHUNK_OP_CALL ? !ck->counts || (ck->list && ck->S != g->n_streams) : !ck->rec || ck->S != g->n_streams)
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(RN_SNAP_THREADS), RN_CHUNK_FIFO_ROW * sizeof(float), st, *g, rec, 0, nullptr, nullptr, -1,
                       ck->op || ck->list ? RN_CHUNK_PITCH_MORE : RN_STATE_PITCH, c, static_cast<const uint8_t *>(nullptr));
    return hipGetLastError();
  }
  // (RN_STATE_THREADS where one record's latency is the call's: a single state moved between two copies; RN_SNAP_THREADS where
  //  many records share the device, the zero state of a stream list included)
  hipLaunchKernelGGL(kernel, dim3(rows < RN_SNAP_GRID_CAP || !snap ? rows : RN_SNAP_GRID_CAP), dim3(snap || !rec ? RN_SNAP_THREADS : RN_STATE_THREADS),
                     0, st, *g, rec, p, list, phase, snap ? rows : 0, RN_STATE_PITCH, c, snap ? out_Ls : nullptr);
  return hipGetLastError();
}
}  // namespace
extern "C" hipError_t rn_launch_state_gather(const RnGroupDev *g, RnRecKind kind, float *rec, const int *list, int rows, int p,
                                             const int *phase, const RnChunkDev *ck, hipStream_t st, const uint8_t *out_Ls) {
  return launch_state(rn_state_gather_kernel, g, kind, rec, list, rows, p, phase, ck, st, out_Ls);
}
extern "C" hipError_t rn_launch_state_scatter(const RnGroupDev *g, RnRecKind kind, const float *rec, const int *list, int rows, int p,
                                              const int *phase, const RnChunkDev *ck, hipStream_t st, const uint8_t *out_Ls) {
  return launch_state(rn_state_scatter_kernel, g, kind, rec, list, rows, p, phase, ck, st, out_Ls);
}
// the zero state for the n streams list[i] of the view (one workgroup each), or for every stream of the view without a list
extern "C" hipError_t rn_launch_state_zero(const RnGroupDev *g, const int *list, int n, const RnChunkDev *ck, hipStream_t st) {
  return launch_state(rn_state_scatter_kernel, g, RN_REC_STATE, static_cast<const float *>(nullptr), list, list ? n : g->n_streams, 0,
                      nullptr, ck, st, nullptr);
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
