// state_kernels.hip -- portable per-stream state (include/rn_layout.h: the 25,128 live bytes of the reference's
// DenoiseState, src/denoise.c:68-88) <-> the batch's structure-of-arrays layout (rn_dev.h), on the device.
// One launch moves `g.n_streams` states (a 1024-thread workgroup each: the per-word field dispatch is latency, 17 us with 256
// threads); the host side needs one memcpy per direction instead of one per field.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rn_dev.h"

// flat[s][RN_STATE_FLOATS] <- stream s of the view.  newest_slot = pitch-ring slot of the latest frame,
// last = spectra slot of the latest frame (the reference's delayed_*).
extern "C" __global__ void __launch_bounds__(1024)
rn_state_gather_kernel(RnGroupDev g, float *__restrict__ flat, int newest_slot, int last) {
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
extern "C" __global__ void __launch_bounds__(1024)
rn_state_scatter_kernel(RnGroupDev g, const float *__restrict__ flat, int newest_slot, int last, const int *__restrict__ list) {
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
  hipLaunchKernelGGL(rn_state_gather_kernel, dim3(g->n_streams), dim3(1024), 0, st, *g, flat, newest_slot, last);
  return hipGetLastError();
}
extern "C" hipError_t rn_launch_state_scatter(const RnGroupDev *g, const float *flat, int newest_slot, int last, hipStream_t st,
                                              const int *list, int n) {
  // (list: n stream indices of the view, one block each; otherwise one block per stream of the view)
  if (list && n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rn_state_scatter_kernel, dim3(list ? n : g->n_streams), dim3(1024), 0, st, *g, flat, newest_slot, last, list);
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
