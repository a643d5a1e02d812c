// batch.cpp -- rnnoise_batch_*: N streams resident on one GPU: create, destroy, reset, the schedule and network-path setters,
// training-feature extraction, timing and the debug taps.  (The frame step: batch_step.cpp; the chunk calls: batch_chunks.cpp.)
#include "shim.h"
#include "device_choice.h"

// the dispatch switches (dispatch.h), read once per process
const RnKnobs &rn_knobs() {
  static const RnKnobs k = rn_knobs_from_env();
  return k;
}
namespace {
template <typename T>
T *carve(uint8_t *&p, size_t count) {
  T *r = reinterpret_cast<T *>(p);
  p += rn_align256(count * sizeof(T));
  return r;
}
// the arrays of rn_dev.h: RN_GROUP_ARRAYS for n streams from `base` on, then the [n] frame phases of per-stream mode (the group
// carries a pointer to them only while a call runs in that mode); returns the bytes used (a null base: the arena's size)
size_t batch_layout(RnGroupDev &g, int *&phase_buf, uint8_t *base, int n) {
  uint8_t *p = base;
  const size_t N = n;
  g.n_streams = n;
  g.n_stride = n;
#define CARVE(m, T, row, planes) g.m = carve<T>(p, (size_t)(planes) * (row) * N);
#define CARVE_TILES(m, T, tile) g.m = carve<T>(p, (N + 15) / 16 * (tile));
#define NOT_CARVED(m, row)
  RN_GROUP_ARRAYS(CARVE, CARVE_TILES, NOT_CARVED)
#undef CARVE
#undef CARVE_TILES
#undef NOT_CARVED
  phase_buf = carve<int>(p, N);
  return (size_t)(p - base);
}

}  // namespace

// rows [first, first + count) of a batch as a group of their own (rn_dev.h: n_stride keeps the plane strides)
RnGroupDev group_view(const RnGroupDev &g, int first, int count) {
  RnGroupDev v = g;
  const size_t f = first;
  v.n_streams = count;
#define ADVANCE(m, T, row, planes) v.m += (row) * f;
#define WHOLE(m, T, tile)
#define ADVANCE_IF_SET(m, row) \
  if (v.m) v.m += (row) * f;
  RN_GROUP_ARRAYS(ADVANCE, WHOLE, ADVANCE_IF_SET)
#undef ADVANCE
#undef WHOLE
#undef ADVANCE_IF_SET
  return v;
}

// the host list of a call is checked before anything moves (shim.h)
bool host_list_ok(const RNNoiseBatch *b, const int *list, int n, bool unique) {
  if (!list) return n <= b->n;
  std::vector<uint8_t> seen(unique ? (size_t)b->n : 0, 0);
  for (int i = 0; i < n; i++) {
    const int s = list[i];
    if (s < 0 || s >= b->n || (unique && seen[s])) return false;
    if (unique) seen[s] = 1;
  }
  return true;
}

namespace {
int batch_flush_timing(RNNoiseBatch *b) {
  for (auto &e : b->pending) {
    float ms = 0;
    HIP_OK(hipEventSynchronize(e.b));
    HIP_OK(hipEventElapsedTime(&ms, e.a, e.b));
    b->ms_sum[e.kind] += ms;
    b->pool.push_back(e);
  }
  b->pending.clear();
  return 0;
}
}  // namespace

// =============================================================================================
// batched API
// =============================================================================================
extern "C" int rnnoise_amd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" RNNoiseBatch *rnnoise_batch_create(RNNModel *model, int n_streams, int device) {
  if (!model || n_streams <= 0) {
    fprintf(stderr, "[rnnoise_amd] rnnoise_batch_create: a model blob is required (no compiled-in weights)\n");
    return nullptr;
  }
  if (!rn_device_index_ok(device, rnnoise_amd_device_count())) {
    fprintf(stderr, "[rnnoise_amd] no HIP device %d (visible devices: %d); there is no CPU fallback\n", device,
            rnnoise_amd_device_count());
    return nullptr;
  }
  RNNoiseBatch *b = new RNNoiseBatch();
  b->model = model;
  b->models[0] = model;
  b->device = device;
  b->n = n_streams;
  b->nn_path = rn_default_nn_path(rn_knobs(), n_streams);
  if (model_on_device(model, device, b->m) || tables_for_device(device, b->tb)) {
    delete b;
    return nullptr;
  }
  RnGroupDev probe{};
  int *no_phases = nullptr;
  b->arena_bytes = batch_layout(probe, no_phases, nullptr, n_streams);
  DeviceGuard guard(device);
  if (!guard.ok || hipMalloc(&b->arena, b->arena_bytes) != hipSuccess) {
    fprintf(stderr, "[rnnoise_amd] cannot allocate %zu bytes of HBM for %d streams\n", b->arena_bytes, n_streams);
    delete b;
    return nullptr;
  }
  // the device's facts the plans need: its compute units, and the large-LDS opt-ins (kept, not fatal: only launches of a refused
  // form fail)
  if (hipDeviceGetAttribute(&b->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || b->cus <= 0) b->cus = 256;
  b->lds_one = rn_nn_one_opt_in();
  rn_nn_gru_opt_in(b->lds_gru);
  batch_layout(b->g, b->phase_buf, static_cast<uint8_t *>(b->arena), n_streams);
  b->scratch_gains = b->g.gains;
  b->scratch_vad = b->g.vad;
  b->features2[0] = b->g.features;
  b->silence2[0] = b->g.silence;
  b->pitch2[0] = b->g.pitch;
  b->features2[1] = b->g.features_b;
  b->silence2[1] = b->g.silence_b;
  b->pitch2[1] = b->g.pitch_b;
  if (rnnoise_batch_reset(b)) {
    rnnoise_batch_destroy(b);
    return nullptr;
  }
  return b;
}

extern "C" void rnnoise_batch_destroy(RNNoiseBatch *b) {
  if (!b) return;
  DeviceGuard guard(b->device);
  hipDeviceSynchronize();
  for (auto &e : b->pending) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  for (auto &e : b->pool) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  host_io_release(b);
  if (b->state_stage) hipFree(b->state_stage);
  if (b->chunk_fifo) hipFree(b->chunk_fifo);
  if (b->chunk_stage) hipFree(b->chunk_stage);
  if (b->split_store) hipFree(b->split_store);
  if (b->arena) hipFree(b->arena);
  if (b->rs_buf) hipFree(b->rs_buf);
  if (b->rate_map) hipFree(b->rate_map);
  if (b->fmt_map) hipFree(b->fmt_map);
  if (b->out_rate_map) hipFree(b->out_rate_map);
  if (b->out_fmt_map) hipFree(b->out_fmt_map);
  if (b->model_map) hipFree(b->model_map);
  if (b->ctl_buf) hipFree(b->ctl_buf);
  if (b->train_mix_buf) hipFree(b->train_mix_buf);
  if (b->train_rir_tw) hipFree(b->train_rir_tw);
  if (b->train_rir_buf) hipFree(b->train_rir_buf);
  if (b->debug_buf) hipFree(b->debug_buf);
  if (b->side) hipStreamDestroy(b->side);
  if (b->side_hp) {
    hipStreamDestroy(b->side_hp);
    hipEventDestroy(b->ev_begin);
    for (int k = 0; k < 8; k++) { hipEventDestroy(b->own_hp[k]); hipEventDestroy(b->own_k1[k]); hipEventDestroy(b->own_k3[k]); }
  }
  delete b;
}

extern "C" int rnnoise_batch_size(const RNNoiseBatch *b) { return b ? b->n : -1; }

extern "C" int rnnoise_batch_reset(RNNoiseBatch *b) {
  if (!b) return -1;
  ON_DEVICE(b->device);
  // a control operation, synchronous like state export / import: whatever the batch (or anybody else) still has in flight on
  // this device is drained first, and the cleared state is in place when the call returns
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemset(b->arena, 0, b->arena_bytes));
  if (b->rs_buf) HIP_OK(hipMemset(b->rs_buf, 0, (size_t)b->n * RN_RS_HIST * sizeof(float)));  // (the histories; rs_up / rs_dn are scratch)
  if (b->g.gate_c) HIP_OK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b->g.gate_c), RN_CTL_NONE, b->n));  // (the table stays)
  if (batch_chunk_restart_all(b)) return -1;  // (the sample FIFOs of the chunk calls)
  HIP_OK(hipDeviceSynchronize());
  b->img_valid = false;
  b->parity = 0;
  b->ring_slot = 0;
  b->frame_no = 0;
  b->per_stream = false;  // (the only way back to lock-step frame phase)
  b->split_pending = 0;   // (pending frames of the split calls are dropped; their store stays)
  return 0;
}

extern "C" int rnnoise_batch_set_schedule(RNNoiseBatch *b, int schedule) {
  if (!b || (schedule != 0 && schedule != 1 && schedule != 9)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int old = b->schedule;
  b->schedule = schedule;
  return old;
}

extern "C" int rnnoise_batch_set_nn_path(RNNoiseBatch *b, int path) {
  if (!b || path < 0 || path > 2) return -1;  // 0 vector, 1 MFMA (layer-wise from $RNNOISE_AMD_NN_LAYERS_MIN streams up), 2 layer-wise
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  int old = b->nn_path;
  b->nn_path = path;
  return old;
}

// ---- training-feature extraction (reference loop src/dump_features.c:466-491) ----
extern "C" int rnnoise_batch_train_features_device(RNNoiseBatch *b, float *d_records, const float *d_clean,
                                                   const float *d_noisy, const float *d_vad, const int *d_lowpass,
                                                   const int *d_band_lp, const int *d_noise_free, int n_frames,
                                                   void *hip_stream) {
  if (!b || !d_records || !d_clean || !d_noisy || !d_vad || !d_lowpass || !d_band_lp || !d_noise_free || n_frames < 0)
    return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (b->per_stream || b->g.rs_L || b->out_Ls || b->row_stride || b->channels > 1) return -1;  // (extraction runs in lock-step frame phase, at 48 kHz in and out, in the default PCM layout, one row per slot, only)
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  const size_t N = b->n;
  for (int f = 0; f < n_frames; f++) {
    RnTrainArgs tr{};  // (step.on = 0: the extraction launch)
    tr.clean = d_clean + f * N * RN_FRAME_SIZE;
    tr.clean_mem = b->g.train_clean_mem;
    tr.vad = d_vad + f * N;
    tr.lowpass = d_lowpass;
    tr.band_lp = d_band_lp;
    tr.noise_free = d_noise_free;
    tr.rec = d_records + f * N * 98;
    HIP_OK(rn_launch_train_features(&b->g, &b->tb, d_noisy + f * N * RN_FRAME_SIZE, b->ring_slot, b->parity, &tr, st));
    b->parity = (b->parity + 1) % RN_SPEC_SLOTS;
    b->ring_slot = (b->ring_slot + 1) % RN_RING_SLOTS;
  }
  return 0;
}

#define D2H(dst, src, count) HIP_OK(hipMemcpy(dst, src, (count) * 4, hipMemcpyDeviceToHost))
#define H2D(dst, src, count) HIP_OK(hipMemcpy(dst, src, (count) * 4, hipMemcpyHostToDevice))

extern "C" int rnnoise_batch_train_features(RNNoiseBatch *b, float *records, const float *clean, const float *noisy,
                                            const float *vad, const int *lowpass, const int *band_lp,
                                            const int *noise_free, int n_frames) {
  if (!b || !records || !clean || !noisy || !vad || !lowpass || !band_lp || !noise_free || n_frames <= 0 || b->per_stream || b->g.rs_L || b->out_Ls || b->row_stride || b->channels > 1)
    return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  const size_t N = b->n, fN = (size_t)n_frames * N, fb = fN * RN_FRAME_SIZE * 4;
  DevScratch d;
  const size_t o_clean = d.carve(fb), o_noisy = d.carve(fb), o_vad = d.carve(fN * 4), o_rec = d.carve(fN * 98 * 4), o_lp = d.carve(N * 4),
               o_bl = d.carve(N * 4), o_nf = d.carve(N * 4);
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_clean), clean, fb, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_noisy), noisy, fb, hipMemcpyHostToDevice));
  H2D(d.at<char>(o_vad), vad, fN);
  H2D(d.at<char>(o_lp), lowpass, N);
  H2D(d.at<char>(o_bl), band_lp, N);
  H2D(d.at<char>(o_nf), noise_free, N);
  if (rnnoise_batch_train_features_device(b, d.at<float>(o_rec), d.at<float>(o_clean), d.at<float>(o_noisy), d.at<float>(o_vad),
                                          d.at<int>(o_lp), d.at<int>(o_bl), d.at<int>(o_nf), n_frames, nullptr))
    return -1;
  HIP_OK(hipDeviceSynchronize());
  D2H(records, d.at<char>(o_rec), fN * 98);
  return 0;
}

extern "C" int rnnoise_batch_debug_last(RNNoiseBatch *b, float *features, int *silence, int *pitch) {
  if (!b) return -1;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (features) {
    std::vector<float> tmp((size_t)b->n * 68);
    D2H(tmp.data(), b->features2[(b->frame_no + 1) & 1], tmp.size());
    for (int s = 0; s < b->n; s++) memcpy(features + (size_t)s * RN_NB_FEATURES, tmp.data() + (size_t)s * 68, RN_NB_FEATURES * 4);
  }
  if (silence) D2H(silence, b->silence2[(b->frame_no + 1) & 1], b->n);
  if (pitch) D2H(pitch, b->pitch2[(b->frame_no + 1) & 1], b->n);
  return 0;
}

#if RN_INSTRUMENT  // ---- test / measurement taps: instrumented build only (include/rnnoise_amd_debug.h) ----
// pitch stage taps of the last step ([N][RN_DBG_FLOATS]); the first call (dst==NULL) arms them
extern "C" int rnnoise_batch_debug_pitch(RNNoiseBatch *b, float *dst) {
  if (!b) return -1;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (!b->debug_buf) {
    HIP_OK(hipMalloc((void **)&b->debug_buf, (size_t)b->n * RN_DBG_FLOATS * 4));
    HIP_OK(hipMemset(b->debug_buf, 0, (size_t)b->n * RN_DBG_FLOATS * 4));
    b->g.debug = b->debug_buf;
  }
  if (dst) D2H(dst, b->debug_buf, (size_t)b->n * RN_DBG_FLOATS);
  return 0;
}

// n independent 960-point transforms through the register-resident FFT (fft_reg.h), `reps` passes each (the spectrum is
// fed back as the next input); variant 0 = all exchanges through ds_bpermute, 1 = the DPP / swizzle forms the kernels use.
// in / out: [n][960][2] host floats (natural order; the 1/960 input scale of kiss_fft.c:582 is applied on the first pass);
// clocks (optional): [n] shader clocks per wave; xlane (optional): [2][6][64] source lane delivered by each exchange
// primitive for xor masks 1,2,4,8,16,32.  Tests and tools only.
extern "C" int rnnoise_amd_debug_fft(int device, int variant, float *out, const float *in, int n, int reps,
                                     unsigned long long *clocks, int *xlane) {
  if (!out || !in || n <= 0 || reps <= 0) return -1;
  ON_DEVICE(device);
  RnTablesDev tb;
  if (tables_for_device(device, tb)) return -1;
  const size_t fb = (size_t)n * 960 * 2 * 4;
  DevScratch d;
  const size_t o_in = d.carve(fb), o_out = d.carve(fb), o_clk = d.carve((size_t)n * 8), o_x = d.carve(2 * 6 * 64 * 4);
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_in), in, fb, hipMemcpyHostToDevice));
  HIP_OK(rn_launch_fft_probe(variant, d.at<float>(o_in), d.at<float>(o_out), d.at<unsigned long long>(o_clk), n, reps, &tb, nullptr));
  HIP_OK(rn_launch_xlane_probe(d.at<int>(o_x), nullptr));
  HIP_OK(hipStreamSynchronize(nullptr));
  HIP_OK(hipMemcpy(out, d.at<char>(o_out), fb, hipMemcpyDeviceToHost));
  if (clocks) HIP_OK(hipMemcpy(clocks, d.at<char>(o_clk), (size_t)n * 8, hipMemcpyDeviceToHost));
  if (xlane) D2H(xlane, d.at<char>(o_x), 2 * 6 * 64);
  return 0;
}

// out[i] = (float)log10(1e-2 + (double)ex[i]) evaluated on the device by the feature stage's function (host buffers; tests only).
// ex == null: the n floats with bit patterns first_bits, first_bits + 1, ...; model 0: as the kernels of this process evaluate it
// (rnnoise_amd_log10_model()), 1: the device library's log10 whatever the process uses
extern "C" int rnnoise_amd_debug_log_energy_range(int device, float *out, const float *ex, unsigned first_bits, unsigned n, int model) {
  if (!out || n == 0) return -1;
  ON_DEVICE(device);
  RnTablesDev tb;
  if (tables_for_device(device, tb)) return -1;
  DevScratch d;
  const size_t o_out = d.carve((size_t)n * 4), o_ex = d.carve(ex ? (size_t)n * 4 : 0);
  if (d.alloc()) return -1;
  if (ex) H2D(d.at<char>(o_ex), ex, (size_t)n);
  HIP_OK(rn_launch_log_energy(ex ? d.at<float>(o_ex) : nullptr, first_bits, d.at<float>(o_out), n, model == 1 ? nullptr : tb.log_tab, nullptr));
  HIP_OK(hipStreamSynchronize(nullptr));
  D2H(out, d.at<char>(o_out), (size_t)n);
  return 0;
}
extern "C" int rnnoise_amd_debug_log_energy(int device, float *out, const float *ex, int n) {
  if (!ex || n <= 0) return -1;
  return rnnoise_amd_debug_log_energy_range(device, out, ex, 0, (unsigned)n, 0);
}

// The functions of the Viterbi VAD's epilogue (include/rn_train_vad.h) on the device against this host's libm, for the n floats with
// bit patterns first_bits, first_bits + stride, ...: mode 1 pow((double)((1.f - f) / f), .5), 2 log(1e-15 + (double)f),
// 3 log((double)f).  *mismatches: how many doubles differ in a bit (two NaNs are equal); *first_bad: the first such float's bits.
extern "C" int rnnoise_amd_debug_train_vad_libm(int device, int mode, unsigned first_bits, unsigned stride, unsigned n,
                                                unsigned long long *mismatches, unsigned *first_bad) {
  if (mode < 1 || mode > 3 || !mismatches || !first_bad || n == 0 || stride == 0) return -1;
  if ((unsigned long long)first_bits + (unsigned long long)(n - 1) * stride > 0xffffffffull) return -1;
  ON_DEVICE(device);
  const unsigned chunk = 1u << 22;
  DevScratch d;
  const size_t o_out = d.carve((size_t)std::min(n, chunk) * 8);
  if (d.alloc()) return -1;
  std::vector<double> got(std::min(n, chunk));
  volatile double half = 0.5;  // (volatile: pow() stays the libm call)
  *mismatches = 0;
  *first_bad = 0;
  for (unsigned at = 0; at < n; at += chunk) {
    const unsigned m = std::min(chunk, n - at);
    HIP_OK(rn_launch_vad_libm(mode, first_bits + at * stride, stride, d.at<double>(o_out), m, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
    HIP_OK(hipMemcpy(got.data(), d.at<char>(o_out), (size_t)m * 8, hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < m; i++) {
      const unsigned u = first_bits + (at + i) * stride;
      float f;
      memcpy(&f, &u, 4);
      const volatile double x = mode == 1 ? (double)((1.f - f) / f) : mode == 2 ? 1e-15 + (double)f : (double)f;
      const double want = mode == 1 ? pow(x, half) : log(x);
      if (memcmp(&want, &got[i], 8) && !(want != want && got[i] != got[i]) && !(*mismatches)++) *first_bad = u;
    }
  }
  return 0;
}

#endif  // RN_INSTRUMENT

extern "C" int rnnoise_batch_enable_timing(RNNoiseBatch *b, int on) {
  if (!b) return -1;
  if (batch_flush_timing(b)) return -1;
  b->timing = on != 0;
  for (double &v : b->ms_sum) v = 0;
  b->launches = 0;
  return 0;
}

extern "C" int rnnoise_batch_kernel_ms(RNNoiseBatch *b, double ms[4], long *launches) {
  if (!b || !ms) return -1;
  if (batch_flush_timing(b)) return -1;
  for (int k = 0; k < 4; k++) ms[k] = b->launches ? b->ms_sum[k] / b->launches : 0.0;
  if (launches) *launches = b->launches;
  for (double &v : b->ms_sum) v = 0;
  b->launches = 0;
  return 0;
}

