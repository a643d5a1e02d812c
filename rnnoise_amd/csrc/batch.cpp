// batch.cpp -- rnnoise_batch_*: N streams resident on one GPU; the frame step as a pipeline over HIP streams.
#include "shim.h"
#include "device_choice.h"

namespace {
template <typename T>
T *carve(uint8_t *&p, size_t count) {
  T *r = reinterpret_cast<T *>(p);
  p += (count * sizeof(T) + 255) & ~size_t(255);
  return r;
}

}  // namespace

// the dispatch switches (dispatch.h), read once per process
const RnKnobs &rn_knobs() {
  static const RnKnobs k = rn_knobs_from_env();
  return k;
}
namespace {
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

// A (start, stop) event pair for one kernel launch while timing is enabled; the launch helper hands it to the
// dispatch packet (hipExtLaunchKernel), the pair is read back in rnnoise_batch_kernel_ms.
struct TimedLaunch {
  RNNoiseBatch *b;
  RNNoiseBatch::Ev ev{};
  bool on;
  TimedLaunch(RNNoiseBatch *b_, int kind) : b(b_), on(b_->timing) {
    if (!on) return;
    if (!b->pool.empty()) {
      ev = b->pool.back();
      b->pool.pop_back();
    } else {
      // timing only: no cache writeback / invalidation at the event
      if (hipEventCreateWithFlags(&ev.a, hipEventDisableSystemFence) != hipSuccess ||
          hipEventCreateWithFlags(&ev.b, hipEventDisableSystemFence) != hipSuccess) {
        fprintf(stderr, "[rnnoise_amd] cannot create timing events; this launch is not timed\n");
        if (ev.a) hipEventDestroy(ev.a);
        ev.a = ev.b = nullptr;
        on = false;
        return;
      }
    }
    ev.kind = kind;
  }
  hipEvent_t start() const { return on ? ev.a : nullptr; }
  hipEvent_t stop() const { return on ? ev.b : nullptr; }
  ~TimedLaunch() {
    if (on) b->pending.push_back(ev);
  }
};

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
  if (b->arena) hipFree(b->arena);
  if (b->rs_buf) hipFree(b->rs_buf);
  if (b->rate_map) hipFree(b->rate_map);
  if (b->fmt_map) hipFree(b->fmt_map);
  if (b->model_map) hipFree(b->model_map);
  if (b->ctl_buf) hipFree(b->ctl_buf);
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
  HIP_OK(hipDeviceSynchronize());
  b->img_valid = false;
  b->parity = 0;
  b->ring_slot = 0;
  b->frame_no = 0;
  b->per_stream = false;  // (the only way back to lock-step frame phase)
  return 0;
}

// PCM rate: K0 upsamples the caller's rows from 48000 / L, K3 downsamples its output back (rn_dev.h: RnGroupDev::rs_L).  48 kHz
// without a rate table leaves g.rs_hist / g.rs_L null: every launch is then the one of a batch that never saw these calls.
namespace {
// the group's resampler fields from the batch's rate and whether it has a rate table (rn_dev.h: RnGroupDev::rs_Ls)
void rs_point(RNNoiseBatch *b, bool table) {
  const size_t N = b->n;
  const bool on = table || b->pcm_rate != 48000;
  b->g.rs_L = on ? 48000 / b->pcm_rate : 0;
  b->g.rs_pitch = on ? RN_FRAME_SIZE / b->g.rs_L : 0;
  b->g.rs_hist = on ? b->rs_buf : nullptr;
  b->g.rs_up = on ? b->rs_buf + N * RN_RS_HIST : nullptr;
  b->g.rs_dn = on ? b->rs_buf + N * (RN_RS_HIST + RN_FRAME_SIZE) : nullptr;
  b->g.rs_Ls = table ? b->rate_map : nullptr;
}
// [N][RN_RS_HIST] histories (zero), then the [N][480] planes rs_up and rs_dn (the 48 kHz frames between the filters and the bodies of
// K0 / K3), on first use; the zeroing is ordered on st
int rs_alloc(RNNoiseBatch *b, hipStream_t st) {
  if (b->rs_buf) return 0;
  const size_t N = b->n, bytes = N * RN_RS_HIST * sizeof(float);
  HIP_OK(hipMalloc((void **)&b->rs_buf, bytes + 2 * N * RN_FRAME_SIZE * sizeof(float)));
  HIP_OK(hipMemsetAsync(b->rs_buf, 0, bytes, st));
  return 0;
}
bool rate_divisor_ok(int v, int Lb) { return (v == 1 || v == 2 || v == 3 || v == 6) && v >= Lb; }
}  // namespace

extern "C" int rnnoise_batch_set_pcm_rate(RNNoiseBatch *b, int hz) {
  if (!b || (hz != 48000 && hz != 24000 && hz != 16000 && hz != 8000)) return -1;
  const int old = b->pcm_rate;
  b->frame_stride = b->row_stride = 0;  // (a PCM layout is in samples of the old rate's frame: dropped by every call)
  if (hz == old && !b->g.rs_Ls) return old;  // (a rate table is dropped by every call: the rows are redefined)
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_reset: nothing of the old rate is in flight)
  if (hz != 48000 && rs_alloc(b, nullptr)) return -1;
  if (b->rs_buf) HIP_OK(hipMemset(b->rs_buf, 0, (size_t)b->n * RN_RS_HIST * sizeof(float)));
  HIP_OK(hipDeviceSynchronize());
  b->pcm_rate = hz;
  rs_point(b, false);
  return old;
}

// ---- per-stream rates (include/rnnoise_amd.h) ----
// The table lives in rate_map from the first set on; while one is set the batch runs its resampling launches at 48 kHz too (rs_L = 1),
// and K0 / K3 and the snapshot kernels take each stream's divisor from it (rn_dev.h: rn_stream_L).
extern "C" int rnnoise_batch_set_stream_rates(RNNoiseBatch *b, const unsigned char *rates) {
  if (!b) return -1;
  const int Lb = 48000 / b->pcm_rate;
  if (rates)
    for (int s = 0; s < b->n; s++)
      if (!rate_divisor_ok(rates[s], Lb)) return -1;
  if (!rates && !b->g.rs_Ls) return 0;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_set_stream_models: a call in flight keeps what it was launched with)
  const size_t N = b->n;
  std::vector<uint8_t> cur(N, (uint8_t)Lb);
  if (b->g.rs_Ls) {
    HIP_OK(hipMemcpy(cur.data(), b->rate_map, N, hipMemcpyDeviceToHost));
    for (auto &v : cur)
      if (!rate_divisor_ok(v, Lb)) v = (uint8_t)Lb;  // (what the kernels read an unchecked entry of the device setter as)
  }
  if (rs_alloc(b, nullptr)) return -1;
  if (rates && !b->rate_map) HIP_OK(hipMalloc((void **)&b->rate_map, N));
  // the history of every stream whose divisor changes restarts from zero: one memset per run of such streams
  for (size_t s = 0; s < N;) {
    if (cur[s] == (rates ? rates[s] : Lb)) {
      s++;
      continue;
    }
    size_t e = s + 1;
    while (e < N && cur[e] != (rates ? rates[e] : Lb)) e++;
    HIP_OK(hipMemsetAsync(b->rs_buf + s * RN_RS_HIST, 0, (e - s) * RN_RS_HIST * sizeof(float), nullptr));
    s = e;
  }
  if (rates) HIP_OK(hipMemcpy(b->rate_map, rates, N, hipMemcpyHostToDevice));
  HIP_OK(hipDeviceSynchronize());
  rs_point(b, rates != nullptr);
  return 0;
}

extern "C" int rnnoise_batch_set_stream_rates_device(RNNoiseBatch *b, const unsigned char *d_rates, void *hip_stream) {
  if (!b || !d_rates) return -1;
  ON_DEVICE(b->device);
  // a copy, not a kernel: ordered on the caller's stream between its calls; the kernels read an entry that names no rate of this
  // batch as the batch's own.  Histories are the caller's to reset (include/rnnoise_amd.h).
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (rs_alloc(b, st)) return -1;
  if (!b->rate_map) HIP_OK(hipMalloc((void **)&b->rate_map, (size_t)b->n));
  if (!b->g.rs_Ls) rs_point(b, true);
  HIP_OK(hipMemcpyAsync(b->rate_map, d_rates, (size_t)b->n, hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int rnnoise_batch_stream_rates(RNNoiseBatch *b, unsigned char *rates) {
  if (!b || !rates) return -1;
  const int Lb = 48000 / b->pcm_rate;
  if (!b->g.rs_Ls) {
    memset(rates, Lb, (size_t)b->n);
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(rates, b->rate_map, (size_t)b->n, hipMemcpyDeviceToHost));
  for (int s = 0; s < b->n; s++)
    if (!rate_divisor_ok(rates[s], Lb)) rates[s] = (unsigned char)Lb;  // (as the kernels read it)
  return 0;
}

extern "C" int rnnoise_batch_pcm_rate(const RNNoiseBatch *b) { return b ? b->pcm_rate : -1; }

// ---- caller-defined PCM strides (include/rnnoise_amd.h) ----
// Two numbers of the batch.  A process call hands the row stride to K0 / K3 (rn_dev.h: RnGroupDev::pcm_pitch) and steps its frame
// pointers by the frame stride (batch_process_device_impl); without a layout both keep their defaults and every launch is the one of
// a batch that never saw these calls.
extern "C" int rnnoise_batch_set_pcm_layout(RNNoiseBatch *b, long frame_stride, long row_stride) {
  if (!b || !rn_pcm_layout_ok(frame_stride, row_stride)) return -1;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_set_pcm_rate: a call in flight keeps what it was launched with)
  b->frame_stride = frame_stride;
  b->row_stride = row_stride;
  return 0;
}

extern "C" int rnnoise_batch_pcm_layout(const RNNoiseBatch *b, long *frame_stride, long *row_stride) {
  if (!b) return -1;
  if (frame_stride) *frame_stride = b->frame_stride;
  if (row_stride) *row_stride = b->row_stride;
  return 0;
}

extern "C" int rnnoise_amd_pcm_layout_fits(long frame_stride, long row_stride, int frame_samples, int n_rows, int n_frames) {
  return rn_pcm_layout_ok(frame_stride, row_stride) && (frame_stride || row_stride) &&
                 rn_pcm_layout_fits(frame_stride, row_stride, frame_samples, n_rows, n_frames)
             ? 1
             : 0;
}

// ---- interleaved channels (include/rnnoise_amd.h) ----
// One number of the batch.  A process call hands it to K0 / K3 (rn_dev.h: RnGroupDev::pcm_chan) and to the step's plan (dispatch.h:
// RnStepShape::channels); at 1 nothing is handed on and every launch is the one of a batch that never saw these calls.
extern "C" int rnnoise_batch_set_pcm_channels(RNNoiseBatch *b, int channels) {
  if (!b || !rn_pcm_channels_ok(channels, b->n)) return -1;
  const int old = b->channels;
  if (channels == old) return old;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_set_pcm_layout: a call in flight keeps what it was launched with)
  b->channels = channels;
  return old;
}

extern "C" int rnnoise_batch_pcm_channels(const RNNoiseBatch *b) { return b ? b->channels : -1; }

extern "C" int rnnoise_amd_pcm_channels_fit(long frame_stride, long row_stride, int frame_samples, int channels, int n_rows, int n_frames) {
  return rn_pcm_layout_ok(frame_stride, row_stride) && (frame_stride || row_stride) &&
                 rn_pcm_channels_fit(frame_stride, row_stride, frame_samples, channels, n_rows, n_frames)
             ? 1
             : 0;
}

// ---- per-stream PCM formats (include/rnnoise_amd.h) ----
// The table lives in fmt_map from the first set on; while one is set (g.pcm_fmt) K0 expands and K3 compresses the rows of the
// companded streams in every int16 call (rn_dev.h: rn_stream_fmt), and those calls plan K0 one wave per stream (dispatch.h).  It is
// configuration: nothing is zeroed when it changes, and nothing but these two setters and the batch's end touches it.
extern "C" int rnnoise_batch_set_stream_formats(RNNoiseBatch *b, const unsigned char *formats) {
  if (!b) return -1;
  if (formats)
    for (int s = 0; s < b->n; s++)
      if (formats[s] > RNNOISE_AMD_PCM_ALAW) return -1;
  if (!formats && !b->g.pcm_fmt) return 0;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_set_stream_models: a call in flight keeps what it was launched with)
  if (formats) {
    if (!b->fmt_map) HIP_OK(hipMalloc((void **)&b->fmt_map, (size_t)b->n));
    HIP_OK(hipMemcpy(b->fmt_map, formats, (size_t)b->n, hipMemcpyHostToDevice));
  }
  b->g.pcm_fmt = formats ? b->fmt_map : nullptr;
  return 0;
}

extern "C" int rnnoise_batch_set_stream_formats_device(RNNoiseBatch *b, const unsigned char *d_formats, void *hip_stream) {
  if (!b || !d_formats) return -1;
  ON_DEVICE(b->device);
  // a copy, not a kernel: ordered on the caller's stream between its calls; the kernels read a byte that names no law as int16 rows
  if (!b->fmt_map) HIP_OK(hipMalloc((void **)&b->fmt_map, (size_t)b->n));
  b->g.pcm_fmt = b->fmt_map;
  HIP_OK(hipMemcpyAsync(b->fmt_map, d_formats, (size_t)b->n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

extern "C" int rnnoise_batch_stream_formats(RNNoiseBatch *b, unsigned char *formats) {
  if (!b || !formats) return -1;
  if (!b->g.pcm_fmt) {
    memset(formats, 0, (size_t)b->n);
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(formats, b->fmt_map, (size_t)b->n, hipMemcpyDeviceToHost));
  for (int s = 0; s < b->n; s++)
    if (formats[s] > RNNOISE_AMD_PCM_ALAW) formats[s] = RNNOISE_AMD_PCM_LINEAR;  // (as the kernels read it)
  return 0;
}

// ---- per-stream models (include/rnnoise_amd.h) ----
// The network of every step is launched once per slot (batch_process_device_impl); the launch of slot k owns the streams the map puts
// on k (rn_dev.h: rn_owns).  The map exists from the first add_model on; before that every stream is on slot 0 and nothing is read.
extern "C" int rnnoise_batch_add_model(RNNoiseBatch *b, RNNModel *model) {
  if (!b || !model || b->n_models >= RNNOISE_AMD_MAX_MODELS) return -1;
  ON_DEVICE(b->device);
  RnModelDev md;
  if (model_on_device(model, b->device, md)) return -1;
  HIP_OK(hipDeviceSynchronize());  // (synchronous: a call in flight keeps the slots it was launched with)
  if (!b->model_map) {
    HIP_OK(hipMalloc((void **)&b->model_map, (size_t)b->n));
    HIP_OK(hipMemset(b->model_map, 0, (size_t)b->n));
    HIP_OK(hipDeviceSynchronize());
  }
  const int k = b->n_models++;
  b->models[k] = model;
  b->slot_m[k] = md;
  b->g.model_of = b->model_map;
  b->g.n_models = b->n_models;
  return k;
}

extern "C" int rnnoise_batch_set_stream_models(RNNoiseBatch *b, const unsigned char *models) {
  if (!b || !models) return -1;
  for (int s = 0; s < b->n; s++)
    if (models[s] >= b->n_models) return -1;
  if (!b->model_map) return 0;  // (one slot: every entry is 0, which is what the batch runs)
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_reset_streams)
  HIP_OK(hipMemcpy(b->model_map, models, (size_t)b->n, hipMemcpyHostToDevice));
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" int rnnoise_batch_set_stream_models_device(RNNoiseBatch *b, const unsigned char *d_models, void *hip_stream) {
  if (!b || !d_models) return -1;
  if (!b->model_map) return 0;  // (one slot: any entry reads as slot 0)
  ON_DEVICE(b->device);
  // a copy, not a kernel: ordered on the caller's stream between its calls; entries naming no slot are read as slot 0 by the kernels
  HIP_OK(hipMemcpyAsync(b->model_map, d_models, (size_t)b->n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

extern "C" int rnnoise_batch_stream_models(RNNoiseBatch *b, unsigned char *models) {
  if (!b || !models) return -1;
  if (!b->model_map) {
    memset(models, 0, (size_t)b->n);
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(models, b->model_map, (size_t)b->n, hipMemcpyDeviceToHost));
  return 0;
}

// ---- per-stream suppression controls (include/rnnoise_amd.h) ----
// The table and the counters live in ctl_buf from the first set on; g.ctl / g.gate_c point into it while a table is set, and K3 reads
// them (rn_dev.h: RnGroupDev::ctl).  Without a table both are null and every launch is the one of a batch that never saw these calls.
static_assert(RN_CTL_FLOATS == RNNOISE_AMD_CTL_FLOATS, "one record size for the kernels and the API");
namespace {
bool ctl_entry_ok(const float *e) {
  const float floor_gain = e[0], thr = e[1], hold = e[2];
  return std::isfinite(floor_gain) && std::isfinite(thr) && std::isfinite(hold) && floor_gain >= 0.f && floor_gain <= 1.f &&
         thr >= 0.f && thr <= 1.f && hold >= 0.f && hold <= 65535.f && hold == std::floor(hold);
}
// memory on first use; a table set after none (or after a NULL set) starts every counter at RN_CTL_NONE, ordered on st
int ctl_arm(RNNoiseBatch *b, hipStream_t st) {
  const size_t N = b->n;
  if (!b->ctl_buf) HIP_OK(hipMalloc((void **)&b->ctl_buf, N * RN_CTL_FLOATS * sizeof(float) + N * sizeof(int)));
  if (!b->g.ctl) {
    int *c = reinterpret_cast<int *>(b->ctl_buf + N * RN_CTL_FLOATS);
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c), RN_CTL_NONE, N, st));
    b->g.ctl = b->ctl_buf;
    b->g.gate_c = c;
  }
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_set_stream_controls(RNNoiseBatch *b, const float *ctl) {
  if (!b) return -1;
  if (ctl)
    for (int s = 0; s < b->n; s++)
      if (!ctl_entry_ok(ctl + (size_t)s * RN_CTL_FLOATS)) return -1;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_set_stream_models: a call in flight keeps what it was launched with)
  if (!ctl) {  // no table: the launches of a batch without one; the counters go with it
    b->g.ctl = nullptr;
    b->g.gate_c = nullptr;
    return 0;
  }
  if (ctl_arm(b, nullptr)) return -1;
  HIP_OK(hipMemcpy(b->ctl_buf, ctl, (size_t)b->n * RN_CTL_FLOATS * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" int rnnoise_batch_set_stream_controls_device(RNNoiseBatch *b, const float *d_ctl, void *hip_stream) {
  if (!b || !d_ctl) return -1;
  ON_DEVICE(b->device);
  // a copy, not a kernel: ordered on the caller's stream between its calls; K3 sanitises what it reads (NaN as 0, clamped, truncated)
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (ctl_arm(b, st)) return -1;
  HIP_OK(hipMemcpyAsync(b->ctl_buf, d_ctl, (size_t)b->n * RN_CTL_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int rnnoise_batch_stream_controls(RNNoiseBatch *b, float *ctl) {
  if (!b || !ctl) return -1;
  const size_t bytes = (size_t)b->n * RN_CTL_FLOATS * sizeof(float);
  if (!b->g.ctl) {
    memset(ctl, 0, bytes);
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(ctl, b->ctl_buf, bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rnnoise_batch_set_schedule(RNNoiseBatch *b, int schedule) {
  if (!b || (schedule != 0 && schedule != 1 && schedule != 9)) return -1;
  const int old = b->schedule;
  b->schedule = schedule;
  return old;
}

extern "C" int rnnoise_batch_set_nn_path(RNNoiseBatch *b, int path) {
  if (!b || path < 0 || path > 2) return -1;  // 0 vector, 1 MFMA (layer-wise from $RNNOISE_AMD_NN_LAYERS_MIN streams up), 2 layer-wise
  int old = b->nn_path;
  b->nn_path = path;
  return old;
}

// PCM frames are float (the reference API's sample type) or, with s16 set, int16 converted at the two ends of the step as the
// reference's only caller does (examples/rnnoise_demo.c:56,58): half the bytes over HBM and, in the host-fed path, PCIe.
// d_active: the presence mask of a masked call ([n_frames][N] bytes, include/rnnoise_amd.h), or null.
// d_list: the streams of a stream-list call (n_rows int32 on the device, include/rnnoise_amd.h), or null; the caller's buffers and
// d_active then have n_rows rows per frame (rn_dev.h: RnGroupDev::list).
int batch_process_device_impl(RNNoiseBatch *b, void *d_out_v, const void *d_in_v, float *d_vad, float *d_gains, int n_frames,
                              void *hip_stream, bool s16, const FrameIoHooks *hk, const uint8_t *d_active, const int *d_list,
                              int n_rows, bool packed) {
  if (!b || n_frames < 0) return -1;
  const bool listed = d_list || n_rows;
  if (listed) {
    if (n_rows < 0 || n_rows > b->n || (n_rows > 0 && !d_list)) return -1;
    if (n_rows == 0) return 0;
  }
  if (!d_out_v || !d_in_v) return -1;
  // the caller's PCM layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout), unless the buffers are the library's own (packed:
  // the staged host path; hk: the pinned ring).  Its frame slots must be disjoint, checked before anything is launched or changed
  // Interleaved channels (rnnoise_batch_set_pcm_channels): the rows are taken `chan` at a time, in the library's staging buffer
  // (packed) as in the caller's; the strides then place group slots of chan rows.  The pinned ring (hk) never sees channels
  const int chan = hk ? 1 : b->channels;
  if (listed && n_rows % chan) return -1;
  const bool laid = b->row_stride && !packed && !hk;
  if (laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, RN_FRAME_SIZE / (b->g.rs_L ? b->g.rs_L : 1), chan,
                                   listed ? n_rows : b->n, n_frames))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  if ((d_active || listed) && !b->per_stream && n_frames > 0) {
    // the first masked or list call puts the batch into per-stream frame phase: every stream starts at the batch's phase.  ring_slot, not
    // frame_no: the training-feature calls advance the slots without counting frames (ring_slot % 3 == parity always)
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->phase_buf), b->ring_slot, b->n, st));
    b->per_stream = true;
  }
  // the phase fields of the group a kernel of frame f gets (all null / 0 in lock-step mode: today's launches)
  auto phased = [&](RnGroupDev &g, int f) {
    if (!b->per_stream) return;
    g.phase = b->phase_buf;
    g.active = d_active;
    g.call_frame = f;
    g.call_frames = n_frames;
    if (listed) {
      g.list = d_list;
      g.list_n = n_rows;
    }
  };
  const size_t N = listed ? n_rows : b->n, esz = s16 ? sizeof(short) : sizeof(float);  // (N: rows of the caller's buffers)
  const size_t fl = RN_FRAME_SIZE / (b->g.rs_L ? b->g.rs_L : 1);  // samples per stream and frame at the batch's PCM rate
  const char *d_in = static_cast<const char *>(d_in_v);
  char *d_out = static_cast<char *>(d_out_v);
  auto buf = [&](int f) -> size_t { return hk ? (size_t)(f % hk->ring) : (size_t)f; };  // frame f's place in the caller's buffers
  // bytes between the frames of the PCM buffers, and the row pitch K0 / K3 get (0: the form's own constant -- today's arguments)
  const size_t fstep = (laid ? (size_t)b->frame_stride : N * fl) * esz;
  const int pcm_pitch = laid ? (int)b->row_stride : 0;
  const int pcm_chan = chan > 1 ? chan : 0;  // (rn_dev.h: RnGroupDev::pcm_chan -- 0: today's addressing)
  // Multi-frame calls are software-pipelined over three streams: C runs the high-pass of frames up to
  // f+2, B the analysis of frame f+1, A (the caller's stream) network + synthesis of frame f.
  // What makes that legal:
  //   * the pitch ring has 6 slots and analysis(g) reads slots g-3..g, so high-pass(f) only has to wait
  //     for analysis(f-3);
  //   * the spectra rotate through 3 slots and the per-step scratch (features, silence, pitch) is
  //     double-buffered, so analysis(f) only has to wait for synthesis(f-2);
  //   * every other piece of state is touched by one kernel only, in frame order on its own stream.
  // (dispatch.h: rn_schedule has the other schedules and rn_plan every kernel's form; one plan serves every frame of the call.  The
  // layer images are indexed by tile of the whole batch; the layer kernels use 32-bit byte offsets into a state plane)
  const RnSchedule sched = rn_schedule(rn_knobs(), n_frames, b->schedule);
  const bool pipelined = sched.pipelined, side_k1 = sched.side_k1;
  const bool whole = b->g.n_streams == b->g.n_stride && (size_t)b->g.n_streams * RN_GRU * 4 < (1ull << 32);
  RnStepShape shape{(int)N, whole && !listed, b->cus, b->nn_path, pipelined, b->per_stream,
                    rn_shape_low_rate(b->pcm_rate, b->g.rs_Ls != nullptr)};
  shape.listed = listed;
  shape.companded = s16 && b->g.pcm_fmt != nullptr;  // (float calls never look at the format table)
  shape.channels = chan;
  const RnPlan plan = rn_plan(rn_knobs(), shape);
  // the two side streams at normal queue priority (the caller's stream, which carries network + synthesis, is whatever the caller
  // made it: normal for torch's)
  if (side_k1 && !b->side) HIP_OK(hipStreamCreateWithPriority(&b->side, hipStreamNonBlocking, 0));
  if (pipelined && !b->side_hp) {
    HIP_OK(hipStreamCreateWithPriority(&b->side_hp, hipStreamNonBlocking, 0));
    // ordering between streams of ONE device: no system-scope fence (it writes back and invalidates the caches at
    // every record, which the next kernels then pay for)
    const unsigned evf = hipEventDisableTiming | (unsigned)hipEventDisableSystemFence;
    HIP_OK(hipEventCreateWithFlags(&b->ev_begin, evf));
    for (int k = 0; k < 8; k++) {
      HIP_OK(hipEventCreateWithFlags(&b->own_hp[k], evf));
      HIP_OK(hipEventCreateWithFlags(&b->own_k1[k], evf));
      HIP_OK(hipEventCreateWithFlags(&b->own_k3[k], evf));
    }
  }
  hipStream_t sb = side_k1 ? b->side : st, sc = pipelined ? b->side_hp : st;
  if (pipelined) {  // B and C start after everything already queued on the caller's stream
    HIP_OK(hipEventRecord(b->ev_begin, st));
    if (side_k1) HIP_OK(hipStreamWaitEvent(b->side, b->ev_begin, 0));
    HIP_OK(hipStreamWaitEvent(b->side_hp, b->ev_begin, 0));
  }
  auto frame_group = [&](int f) {
    RnGroupDev g = b->g;
    g.pcm_pitch = pcm_pitch;
    g.pcm_chan = pcm_chan;
    const int c = (int)((b->frame_no + f) & 1);
    g.features = b->features2[c];
    g.silence = b->silence2[c];
    g.pitch = b->pitch2[c];
    g.vad = d_vad ? d_vad + buf(f) * N : b->scratch_vad;
    g.gains = d_gains ? d_gains + buf(f) * N * RN_NB_BANDS : b->scratch_gains;
    phased(g, f);
    if (listed) {  // the network writes the per-stream scratch, K3 copies the listed rows out (rn_dev.h: RnGroupDev::list)
      g.list_vad = d_vad ? g.vad : nullptr;
      g.list_gains = d_gains ? g.gains : nullptr;
      g.vad = b->scratch_vad;
      g.gains = b->scratch_gains;
    }
    return g;
  };
  auto highpass = [&](int f) -> int {  // K0 of frame f on stream sc
    // completion events ride in the dispatch packets (stop event of hipExtLaunchKernel): no record packets between
    // the kernels of a stream
    if (pipelined && f >= 3) HIP_OK(hipStreamWaitEvent(sc, b->cur_k1[(f - 3) & 7], 0));
    // ... and not before synthesis(f-4) is done, which is when analysis(f-2) starts: left to the ring alone, the high-pass
    // starts the moment analysis(f-3) ends -- together with the GRU layer kernels of frame f-4.  Its 1024 waves are one per
    // SIMD for 0.18 ms, and a GRU workgroup (2 waves x 240 VGPRs per SIMD) does not fit beside even one of them: the first
    // layer kernel of every frame waited that long (rocprofv3 timeline: 283 us instead of 115).  Beside the analysis kernel
    // (4 waves x 56 VGPRs per SIMD) it costs nothing.
    if (side_k1 && f >= 4) HIP_OK(hipStreamWaitEvent(sc, b->cur_k3[(f - 4) & 7], 0));
    // ... and the same concern when only the high-pass runs aside (schedule 1: the host-fed path): there analysis(f-2) follows
    // synthesis(f-3) on the main stream, so that is the event to start behind -- the high-pass of frame f is launched after it (see the
    // frame loop).  Started at the ring's earliest moment it ran beside the layer kernels of frame f-3: network 0.73 ms instead of 0.57
    // (profiles/r5_hostio_sdma.txt).
    if (pipelined && !side_k1 && f >= 3) HIP_OK(hipStreamWaitEvent(sc, b->cur_k3[(f - 3) & 7], 0));
    if (hk && hk->before_hp(f, sc)) return -1;
    {
      TimedLaunch t(b, 3);
      b->cur_hp[f & 7] = t.on ? t.stop() : (pipelined ? b->own_hp[f & 7] : nullptr);
      RnGroupDev gh = b->g;
      gh.pcm_pitch = pcm_pitch;
      gh.pcm_chan = pcm_chan;
      phased(gh, f);
      HIP_OK(rn_launch_hp(&gh, d_in + buf(f) * fstep, s16, (b->ring_slot + f) % RN_RING_SLOTS, plan.hp, sc, t.start(),
                          b->cur_hp[f & 7]));
    }
    if (hk && hk->after_hp(f, sc)) return -1;
    return 0;
  };
  auto analysis = [&](int f) -> int {  // K1 of frame f on stream sb
    RnGroupDev g = frame_group(f);
    if (pipelined) {
      HIP_OK(hipStreamWaitEvent(sb, b->cur_hp[f & 7], 0));
      if (side_k1 && f >= 2) HIP_OK(hipStreamWaitEvent(sb, b->cur_k3[(f - 2) & 7], 0));
    }
    {
      TimedLaunch t(b, 0);
      b->cur_k1[f & 7] = t.on ? t.stop() : (pipelined ? b->own_k1[f & 7] : nullptr);
      HIP_OK(rn_launch_analysis(&g, &b->tb, (b->ring_slot + f) % RN_RING_SLOTS, (b->parity + f) % RN_SPEC_SLOTS, plan.k1, sb, t.start(),
                                b->cur_k1[f & 7]));
    }
    return 0;
  };
  if (pipelined) {
    for (int f = 0; f < 3 && f < n_frames; f++)
      if (highpass(f)) return -1;
    if (analysis(0)) return -1;
  }
  for (int f = 0; f < n_frames; f++) {
    RnGroupDev g = frame_group(f);
    const int cur = (b->parity + f) % RN_SPEC_SLOTS, prev = (cur + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
    if (!pipelined) {
      if (highpass(f) || analysis(f)) return -1;
    } else {
      if (side_k1 && f + 3 < n_frames && highpass(f + 3)) return -1;
      if (f + 1 < n_frames && analysis(f + 1)) return -1;
      if (side_k1) HIP_OK(hipStreamWaitEvent(st, b->cur_k1[f & 7], 0));
    }
    if (hk && hk->before_nn(f, st)) return -1;
    // the network once per model slot (one slot without a map: exactly the launches of a one-model batch).  Slot k's launch owns the
    // streams the map puts on k (rn_dev.h: rn_owns).  Layer-wise, a slot's whole network runs before the next slot's front: act_q[0]
    // and nn_act are the tile's scratch, which the next front overwrites for every column.
    for (int k = 0; k < b->n_models; k++) {
      g.model_sel = k;
      const RnModelDev *mk = k ? &b->slot_m[k] : &b->m;
      if (plan.nn == RN_NN_LAYERS) {
        if (!b->img_valid) HIP_OK(rn_launch_nn_requant(&g, st));
        b->img_valid = true;
        // five launches, each timed on its own (kind 1: the durations add up to the network's)
        std::unique_ptr<TimedLaunch> tl[5];
        hipEvent_t ev[5][2] = {};
        for (int i = 0; i < 5; i++) {
          tl[i].reset(new TimedLaunch(b, 1));
          ev[i][0] = tl[i]->start();
          ev[i][1] = tl[i]->stop();
        }
        HIP_OK(rn_launch_nn_layers(&g, mk, &b->tb, plan.gru, b->lds_gru, st, ev));
      } else {
        TimedLaunch t(b, 1);
        b->img_valid = b->img_valid && listed;  // (a list call re-quantises its rows' tiles behind its last frame, below)
        if (plan.nn == RN_NN_ONE) HIP_OK(rn_launch_nn_one(&g, mk, &b->tb, b->lds_one, st, t.start(), t.stop()));
        else if (plan.nn == RN_NN_VECTOR) HIP_OK(rn_launch_nn_vector(&g, mk, &b->tb, st, t.start(), t.stop()));
        else HIP_OK(rn_launch_nn_mfma(&g, mk, &b->tb, plan.nn, st, t.start(), t.stop()));
      }
    }
    {
      TimedLaunch t(b, 2);
      b->cur_k3[f & 7] = t.on ? t.stop() : (pipelined ? b->own_k3[f & 7] : nullptr);
      HIP_OK(rn_launch_synthesis(&g, &b->tb, d_out + buf(f) * fstep, s16, cur, prev, plan.k3, st, t.start(), b->cur_k3[f & 7]));
    }
    if (hk && hk->after_k3(f, st)) return -1;
    // (schedule 1: the high-pass three frames ahead goes out HERE, behind the synthesis launch whose end it starts at)
    if (pipelined && !side_k1 && f + 3 < n_frames && highpass(f + 3)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  // a list call keeps the layer-wise network's state images: only its rows' tiles are rebuilt (rn_dev.h: act_q), as after
  // rnnoise_batch_reset_streams -- not the whole batch at the next lock-step step
  if (listed && b->img_valid && n_frames > 0) HIP_OK(rn_launch_nn_requant(&b->g, st, d_list, n_rows));
  b->parity = (b->parity + n_frames) % RN_SPEC_SLOTS;
  b->ring_slot = (b->ring_slot + n_frames) % RN_RING_SLOTS;
  b->frame_no += n_frames;
  return 0;
}

extern "C" int rnnoise_batch_process_device(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad,
                                            float *d_gains, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, false);
}

extern "C" int rnnoise_batch_process_device_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                float *d_gains, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, true);
}

// ---- masked calls and per-stream reset (include/rnnoise_amd.h) ----
extern "C" int rnnoise_batch_process_device_masked(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad, float *d_gains,
                                                   const unsigned char *d_active, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, false, nullptr, d_active);
}

extern "C" int rnnoise_batch_process_device_masked_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                       float *d_gains, const unsigned char *d_active, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, true, nullptr, d_active);
}

// The convenience form on host buffers: everything staged through one device allocation with plain synchronous copies (no pinned
// ring, no copy engines -- rnnoise_batch_process is the fast host path).  `out` goes up too, so that its absent rows come back as
// the caller left them.  The masked host calls, every host call at a PCM rate other than 48 kHz or with a rate table, the int16
// host calls of a batch with a format table, and every host call of a batch with a PCM layout or with interleaved channels come here.
// A list call (list set: n_rows host int32 entries, checked by the caller) stages the list too, and its buffers have n_rows rows.
int batch_process_staged(RNNoiseBatch *b, void *out, const void *in, float *vad, float *gains, const unsigned char *active,
                         int n_frames, bool s16, const int *list, int n_rows) {
  if (!b || !out || !in || n_frames < 0) return -1;
  if (n_frames == 0) return 0;
  const size_t rows = list ? n_rows : b->n;
  const size_t M = RN_FRAME_SIZE / (b->g.rs_L ? b->g.rs_L : 1), esz = s16 ? 2 : 4;
  // a caller-defined layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout): the frame slots travel by strided copies between
  // the caller's buffers and the default layout in device memory -- one 2-D copy per frame, its rows row_stride apart --, so the
  // device runs the launches of the default layout and nothing but the slots themselves is read or written on the host
  // Interleaved channels (rnnoise_batch_set_pcm_channels): what travels is the group slot, C rows of M samples interleaved, and the
  // device works on the staging buffer with the same channel count (batch_process_device_impl: packed) -- no de-interleave here
  const size_t C = b->channels;
  if (rows % C) return -1;
  const bool laid = b->row_stride != 0;
  if (laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, (int)M, (int)C, (int)rows, n_frames)) return -1;
  ON_DEVICE(b->device);
  auto pcm_copy = [&](void *dst, const void *src, bool up) -> bool {
    if (!laid) return hipMemcpy(dst, src, (size_t)n_frames * rows * M * esz, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost) == hipSuccess;
    const size_t hp = (size_t)b->row_stride * esz, hf = (size_t)b->frame_stride * esz, dp = M * C * esz, df = rows * M * esz;
    for (int f = 0; f < n_frames; f++) {
      const hipError_t e = up ? hipMemcpy2D(static_cast<char *>(dst) + f * df, dp, static_cast<const char *>(src) + f * hf, hp, dp, rows / C,
                                            hipMemcpyHostToDevice)
                              : hipMemcpy2D(static_cast<char *>(dst) + f * hf, hp, static_cast<const char *>(src) + f * df, dp, dp, rows / C,
                                            hipMemcpyDeviceToHost);
      if (e != hipSuccess) return false;
    }
    return true;
  };
  const size_t fs = (size_t)n_frames * rows, pcm = fs * M * esz;
  const size_t o_in = 0, o_out = pcm, o_vad = 2 * pcm, o_gains = o_vad + fs * 4, o_act = o_gains + fs * RN_NB_BANDS * 4,
               o_list = (o_act + fs + 255) & ~size_t(255), total = o_list + (list ? rows * sizeof(int) : 0);
  char *d = nullptr;
  HIP_OK(hipMalloc((void **)&d, total));
  int rc = -1;
  if (pcm_copy(d + o_in, in, true) &&
      // (absent rows, and the part of a row behind the frame of a stream of a rate table or behind a companded stream's bytes, keep
      //  the caller's values)
      ((!active && !list && !b->g.rs_Ls && !(s16 && b->g.pcm_fmt)) || pcm_copy(d + o_out, out, true)) &&
      (!active || hipMemcpy(d + o_act, active, fs, hipMemcpyHostToDevice) == hipSuccess) &&
      (!list || hipMemcpy(d + o_list, list, rows * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) &&
      batch_process_device_impl(b, d + o_out, d + o_in, vad ? (float *)(d + o_vad) : nullptr, gains ? (float *)(d + o_gains) : nullptr,
                                n_frames, nullptr, s16, nullptr, active ? (const uint8_t *)(d + o_act) : nullptr,
                                list ? (const int *)(d + o_list) : nullptr, list ? n_rows : 0, true) == 0 &&
      hipDeviceSynchronize() == hipSuccess && pcm_copy(out, d + o_out, false) &&
      (!vad || hipMemcpy(vad, d + o_vad, fs * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
      (!gains || hipMemcpy(gains, d + o_gains, fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost) == hipSuccess))
    rc = 0;
  hipFree(d);
  return rc;
}

namespace {
int batch_process_masked_host(RNNoiseBatch *b, void *out, const void *in, float *vad, float *gains, const unsigned char *active,
                              int n_frames, bool s16) {
  if (!b || !out || !in || n_frames < 0) return -1;
  if (!active) return s16 ? rnnoise_batch_process_s16(b, (short *)out, (const short *)in, vad, gains, n_frames)
                          : rnnoise_batch_process(b, (float *)out, (const float *)in, vad, gains, n_frames);
  return batch_process_staged(b, out, in, vad, gains, active, n_frames, s16);
}

// zero state for the n streams of the device list d_list, on st; the layer-wise network's state images of their tiles follow
// (rn_dev.h: act_q) while they are in use, so that a reset costs no re-quantisation of the whole batch at the next step
int reset_streams_on(RNNoiseBatch *b, const int *d_list, int n, hipStream_t st) {
  HIP_OK(rn_launch_state_zero(&b->g, d_list, n, st));
  if (b->img_valid) HIP_OK(rn_launch_nn_requant(&b->g, st, d_list, n));
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_process_masked(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains,
                                            const unsigned char *active, int n_frames) {
  return batch_process_masked_host(b, out, in, vad, gains, active, n_frames, false);
}

extern "C" int rnnoise_batch_process_masked_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                                const unsigned char *active, int n_frames) {
  return batch_process_masked_host(b, out, in, vad, gains, active, n_frames, true);
}

// ---- stream-list calls (include/rnnoise_amd.h) ----
extern "C" int rnnoise_batch_process_device_list(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad, float *d_gains,
                                                 const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                 void *hip_stream) {
  if (!d_streams && n_rows == 0) return b ? 0 : -1;
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, false, nullptr, d_active, d_streams, n_rows);
}

extern "C" int rnnoise_batch_process_device_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad, float *d_gains,
                                                     const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                     void *hip_stream) {
  if (!d_streams && n_rows == 0) return b ? 0 : -1;
  return batch_process_device_impl(b, d_out, d_in, d_vad, d_gains, n_frames, hip_stream, true, nullptr, d_active, d_streams, n_rows);
}

namespace {
// the host list is checked before anything moves: an entry outside the batch or a stream listed twice refuses the call
int batch_process_list_host(RNNoiseBatch *b, void *out, const void *in, float *vad, float *gains, const int *streams, int n_rows,
                            const unsigned char *active, int n_frames, bool s16) {
  if (!b || n_rows < 0 || n_rows > b->n || (n_rows > 0 && !streams) || n_frames < 0) return -1;
  if (n_rows == 0) return 0;
  std::vector<uint8_t> seen((size_t)b->n, 0);
  for (int i = 0; i < n_rows; i++) {
    const int s = streams[i];
    if (s < 0 || s >= b->n || seen[s]) return -1;
    seen[s] = 1;
  }
  return batch_process_staged(b, out, in, vad, gains, active, n_frames, s16, streams, n_rows);
}
}  // namespace

extern "C" int rnnoise_batch_process_list(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains, const int *streams,
                                          int n_rows, const unsigned char *active, int n_frames) {
  return batch_process_list_host(b, out, in, vad, gains, streams, n_rows, active, n_frames, false);
}

extern "C" int rnnoise_batch_process_list_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                              const int *streams, int n_rows, const unsigned char *active, int n_frames) {
  return batch_process_list_host(b, out, in, vad, gains, streams, n_rows, active, n_frames, true);
}

extern "C" int rnnoise_batch_reset_streams(RNNoiseBatch *b, const int *streams, int n) {
  if (!b || n < 0 || (n > 0 && !streams)) return -1;
  for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= b->n) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous, like rnnoise_batch_reset and import_state)
  int *d = nullptr;
  HIP_OK(hipMalloc((void **)&d, (size_t)n * sizeof(int)));
  int rc = -1;
  if (hipMemcpy(d, streams, (size_t)n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess && reset_streams_on(b, d, n, nullptr) == 0 &&
      hipDeviceSynchronize() == hipSuccess)
    rc = 0;
  hipFree(d);
  return rc;
}

extern "C" int rnnoise_batch_reset_streams_device(RNNoiseBatch *b, const int *d_streams, int n, void *hip_stream) {
  if (!b || n < 0 || (n > 0 && !d_streams)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return reset_streams_on(b, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

// ---- training-feature extraction (reference loop src/dump_features.c:466-491) ----
extern "C" int rnnoise_batch_train_features_device(RNNoiseBatch *b, float *d_records, const float *d_clean,
                                                   const float *d_noisy, const float *d_vad, const int *d_lowpass,
                                                   const int *d_band_lp, const int *d_noise_free, int n_frames,
                                                   void *hip_stream) {
  if (!b || !d_records || !d_clean || !d_noisy || !d_vad || !d_lowpass || !d_band_lp || !d_noise_free || n_frames < 0)
    return -1;
  if (b->per_stream || b->g.rs_L || b->row_stride || b->channels > 1) return -1;  // (extraction runs in lock-step frame phase, at 48 kHz, in the default PCM layout, one row per slot, only)
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  const size_t N = b->n;
  for (int f = 0; f < n_frames; f++) {
    RnTrainArgs tr;
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

extern "C" int rnnoise_batch_train_features(RNNoiseBatch *b, float *records, const float *clean, const float *noisy,
                                            const float *vad, const int *lowpass, const int *band_lp,
                                            const int *noise_free, int n_frames) {
  if (!b || !records || !clean || !noisy || !vad || !lowpass || !band_lp || !noise_free || n_frames <= 0 || b->per_stream || b->g.rs_L || b->row_stride || b->channels > 1)
    return -1;
  ON_DEVICE(b->device);
  const size_t N = b->n, fb = (size_t)n_frames * N * RN_FRAME_SIZE * 4;
  char *dev = nullptr;
  const size_t o_clean = 0, o_noisy = fb, o_vad = 2 * fb, o_rec = o_vad + (size_t)n_frames * N * 4,
               o_lp = o_rec + (size_t)n_frames * N * 98 * 4, o_bl = o_lp + N * 4, o_nf = o_bl + N * 4, total = o_nf + N * 4;
  HIP_OK(hipMalloc((void **)&dev, total));
  int rc = -1;
  if (hipMemcpy(dev + o_clean, clean, fb, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dev + o_noisy, noisy, fb, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dev + o_vad, vad, (size_t)n_frames * N * 4, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dev + o_lp, lowpass, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dev + o_bl, band_lp, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dev + o_nf, noise_free, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
      rnnoise_batch_train_features_device(b, (float *)(dev + o_rec), (const float *)(dev + o_clean),
                                          (const float *)(dev + o_noisy), (const float *)(dev + o_vad),
                                          (const int *)(dev + o_lp), (const int *)(dev + o_bl), (const int *)(dev + o_nf),
                                          n_frames, nullptr) == 0 &&
      hipDeviceSynchronize() == hipSuccess &&
      hipMemcpy(records, dev + o_rec, (size_t)n_frames * N * 98 * 4, hipMemcpyDeviceToHost) == hipSuccess)
    rc = 0;
  hipFree(dev);
  return rc;
}

#define D2H(dst, src, count) HIP_OK(hipMemcpy(dst, src, (count) * 4, hipMemcpyDeviceToHost))
#define H2D(dst, src, count) HIP_OK(hipMemcpy(dst, src, (count) * 4, hipMemcpyHostToDevice))

namespace {
// what every state produced by the reference or by export_state satisfies, and what lets the batch not store analysis_mem (rn_dev.h)
bool analysis_is_pitch_tail(const float *f) {
  return !memcmp(f + RN_OFF_ANALYSIS, f + RN_OFF_PITCH_BUF + RN_PITCH_BUF_SIZE - RN_FRAME_SIZE, RN_FRAME_SIZE * sizeof(float));
}
// the one-state staging row of export / import (16-byte aligned, as the scatter kernel wants its records)
int stage_ready(RNNoiseBatch *b) {
  if (!b->state_stage) HIP_OK(hipMalloc((void **)&b->state_stage, RN_STATE_FLOATS * sizeof(float)));
  return 0;
}
// where the state kernels find the frame phases of streams s, s + 1, ... in per-stream mode (they read them on the device; null in
// lock-step mode, where the launch carries b->ring_slot: the slots its next frame writes, ring slot p % RN_RING_SLOTS, spectra slot
// p % RN_SPEC_SLOTS)
const int *phase_of(const RNNoiseBatch *b, int s) { return b->per_stream ? b->phase_buf + s : nullptr; }
}  // namespace

// State migration: one gather / scatter kernel (state_kernels.hip) and one copy per call.  Synchronous with everything
// the batch has in flight (the caller's streams are not known here, so the device is drained first).
extern "C" int rnnoise_batch_export_state(RNNoiseBatch *b, int s, float *f) {
  if (!b || !f || s < 0 || s >= b->n) return -1;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (stage_ready(b)) return -1;
  const RnGroupDev v = group_view(b->g, s, 1);
  HIP_OK(rn_launch_state_gather(&v, RN_REC_STATE, b->state_stage, nullptr, 1, b->ring_slot, phase_of(b, s), nullptr));
  D2H(f, b->state_stage, RN_STATE_FLOATS);  // (a blocking copy on the null stream: ordered after the kernel)
  return 0;
}

extern "C" int rnnoise_batch_import_state(RNNoiseBatch *b, int s, const float *f) {
  if (!b || !f || s < 0 || s >= b->n) return -1;
  if (!analysis_is_pitch_tail(f)) {
    fprintf(stderr, "[rnnoise_amd] import_state: analysis_mem differs from the tail of pitch_buf\n");
    return -1;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  if (stage_ready(b)) return -1;
  H2D(b->state_stage, f, RN_STATE_FLOATS);
  b->img_valid = false;
  const RnGroupDev v = group_view(b->g, s, 1);
  HIP_OK(rn_launch_state_scatter(&v, RN_REC_STATE, b->state_stage, nullptr, 1, b->ring_slot, phase_of(b, s), nullptr));
  HIP_OK(hipStreamSynchronize(nullptr));
  return 0;
}

// ---- stream snapshots (include/rnnoise_amd.h: rnnoise_batch_save_streams) ----
// The device forms are two launches at the most, ordered on the caller's stream like rnnoise_batch_reset_streams_device.  Nothing
// has to be joined here: a pipelined call ends with the synthesis of its last frame on the caller's stream, which waited for that
// frame's analysis (cur_k1) on the side stream, which waited for its high-pass (cur_hp) on the other one -- both side streams run
// in frame order, so everything the call queued anywhere is complete before a kernel that follows it on the caller's stream; and the
// next pipelined call records ev_begin on the caller's stream behind these launches and makes both side streams wait for it.
static_assert(RNNOISE_AMD_SNAP_FLOATS == RN_SNAP_FLOATS && RN_SNAP_FLOATS % 4 == 0, "one record size for the kernels and the API");
namespace {
bool snap_args_ok(const RNNoiseBatch *b, const void *snap, const int *streams, int n) {
  if (!b || n < 0 || n > b->n || (n > 0 && !snap)) return false;
  if (n > 0 && !streams && n != b->n) return false;  // (no list: the whole batch, stream i = row i)
  return true;
}
int save_on(RNNoiseBatch *b, float *d_snap, const int *d_list, int n, hipStream_t st) {
  HIP_OK(rn_launch_state_gather(&b->g, RN_REC_SNAP, d_snap, d_list, n, b->ring_slot, phase_of(b, 0), st));
  return 0;
}
// the listed rows' tiles of the layer-wise network's state images follow the load while they are live (rn_dev.h: act_q), as after
// a per-stream reset; without a list that is every tile
int load_on(RNNoiseBatch *b, const float *d_snap, const int *d_list, int n, hipStream_t st) {
  HIP_OK(rn_launch_state_scatter(&b->g, RN_REC_SNAP, d_snap, d_list, n, b->ring_slot, phase_of(b, 0), st));
  if (b->img_valid) HIP_OK(rn_launch_nn_requant(&b->g, st, d_list, d_list ? n : 0));
  return 0;
}
constexpr int SNAP_CHUNK = 1024;  // rows of the host forms' staging buffer (27 MB)

// the host forms: the list is checked, the device drained (the caller's streams are not known here), then chunks of SNAP_CHUNK rows
// go through one staging allocation with blocking copies
int snap_host(RNNoiseBatch *b, float *snap, const int *streams, int n, bool load) {
  if (!snap_args_ok(b, snap, streams, n)) return -1;
  if (n == 0) return 0;
  std::vector<int> list((size_t)n);
  std::vector<uint8_t> seen(load ? (size_t)b->n : 0, 0);
  for (int i = 0; i < n; i++) {
    const int s = streams ? streams[i] : i;
    if (s < 0 || s >= b->n) return -1;
    if (load) {
      if (seen[s]) return -1;
      seen[s] = 1;
      const float *f = snap + (size_t)i * RN_SNAP_FLOATS;
      int magic;
      memcpy(&magic, f + RN_SNAP_OFF_MAGIC, sizeof magic);
      if (magic != RN_SNAP_MAGIC) return -1;
      if (!analysis_is_pitch_tail(f)) {
        fprintf(stderr, "[rnnoise_amd] load_streams: row %d: analysis_mem differs from the tail of pitch_buf\n", i);
        return -1;
      }
    }
    list[i] = s;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  const size_t chunk = n < SNAP_CHUNK ? n : SNAP_CHUNK, row_bytes = RN_SNAP_FLOATS * sizeof(float);
  char *d = nullptr;
  HIP_OK(hipMalloc((void **)&d, chunk * row_bytes + chunk * sizeof(int)));
  float *d_snap = reinterpret_cast<float *>(d);
  int *d_list = reinterpret_cast<int *>(d + chunk * row_bytes);
  int rc = 0;
  for (size_t r0 = 0; r0 < (size_t)n && rc == 0; r0 += chunk) {
    const int rows = (int)std::min(chunk, (size_t)n - r0);
    float *h = snap + r0 * RN_SNAP_FLOATS;
    rc = -1;
    if (hipMemcpy(d_list, list.data() + r0, rows * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) break;
    if (load) {
      if (hipMemcpy(d_snap, h, rows * row_bytes, hipMemcpyHostToDevice) == hipSuccess && load_on(b, d_snap, d_list, rows, nullptr) == 0 &&
          hipStreamSynchronize(nullptr) == hipSuccess)
        rc = 0;
    } else if (save_on(b, d_snap, d_list, rows, nullptr) == 0 && hipStreamSynchronize(nullptr) == hipSuccess &&
               hipMemcpy(h, d_snap, rows * row_bytes, hipMemcpyDeviceToHost) == hipSuccess) {
      rc = 0;
    }
  }
  hipFree(d);
  return rc;
}
}  // namespace

extern "C" int rnnoise_batch_save_streams_device(RNNoiseBatch *b, float *d_snap, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_snap, d_streams, n) || (reinterpret_cast<uintptr_t>(d_snap) & 15)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return save_on(b, d_snap, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_load_streams_device(RNNoiseBatch *b, const float *d_snap, const int *d_streams, int n, void *hip_stream) {
  if (!snap_args_ok(b, d_snap, d_streams, n) || (reinterpret_cast<uintptr_t>(d_snap) & 15)) return -1;
  if (n == 0) return 0;
  ON_DEVICE(b->device);
  return load_on(b, d_snap, d_streams, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_save_streams(RNNoiseBatch *b, float *snap, const int *streams, int n) {
  return snap_host(b, snap, streams, n, false);
}

extern "C" int rnnoise_batch_load_streams(RNNoiseBatch *b, const float *snap, const int *streams, int n) {
  return snap_host(b, const_cast<float *>(snap), streams, n, true);
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
  char *d = nullptr;
  HIP_OK(hipMalloc((void **)&d, 2 * fb + (size_t)n * 8 + 2 * 6 * 64 * 4));
  float *d_in = (float *)d, *d_out = (float *)(d + fb);
  unsigned long long *d_clk = (unsigned long long *)(d + 2 * fb);
  int *d_x = (int *)(d + 2 * fb + (size_t)n * 8);
  int rc = -1;
  if (hipMemcpy(d_in, in, fb, hipMemcpyHostToDevice) == hipSuccess &&
      rn_launch_fft_probe(variant, d_in, d_out, d_clk, n, reps, &tb, nullptr) == hipSuccess &&
      rn_launch_xlane_probe(d_x, nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
      hipMemcpy(out, d_out, fb, hipMemcpyDeviceToHost) == hipSuccess &&
      (!clocks || hipMemcpy(clocks, d_clk, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess) &&
      (!xlane || hipMemcpy(xlane, d_x, 2 * 6 * 64 * 4, hipMemcpyDeviceToHost) == hipSuccess))
    rc = 0;
  hipFree(d);
  return rc;
}

// out[i] = (float)log10(1e-2 + (double)ex[i]) evaluated on the device by the feature stage's function (host buffers; tests only).
// ex == null: the n floats with bit patterns first_bits, first_bits + 1, ...; model 0: as the kernels of this process evaluate it
// (rnnoise_amd_log10_model()), 1: the device library's log10 whatever the process uses
extern "C" int rnnoise_amd_debug_log_energy_range(int device, float *out, const float *ex, unsigned first_bits, unsigned n, int model) {
  if (!out || n == 0) return -1;
  ON_DEVICE(device);
  RnTablesDev tb;
  if (tables_for_device(device, tb)) return -1;
  float *d = nullptr;
  HIP_OK(hipMalloc((void **)&d, (size_t)n * (ex ? 8 : 4)));
  int rc = -1;
  if ((!ex || hipMemcpy(d + n, ex, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess) &&
      rn_launch_log_energy(ex ? d + n : nullptr, first_bits, d, n, model == 1 ? nullptr : tb.log_tab, nullptr) == hipSuccess &&
      hipStreamSynchronize(nullptr) == hipSuccess && hipMemcpy(out, d, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess)
    rc = 0;
  hipFree(d);
  return rc;
}
extern "C" int rnnoise_amd_debug_log_energy(int device, float *out, const float *ex, int n) {
  if (!ex || n <= 0) return -1;
  return rnnoise_amd_debug_log_energy_range(device, out, ex, 0, (unsigned)n, 0);
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

