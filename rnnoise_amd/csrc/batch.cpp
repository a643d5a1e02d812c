// batch.cpp -- rnnoise_batch_*: N streams resident on one GPU; the frame step as a pipeline over HIP streams.
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

// The network of one frame, once per model slot (one slot without a map: exactly the launches of a one-model batch).  Slot k's launch
// owns the streams the map puts on k (rn_dev.h: rn_owns).  Layer-wise, a slot's whole network runs before the next slot's front:
// act_q[0] and nn_act are the tile's scratch, which the next front overwrites for every column.  g: the frame's group (it leaves with
// model_sel at the last slot); listed: a list call, which keeps the layer images (batch_process_device_impl).  The process step and
// the feature calls (batch_eval.cpp) both launch the network here, timed as kind 1.
int batch_network_step(RNNoiseBatch *b, RnGroupDev &g, const RnPlan &plan, bool listed, hipStream_t st) {
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
      b->img_valid = b->img_valid && listed;  // (a list call re-quantises its rows' tiles behind its last frame)
      if (plan.nn == RN_NN_ONE) HIP_OK(rn_launch_nn_one(&g, mk, &b->tb, b->lds_one, st, t.start(), t.stop()));
      else if (plan.nn == RN_NN_VECTOR) HIP_OK(rn_launch_nn_vector(&g, mk, &b->tb, st, t.start(), t.stop()));
      else HIP_OK(rn_launch_nn_mfma(&g, mk, &b->tb, plan.nn, st, t.start(), t.stop()));
    }
  }
  return 0;
}

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

// The step: the frames of one process call (shim.h: ProcessCall), every pointer of it device memory.  PCM frames are float (the
// reference API's sample type) or, with s16 set, int16 converted at the two ends of the step as the reference's only caller does
// (examples/rnnoise_demo.c:56,58): half the bytes over HBM and, in the host-fed path, PCIe.
int batch_process_device_impl(RNNoiseBatch *b, const ProcessCall &c) {
  const int n_frames = c.n_frames, n_rows = c.n_rows;
  const bool s16 = c.s16;
  FrameIo *hk = c.hooks;
  if (!b || n_frames < 0) return -1;
  // one half of the step alone (shim.h: SplitCall; batch_split.cpp has checked the call): the analysis half launches K0, K1 and an
  // export step per frame, the synthesis half an import step and K3 -- with the plan, the groups and the PCM addressing of the whole
  // step, which launches what it always did.  A whole step is refused while frames are pending
  const SplitCall *const sp = c.split;
  const bool ana = sp && sp->analyze, syn = sp && !sp->analyze;
  if (!sp && batch_split_busy(b)) return -1;
  const bool listed = c.list || n_rows;
  if (listed) {
    if (n_rows < 0 || n_rows > b->n || (n_rows > 0 && !c.list)) return -1;
    if (n_rows == 0) return 0;
  }
  if ((!c.out && !ana) || (!c.in && !syn)) return -1;
  // the caller's PCM layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout), unless the buffers are the library's own (packed:
  // the staged host path; hk: the pinned ring).  Its frame slots must be disjoint, checked before anything is launched or changed
  // Interleaved channels (rnnoise_batch_set_pcm_channels): the rows are taken `chan` at a time, in the library's staging buffer
  // (packed) as in the caller's; the strides then place group slots of chan rows.  The pinned ring (hk) never sees channels
  const int chan = hk ? 1 : b->channels;
  if (listed && n_rows % chan) return -1;
  // Linked gains (rnnoise_batch_set_gain_link): the rows are taken `link` at a time too, whatever the channel count; the pinned ring
  // (hk) never sees a link either (shim.h: batch_host_call_staged)
  const int link = hk ? 1 : b->link;
  if (listed && n_rows % link) return -1;
  const bool laid = b->row_stride && !c.packed && !hk;
  if (laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, batch_frame_samples(b), chan, listed ? n_rows : b->n, n_frames))
    return -1;
  const hipStream_t st = static_cast<hipStream_t>(c.stream);
  ON_DEVICE(b->device);
  if ((c.active || listed) && !b->per_stream && n_frames > 0) {
    // the first masked or list call puts the batch into per-stream frame phase: every stream starts at the batch's phase.  ring_slot, not
    // frame_no: the training-feature calls advance the slots without counting frames (ring_slot % 3 == parity always)
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->phase_buf), b->ring_slot, b->n, st));
    b->per_stream = true;
  }
  const size_t N = listed ? n_rows : b->n, esz = s16 ? sizeof(short) : sizeof(float);  // (N: rows of the caller's buffers)
  const size_t fl = batch_frame_samples(b);
  const char *d_in = static_cast<const char *>(c.in);
  char *d_out = static_cast<char *>(c.out);
  auto buf = [&](int f) -> size_t { return hk ? (size_t)(f % hk->ring) : (size_t)f; };  // frame f's place in the caller's buffers
  // bytes between the frames of the PCM buffers, and the row pitch K0 / K3 get (0: the form's own constant -- today's arguments)
  const size_t fstep = (laid ? (size_t)b->frame_stride : N * fl) * esz;
  const int pcm_pitch = laid ? (int)b->row_stride : 0;
  const int pcm_chan = chan > 1 ? chan : 0;  // (rn_dev.h: RnGroupDev::pcm_chan -- 0: today's addressing)
  // the batch's group with what every launch of frame f gets from the call: the PCM addressing, and in per-stream mode the phase and
  // list fields (all null / 0 in lock-step mode).  The high-pass takes it as it is, the other kernels through frame_group
  auto call_group = [&](int f) {
    RnGroupDev g = b->g;
    g.pcm_pitch = pcm_pitch;
    g.pcm_chan = pcm_chan;
    if (b->per_stream) {
      g.phase = b->phase_buf;
      g.active = c.active;
      g.call_frame = f;
      g.call_frames = n_frames;
      if (listed) {
        g.list = c.list;
        g.list_n = n_rows;
      }
    }
    return g;
  };
  // Multi-frame calls are software-pipelined over three streams: C runs the high-pass up to three frames ahead (f+3), B the analysis
  // of frame f+1, A (the caller's stream) network + synthesis of frame f; under schedule 1 (the host-fed path) analysis stays on A.
  // What makes that legal:
  //   * the pitch ring has 6 slots and analysis(g) reads slots g-3..g, so high-pass(f) only has to wait
  //     for analysis(f-3);
  //   * the spectra rotate through 3 slots and the per-step scratch (features, silence, pitch) is
  //     double-buffered, so analysis(f) only has to wait for synthesis(f-2);
  //   * every other piece of state is touched by one kernel only, in frame order on its own stream.
  // (dispatch.h: rn_schedule has the other schedules and rn_plan every kernel's form; one plan serves every frame of the call.  The
  // layer images are indexed by tile of the whole batch; the layer kernels use 32-bit byte offsets into a state plane)
  // (a split call: the analysis half keeps K1 on the caller's stream, with its export step behind it, and K0 runs ahead on the side
  //  stream as far as the ring allows; the synthesis half has nothing to overlap)
  const RnSchedule sched = rn_schedule(rn_knobs(), n_frames, b->schedule);
  const bool pipelined = sched.pipelined && !syn, side_k1 = sched.side_k1 && !sp;
  const bool whole = b->g.n_streams == b->g.n_stride && (size_t)b->g.n_streams * RN_GRU * 4 < (1ull << 32);
  RnStepShape shape{(int)N, whole && !listed, b->cus, b->nn_path, pipelined, b->per_stream,
                    rn_shape_low_rate(b->pcm_rate, b->g.rs_Ls != nullptr)};
  shape.listed = listed;
  shape.companded = s16 && b->g.pcm_fmt != nullptr;  // (float calls never look at the format table)
  shape.channels = chan;
  // output tables (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates): the fields above are then the input side, what K0
  // reads, and these the output side, what K3 writes through its own copy of the group (shim.h: batch_k3_group)
  shape.split = b->out_Ls || b->out_fmt;
  shape.out_low_rate = shape.low_rate || b->out_Ls;
  shape.out_companded = s16 && (b->out_fmt || b->g.pcm_fmt);
  const RnPlan plan = rn_plan(rn_knobs(), shape);
  if (plan.k3_rs != (b->g.rs_L != 0 || b->out_Ls != nullptr)) return -1;  // (the launcher tells the epilogue by its group's rs_L: batch_k3_group)
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
    RnGroupDev g = call_group(f);
    const int k = (int)((b->frame_no + f) & 1);
    g.features = b->features2[k];
    g.silence = b->silence2[k];
    g.pitch = b->pitch2[k];
    g.vad = c.vad ? c.vad + buf(f) * N : b->scratch_vad;
    g.gains = c.gains ? c.gains + buf(f) * N * RN_NB_BANDS : b->scratch_gains;
    if (listed) {  // the network writes the per-stream scratch, K3 copies the listed rows out (rn_dev.h: RnGroupDev::list)
      g.list_vad = c.vad ? g.vad : nullptr;
      g.list_gains = c.gains ? g.gains : nullptr;
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
    if (pipelined && !side_k1 && !ana && f >= 3) HIP_OK(hipStreamWaitEvent(sc, b->cur_k3[(f - 3) & 7], 0));
    if (hk && hk->before_hp(f, sc)) return -1;
    {
      TimedLaunch t(b, 3);
      b->cur_hp[f & 7] = t.on ? t.stop() : (pipelined ? b->own_hp[f & 7] : nullptr);
      const RnGroupDev gh = call_group(f);
      HIP_OK(rn_launch_hp(&gh, d_in + buf(f) * fstep, s16, (b->ring_slot + f) % RN_RING_SLOTS, plan.hp, sc, t.start(),
                          b->cur_hp[f & 7]));
    }
    if (hk && hk->after_hp(f, sc)) return -1;
    return 0;
  };
  auto analysis = [&](int f) -> int {  // K1 of frame f on stream sb
    RnGroupDev g = frame_group(f);
    const int slot = (b->parity + f) % RN_SPEC_SLOTS;
    if (ana && f + 1 < n_frames) {  // a pending frame's spectra go to its entry of the store; the call's last to the batch's own slot
      const SplitEntry e = batch_split_entry(b, f);
      g.spec_X[slot] = e.X, g.spec_P[slot] = e.P, g.spec_E[slot] = e.E;
    } else if (ana && b->split_prev_kept) {
      // ... which, in a call of a multiple of RN_SPEC_SLOTS frames, still holds what synthesis of frame 0 reads as the delayed
      // spectra: they move to the store's last entry first, on K1's stream
      const SplitEntry e = batch_split_entry(b, f);
      const size_t N = b->n;
      HIP_OK(hipMemcpyAsync(e.X, b->g.spec_X[slot], N * RN_SPEC_STRIDE * 4, hipMemcpyDeviceToDevice, sb));
      HIP_OK(hipMemcpyAsync(e.P, b->g.spec_P[slot], N * RN_SPEC_STRIDE * 4, hipMemcpyDeviceToDevice, sb));
      HIP_OK(hipMemcpyAsync(e.E, b->g.spec_E[slot], N * RN_SPEC_E_ROW * 4, hipMemcpyDeviceToDevice, sb));
    }
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
    if (ana) {  // the frame's features and silence words out of the per-step scratch, behind K1 on K1's stream
      RnSplitStep x{};
      x.feat = sp->features + (size_t)f * sp->feat_fs;
      x.feat_stride = sp->feat_rs;
      x.sil_keep = batch_split_entry(b, f).silence;
      x.sil_out = sp->silence ? sp->silence + (size_t)f * b->n : nullptr;
      HIP_OK(rn_launch_split_step(&g, &b->tb, &x, RN_STEP_EXPORT, sb));
    }
    return 0;
  };
  if (pipelined) {
    for (int f = 0; f < 3 && f < n_frames; f++)
      if (highpass(f)) return -1;
    if (!ana && analysis(0)) return -1;
  }
  for (int f = 0; ana && f < n_frames; f++) {  // the analysis half: K1 in frame order, K0 three frames ahead where the call is pipelined
    if (!pipelined && highpass(f)) return -1;
    if (analysis(f)) return -1;
    if (pipelined && f + 3 < n_frames && highpass(f + 3)) return -1;  // (a timed pair counts its frames once, in the synthesis half)
  }
  auto synthesis = [&](int f, RnGroupDev &g, int cur, int prev) -> int {  // K3 of frame f on the caller's stream
    TimedLaunch t(b, 2);
    b->cur_k3[f & 7] = t.on ? t.stop() : (pipelined ? b->own_k3[f & 7] : nullptr);
    g.link = link > 1 ? link : 0;  // (rn_dev.h: RnGroupDev::link -- K3's copy alone; 0: today's launch)
    const RnGroupDev g3 = batch_k3_group(b, g);  // (... with the effective output tables; without out tables g itself)
    HIP_OK(rn_launch_synthesis(&g3, &b->tb, d_out + buf(f) * fstep, s16, cur, prev, plan.k3, st, t.start(), b->cur_k3[f & 7]));
    return 0;
  };
  // The synthesis half: per pending frame an import step and K3, at the slots the frame was analysed at (the batch's have moved on).
  // K3's copy of the group gets the frame's spectra and silence words in the place of the batch's slots (shim.h:
  // RNNoiseBatch::split_store), and the caller's gains and vad -- zeros on a silent frame -- go into the scratch K3 reads, where the
  // network would have left its own.  The analysis half has moved the frame counters
  for (int f = 0; syn && f < n_frames; f++) {
    RnGroupDev g = frame_group(f);
    const int cur = (b->split_parity + f) % RN_SPEC_SLOTS, prev = (cur + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
    if (f + 1 < n_frames) {
      const SplitEntry e = batch_split_entry(b, f);
      g.spec_X[cur] = e.X, g.spec_P[cur] = e.P, g.spec_E[cur] = e.E;
    }
    if (f > 0 || b->split_prev_kept) {
      const SplitEntry e = batch_split_entry(b, f > 0 ? f - 1 : n_frames - 1);
      g.spec_X[prev] = e.X, g.spec_P[prev] = e.P, g.spec_E[prev] = e.E;
    }
    g.silence = batch_split_entry(b, f).silence;
    RnSplitStep x{};
    x.sil = g.silence;
    x.gains = sp->gains + (size_t)f * sp->gains_fs;
    x.gains_stride = sp->gains_rs;
    x.vad = sp->vad + (size_t)f * sp->vad_fs;
    x.vad_stride = sp->vad_rs;
    HIP_OK(rn_launch_split_step(&g, &b->tb, &x, RN_STEP_IMPORT, st));
    if (synthesis(f, g, cur, prev)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  if (syn) return 0;
  for (int f = 0; !sp && f < n_frames; f++) {
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
    // the network once per model slot (batch_network_step, above)
    if (batch_network_step(b, g, plan, listed, st)) return -1;
    if (synthesis(f, g, cur, prev)) return -1;
    if (hk && hk->after_k3(f, st)) return -1;
    // (schedule 1: the high-pass three frames ahead goes out HERE, behind the synthesis launch whose end it starts at)
    if (pipelined && !side_k1 && f + 3 < n_frames && highpass(f + 3)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  // a list call keeps the layer-wise network's state images: only its rows' tiles are rebuilt (rn_dev.h: act_q), as after
  // rnnoise_batch_reset_streams -- not the whole batch at the next lock-step step
  if (listed && b->img_valid && n_frames > 0) HIP_OK(rn_launch_nn_requant(&b->g, st, c.list, n_rows));
  b->parity = (b->parity + n_frames) % RN_SPEC_SLOTS;
  b->ring_slot = (b->ring_slot + n_frames) % RN_RING_SLOTS;
  b->frame_no += n_frames;
  return 0;
}

extern "C" int rnnoise_batch_process_device(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad,
                                            float *d_gains, int n_frames, void *hip_stream) {
  return batch_process_device_impl(
      b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames, .stream = hip_stream});
}

extern "C" int rnnoise_batch_process_device_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                float *d_gains, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames,
                                       .stream = hip_stream, .s16 = true});
}

// ---- masked calls (include/rnnoise_amd.h) ----
extern "C" int rnnoise_batch_process_device_masked(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad, float *d_gains,
                                                   const unsigned char *d_active, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames,
                                       .stream = hip_stream, .active = d_active});
}

extern "C" int rnnoise_batch_process_device_masked_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                       float *d_gains, const unsigned char *d_active, int n_frames, void *hip_stream) {
  return batch_process_device_impl(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames,
                                       .stream = hip_stream, .s16 = true, .active = d_active});
}

// The convenience form on host buffers: every pointer of the call is host memory, staged through one device allocation with plain
// synchronous copies (no pinned ring, no copy engines -- rnnoise_batch_process is the fast host path).  The masked and the list host
// calls come here, and the plain ones that batch_host_call_staged (shim.h) names.  A list call (its n_rows entries checked by the
// caller) stages the list too, and its buffers have n_rows rows.
int batch_process_staged(RNNoiseBatch *b, const ProcessCall &c) {
  const int n_frames = c.n_frames;
  // one half of the step (shim.h: SplitCall; batch_split.cpp): its rows are host memory too, under the caller's strides
  const SplitCall *const sp = c.split;
  const bool ana = sp && sp->analyze, syn = sp && !sp->analyze;
  if ((batch_split_busy(b) && !sp) || !b || (!c.out && !ana) || (!c.in && !syn) || n_frames < 0) return -1;
  if (n_frames == 0) return 0;
  const size_t rows = c.list ? c.n_rows : b->n;
  const size_t M = batch_frame_samples(b), esz = c.s16 ? 2 : 4;
  // a caller-defined layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout): the frame slots travel by strided copies between
  // the caller's buffers and the default layout in device memory -- one 2-D copy per frame, its rows row_stride apart --, so the
  // device runs the launches of the default layout and nothing but the slots themselves is read or written on the host
  // Interleaved channels (rnnoise_batch_set_pcm_channels): what travels is the group slot, C rows of M samples interleaved, and the
  // device works on the staging buffer with the same channel count (batch_process_device_impl: packed) -- no de-interleave here
  const size_t C = b->channels;
  if (rows % C || rows % (size_t)b->link) return -1;
  const bool laid = b->row_stride != 0;
  if (laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, (int)M, (int)C, (int)rows, n_frames)) return -1;
  ON_DEVICE(b->device);
  auto pcm_copy = [&](void *dst, const void *src, bool up) -> int {
    if (!laid) {
      HIP_OK(hipMemcpy(dst, src, (size_t)n_frames * rows * M * esz, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
      return 0;
    }
    const size_t hp = (size_t)b->row_stride * esz, hf = (size_t)b->frame_stride * esz, dp = M * C * esz, df = rows * M * esz;
    for (int f = 0; f < n_frames; f++) {
      if (up) HIP_OK(hipMemcpy2D(static_cast<char *>(dst) + f * df, dp, static_cast<const char *>(src) + f * hf, hp, dp, rows / C,
                                 hipMemcpyHostToDevice));
      else HIP_OK(hipMemcpy2D(static_cast<char *>(dst) + f * hf, hp, static_cast<const char *>(src) + f * df, dp, dp, rows / C,
                              hipMemcpyDeviceToHost));
    }
    return 0;
  };
  const size_t fs = (size_t)n_frames * rows, pcm = fs * M * esz;
  DevScratch d;
  // (a half of the step has no use for the other half's PCM buffer, the analysis half none for vad and gains)
  const size_t o_in = d.carve(syn ? 0 : pcm), o_out = d.carve(ana ? 0 : pcm), o_vad = d.carve(ana ? 0 : fs * 4),
               o_gains = d.carve(ana ? 0 : fs * RN_NB_BANDS * 4),
               o_act = d.carve(fs), o_list = d.carve(c.list ? rows * sizeof(int) : 0),
               o_feat = d.carve(ana ? fs * RN_NB_FEATURES * 4 : 0), o_sil = d.carve(ana ? fs * 4 : 0);
  if (d.alloc()) return -1;
  // the half's rows in the default layout on the device: [frame][stream][row]
  SplitCall dsp;
  std::vector<float> tight;
  if (sp) {
    const long N = (long)rows;
    dsp.analyze = ana;
    dsp.features = d.at<float>(o_feat), dsp.feat_fs = N * RN_NB_FEATURES, dsp.feat_rs = RN_NB_FEATURES;
    dsp.silence = d.at<int>(o_sil);
    dsp.gains = d.at<float>(o_gains), dsp.gains_fs = N * RN_NB_BANDS, dsp.gains_rs = RN_NB_BANDS;
    dsp.vad = d.at<float>(o_vad), dsp.vad_fs = N, dsp.vad_rs = 1;
  }
  if (syn) {  // (rows of a silent frame go up with the others; the device does not read them)
    tight.resize(fs * RN_NB_BANDS);
    for (size_t f = 0; f < (size_t)n_frames; f++)
      for (size_t r = 0; r < rows; r++)
        memcpy(&tight[(f * rows + r) * RN_NB_BANDS], sp->gains + f * sp->gains_fs + r * sp->gains_rs, RN_NB_BANDS * 4);
    HIP_OK(hipMemcpy(d.at<char>(o_gains), tight.data(), fs * RN_NB_BANDS * 4, hipMemcpyHostToDevice));
    for (size_t f = 0; f < (size_t)n_frames; f++)
      for (size_t r = 0; r < rows; r++) tight[f * rows + r] = sp->vad[f * sp->vad_fs + r * sp->vad_rs];
    HIP_OK(hipMemcpy(d.at<char>(o_vad), tight.data(), fs * 4, hipMemcpyHostToDevice));
  }
  const ProcessCall dc{.out = d.at<char>(o_out), .in = d.at<char>(o_in), .vad = c.vad ? d.at<float>(o_vad) : nullptr,
                       .gains = c.gains ? d.at<float>(o_gains) : nullptr, .n_frames = n_frames, .s16 = c.s16,
                       .active = c.active ? d.at<uint8_t>(o_act) : nullptr, .list = c.list ? d.at<int>(o_list) : nullptr,
                       .n_rows = c.list ? c.n_rows : 0, .packed = true,
                       .split = sp ? &dsp : nullptr};  // the same call on the staged copies, on the null stream
  if (!syn && pcm_copy(d.at<char>(o_in), c.in, true)) return -1;
  // `out` goes up too where the device leaves parts of it alone: absent rows, the part of a row behind the frame of a stream of a
  // rate table or an out-rate table, or behind a companded stream's bytes, keep the caller's values
  if (!ana && (c.active || c.list || b->g.rs_Ls || b->out_Ls || (c.s16 && (b->g.pcm_fmt || b->out_fmt))) && pcm_copy(dc.out, c.out, true)) return -1;
  if (c.active) HIP_OK(hipMemcpy(d.at<uint8_t>(o_act), c.active, fs, hipMemcpyHostToDevice));
  if (c.list) HIP_OK(hipMemcpy(d.at<int>(o_list), c.list, rows * sizeof(int), hipMemcpyHostToDevice));
  if (batch_process_device_impl(b, dc)) return -1;
  HIP_OK(hipDeviceSynchronize());
  if (ana) {  // the features to the caller's rows, 65 floats each and nothing around them; the silence words as they lie
    tight.resize(fs * RN_NB_FEATURES);
    HIP_OK(hipMemcpy(tight.data(), dsp.features, fs * RN_NB_FEATURES * 4, hipMemcpyDeviceToHost));
    for (size_t f = 0; f < (size_t)n_frames; f++)
      for (size_t r = 0; r < rows; r++)
        memcpy(sp->features + f * sp->feat_fs + r * sp->feat_rs, &tight[(f * rows + r) * RN_NB_FEATURES], RN_NB_FEATURES * 4);
    if (sp->silence) HIP_OK(hipMemcpy(sp->silence, dsp.silence, fs * 4, hipMemcpyDeviceToHost));
    return 0;
  }
  if (pcm_copy(c.out, dc.out, false)) return -1;
  if (c.vad) HIP_OK(hipMemcpy(c.vad, dc.vad, fs * 4, hipMemcpyDeviceToHost));
  if (c.gains) HIP_OK(hipMemcpy(c.gains, dc.gains, fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rnnoise_batch_process_masked(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains,
                                            const unsigned char *active, int n_frames) {
  if (!active) return rnnoise_batch_process(b, out, in, vad, gains, n_frames);
  return batch_process_staged(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .active = active});
}

extern "C" int rnnoise_batch_process_masked_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                                const unsigned char *active, int n_frames) {
  if (!active) return rnnoise_batch_process_s16(b, out, in, vad, gains, n_frames);
  return batch_process_staged(
      b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .s16 = true, .active = active});
}

// ---- stream-list calls (include/rnnoise_amd.h) ----
extern "C" int rnnoise_batch_process_device_list(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad, float *d_gains,
                                                 const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                 void *hip_stream) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!d_streams && n_rows == 0) return b ? 0 : -1;
  return batch_process_device_impl(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames,
                                       .stream = hip_stream, .active = d_active, .list = d_streams, .n_rows = n_rows});
}

extern "C" int rnnoise_batch_process_device_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad, float *d_gains,
                                                     const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                     void *hip_stream) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!d_streams && n_rows == 0) return b ? 0 : -1;
  return batch_process_device_impl(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames,
                                       .stream = hip_stream, .s16 = true, .active = d_active, .list = d_streams, .n_rows = n_rows});
}

namespace {
// the host list is checked before anything moves: an entry outside the batch or a stream listed twice refuses the call
int batch_process_list_host(RNNoiseBatch *b, const ProcessCall &c) {
  if (!b || c.n_rows < 0 || c.n_rows > b->n || (c.n_rows > 0 && !c.list) || c.n_frames < 0) return -1;
  if (c.n_rows == 0) return 0;
  std::vector<uint8_t> seen((size_t)b->n, 0);
  for (int i = 0; i < c.n_rows; i++) {
    const int s = c.list[i];
    if (s < 0 || s >= b->n || seen[s]) return -1;
    seen[s] = 1;
  }
  return batch_process_staged(b, c);
}
}  // namespace

extern "C" int rnnoise_batch_process_list(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains, const int *streams,
                                          int n_rows, const unsigned char *active, int n_frames) {
  return batch_process_list_host(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .active = active,
                                     .list = streams, .n_rows = n_rows});
}

extern "C" int rnnoise_batch_process_list_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                              const int *streams, int n_rows, const unsigned char *active, int n_frames) {
  return batch_process_list_host(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .s16 = true,
                                     .active = active, .list = streams, .n_rows = n_rows});
}

// ---- chunk calls (include/rnnoise_amd.h) ----
// Any number of samples per stream and call: the streams' sample FIFOs live on the device (chunk_plan.h has the rule), and a call is
// three steps on the caller's stream -- the scatter kernel's chunk form (pending samples ++ the caller's rows -> whole frames in the
// batch's own staging buffer, their mask, the new tails), the masked float call on that buffer in place, the gather kernel's chunk form
// (output FIFO ++ the frames' output -> the caller's rows, the rest kept).  The int16 forms differ in the two staging steps alone.
extern "C" int rnnoise_amd_chunk_frames(int frame_samples, int max_count) { return rn_chunk_frames(frame_samples, max_count); }

// every stream's FIFOs as after create; the caller has selected the device and drained it, and drains it again
int batch_chunk_restart_all(RNNoiseBatch *b) {
  if (!b->chunk_fifo) return 0;
  HIP_OK(hipMemset(b->chunk_fifo, 0, (size_t)b->n * RN_CHUNK_REC * sizeof(float)));  // (chunk_plan.h: a record of zeros)
  return 0;
}

// the FIFOs, where the batch has none yet: every stream's as after create, written on st ahead of what follows there
int batch_chunk_fifos_ready(RNNoiseBatch *b, hipStream_t st) {
  if (b->chunk_fifo) return 0;
  const size_t bytes = (size_t)b->n * RN_CHUNK_REC * sizeof(float);
  HIP_OK(hipMalloc((void **)&b->chunk_fifo, bytes));
  HIP_OK(hipMemsetAsync(b->chunk_fifo, 0, bytes, st));
  return 0;
}

namespace {
// what a chunk call does not combine with (include/rnnoise_amd.h): per-stream rates and formats, on the input or on the output side,
// a PCM layout, channels, linked gains
bool chunk_refused(const RNNoiseBatch *b) {
  return b->g.rs_Ls || b->g.pcm_fmt || b->out_Ls || b->out_fmt || b->row_stride || b->channels > 1 || b->link > 1;
}
// The FIFOs, on the first chunk call (their first state written on st, ahead of the call), and a staging buffer for F frames of
// `rows` rows with their mask behind them: frames of RN_FRAME_SIZE floats whatever the rate, so that a rate change keeps it.  It is
// sized in bytes and shared by the full-size and the list form: a call that fits leaves it alone.  Growing it drains the device first
// -- the old buffer may be in use by a call in flight on another stream.
int chunk_ready(RNNoiseBatch *b, int F, size_t rows, hipStream_t st) {
  if (batch_chunk_fifos_ready(b, st)) return -1;
  const size_t need = (size_t)F * rows * (RN_FRAME_SIZE * sizeof(float) + 1);
  if (need > b->chunk_stage_bytes) {
    if (b->chunk_stage) {
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipFree(b->chunk_stage));
      b->chunk_stage = nullptr;
      b->chunk_stage_bytes = 0;
    }
    HIP_OK(hipMalloc(&b->chunk_stage, need));
    b->chunk_stage_bytes = need;
  }
  return 0;
}

// d_streams: the list form -- every buffer has n_rows rows and row i belongs to stream d_streams[i]; null: the full-size form
int chunks_device(RNNoiseBatch *b, void *d_out, const void *d_in, const int *d_counts, int max_count, const int *d_streams, int n_rows,
                  float *d_vad, float *d_gains, int *d_frames, void *hip_stream, bool s16) {
  if (!b || !d_out || !d_in || !d_counts || max_count < 0 || chunk_refused(b)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const bool listed = d_streams || n_rows;
  if (listed && (n_rows < 0 || n_rows > b->n || (n_rows > 0 && !d_streams))) return -1;
  if (max_count == 0 || (listed && n_rows == 0)) return 0;
  const int M = batch_frame_samples(b), F = rn_chunk_frames(M, max_count), rows = listed ? n_rows : b->n;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  if (chunk_ready(b, F, rows, st)) return -1;
  RnChunkDev ck = batch_chunk_fifos(b, 0);
  ck.N = rows;
  ck.max_count = max_count;
  ck.F = F;
  ck.s16 = s16;
  ck.counts = d_counts;
  ck.in = d_in;
  ck.out = d_out;
  ck.stage = static_cast<float *>(b->chunk_stage);
  // (the mask behind the frames THIS call can have, at the longest frame: inside the allocation whatever it was sized for)
  ck.active = reinterpret_cast<unsigned char *>(ck.stage + (size_t)F * rows * RN_FRAME_SIZE);
  ck.frames = d_frames;
  ck.list = d_streams;
  ck.S = b->n;
  HIP_OK(rn_launch_state_scatter(&b->g, RN_REC_CHUNK, nullptr, nullptr, rows, 0, nullptr, &ck, st));
  // (the masked call reads frame f's rows in K0 and writes them in K3 of the same frame: in place.  The list form: the list call on
  //  the compact buffer -- every launch sized by n_rows)
  if (batch_process_device_impl(b, {.out = ck.stage, .in = ck.stage, .vad = d_vad, .gains = d_gains, .n_frames = F, .stream = hip_stream,
                                    .active = ck.active, .list = d_streams, .n_rows = listed ? n_rows : 0, .packed = true}))
    return -1;
  HIP_OK(rn_launch_state_gather(&b->g, RN_REC_CHUNK, nullptr, nullptr, rows, 0, nullptr, &ck, st));
  return 0;
}

// the convenience form on host buffers: the counts (and the list: an entry outside the batch or listed twice) are checked before
// anything moves; whole rows go up, and only the first counts[i] samples of a row come back into the caller's `out`
int chunks_host(RNNoiseBatch *b, void *out, const void *in, const int *counts, int max_count, const int *streams, int n_rows, float *vad,
                float *gains, int *frames, bool s16) {
  if (!b || !out || !in || !counts || max_count < 0 || chunk_refused(b)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const bool listed = streams || n_rows;
  if (listed && (n_rows < 0 || n_rows > b->n || (n_rows > 0 && !streams))) return -1;
  const size_t N = listed ? n_rows : b->n;
  if (listed) {
    std::vector<uint8_t> seen((size_t)b->n, 0);
    for (size_t i = 0; i < N; i++) {
      const int s = streams[i];
      if (s < 0 || s >= b->n || seen[s]) return -1;
      seen[s] = 1;
    }
  }
  for (size_t i = 0; i < N; i++)
    if (counts[i] < 0 || counts[i] > max_count) return -1;
  if (max_count == 0 || N == 0) return 0;
  const size_t esz = s16 ? sizeof(short) : sizeof(float), row = (size_t)max_count * esz;
  const size_t fs = (size_t)rn_chunk_frames(batch_frame_samples(b), max_count) * N;
  ON_DEVICE(b->device);
  DevScratch d;
  const size_t o_in = d.carve(N * row), o_out = d.carve(N * row), o_counts = d.carve(N * sizeof(int)), o_vad = d.carve(fs * 4),
               o_gains = d.carve(fs * RN_NB_BANDS * 4), o_frames = d.carve(N * sizeof(int)), o_list = d.carve(listed ? N * sizeof(int) : 0);
  if (d.alloc()) return -1;
  HIP_OK(hipMemcpy(d.at<char>(o_in), in, N * row, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d.at<char>(o_counts), counts, N * sizeof(int), hipMemcpyHostToDevice));
  if (listed) HIP_OK(hipMemcpy(d.at<char>(o_list), streams, N * sizeof(int), hipMemcpyHostToDevice));
  if (chunks_device(b, d.at<char>(o_out), d.at<char>(o_in), d.at<int>(o_counts), max_count, listed ? d.at<int>(o_list) : nullptr,
                    listed ? n_rows : 0, vad ? d.at<float>(o_vad) : nullptr, gains ? d.at<float>(o_gains) : nullptr,
                    frames ? d.at<int>(o_frames) : nullptr, nullptr, s16))
    return -1;
  HIP_OK(hipDeviceSynchronize());
  std::vector<char> rows(N * row);
  HIP_OK(hipMemcpy(rows.data(), d.at<char>(o_out), N * row, hipMemcpyDeviceToHost));
  for (size_t s = 0; s < N; s++) memcpy(static_cast<char *>(out) + s * row, rows.data() + s * row, (size_t)counts[s] * esz);
  if (vad) HIP_OK(hipMemcpy(vad, d.at<char>(o_vad), fs * 4, hipMemcpyDeviceToHost));
  if (gains) HIP_OK(hipMemcpy(gains, d.at<char>(o_gains), fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost));
  if (frames) HIP_OK(hipMemcpy(frames, d.at<char>(o_frames), N * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_process_device_chunks(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts, int max_count,
                                                   float *d_vad, float *d_gains, int *d_frames, void *hip_stream) {
  return chunks_device(b, d_out, d_in, d_counts, max_count, nullptr, 0, d_vad, d_gains, d_frames, hip_stream, false);
}
extern "C" int rnnoise_batch_process_device_chunks_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                       int max_count, float *d_vad, float *d_gains, int *d_frames, void *hip_stream) {
  return chunks_device(b, d_out, d_in, d_counts, max_count, nullptr, 0, d_vad, d_gains, d_frames, hip_stream, true);
}
extern "C" int rnnoise_batch_process_chunks(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count, float *vad,
                                            float *gains, int *frames) {
  return chunks_host(b, out, in, counts, max_count, nullptr, 0, vad, gains, frames, false);
}
extern "C" int rnnoise_batch_process_chunks_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts, int max_count,
                                                float *vad, float *gains, int *frames) {
  return chunks_host(b, out, in, counts, max_count, nullptr, 0, vad, gains, frames, true);
}
// the same on a stream list (include/rnnoise_amd.h): an empty list is a no-op even without a list pointer
extern "C" int rnnoise_batch_process_device_chunks_list(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts,
                                                        int max_count, const int *d_streams, int n_rows, float *d_vad, float *d_gains,
                                                        int *d_frames, void *hip_stream) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!d_streams && n_rows == 0) return b && d_out && d_in && d_counts && max_count >= 0 && !chunk_refused(b) ? 0 : -1;
  return chunks_device(b, d_out, d_in, d_counts, max_count, d_streams, n_rows, d_vad, d_gains, d_frames, hip_stream, false);
}
extern "C" int rnnoise_batch_process_device_chunks_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                            int max_count, const int *d_streams, int n_rows, float *d_vad,
                                                            float *d_gains, int *d_frames, void *hip_stream) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!d_streams && n_rows == 0) return b && d_out && d_in && d_counts && max_count >= 0 && !chunk_refused(b) ? 0 : -1;
  return chunks_device(b, d_out, d_in, d_counts, max_count, d_streams, n_rows, d_vad, d_gains, d_frames, hip_stream, true);
}
extern "C" int rnnoise_batch_process_chunks_list(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count,
                                                 const int *streams, int n_rows, float *vad, float *gains, int *frames) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!streams && n_rows == 0) return b && out && in && counts && max_count >= 0 && !chunk_refused(b) ? 0 : -1;
  return chunks_host(b, out, in, counts, max_count, streams, n_rows, vad, gains, frames, false);
}
extern "C" int rnnoise_batch_process_chunks_list_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts, int max_count,
                                                     const int *streams, int n_rows, float *vad, float *gains, int *frames) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!streams && n_rows == 0) return b && out && in && counts && max_count >= 0 && !chunk_refused(b) ? 0 : -1;
  return chunks_host(b, out, in, counts, max_count, streams, n_rows, vad, gains, frames, true);
}
extern "C" int rnnoise_batch_chunk_fill(RNNoiseBatch *b, int *fill) {
  if (!b || !fill) return -1;
  if (!b->chunk_fifo) {  // (no chunk call yet: nothing pending anywhere)
    memset(fill, 0, (size_t)b->n * sizeof(int));
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  // (one word of every record)
  HIP_OK(hipMemcpy2D(fill, sizeof(int), b->chunk_fifo + 2 * RN_CHUNK_FIFO_ROW, RN_CHUNK_REC * sizeof(float), sizeof(int), b->n,
                     hipMemcpyDeviceToHost));
  return 0;
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

