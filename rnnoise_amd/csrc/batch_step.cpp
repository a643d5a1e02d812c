// batch_step.cpp -- the frame step: the stages of one process call (batch_step.h: Step), the whole step as a pipeline over HIP streams,
// its host-buffer form, and the plain, masked and list entry points.  (The halves of the split calls drive the same stages:
// batch_split.cpp.)
#include "batch_step.h"

namespace {
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
// model_sel at the last slot); listed: a list call, which keeps the layer images (Step::finish).  The process step and
// the feature calls (batch_eval.cpp) both launch the network here, timed as kind 1.
int batch_network_step(RNNoiseBatch *b, RnGroupDev &g, const RnPlan &plan, bool listed, hipStream_t st) {
  for (int k = 0; k < b->n_models; k++) {
    g.model_sel = k;
    const RnModelDev *mk = k ? &b->slot_m[k] : &b->m;
    if (plan.nn == RN_NN_LAYERS) {
      if (!b->img_valid) HIP_OK(rn_launch_nn_requant(&g, st));
      b->img_valid = true;
      // five launches, each timed on its own (kind 1: the durations add up to the network's)
      std::optional<TimedLaunch> tl[5];
      hipEvent_t ev[5][2] = {};
      for (int i = 0; i < 5; i++) {
        tl[i].emplace(b, 1);
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

// The step: the frames of one process call (shim.h: ProcessCall), every pointer of it device memory.  PCM frames are float (the
// reference API's sample type) or, with s16 set, int16 converted at the two ends of the step as the reference's only caller does
// (examples/rnnoise_demo.c:56,58): half the bytes over HBM and, in the host-fed path, PCIe.
int Step::begin(RNNoiseBatch *batch, const ProcessCall &call, StepKind kind) {
  if (!batch || call.n_frames < 0) return -1;
  b = batch, c = call;
  const int n_frames = c.n_frames, n_rows = c.n_rows;
  FrameIo *hk = c.hooks;
  listed = c.list || n_rows;
  if (listed) {
    if (n_rows < 0 || n_rows > b->n || (n_rows > 0 && !c.list)) return -1;
    if (n_rows == 0) return 1;
  }
  if ((!c.out && kind.k3) || (!c.in && kind.k0)) return -1;
  // the caller's PCM layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout), unless the buffers are the library's own (packed:
  // the staged host path; hk: the pinned ring).  Its frame slots must be disjoint, checked before anything is launched or changed
  // Interleaved channels (rnnoise_batch_set_pcm_channels): the rows are taken `chan` at a time, in the library's staging buffer
  // (packed) as in the caller's; the strides then place group slots of chan rows.  The pinned ring (hk) never sees channels
  const int chan = hk ? 1 : b->channels;
  if (listed && n_rows % chan) return -1;
  // Linked gains (rnnoise_batch_set_gain_link): the rows are taken `link` at a time too, whatever the channel count; the pinned ring
  // (hk) never sees a link either (shim.h: batch_host_call_staged)
  link = hk ? 1 : b->link;
  if (listed && n_rows % link) return -1;
  const bool laid = b->row_stride && !c.packed && !hk;
  if (laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, batch_frame_samples(b), chan, listed ? n_rows : b->n, n_frames))
    return -1;
  st = static_cast<hipStream_t>(c.stream);
  guard.emplace(b->device);
  if (!guard->ok) {
    fprintf(stderr, "[rnnoise_amd] cannot select HIP device %d (%s:%d)\n", b->device, __FILE__, __LINE__);
    return -1;
  }
  if ((c.active || listed) && !b->per_stream && n_frames > 0) {
    // the first masked or list call puts the batch into per-stream frame phase: every stream starts at the batch's phase.  ring_slot, not
    // frame_no: the training-feature calls advance the slots without counting frames (ring_slot % 3 == parity always)
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->phase_buf), b->ring_slot, b->n, st));
    b->per_stream = true;
  }
  N = listed ? n_rows : b->n;  // (rows of the caller's buffers)
  const size_t esz = c.s16 ? sizeof(short) : sizeof(float);
  const size_t fl = batch_frame_samples(b);
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
  const RnSchedule sched = rn_schedule(rn_knobs(), n_frames, b->schedule);
  pipelined = sched.pipelined && kind.k0, side_k1 = sched.side_k1 && kind.side_k1, k3 = kind.k3;
  const bool whole = b->g.n_streams == b->g.n_stride && (size_t)b->g.n_streams * RN_GRU * 4 < (1ull << 32);
  RnStepShape shape{(int)N, whole && !listed, b->cus, b->nn_path, pipelined, b->per_stream,
                    rn_shape_low_rate(b->pcm_rate, b->g.rs_Ls != nullptr)};
  shape.listed = listed;
  shape.companded = c.s16 && b->g.pcm_fmt != nullptr;  // (float calls never look at the format table)
  shape.channels = chan;
  // output tables (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates): the fields above are then the input side, what K0
  // reads, and these the output side, what K3 writes through its own copy of the group (shim.h: batch_k3_group)
  shape.split = b->out_Ls || b->out_fmt;
  shape.out_low_rate = shape.low_rate || b->out_Ls;
  shape.out_companded = c.s16 && (b->out_fmt || b->g.pcm_fmt);
  plan = rn_plan(rn_knobs(), shape);
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
  if (pipelined) {  // B and C start after everything already queued on the caller's stream
    HIP_OK(hipEventRecord(b->ev_begin, st));
    if (side_k1) HIP_OK(hipStreamWaitEvent(b->side, b->ev_begin, 0));
    HIP_OK(hipStreamWaitEvent(b->side_hp, b->ev_begin, 0));
  }
  sb = side_k1 ? b->side : st, sc = pipelined ? b->side_hp : st;
  // bytes between the frames of the PCM buffers, and the row pitch K0 / K3 get (0: the form's own constant -- today's arguments)
  fstep = (laid ? (size_t)b->frame_stride : N * fl) * esz;
  pcm_pitch = laid ? (int)b->row_stride : 0;
  pcm_chan = chan > 1 ? chan : 0;  // (rn_dev.h: RnGroupDev::pcm_chan -- 0: today's addressing)
  return 0;
}

// the batch's group with what every launch of frame f gets from the call: the PCM addressing, and in per-stream mode the phase and
// list fields (all null / 0 in lock-step mode).  The high-pass takes it as it is, the other kernels through frame_group
RnGroupDev Step::call_group(int f) const {
  RnGroupDev g = b->g;
  g.pcm_pitch = pcm_pitch;
  g.pcm_chan = pcm_chan;
  if (b->per_stream) {
    g.phase = b->phase_buf;
    g.active = c.active;
    g.call_frame = f;
    g.call_frames = c.n_frames;
    if (listed) {
      g.list = c.list;
      g.list_n = c.n_rows;
    }
  }
  return g;
}

RnGroupDev Step::frame_group(int f) const {
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
}

int Step::highpass(int f) {
  FrameIo *hk = c.hooks;
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
  if (pipelined && !side_k1 && k3 && f >= 3) HIP_OK(hipStreamWaitEvent(sc, b->cur_k3[(f - 3) & 7], 0));
  if (hk && hk->before_hp(f, sc)) return -1;
  {
    TimedLaunch t(b, 3);
    b->cur_hp[f & 7] = t.on ? t.stop() : (pipelined ? b->own_hp[f & 7] : nullptr);
    const RnGroupDev gh = call_group(f);
    HIP_OK(rn_launch_hp(&gh, static_cast<const char *>(c.in) + buf(f) * fstep, c.s16, (b->ring_slot + f) % RN_RING_SLOTS, plan.hp, sc,
                        t.start(), b->cur_hp[f & 7]));
  }
  if (hk && hk->after_hp(f, sc)) return -1;
  return 0;
}

int Step::analysis(int f, RnGroupDev &g) {
  if (pipelined) {
    HIP_OK(hipStreamWaitEvent(sb, b->cur_hp[f & 7], 0));
    if (side_k1 && f >= 2) HIP_OK(hipStreamWaitEvent(sb, b->cur_k3[(f - 2) & 7], 0));
  }
  TimedLaunch t(b, 0);
  b->cur_k1[f & 7] = t.on ? t.stop() : (pipelined ? b->own_k1[f & 7] : nullptr);
  HIP_OK(rn_launch_analysis(&g, &b->tb, (b->ring_slot + f) % RN_RING_SLOTS, (b->parity + f) % RN_SPEC_SLOTS, plan.k1, sb, t.start(),
                            b->cur_k1[f & 7]));
  return 0;
}

// the network once per model slot (batch_network_step, above)
int Step::network(int, RnGroupDev &g) { return batch_network_step(b, g, plan, listed, st); }

int Step::synthesis(int f, RnGroupDev &g, int cur, int prev) {
  TimedLaunch t(b, 2);
  b->cur_k3[f & 7] = t.on ? t.stop() : (pipelined ? b->own_k3[f & 7] : nullptr);
  g.link = link > 1 ? link : 0;  // (rn_dev.h: RnGroupDev::link -- K3's copy alone; 0: today's launch)
  const RnGroupDev g3 = batch_k3_group(b, g);  // (... with the effective output tables; without out tables g itself)
  HIP_OK(rn_launch_synthesis(&g3, &b->tb, static_cast<char *>(c.out) + buf(f) * fstep, c.s16, cur, prev, plan.k3, st, t.start(),
                             b->cur_k3[f & 7]));
  return 0;
}

int Step::finish() {
  const int n_frames = c.n_frames;
  // a list call keeps the layer-wise network's state images: only its rows' tiles are rebuilt (rn_dev.h: act_q), as after
  // rnnoise_batch_reset_streams -- not the whole batch at the next lock-step step
  if (listed && b->img_valid && n_frames > 0) HIP_OK(rn_launch_nn_requant(&b->g, st, c.list, c.n_rows));
  b->parity = (b->parity + n_frames) % RN_SPEC_SLOTS;
  b->ring_slot = (b->ring_slot + n_frames) % RN_RING_SLOTS;
  b->frame_no += n_frames;
  return 0;
}

// The whole step.  (A whole step is refused while frames of a split call are pending: include/rnnoise_amd.h)
int batch_process_device_impl(RNNoiseBatch *b, const ProcessCall &c) {
  if (batch_split_busy(b)) return -1;
  Step s;
  if (const int r = s.begin(b, c, {.side_k1 = true, .k0 = true, .k3 = true})) return r < 0 ? -1 : 0;
  const int n_frames = c.n_frames;
  FrameIo *hk = c.hooks;
  RnGroupDev ahead;  // the group of the frame whose analysis runs ahead of the loop's
  if (s.pipelined) {
    for (int f = 0; f < 3 && f < n_frames; f++)
      if (s.highpass(f)) return -1;
    if (s.analysis(0, ahead = s.frame_group(0))) return -1;
  }
  for (int f = 0; f < n_frames; f++) {
    RnGroupDev g = s.frame_group(f);
    const int cur = (b->parity + f) % RN_SPEC_SLOTS, prev = (cur + RN_SPEC_SLOTS - 1) % RN_SPEC_SLOTS;
    if (!s.pipelined) {
      if (s.highpass(f) || s.analysis(f, g)) return -1;
    } else {
      if (s.side_k1 && f + 3 < n_frames && s.highpass(f + 3)) return -1;
      if (f + 1 < n_frames && s.analysis(f + 1, ahead = s.frame_group(f + 1))) return -1;
      if (s.side_k1) HIP_OK(hipStreamWaitEvent(s.st, b->cur_k1[f & 7], 0));
    }
    if (hk && hk->before_nn(f, s.st)) return -1;
    if (s.network(f, g)) return -1;
    if (s.synthesis(f, g, cur, prev)) return -1;
    if (hk && hk->after_k3(f, s.st)) return -1;
    // (schedule 1: the high-pass three frames ahead goes out HERE, behind the synthesis launch whose end it starts at)
    if (s.pipelined && !s.side_k1 && f + 3 < n_frames && s.highpass(f + 3)) return -1;
    b->launches += b->timing ? 1 : 0;
  }
  return s.finish();
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

// ---- the host-buffer form ----
// a caller-defined layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout): the frame slots travel by strided copies between
// the caller's buffers and the default layout in device memory -- one 2-D copy per frame, its rows row_stride apart --, so the
// device runs the launches of the default layout and nothing but the slots themselves is read or written on the host
// Interleaved channels (rnnoise_batch_set_pcm_channels): what travels is the group slot, C rows of M samples interleaved, and the
// device works on the staging buffer with the same channel count (Step::begin: packed) -- no de-interleave here
int staged_begin(StagedCall &s, RNNoiseBatch *b, const ProcessCall &c) {
  s.b = b;
  s.n_frames = c.n_frames;
  s.rows = c.list ? c.n_rows : b->n;
  s.M = batch_frame_samples(b), s.esz = c.s16 ? 2 : 4;
  s.C = b->channels;
  if (s.rows % s.C || s.rows % (size_t)b->link) return -1;
  s.laid = b->row_stride != 0;
  if (s.laid && !rn_pcm_channels_fit(b->frame_stride, b->row_stride, (int)s.M, (int)s.C, (int)s.rows, c.n_frames)) return -1;
  s.fs = (size_t)c.n_frames * s.rows, s.pcm = s.fs * s.M * s.esz;
  return 0;
}

int StagedCall::pcm_copy(void *dst, const void *src, bool up) const {
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
}

int StagedCall::out_up(void *dst, const ProcessCall &c) const {
  if (c.active || c.list || b->g.rs_Ls || b->out_Ls || (c.s16 && (b->g.pcm_fmt || b->out_fmt))) return pcm_copy(dst, c.out, true);
  return 0;
}

// The convenience form on host buffers: every pointer of the call is host memory, staged through one device allocation with plain
// synchronous copies (no pinned ring, no copy engines -- rnnoise_batch_process is the fast host path).  The masked and the list host
// calls come here, and the plain ones that batch_host_call_staged (shim.h) names.  A list call (its n_rows entries checked by the
// caller) stages the list too, and its buffers have n_rows rows.
int batch_process_staged(RNNoiseBatch *b, const ProcessCall &c) {
  const int n_frames = c.n_frames;
  if (batch_split_busy(b) || !b || !c.out || !c.in || n_frames < 0) return -1;
  if (n_frames == 0) return 0;
  StagedCall s;
  if (staged_begin(s, b, c)) return -1;
  ON_DEVICE(b->device);
  DevScratch d;
  const size_t o_in = d.carve(s.pcm), o_out = d.carve(s.pcm), o_vad = d.carve(s.fs * 4), o_gains = d.carve(s.fs * RN_NB_BANDS * 4),
               o_act = d.carve(s.fs), o_list = d.carve(c.list ? s.rows * sizeof(int) : 0);
  if (d.alloc()) return -1;
  const ProcessCall dc{.out = d.at<char>(o_out), .in = d.at<char>(o_in), .vad = c.vad ? d.at<float>(o_vad) : nullptr,
                       .gains = c.gains ? d.at<float>(o_gains) : nullptr, .n_frames = n_frames, .s16 = c.s16,
                       .active = c.active ? d.at<uint8_t>(o_act) : nullptr, .list = c.list ? d.at<int>(o_list) : nullptr,
                       .n_rows = c.list ? c.n_rows : 0, .packed = true};  // the same call on the staged copies, on the null stream
  if (s.pcm_copy(d.at<char>(o_in), c.in, true) || s.out_up(dc.out, c)) return -1;
  if (c.active) HIP_OK(hipMemcpy(d.at<uint8_t>(o_act), c.active, s.fs, hipMemcpyHostToDevice));
  if (c.list) HIP_OK(hipMemcpy(d.at<int>(o_list), c.list, s.rows * sizeof(int), hipMemcpyHostToDevice));
  if (batch_process_device_impl(b, dc)) return -1;
  HIP_OK(hipDeviceSynchronize());
  if (s.pcm_copy(c.out, dc.out, false)) return -1;
  if (c.vad) HIP_OK(hipMemcpy(c.vad, dc.vad, s.fs * 4, hipMemcpyDeviceToHost));
  if (c.gains) HIP_OK(hipMemcpy(c.gains, dc.gains, s.fs * RN_NB_BANDS * 4, hipMemcpyDeviceToHost));
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
namespace {
// an empty list is a no-op even without a list pointer -- never a full-size call
int list_device(RNNoiseBatch *b, const ProcessCall &c) {
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!c.list && c.n_rows == 0) return b ? 0 : -1;
  return batch_process_device_impl(b, c);
}
// the host list is checked before anything moves: an entry outside the batch or a stream listed twice refuses the call
int list_host(RNNoiseBatch *b, const ProcessCall &c) {
  if (!b || c.n_rows < 0 || c.n_rows > b->n || (c.n_rows > 0 && !c.list) || c.n_frames < 0) return -1;
  if (c.n_rows == 0) return 0;
  if (!host_list_ok(b, c.list, c.n_rows, true)) return -1;
  return batch_process_staged(b, c);
}
}  // namespace

extern "C" int rnnoise_batch_process_device_list(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad, float *d_gains,
                                                 const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                 void *hip_stream) {
  return list_device(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames, .stream = hip_stream,
                         .active = d_active, .list = d_streams, .n_rows = n_rows});
}

extern "C" int rnnoise_batch_process_device_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad, float *d_gains,
                                                     const int *d_streams, int n_rows, const unsigned char *d_active, int n_frames,
                                                     void *hip_stream) {
  return list_device(b, {.out = d_out, .in = d_in, .vad = d_vad, .gains = d_gains, .n_frames = n_frames, .stream = hip_stream,
                         .s16 = true, .active = d_active, .list = d_streams, .n_rows = n_rows});
}

extern "C" int rnnoise_batch_process_list(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains, const int *streams,
                                          int n_rows, const unsigned char *active, int n_frames) {
  return list_host(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .active = active, .list = streams,
                       .n_rows = n_rows});
}

extern "C" int rnnoise_batch_process_list_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                              const int *streams, int n_rows, const unsigned char *active, int n_frames) {
  return list_host(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .s16 = true, .active = active,
                       .list = streams, .n_rows = n_rows});
}
