// host_io.cpp -- host-fed calls: pinned caller memory through a frame-granular ring beside one pipelined
// device call, pageable memory through double-buffered bounce chunks.
#include "shim.h"

#include <hsa/amd_hsa_signal.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <chrono>
#include <optional>

#define HSA_OK(x) do { hsa_status_t s_ = (x); if (s_ != HSA_STATUS_SUCCESS) { const char *m_ = nullptr; hsa_status_string(s_, &m_); \
    fprintf(stderr, "[rnnoise_amd] %s: %s\n", #x, m_ ? m_ : "?"); return -1; } } while (0)

// Copy mode "sdma": the two PCIe directions on two NAMED copy engines, at once.
// HIP picks the engine of a hipMemcpyAsync itself, and with an upload and a download in flight it runs one of them as a blit kernel
// whose PCIe-bound stores stall the kernels beside it (profiles/r3_hostio_traces.txt) -- which is why the other modes move an int16
// frame's 2 x 63 MB one direction at a time.  Underneath HIP, ROCr takes copies for a named engine
// (hsa_amd_memory_async_copy_on_engine); what it does not have is HIP's stream ordering, so the three cross-dependencies of the
// frame ring are built from pieces that profiles/r5_sdma_probe.txt shows working on this runtime:
//   copy engine -> stream  a second, 8-byte copy queued behind the payload on the same engine writes the running count of landed
//                          frames into a word of device memory; the stream waits for it with hipStreamWaitValue64;
//   stream -> copy engine  a one-thread kernel on the stream stores 0 (system-scope release) into the value word of an HSA signal that
//                          the copy lists as its dependency (rn_release_store_kernel);
//   copy engine -> host    the completion signal of the call's last copy (hsa_signal_wait).
struct Sdma {
  bool ok = false, hsa_ref = false;
  hsa_agent_t gpu{}, cpu{};
  hsa_amd_sdma_engine_id_t e_up{}, e_dn{};
  uint64_t *d_flags = nullptr;  // device memory: [0] uploads landed so far, [32] downloads landed so far (separate lines)
  uint64_t *h_seq = nullptr;    // pinned [SEQ]: the source words of the count copies
  static constexpr int SEQ = 2048;
  uint64_t up_count = 0, dn_count = 0;
  std::vector<hsa_signal_t> pool;
  size_t used = 0;
  hsa_signal_t take(hsa_signal_value_t v) {
    if (used == pool.size()) {
      hsa_signal_t s{};
      if (hsa_signal_create(v, 0, nullptr, &s) != HSA_STATUS_SUCCESS) return hsa_signal_t{0};
      pool.push_back(s);
    }
    hsa_signal_t s = pool[used++];
    hsa_signal_store_relaxed(s, v);
    return s;
  }
};

namespace {
bool host_pinned(const void *p) {  // memory the DMA engines can reach directly (hipHostMalloc / hipHostRegister)
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) == hipSuccess) return a.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  return false;
}
// Wait until the signal drops below 1, for at most `seconds` of WALL-CLOCK time.  hsa_signal_wait's timeout hint is in ticks of the
// HSA system timestamp (HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, 100 MHz here -- not nanoseconds: round 5's "30 s" was 300 s), and the
// call may return early with the condition unmet: so it is asked for 0.1 s worth of ticks at a time until a steady clock says stop.
bool sdma_wait(hsa_signal_t s, double seconds) {
  uint64_t freq = 0;
  if (hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &freq) != HSA_STATUS_SUCCESS || !freq) freq = 100000000ull;
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(seconds);
  for (;;) {
    if (hsa_signal_wait_scacquire(s, HSA_SIGNAL_CONDITION_LT, 1, freq / 10, HSA_WAIT_STATE_BLOCKED) < 1) return true;
    if (std::chrono::steady_clock::now() >= deadline) return false;
  }
}
// The value word of an HSA signal as a kernel can store to it.  This reaches INTO ROCr: hsa_signal_t::handle is the address of an
// amd_signal_t (hsa/amd_hsa_signal.h, a public header of the runtime, but the identity handle == address is the runtime's own
// business).  Developed and soaked on the runtime profiles/r6_hostio_timeline.txt names (ROCm 7.2.0's ROCr); sdma_selftest() below
// proves the assumption -- a kernel's store into this word releases a copy that lists the signal as its dependency -- on whatever
// runtime the process has, once per batch, BEFORE the mode is used; a runtime where it does not hold gets the runtime's own copies.
void *sdma_value_word(hsa_signal_t s) { return static_cast<void *>(const_cast<int64_t *>(&reinterpret_cast<amd_signal_t *>(s.handle)->value)); }
bool sdma_owner(const void *p, hsa_agent_t &agent, const void *&agent_ptr) {  // who owns p, and p as that side's engines address it
  hsa_amd_pointer_info_t info;
  memset(&info, 0, sizeof info);
  info.size = sizeof info;
  if (hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || info.type == HSA_EXT_POINTER_TYPE_UNKNOWN) return false;
  agent = info.agentOwner;
  agent_ptr = p;
  if (info.type == HSA_EXT_POINTER_TYPE_LOCKED && info.hostBaseAddress && info.agentBaseAddress)  // hipHostRegister-ed memory
    agent_ptr = static_cast<const char *>(info.agentBaseAddress) + (static_cast<const char *>(p) - static_cast<const char *>(info.hostBaseAddress));
  return true;
}
// The engines and the streams back in a known state after a copy-engine call that did not complete normally.  `deps`: the dependency
// signals that a kernel would have released; `done`: the completion signals of what was queued, in queue order.  Whether all landed.
bool sdma_drain(Sdma *s, const std::vector<hsa_signal_t> &deps, const std::vector<hsa_signal_t> &done) {
  for (hsa_signal_t d : deps)  // (copies parked on signals that no kernel will release any more: by hand)
    if (d.handle) hsa_signal_store_screlease(d, 0);
  bool landed = true;
  for (hsa_signal_t d : done)  // (in order on one engine: the first copy that does not land in 2 s ends the waiting)
    if (!(landed = sdma_wait(d, 2.0))) break;
  // and streams parked on a count that a copy which never completes, or was never queued, would have written: both counts past any wait
  const uint64_t past = ~0ull >> 1;
  (void)hipMemcpy(&s->d_flags[0], &past, 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(&s->d_flags[32], &past, 8, hipMemcpyHostToDevice);
  s->ok = false;  // (the counts no longer mean anything: this batch goes on with the runtime's copies)
  // A signal with a copy still pending must not be handed out again, nor destroyed under the engine by sdma_free: the pool is LEAKED
  // on purpose.  Nothing takes from it any more (ok is false), and a leaked signal is the lesser evil.
  if (!landed) s->pool.clear(), s->used = 0;
  return landed;
}
// Everything copy mode "sdma" assumes about the runtime, exercised once with 8 bytes and wall-clock deadlines before the mode is
// trusted with a caller's frames (a runtime where the assumptions half-hold must fail HERE, at set-up, not as a stall in
// the middle of a call):
//   stream -> engine   an upload on the named upload engine that lists a signal as its dependency starts when a KERNEL stores 0 into
//                      the signal's value word (sdma_value_word: the amd_signal_t layout);
//   engine -> stream   the word the upload writes into device memory releases a stream parked on it by hipStreamWaitValue64;
//   engine -> engine   a download on the named download engine that depends on the upload's completion signal brings the word back;
//   engine -> host     hsa_signal_wait sees the download complete.
// Returns nullptr when all four hold, else the name of the step that did not.
const char *sdma_selftest(Sdma *s) {
  const uint64_t magic = 0x5EEDF00D5EEDull;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return "self-test: stream";
  const hsa_signal_t dep = s->take(1), up = s->take(1), dn = s->take(1);
  std::vector<hsa_signal_t> queued;  // the completion signals that have a copy behind them
  const char *bad = nullptr;
  s->h_seq[0] = magic, s->h_seq[1] = 0;
  if (!dep.handle || !up.handle || !dn.handle) bad = "self-test: signals";
  else if (hsa_amd_memory_async_copy_on_engine(&s->d_flags[16], s->gpu, &s->h_seq[0], s->cpu, 8, 1, &dep, up, s->e_up, false) != HSA_STATUS_SUCCESS)
    bad = "self-test: upload on the named engine";
  else {
    queued.push_back(up);
    if (hsa_amd_memory_async_copy_on_engine(&s->h_seq[1], s->cpu, &s->d_flags[16], s->gpu, 8, 1, &up, dn, s->e_dn, false) != HSA_STATUS_SUCCESS)
      bad = "self-test: download on the named engine";
    else queued.push_back(dn);
  }
  if (!bad) {
    // nothing may have moved yet: the upload waits for `dep`
    if (hsa_signal_load_scacquire(up) < 1) bad = "self-test: the upload did not wait for its dependency";
    else if (rn_launch_release_store(sdma_value_word(dep), 0, st) != hipSuccess) bad = "self-test: release kernel";
    else if (hipStreamWaitValue64(st, &s->d_flags[16], magic, hipStreamWaitValueEq, ~0ull) != hipSuccess) bad = "self-test: hipStreamWaitValue64";
    else if (!sdma_wait(dn, 2.0)) bad = "self-test: a kernel's store into the signal's value word did not release the copy (amd_signal_t layout?)";
    else if (s->h_seq[1] != magic) bad = "self-test: the word did not come back";
  }
  // a failed test leaves nothing queued behind `dep`: released by hand, and what was queued -- only that -- waited for (again)
  if (bad) (void)sdma_drain(s, {dep}, queued);
  if (queued.size() == 2) {
    // the stream parked on the word: released by the upload -- or by hand, so that nothing stays parked behind a failed test
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
    while (hipStreamQuery(st) == hipErrorNotReady && std::chrono::steady_clock::now() < deadline) {}
    if (hipStreamQuery(st) == hipErrorNotReady) {
      bad = bad ? bad : "self-test: hipStreamWaitValue64 did not see the engine's write";
      (void)hipMemcpy(&s->d_flags[16], &magic, 8, hipMemcpyHostToDevice);
    }
  }
  (void)hipStreamSynchronize(st);
  (void)hipGetLastError();
  (void)hipStreamDestroy(st);
  s->used = 0;  // (the three signals go back to the pool -- unless the drain took the pool away)
  return bad;
}

Sdma *sdma_get(RNNoiseBatch *b, const void *host_ptr) {
  RNNoiseBatch::HostIo &io = b->io;
  if (io.sdma) return io.sdma->ok ? io.sdma : nullptr;
  Sdma *s = io.sdma = new Sdma();
  auto fail = [&](const char *what, hsa_status_t st) -> Sdma * {
    const char *m = nullptr;
    hsa_status_string(st, &m);
    fprintf(stderr, "[rnnoise_amd] copy mode sdma unavailable (%s: %s); using the runtime's copies\n", what, m ? m : "?");
    return nullptr;
  };
  hsa_status_t st = hsa_init();  // (reference-counted; the HIP runtime holds the first reference; ours is dropped in sdma_free)
  if (st != HSA_STATUS_SUCCESS) return fail("hsa_init", st);
  s->hsa_ref = true;
  const void *ap = nullptr;
  if (!sdma_owner(io.ring_mem, s->gpu, ap) || !sdma_owner(host_ptr, s->cpu, ap)) return fail("hsa_amd_pointer_info", HSA_STATUS_ERROR);
  uint32_t free_up = 0, free_dn = 0, pref_up = 0, pref_dn = 0;
  if ((st = hsa_amd_memory_copy_engine_status(s->gpu, s->cpu, &free_up)) != HSA_STATUS_SUCCESS && st != HSA_STATUS_ERROR_OUT_OF_RESOURCES)
    return fail("hsa_amd_memory_copy_engine_status", st);
  (void)hsa_amd_memory_copy_engine_status(s->cpu, s->gpu, &free_dn);
  (void)hsa_amd_memory_get_preferred_copy_engine(s->gpu, s->cpu, &pref_up);
  (void)hsa_amd_memory_get_preferred_copy_engine(s->cpu, s->gpu, &pref_dn);
  auto lowest = [](uint32_t m) { return m ? m & (~m + 1u) : 0u; };
  const uint32_t up = lowest(pref_up & free_up ? pref_up & free_up : free_up);
  uint32_t dn = lowest((pref_dn & free_dn & ~up) ? (pref_dn & free_dn & ~up) : (free_dn & ~up));
  if (!up || !dn) return fail("two free copy engines", HSA_STATUS_ERROR_OUT_OF_RESOURCES);
  s->e_up = (hsa_amd_sdma_engine_id_t)up;
  s->e_dn = (hsa_amd_sdma_engine_id_t)dn;
  if (hipMalloc((void **)&s->d_flags, 512) != hipSuccess || hipMemset(s->d_flags, 0, 512) != hipSuccess ||
      hipHostMalloc((void **)&s->h_seq, Sdma::SEQ * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    return fail("flag memory", HSA_STATUS_ERROR_OUT_OF_RESOURCES);
  }
  int can = 0;
  if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, b->device) != hipSuccess || !can) return fail("hipStreamWaitValue64", HSA_STATUS_ERROR);
  if (const char *what = sdma_selftest(s)) return fail(what, HSA_STATUS_ERROR);
  s->ok = true;
  return s;
}
void sdma_free(RNNoiseBatch::HostIo &io) {
  if (!io.sdma) return;
  for (hsa_signal_t sg : io.sdma->pool) hsa_signal_destroy(sg);
  if (io.sdma->d_flags) hipFree(io.sdma->d_flags);
  if (io.sdma->h_seq) hipHostFree(io.sdma->h_seq);
  if (io.sdma->hsa_ref) (void)hsa_shut_down();
  delete io.sdma;
  io.sdma = nullptr;
}
}  // namespace

void host_io_release(RNNoiseBatch *b) {
  RNNoiseBatch::HostIo &io = b->io;
  sdma_free(io);
  for (int k = 0; k < 2; k++) {
    if (io.d_in[k]) hipFree(io.d_in[k]);
    if (io.h_in[k]) hipHostFree(io.h_in[k]);
    if (io.up_done[k]) { hipEventDestroy(io.up_done[k]); hipEventDestroy(io.run_done[k]); hipEventDestroy(io.down_done[k]); }
  }
  for (hipStream_t s : {io.up, io.run, io.down})
    if (s) hipStreamDestroy(s);
  if (io.ring_mem) hipFree(io.ring_mem);
  for (int k = 0; k < RNNoiseBatch::HostIo::RING; k++)
    for (hipEvent_t e : {io.r_k3[k], io.r_down[k], io.r_up[k], io.r_hp[k]})
      if (e) hipEventDestroy(e);
  io = RNNoiseBatch::HostIo();
}

// device and pinned host staging for two chunks of `frames` frames each (pageable callers): one allocation per side and chunk,
// carved into in | out | vad | gains
static int host_io_prepare(RNNoiseBatch *b, int frames, size_t esz) {
  RNNoiseBatch::HostIo &io = b->io;
  const size_t N = b->n;
  size_t n_in = ((size_t)frames * N * RN_FRAME_SIZE * esz + 255) / 256 * 64;  // floats' worth of PCM per chunk and direction
  if (io.chunk_frames >= frames && io.pcm_floats >= n_in) return 0;
  frames = std::max(frames, io.chunk_frames);  // (float and s16 callers alternating on one batch: grow once, to both)
  n_in = std::max(n_in, io.pcm_floats);
  host_io_release(b);
  const size_t fr = (size_t)frames, n_vad = fr * N, n_g = fr * N * RN_NB_BANDS, total = (2 * n_in + n_vad + n_g) * sizeof(float);
  for (hipStream_t *s : {&io.up, &io.run, &io.down}) HIP_OK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  auto carve = [&](float *in, float *&out, float *&vad, float *&gains) { out = in + n_in, vad = out + n_in, gains = vad + n_vad; };
  for (int k = 0; k < 2; k++) {
    HIP_OK(hipMalloc((void **)&io.d_in[k], total));
    carve(io.d_in[k], io.d_out[k], io.d_vad[k], io.d_gains[k]);
    HIP_OK(hipHostMalloc((void **)&io.h_in[k], total, hipHostMallocDefault));
    carve(io.h_in[k], io.h_out[k], io.h_vad[k], io.h_gains[k]);
    for (hipEvent_t *e : {&io.up_done[k], &io.run_done[k], &io.down_done[k]}) HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  io.chunk_frames = frames;
  io.pcm_floats = n_in;
  return 0;
}

// ---- the pinned ring: RING frame slots in HBM, filled and drained frame by frame beside the kernels of ONE device call ----
namespace {
constexpr int RING = RNNoiseBatch::HostIo::RING;
struct RingRoom {  // where the RING slots of each kind begin: PCM in at 0, PCM out (a float frame's room per slot), vad, gains; the end
  size_t out, vad, g, bytes;
  explicit RingRoom(size_t N)
      : out(RING * rn_align256(N * RN_FRAME_SIZE * 4)), vad(2 * out), g(vad + RING * rn_align256(N * 4)), bytes(g + RING * rn_align256(N * RN_NB_BANDS * 4)) {}
};
// What both copy back ends share: the ring as ONE call addresses it.  The PCM slots are addressed with the stride of the CALL's frame
// size (s16 frames use the first half of a slot's room).
struct Ring {
  char *r_in, *r_out;
  float *r_vad, *r_g;
  size_t N, fsz;  // streams; bytes of PCM per frame
  Ring(char *mem, const RingRoom &at, size_t n, size_t esz)
      : r_in(mem), r_out(mem + at.out), r_vad(reinterpret_cast<float *>(mem + at.vad)), r_g(reinterpret_cast<float *>(mem + at.g)), N(n), fsz(n * RN_FRAME_SIZE * esz) {}
};
int ring_build(RNNoiseBatch::HostIo &io, size_t N) {  // streams, ring and events
  if (!io.run)
    for (hipStream_t *s : {&io.run, &io.down}) HIP_OK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  HIP_OK(hipMalloc((void **)&io.ring_mem, RingRoom(N).bytes));
  for (int k = 0; k < RING; k++) {
    for (hipEvent_t *e : {&io.r_k3[k], &io.r_down[k], &io.r_up[k]})  // (a copy engine follows a kernel: system scope)
      HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&io.r_hp[k], hipEventDisableTiming | hipEventDisableSystemFence));  // (read-after-read ordering only)
  }
  return 0;
}

// Copies.  Default: the two named copy engines above (mode sdma).  The runtime's own copies remain as the fallback (no two free
// engines, no hipStreamWaitValue64, calls longer than the count ring, a batch whose engines once failed) and for A/B runs:
// int16 frames: uploads and downloads ALTERNATE ON ONE COPY STREAM (io.down), in the order the frame pipeline asks for them: each
// then finds the DMA engine free.  Two copies in flight make one a blit kernel (256 workgroups x 512 lanes; the analysis kernel took
// 2.3 ms instead of 1.1 beside it), and a copy stream per direction plus the pipeline's three streams is more than the four hardware
// queues the runtime multiplexes streams onto.  One direction at a time moves an int16 step's 2 x 63 MB in 2.2 ms, just above the
// kernels' time: 28.0 M frames/s either way (profiles/r4_hostio_modes.txt).
// float frames (2 x 126 MB per step) are bound by the link whatever the kernels do, and there both directions at once win:
// uploads ride on the high-pass stream, downloads keep the copy stream -- 19.9 M frames/s against 14.6 M.
// $RNNOISE_AMD_HOSTIO_COPY = one | hp | sdma forces a mode (A/B runs); profiles/r5_hostio_sdma.txt has the three side by side.
int copy_mode() {  // 0 default, 1 one, 2 hp (and anything unrecognised), 3 sdma; read once per process
  static const char *const e = getenv("RNNOISE_AMD_HOSTIO_COPY");
  return !e ? 0 : (!strcmp(e, "one") ? 1 : (!strcmp(e, "sdma") ? 3 : 2));
}

// Copy modes "one" and "hp": the runtime's copies, on one stream (io.down) or on two (uploads on the high-pass stream).
struct RuntimeCopies final : FrameIo, Ring {
  RNNoiseBatch::HostIo &io;
  char *out;  // the caller's four
  const char *in;
  float *vad, *gains;
  bool one_copy_stream;
  RuntimeCopies(RNNoiseBatch::HostIo &io_, const Ring &r, char *o, const char *i, float *v, float *g, bool one)
      : Ring(r), io(io_), out(o), in(i), vad(v), gains(g), one_copy_stream(one) { ring = RING; }
  int before_hp(int f, hipStream_t sc) override {
    if (!one_copy_stream) {
      HIP_OK(hipMemcpyAsync(r_in + (size_t)(f % RING) * fsz, in + (size_t)f * fsz, fsz, hipMemcpyHostToDevice, sc));
      return 0;
    }
    if (f >= RING) HIP_OK(hipStreamWaitEvent(io.down, io.r_hp[f % RING], 0));   // high-pass(f - RING) has read the slot
    HIP_OK(hipMemcpyAsync(r_in + (size_t)(f % RING) * fsz, in + (size_t)f * fsz, fsz, hipMemcpyHostToDevice, io.down));
    HIP_OK(hipEventRecord(io.r_up[f % RING], io.down));
    HIP_OK(hipStreamWaitEvent(sc, io.r_up[f % RING], 0));
    return 0;
  }
  int after_hp(int f, hipStream_t sc) override { if (one_copy_stream) HIP_OK(hipEventRecord(io.r_hp[f % RING], sc)); return 0; }
  // (network(f) writes vad / gains, synthesis(f) the PCM of slot f % RING)
  int before_nn(int f, hipStream_t st) override { if (f >= RING) HIP_OK(hipStreamWaitEvent(st, io.r_down[f % RING], 0)); return 0; }
  int after_k3(int f, hipStream_t st) override {
    const int k = f % RING;
    HIP_OK(hipEventRecord(io.r_k3[k], st));
    HIP_OK(hipStreamWaitEvent(io.down, io.r_k3[k], 0));
    HIP_OK(hipMemcpyAsync(out + (size_t)f * fsz, r_out + (size_t)k * fsz, fsz, hipMemcpyDeviceToHost, io.down));
    if (vad) HIP_OK(hipMemcpyAsync(vad + (size_t)f * N, r_vad + (size_t)k * N, N * sizeof(float), hipMemcpyDeviceToHost, io.down));
    if (gains) HIP_OK(hipMemcpyAsync(gains + (size_t)f * N * RN_NB_BANDS, r_g + (size_t)k * N * RN_NB_BANDS, N * RN_NB_BANDS * sizeof(float),
                                     hipMemcpyDeviceToHost, io.down));
    HIP_OK(hipEventRecord(io.r_down[k], io.down));
    return 0;
  }
};

// Copy mode "sdma": the two named copy engines (struct Sdma above).
struct EngineCopies final : FrameIo, Ring {
  Sdma *const sd;
  // per call: the signals of its frames (reused from call to call: the previous call ended with every copy complete)
  struct FrameSig { hsa_signal_t hp_read, k3_done, up, up_flag, dn, dn_flag; uint64_t dn_target; };
  std::vector<FrameSig> fs;
  // the caller's four buffers: who owns each, and its address as that side's engines see it (p_vad, p_g: null where the caller's is)
  hsa_agent_t a_in{}, a_out{}, a_vad{}, a_g{};
  const void *p_in = nullptr, *p_out = nullptr, *p_vad = nullptr, *p_g = nullptr;
  EngineCopies(Sdma *s, const Ring &r, int n_frames) : Ring(r), sd(s), fs((size_t)n_frames) { ring = RING, sd->used = 0; }
  bool owners(const void *in, const void *out, const void *vad, const void *gains) {
    return sdma_owner(in, a_in, p_in) && sdma_owner(out, a_out, p_out) && (!vad || sdma_owner(vad, a_vad, p_vad)) && (!gains || sdma_owner(gains, a_g, p_g));
  }
  bool take(FrameSig &q) {  // the six signals of a frame, or failure as a whole (what was taken is in q: drain() releases it)
    q.hp_read = sd->take(1);
    q.k3_done = sd->take(1);
    q.up = sd->take(1);
    q.up_flag = sd->take(1);
    q.dn = sd->take(1 + (p_vad ? 1 : 0) + (p_g ? 1 : 0));
    q.dn_flag = sd->take(1);
    return q.hp_read.handle && q.k3_done.handle && q.up.handle && q.up_flag.handle && q.dn.handle && q.dn_flag.handle;
  }
  int before_hp(int f, hipStream_t sc) override {
    FrameSig &q = fs[(size_t)f];
    if (!take(q)) return -1;
    // upload(f) on the upload engine, once high-pass(f - RING) has read the slot; the count of landed uploads behind it
    const hsa_signal_t *dep = f >= RING ? &fs[(size_t)(f - RING)].hp_read : nullptr;
    HSA_OK(hsa_amd_memory_async_copy_on_engine(r_in + (size_t)(f % RING) * fsz, sd->gpu, static_cast<const char *>(p_in) + (size_t)f * fsz, a_in, fsz,
                                               dep ? 1 : 0, dep, q.up, sd->e_up, false));
    const uint64_t c = ++sd->up_count;
    sd->h_seq[c % (Sdma::SEQ / 2)] = c;
    HSA_OK(hsa_amd_memory_async_copy_on_engine(&sd->d_flags[0], sd->gpu, &sd->h_seq[c % (Sdma::SEQ / 2)], sd->cpu, 8, 1, &q.up, q.up_flag, sd->e_up, false));
    HIP_OK(hipStreamWaitValue64(sc, &sd->d_flags[0], c, hipStreamWaitValueGte, ~0ull));
    return 0;
  }
  int after_hp(int f, hipStream_t sc) override { return rn_launch_release_store(sdma_value_word(fs[(size_t)f].hp_read), 0, sc) == hipSuccess ? 0 : -1; }
  int before_nn(int f, hipStream_t st) override {  // network(f) writes vad / gains, synthesis(f) the PCM of slot f % RING
    if (f >= RING) HIP_OK(hipStreamWaitValue64(st, &sd->d_flags[32], fs[(size_t)(f - RING)].dn_target, hipStreamWaitValueGte, ~0ull));
    return 0;
  }
  int after_k3(int f, hipStream_t st) override {
    const int k = f % RING;
    FrameSig &q = fs[(size_t)f];
    // download(f) on the download engine, released by a store on the kernels' stream; the count of landed downloads behind it
    HIP_OK(rn_launch_release_store(sdma_value_word(q.k3_done), 0, st));
    HSA_OK(hsa_amd_memory_async_copy_on_engine(const_cast<char *>(static_cast<const char *>(p_out)) + (size_t)f * fsz, a_out, r_out + (size_t)k * fsz, sd->gpu, fsz,
                                               1, &q.k3_done, q.dn, sd->e_dn, false));
    if (p_vad) HSA_OK(hsa_amd_memory_async_copy_on_engine(const_cast<char *>(static_cast<const char *>(p_vad)) + (size_t)f * N * 4, a_vad, r_vad + (size_t)k * N, sd->gpu,
                                                          N * sizeof(float), 1, &q.k3_done, q.dn, sd->e_dn, false));
    if (p_g) HSA_OK(hsa_amd_memory_async_copy_on_engine(const_cast<char *>(static_cast<const char *>(p_g)) + (size_t)f * N * RN_NB_BANDS * 4, a_g,
                                                        r_g + (size_t)k * N * RN_NB_BANDS, sd->gpu, N * RN_NB_BANDS * sizeof(float), 1, &q.k3_done, q.dn, sd->e_dn, false));
    const uint64_t c = ++sd->dn_count;
    sd->h_seq[Sdma::SEQ / 2 + c % (Sdma::SEQ / 2)] = c;
    q.dn_target = c;
    HSA_OK(hsa_amd_memory_async_copy_on_engine(&sd->d_flags[32], sd->gpu, &sd->h_seq[Sdma::SEQ / 2 + c % (Sdma::SEQ / 2)], sd->cpu, 8, 1, &q.dn, q.dn_flag, sd->e_dn, false));
    return 0;
  }
  // every copy of the call is complete once the last frame's download count has landed (the engines work in order)
  bool wait_last(double seconds) const { return fs.empty() || sdma_wait(fs.back().dn_flag, seconds); }
  void drain() {  // every frame's two dependency signals by hand; the download counts that were queued, in order
    std::vector<hsa_signal_t> deps, done;
    for (const FrameSig &q : fs) {
      deps.insert(deps.end(), {q.hp_read, q.k3_done});
      if (q.dn_flag.handle && q.dn_target) done.push_back(q.dn_flag);
    }
    (void)sdma_drain(sd, deps, done);
  }
};
}  // namespace

// Host-fed path for pinned caller memory (hipHostMalloc / hipHostRegister): the DMA engines read and write it in place, one
// frame per copy, while ONE multi-frame device call runs the kernels as a frame pipeline (the high-pass up to three frames
// ahead on a side stream) over a ring of RING frame slots in HBM.  Per frame f: upload(f) [after high-pass(f - RING) has read the slot] -> high-pass(f) -> ... ->
// network(f), synthesis(f) [after download(f - RING) has drained the slot] -> download(f).  A call pays one frame's upload
// before and one frame's download after its kernels, whatever its length.
static int batch_process_pinned(RNNoiseBatch *b, char *out, const char *in, float *vad, float *gains, int n_frames, bool s16) {
  RNNoiseBatch::HostIo &io = b->io;
  // streams, ring and events together or not at all: a half-built set is torn down and retried
  if ((!io.ring_mem || !io.run) && ring_build(io, b->n)) return host_io_release(b), -1;
  const Ring ring(io.ring_mem, RingRoom(b->n), b->n, s16 ? sizeof(short) : sizeof(float));
  // the copy back end of this call (copy_mode).  The engines also step aside for a call longer than the count ring: a call's copies
  // are all queued while its kernels are, and the count words' source ring must not wrap inside one call
  const int mode = copy_mode();
  std::optional<EngineCopies> engines;
  std::optional<RuntimeCopies> runtime;
  if (Sdma *sd = ((mode == 3 || mode == 0) && n_frames <= Sdma::SEQ / 2) ? sdma_get(b, in) : nullptr) {
    engines.emplace(sd, ring, n_frames);
    if (!engines->owners(in, out, vad, gains)) engines.reset();
  }
  if (!engines) runtime.emplace(io, ring, out, in, vad, gains, (mode == 1 || mode == 2) ? mode == 1 : s16);
  FrameIo *copies = engines ? static_cast<FrameIo *>(&*engines) : &*runtime;
  // Stream budget: the runtime multiplexes HIP streams onto four hardware queues, one of which belongs to the application's
  // own stream.  The three-stream frame pipeline plus the copy stream would be four more, and the high-pass and analysis
  // streams then share a queue: what the high-pass stream carries queues up behind analysis kernels and the whole step
  // serialises (rocprofv3 trace: 3.5 ms per 65,536-stream s16 step).  Analysis therefore stays on the main stream here
  // (schedule 1: only the high-pass runs ahead on a side stream), which costs the 2-3 % the analysis overlap is worth.
  const int keep = b->schedule;
  if (b->schedule == 0) b->schedule = 1;
  const int rc = batch_process_device_impl(
      b, {.out = ring.r_out, .in = ring.r_in, .vad = ring.r_vad, .gains = ring.r_g, .n_frames = n_frames, .stream = io.run, .s16 = s16, .hooks = copies});
  b->schedule = keep;
  // a copy that never completes leaves streams parked on the count words for ever: give the mode up for this batch, drain, reset
  const bool stuck = engines && !rc && !engines->wait_last(30.0);
  if (stuck) fprintf(stderr, "[rnnoise_amd] rnnoise_batch_process: the copy engines did not finish within 30 s; falling back to the runtime's copies\n");
  if (rc || stuck) {
    // whatever was queued must not outlive the caller's buffers; and some of the call's frames may have run while the batch's
    // frame bookkeeping was not advanced: the streams are no longer in a state any caller knows -- back to the initial one
    if (engines) engines->drain();
    (void)hipDeviceSynchronize();
    if (rc) fprintf(stderr, "[rnnoise_amd] rnnoise_batch_process: a GPU step failed inside the call; the batch has been reset\n");
    (void)rnnoise_batch_reset(b);
    return -1;
  }
  HIP_OK(hipStreamSynchronize(io.down));
  HIP_OK(hipStreamSynchronize(io.run));  // (the side streams of the pipelined schedule join `run` before its last kernel)
  return 0;
}

// Pageable caller memory goes through pinned bounce buffers (the copy in and out of them is the calling thread's work): chunks of
// about 32 MB of PCM each way (at least one frame), two in flight -- H2D of chunk c+1 and D2H of chunk c-1 overlap the kernels of
// chunk c.
static int batch_process_pageable(RNNoiseBatch *b, char *out, const char *in, float *vad, float *gains, int n_frames, bool s16) {
  const size_t N = b->n, esz = s16 ? sizeof(short) : sizeof(float), fsz = N * RN_FRAME_SIZE * esz;  // (fsz: bytes of PCM per frame step)
  const int chunk = (int)std::min<size_t>((size_t)n_frames, std::max<size_t>(1, ((size_t)32 << 20) / fsz));
  if (host_io_prepare(b, chunk, esz)) return -1;
  RNNoiseBatch::HostIo &io = b->io;
  const int n_chunks = (n_frames + chunk - 1) / chunk;
  auto frames_of = [&](int c) { return std::min(chunk, n_frames - c * chunk); };
  auto upload = [&](int c) -> int {  // chunk c -> staging set c & 1 (free once chunk c-2 has been downloaded)
    const int k = c & 1, f = frames_of(c);
    if (c >= 2) HIP_OK(hipStreamWaitEvent(io.up, io.run_done[k], 0));  // its kernels no longer read d_in[k]
    if (c >= 2) HIP_OK(hipEventSynchronize(io.up_done[k]));            // the bounce buffer has been sent
    memcpy(io.h_in[k], in + (size_t)c * chunk * fsz, (size_t)f * fsz);
    HIP_OK(hipMemcpyAsync(io.d_in[k], io.h_in[k], (size_t)f * fsz, hipMemcpyHostToDevice, io.up));
    HIP_OK(hipEventRecord(io.up_done[k], io.up));
    return 0;
  };
  auto collect = [&](int c) -> int {  // bounce buffer of chunk c -> caller memory
    const int k = c & 1, f = frames_of(c);
    HIP_OK(hipEventSynchronize(io.down_done[k]));
    memcpy(out + (size_t)c * chunk * fsz, io.h_out[k], (size_t)f * fsz);
    if (vad) memcpy(vad + (size_t)c * chunk * N, io.h_vad[k], (size_t)f * N * sizeof(float));
    if (gains) memcpy(gains + (size_t)c * chunk * N * RN_NB_BANDS, io.h_gains[k], (size_t)f * N * RN_NB_BANDS * sizeof(float));
    return 0;
  };
  // the chunk loop as one unit: any failure inside it leaves copies and kernels in flight on three streams and the batch's frame
  // bookkeeping out of step with what the GPU ran -- drain everything and put the batch back to its initial state, like the
  // pinned path does
  auto chunks = [&]() -> int {
    if (upload(0)) return -1;
    for (int c = 0; c < n_chunks; c++) {
      const int k = c & 1, f = frames_of(c);
      if (c + 1 < n_chunks && upload(c + 1)) return -1;
      HIP_OK(hipStreamWaitEvent(io.run, io.up_done[k], 0));
      if (c >= 2) HIP_OK(hipStreamWaitEvent(io.run, io.down_done[k], 0));  // d_out[k] of chunk c-2 has left
      if (batch_process_device_impl(b, {.out = io.d_out[k], .in = io.d_in[k], .vad = io.d_vad[k], .gains = io.d_gains[k], .n_frames = f,
                                        .stream = io.run, .s16 = s16}))
        return -1;
      HIP_OK(hipEventRecord(io.run_done[k], io.run));
      if (c >= 2 && collect(c - 2)) return -1;  // frees h_out[k] for the download queued below
      HIP_OK(hipStreamWaitEvent(io.down, io.run_done[k], 0));
      HIP_OK(hipMemcpyAsync(io.h_out[k], io.d_out[k], (size_t)f * fsz, hipMemcpyDeviceToHost, io.down));
      if (vad) HIP_OK(hipMemcpyAsync(io.h_vad[k], io.d_vad[k], (size_t)f * N * sizeof(float), hipMemcpyDeviceToHost, io.down));
      if (gains) HIP_OK(hipMemcpyAsync(io.h_gains[k], io.d_gains[k], (size_t)f * N * RN_NB_BANDS * sizeof(float), hipMemcpyDeviceToHost, io.down));
      HIP_OK(hipEventRecord(io.down_done[k], io.down));
    }
    for (int c = std::max(0, n_chunks - 2); c < n_chunks; c++)
      if (collect(c)) return -1;
    HIP_OK(hipStreamSynchronize(io.down));
    HIP_OK(hipStreamSynchronize(io.run));  // (the side streams of the pipelined schedule join `run` before its last kernel)
    return 0;
  };
  if (!chunks()) return 0;
  (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  fprintf(stderr, "[rnnoise_amd] rnnoise_batch_process: a GPU step or copy failed inside the call; the batch has been reset\n");
  (void)rnnoise_batch_reset(b);
  return -1;
}

static int batch_process_host_impl(RNNoiseBatch *b, void *out_v, const void *in_v, float *vad, float *gains, int n_frames, bool s16) {
  if (!b || !out_v || !in_v || n_frames < 0) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (n_frames == 0) return 0;
  ON_DEVICE(b->device);
  const char *in = static_cast<const char *>(in_v);
  char *out = static_cast<char *>(out_v);
  const bool pinned = host_pinned(in) && host_pinned(out) && (!vad || host_pinned(vad)) && (!gains || host_pinned(gains));
  return (pinned ? batch_process_pinned : batch_process_pageable)(b, out, in, vad, gains, n_frames, s16);
}

// (the calls that batch_host_call_staged names take the staged convenience path of the masked calls: batch_step.cpp)
extern "C" int rnnoise_batch_process(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains, int n_frames) {
  if (b && batch_host_call_staged(b, false))
    return batch_process_staged(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames});
  return batch_process_host_impl(b, out, in, vad, gains, n_frames, false);
}

extern "C" int rnnoise_batch_process_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains, int n_frames) {
  if (b && batch_host_call_staged(b, true))
    return batch_process_staged(b, {.out = out, .in = in, .vad = vad, .gains = gains, .n_frames = n_frames, .s16 = true});
  return batch_process_host_impl(b, out, in, vad, gains, n_frames, true);
}
