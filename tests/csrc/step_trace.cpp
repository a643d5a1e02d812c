// step_trace.cpp -- the batch host code (rnnoise_amd/csrc/batch*.cpp) linked against RECORDING STUBS of everything it calls: the HIP
// runtime, the kernel launchers, the model and table loaders.  No GPU and no ROCm library: device addresses come from a bump counter
// and are never dereferenced, streams and events are numbered in creation order, and every call appends one text line to a trace --
// its name, stream, events, scalars and pointers, and every field of the argument structs (RnGroupDev, RnSplitStep, RnChunkDev).  The
// cases below are fixed sequences of API calls; a case's trace is what the host code enqueues for them, in order.
//   step_trace                 one line per case: name, records, SHA-256 of the trace
//   step_trace --dump CASE     the case's trace
// tests/test_step_trace_cpu.py compares the lines with tests/golden/step_trace.txt, recorded from the commit its first line names.
#include "../../rnnoise_amd/csrc/shim.h"

#include <functional>
#include <stdarg.h>

// ---- the trace ----
static std::vector<std::string> g_trace;
static void rec(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void rec(const char *fmt, ...) {
  char buf[8192];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_trace.push_back(buf);
}

// ---- names for pointers: device memory by offset from the bump counter's base, the cases' own "device" buffers by offset from
// theirs, registered host buffers by name and offset; any other host address (the library's temporaries) as "host"
static const uintptr_t DEV_BASE = 0x100000000000ull, USR_BASE = 0x200000000000ull, USR_END = 0x300000000000ull;
static uintptr_t g_bump;
struct HostBuf { const char *name; const char *p; size_t bytes; };
static std::vector<HostBuf> g_host;
static std::string P(const void *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  char buf[64];
  if (!p) return "0";
  if (a >= DEV_BASE && a < USR_BASE) snprintf(buf, sizeof buf, "D+%llx", (unsigned long long)(a - DEV_BASE));
  else if (a >= USR_BASE && a < USR_END) snprintf(buf, sizeof buf, "U+%llx", (unsigned long long)(a - USR_BASE));
  else {
    for (const HostBuf &h : g_host)
      if ((const char *)p >= h.p && (const char *)p < h.p + h.bytes) {
        snprintf(buf, sizeof buf, "%s+%llx", h.name, (unsigned long long)((const char *)p - h.p));
        return buf;
      }
    return "host";
  }
  return buf;
}
#define PS(p) P(p).c_str()
template <typename T>
static T *usr(size_t off) { return reinterpret_cast<T *>(USR_BASE + off); }
static bool is_fake(const void *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  return a >= DEV_BASE && a < USR_END;
}

// streams and events: handle k is the k-th created (from 1); 0 is null
static uintptr_t g_streams, g_events;
static long SN(hipStream_t s) { return (long)reinterpret_cast<uintptr_t>(s); }
static long EN(hipEvent_t e) { return (long)reinterpret_cast<uintptr_t>(e); }
static int g_cus = 256, g_device = 0;
static const char *kind_name(hipMemcpyKind k) {
  return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : "other";
}
// host memory a copy reads is read and host memory it writes is zeroed, so that the sanitizers see its extent
static void touch(void *dst, const void *src, size_t n, hipMemcpyKind k) {
  if (k == hipMemcpyHostToDevice && !is_fake(src)) {
    volatile unsigned char sink = 0;
    for (size_t i = 0; i < n; i++) sink = sink + static_cast<const unsigned char *>(src)[i];
  }
  if (k == hipMemcpyDeviceToHost && !is_fake(dst)) memset(dst, 0, n);
}

// ---- the HIP runtime ----
extern "C" {
hipError_t hipGetDevice(int *d) { *d = g_device; return hipSuccess; }
hipError_t hipSetDevice(int d) { rec("hipSetDevice %d", d); g_device = d; return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t a, int d) {
  rec("hipDeviceGetAttribute %s dev=%d", a == hipDeviceAttributeMultiprocessorCount ? "cus" : "other", d);
  *v = g_cus;
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { rec("hipDeviceSynchronize"); return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void **p, size_t n) {
  *p = reinterpret_cast<void *>(DEV_BASE + g_bump);
  rec("hipMalloc %zu -> %s", n, PS(*p));
  g_bump += (n + 4095) & ~size_t(4095);
  return hipSuccess;
}
hipError_t hipFree(void *p) { rec("hipFree %s", PS(p)); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind k) {
  rec("hipMemcpy %s dst=%s src=%s bytes=%zu", kind_name(k), PS(dst), PS(src), n);
  touch(dst, src, n, k);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind k, hipStream_t s) {
  rec("hipMemcpyAsync %s dst=%s src=%s bytes=%zu S%ld", kind_name(k), PS(dst), PS(src), n, SN(s));
  touch(dst, src, n, k);
  return hipSuccess;
}
hipError_t hipMemcpy2D(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind k) {
  rec("hipMemcpy2D %s dst=%s dpitch=%zu src=%s spitch=%zu width=%zu height=%zu", kind_name(k), PS(dst), dpitch, PS(src), spitch, width,
      height);
  for (size_t r = 0; r < height; r++) touch(static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width, k);
  return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t n) { rec("hipMemset %s v=%d bytes=%zu", PS(p), v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t s) {
  rec("hipMemsetAsync %s v=%d bytes=%zu S%ld", PS(p), v, n, SN(s));
  return hipSuccess;
}
hipError_t hipMemset2DAsync(void *p, size_t pitch, int v, size_t w, size_t h, hipStream_t s) {
  rec("hipMemset2DAsync %s pitch=%zu v=%d w=%zu h=%zu S%ld", PS(p), pitch, v, w, h, SN(s));
  return hipSuccess;
}
hipError_t hipMemsetD32(hipDeviceptr_t p, int v, size_t n) { rec("hipMemsetD32 %s v=%d count=%zu", PS(p), v, n); return hipSuccess; }
hipError_t hipMemsetD32Async(hipDeviceptr_t p, int v, size_t n, hipStream_t s) {
  rec("hipMemsetD32Async %s v=%d count=%zu S%ld", PS(p), v, n, SN(s));
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
  *e = reinterpret_cast<hipEvent_t>(++g_events);
  rec("hipEventCreateWithFlags flags=%x -> E%ld", flags, EN(*e));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { rec("hipEventDestroy E%ld", EN(e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  rec("hipEventElapsedTime E%ld E%ld", EN(a), EN(b));
  *ms = 1.0f;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { rec("hipEventRecord E%ld S%ld", EN(e), SN(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { rec("hipEventSynchronize E%ld", EN(e)); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int prio) {
  *s = reinterpret_cast<hipStream_t>(++g_streams);
  rec("hipStreamCreateWithPriority flags=%x prio=%d -> S%ld", flags, prio, SN(*s));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { rec("hipStreamDestroy S%ld", SN(s)); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { rec("hipStreamSynchronize S%ld", SN(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
  rec("hipStreamWaitEvent S%ld E%ld flags=%x", SN(s), EN(e), flags);
  return hipSuccess;
}
}  // extern "C"

// ---- the argument structs, field by field ----
static std::string group_text(const RnGroupDev *g) {
  std::string s;
  char buf[256];
#define FIELD_I(m) snprintf(buf, sizeof buf, " " #m "=%d", (int)g->m), s += buf;
#define FIELD_P(m) snprintf(buf, sizeof buf, " " #m "=%s", PS(g->m)), s += buf;
#define ARR(m, T, row, planes) s += " " #m, snprintf(buf, sizeof buf, "(%d)=%s", k_of(#m, k), PS(g->m)), s += buf;
#define TIL(m, T, tile) ARR(m, T, tile, 1)
#define OPT(m, row) ARR(m, void, row, 1)
  auto k_of = [](const char *name, int k) { return strchr(name, '[') ? k : 0; };
  const int k = 0;  // (RN_EACH declares its own k around the slotted arrays)
  (void)k;
  FIELD_I(n_streams) FIELD_I(n_stride)
  RN_GROUP_ARRAYS(ARR, TIL, OPT)
  FIELD_I(call_frame) FIELD_I(call_frames) FIELD_P(list) FIELD_I(list_n) FIELD_P(list_vad) FIELD_P(list_gains) FIELD_P(rs_out)
  FIELD_I(rs_L) FIELD_I(rs_pitch) FIELD_I(pcm_pitch) FIELD_I(pcm_chan) FIELD_I(link) FIELD_I(model_sel) FIELD_I(n_models)
#undef ARR
#undef TIL
#undef OPT
  return s;
}
static std::string split_text(const RnSplitStep *x) {
  char buf[512];
  snprintf(buf, sizeof buf, " feat=%s feat_stride=%lld sil_keep=%s sil_out=%s sil=%s gains=%s gains_stride=%lld vad=%s vad_stride=%lld",
           PS(x->feat), x->feat_stride, PS(x->sil_keep), PS(x->sil_out), PS(x->sil), PS(x->gains), x->gains_stride, PS(x->vad),
           x->vad_stride);
  return buf;
}
static std::string chunk_text(const RnChunkDev *c) {
  if (!c) return " ck=0";
  char buf[768];
  snprintf(buf, sizeof buf,
           " ck.fifo=%s M=%d N=%d max_count=%d F=%d s16=%d counts=%s in=%s out=%s stage=%s active=%s frames=%s list=%s S=%d op=%d rec=%s",
           PS(c->fifo), c->M, c->N, c->max_count, c->F, c->s16, PS(c->counts), PS(c->in), PS(c->out), PS(c->stage), PS(c->active),
           PS(c->frames), PS(c->list), c->S, c->op, PS(c->rec));
  return buf;
}
#define GT(g) group_text(g).c_str()
// (the stub of model_on_device puts the model's number into conv1.nin)
static int model_no(const RnModelDev *m) { return m->conv1.nin; }

// ---- the kernel launchers and the loaders ----
extern "C" {
hipError_t rn_launch_hp(const RnGroupDev *g, const void *in, int s16, int slot, RnHpForm form, hipStream_t s, hipEvent_t a, hipEvent_t b) {
  rec("rn_launch_hp S%ld E%ld E%ld in=%s s16=%d slot=%d form=%d%s", SN(s), EN(a), EN(b), PS(in), s16, slot, (int)form, GT(g));
  return hipSuccess;
}
hipError_t rn_launch_analysis(const RnGroupDev *g, const RnTablesDev *, int slot, int spec, RnK1Form form, hipStream_t s, hipEvent_t a,
                              hipEvent_t b) {
  rec("rn_launch_analysis S%ld E%ld E%ld slot=%d spec=%d form=%d%s", SN(s), EN(a), EN(b), slot, spec, (int)form, GT(g));
  return hipSuccess;
}
hipError_t rn_launch_synthesis(const RnGroupDev *g, const RnTablesDev *, void *out, int s16, int cur, int prev, RnK3Form form, hipStream_t s,
                               hipEvent_t a, hipEvent_t b) {
  rec("rn_launch_synthesis S%ld E%ld E%ld out=%s s16=%d cur=%d prev=%d form=%d%s", SN(s), EN(a), EN(b), PS(out), s16, cur, prev, (int)form,
      GT(g));
  return hipSuccess;
}
hipError_t rn_launch_train_features(const RnGroupDev *g, const RnTablesDev *, const float *noisy, int slot, int spec, const RnTrainArgs *tr,
                                    hipStream_t s) {
  rec("rn_launch_train_features S%ld noisy=%s slot=%d spec=%d clean=%s vad=%s rec=%s%s", SN(s), PS(noisy), slot, spec, PS(tr->clean),
      PS(tr->vad), PS(tr->rec), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_eval_step(const RnGroupDev *g, const RnTablesDev *, const RnEvalStep *x, hipStream_t s) {
  rec("rn_launch_eval_step S%ld on=%d stage=%s target=%s%s", SN(s), x->on, PS(x->stage), PS(x->target), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_split_step(const RnGroupDev *g, const RnTablesDev *, const RnSplitStep *x, int mode, hipStream_t s) {
  rec("rn_launch_split_step S%ld mode=%d%s%s", SN(s), mode, split_text(x).c_str(), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_nn_vector(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *, hipStream_t s, hipEvent_t a, hipEvent_t b) {
  rec("rn_launch_nn_vector S%ld E%ld E%ld model=%d%s", SN(s), EN(a), EN(b), model_no(m), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_nn_one(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *, hipError_t opt, hipStream_t s, hipEvent_t a,
                            hipEvent_t b) {
  rec("rn_launch_nn_one S%ld E%ld E%ld model=%d opt_in=%d%s", SN(s), EN(a), EN(b), model_no(m), (int)opt, GT(g));
  return hipSuccess;
}
hipError_t rn_launch_nn_mfma(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *, RnNnForm form, hipStream_t s, hipEvent_t a,
                             hipEvent_t b) {
  rec("rn_launch_nn_mfma S%ld E%ld E%ld model=%d form=%d%s", SN(s), EN(a), EN(b), model_no(m), (int)form, GT(g));
  return hipSuccess;
}
hipError_t rn_launch_nn_layers(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *, RnGruForm form, const hipError_t opt[2],
                               hipStream_t s, hipEvent_t ev[5][2]) {
  rec("rn_launch_nn_layers S%ld ev=%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld model=%d form=%d opt_in=%d,%d%s", SN(s), EN(ev[0][0]), EN(ev[0][1]),
      EN(ev[1][0]), EN(ev[1][1]), EN(ev[2][0]), EN(ev[2][1]), EN(ev[3][0]), EN(ev[3][1]), EN(ev[4][0]), EN(ev[4][1]), model_no(m), (int)form,
      (int)opt[0], (int)opt[1], GT(g));
  return hipSuccess;
}
hipError_t rn_launch_nn_requant(const RnGroupDev *g, hipStream_t s, const int *list, int n) {
  rec("rn_launch_nn_requant S%ld list=%s n=%d%s", SN(s), PS(list), n, GT(g));
  return hipSuccess;
}
hipError_t rn_nn_one_opt_in(void) { rec("rn_nn_one_opt_in"); return hipSuccess; }
void rn_nn_gru_opt_in(hipError_t out[2]) { rec("rn_nn_gru_opt_in"); out[0] = out[1] = hipSuccess; }
hipError_t rn_launch_state_gather(const RnGroupDev *g, RnRecKind kind, float *r, const int *list, int rows, int p, const int *phase,
                                  const RnChunkDev *ck, hipStream_t s, const uint8_t *out_Ls) {
  rec("rn_launch_state_gather S%ld kind=%d rec=%s list=%s rows=%d p=%d phase=%s out_Ls=%s%s%s", SN(s), (int)kind, PS(r), PS(list), rows, p,
      PS(phase), PS(out_Ls), chunk_text(ck).c_str(), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_state_scatter(const RnGroupDev *g, RnRecKind kind, const float *r, const int *list, int rows, int p, const int *phase,
                                   const RnChunkDev *ck, hipStream_t s, const uint8_t *out_Ls) {
  rec("rn_launch_state_scatter S%ld kind=%d rec=%s list=%s rows=%d p=%d phase=%s out_Ls=%s%s%s", SN(s), (int)kind, PS(r), PS(list), rows, p,
      PS(phase), PS(out_Ls), chunk_text(ck).c_str(), GT(g));
  return hipSuccess;
}
hipError_t rn_launch_state_zero(const RnGroupDev *g, const int *list, int n, const RnChunkDev *ck, hipStream_t s) {
  rec("rn_launch_state_zero S%ld list=%s n=%d%s%s", SN(s), PS(list), n, chunk_text(ck).c_str(), GT(g));
  return hipSuccess;
}
// host_io.cpp's entry points, which the masked host calls hand a call without a mask to
int rnnoise_batch_process(RNNoiseBatch *, float *, const float *, float *, float *, int n_frames) {
  rec("rnnoise_batch_process n_frames=%d", n_frames);
  return 0;
}
int rnnoise_batch_process_s16(RNNoiseBatch *, short *, const short *, float *, float *, int n_frames) {
  rec("rnnoise_batch_process_s16 n_frames=%d", n_frames);
  return 0;
}
}  // extern "C"
int tables_for_device(int device, RnTablesDev &out) {
  rec("tables_for_device %d", device);
  memset(&out, 0, sizeof out);
  return 0;
}
int model_on_device(RNNModel *m, int device, RnModelDev &out) {
  rec("model_on_device model=%d dev=%d", m->blob_len, device);
  memset(&out, 0, sizeof out);
  out.conv1.nin = m->blob_len;
  return 0;
}
void host_io_release(RNNoiseBatch *) { rec("host_io_release"); }

// the pinned ring's hooks as host_io.cpp hangs them into a call
struct RecIo final : FrameIo {
  RecIo() { ring = 6; }
  int before_hp(int f, hipStream_t s) override { rec("hook before_hp f=%d S%ld", f, SN(s)); return 0; }
  int after_hp(int f, hipStream_t s) override { rec("hook after_hp f=%d S%ld", f, SN(s)); return 0; }
  int before_nn(int f, hipStream_t s) override { rec("hook before_nn f=%d S%ld", f, SN(s)); return 0; }
  int after_k3(int f, hipStream_t s) override { rec("hook after_k3 f=%d S%ld", f, SN(s)); return 0; }
};

// ---- SHA-256 (FIPS 180-4) ----
static std::string sha256(const std::string &msg) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::string m = msg;
  const uint64_t bits = (uint64_t)msg.size() * 8;
  m.push_back((char)0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int i = 7; i >= 0; i--) m.push_back((char)(bits >> (8 * i)));
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  for (size_t off = 0; off < m.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
      w[i] = (uint32_t)(uint8_t)m[off + 4 * i] << 24 | (uint32_t)(uint8_t)m[off + 4 * i + 1] << 16 | (uint32_t)(uint8_t)m[off + 4 * i + 2] << 8 |
             (uint32_t)(uint8_t)m[off + 4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  }
  char out[65];
  for (int i = 0; i < 8; i++) snprintf(out + 8 * i, 9, "%08x", h[i]);
  return out;
}

// ---- what the cases are made of ----
static RNNModel *g_models[3];
static RNNoiseBatch *g_b;
// the return value of an API call and the host-side state it may have moved
static int ret(const char *what, int r) {
  const RNNoiseBatch *b = g_b;
  if (b)
    rec("-> %s = %d | parity=%d ring_slot=%d frame_no=%ld per_stream=%d img_valid=%d split_pending=%d launches=%ld", what, r, b->parity,
        b->ring_slot, b->frame_no, (int)b->per_stream, (int)b->img_valid, b->split_pending, b->launches);
  else rec("-> %s = %d", what, r);
  return r;
}
#define CALL(expr) ret(#expr, (expr))
static void open_batch(int n, int cus = 256) {
  g_cus = cus;
  g_b = rnnoise_batch_create(g_models[0], n, 0);
  ret("create", g_b ? 0 : -1);
}
static void close_batch() {
  rnnoise_batch_destroy(g_b);
  g_b = nullptr;
}
// the cases' device buffers: fixed places far apart
static float *d_out() { return usr<float>(0x10000000); }
static float *d_in() { return usr<float>(0x20000000); }
static float *d_vad() { return usr<float>(0x30000000); }
static float *d_gains() { return usr<float>(0x40000000); }
static unsigned char *d_mask() { return usr<unsigned char>(0x50000000); }
static int *d_list() { return usr<int>(0x60000000); }
static float *d_feat() { return usr<float>(0x70000000); }
static int *d_sil() { return usr<int>(0x80000000); }
static int *d_counts() { return usr<int>(0x90000000); }
static int *d_frames() { return usr<int>(0xa0000000); }
static unsigned char *d_table() { return usr<unsigned char>(0xb0000000); }
static hipStream_t caller_stream() { return reinterpret_cast<hipStream_t>(uintptr_t(100)); }  // (a stream of the caller's own)

static const int FRAMES[] = {0, 1, 2, 3, 4, 5, 9};
// every call length twice in a row -- float with vad and gains on the caller's stream, then int16 without on the null stream
static void frames_case(int schedule, bool timing, int n = 64) {
  open_batch(n);
  CALL(rnnoise_batch_set_schedule(g_b, schedule));
  if (timing) CALL(rnnoise_batch_enable_timing(g_b, 1));
  for (int F : FRAMES) {
    CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), F, caller_stream()));
    CALL(rnnoise_batch_process_device_s16(g_b, (short *)d_out(), (const short *)d_in(), nullptr, nullptr, F, nullptr));
  }
  double ms[4];
  long launches = 0;
  if (timing) CALL(rnnoise_batch_kernel_ms(g_b, ms, &launches));
  CALL(rnnoise_batch_process_device(g_b, nullptr, d_in(), nullptr, nullptr, 1, nullptr));
  CALL(rnnoise_batch_process_device(g_b, d_out(), nullptr, nullptr, nullptr, 1, nullptr));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, -1, nullptr));
  CALL(rnnoise_batch_process_device(nullptr, d_out(), d_in(), nullptr, nullptr, 1, nullptr));
  close_batch();
}
// one network form: one frame, two frames (the second step of the layer-wise network has no requant), five pipelined, with timing
static void nn_case(int n, int path, int cus, int n_models, bool timing) {
  open_batch(n, cus);
  if (path >= 0) CALL(rnnoise_batch_set_nn_path(g_b, path));
  for (int k = 1; k < n_models; k++) CALL(rnnoise_batch_add_model(g_b, g_models[k]));
  if (n_models > 1) CALL(rnnoise_batch_set_stream_models_device(g_b, d_table(), nullptr));
  if (timing) CALL(rnnoise_batch_enable_timing(g_b, 1));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), 1, nullptr));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), 2, nullptr));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 5, caller_stream()));
  CALL(rnnoise_batch_set_schedule(g_b, 9));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
  double ms[4];
  if (timing) CALL(rnnoise_batch_kernel_ms(g_b, ms, nullptr));
  close_batch();
}
static void split_case(int schedule, bool s16, bool strided, bool silence, bool timing) {
  open_batch(64);
  CALL(rnnoise_batch_set_schedule(g_b, schedule));
  if (timing) CALL(rnnoise_batch_enable_timing(g_b, 1));
  CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));  // (parity is not 0 from here)
  for (int T : {1, 2, 3, 4, 6, 9}) {
    const RNNoiseRows fr{65, 65L * T}, gr{32, 32L * T}, vr{1, T};
    if (s16) CALL(rnnoise_batch_analyze_device_s16(g_b, d_feat(), strided ? &fr : nullptr, silence ? d_sil() : nullptr, (const short *)d_in(), T, caller_stream()));
    else CALL(rnnoise_batch_analyze_device(g_b, d_feat(), strided ? &fr : nullptr, silence ? d_sil() : nullptr, d_in(), T, caller_stream()));
    if (T == 2) {  // what is refused while frames are pending, and a synthesis of another length
      CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 1, nullptr));
      CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 4, nullptr, 1, nullptr));
      CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, nullptr, 0, nullptr, 1, nullptr));
      CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 100, nullptr, nullptr, nullptr, nullptr));
      CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 100, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
      CALL(rnnoise_batch_set_schedule(g_b, 9));
      CALL(rnnoise_batch_set_nn_path(g_b, 1));
      CALL(rnnoise_batch_set_pcm_rate(g_b, 16000));
      CALL(rnnoise_batch_analyze_device(g_b, d_feat(), nullptr, nullptr, d_in(), 1, nullptr));
      CALL(rnnoise_batch_synthesize_device(g_b, d_out(), d_gains(), nullptr, d_vad(), nullptr, 3, nullptr));
      float host_pcm[4];
      CALL(rnnoise_batch_process_masked(g_b, host_pcm, host_pcm, nullptr, nullptr, (const unsigned char *)host_pcm, 1));
    }
    if (s16) CALL(rnnoise_batch_synthesize_device_s16(g_b, (short *)d_out(), d_gains(), strided ? &gr : nullptr, d_vad(), strided ? &vr : nullptr, T, caller_stream()));
    else CALL(rnnoise_batch_synthesize_device(g_b, d_out(), d_gains(), strided ? &gr : nullptr, d_vad(), strided ? &vr : nullptr, T, caller_stream()));
    CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), T == 3 ? 4 : 1, nullptr));
  }
  CALL(rnnoise_batch_analyze_device(g_b, d_feat(), nullptr, nullptr, d_in(), 0, nullptr));
  CALL(rnnoise_batch_synthesize_device(g_b, d_out(), d_gains(), nullptr, d_vad(), nullptr, 0, nullptr));
  CALL(rnnoise_batch_synthesize_device(g_b, d_out(), d_gains(), nullptr, d_vad(), nullptr, 1, nullptr));
  double ms[4];
  if (timing) CALL(rnnoise_batch_kernel_ms(g_b, ms, nullptr));
  close_batch();
}

struct Case { const char *name; std::function<void()> run; };
static const std::vector<Case> &cases() {
  static const std::vector<Case> all = {
      {"frames_sched0", [] { frames_case(0, false); }},
      {"frames_sched1", [] { frames_case(1, false); }},
      {"frames_sched9", [] { frames_case(9, false); }},
      {"frames_sched0_timed", [] { frames_case(0, true); }},
      {"frames_sched1_timed", [] { frames_case(1, true); }},
      {"frames_sched9_timed", [] { frames_case(9, true); }},
      {"frames_sched0_4096", [] { frames_case(0, false, 4096); }},  // (K0 lane = stream, K1 four streams per workgroup, K3 wide)
      {"nn_one", [] { nn_case(64, 0, 256, 1, false); }},
      {"nn_one_timed", [] { nn_case(64, 0, 256, 1, true); }},
      {"nn_vector", [] { nn_case(513, 0, 256, 1, false); }},
      {"nn_tiles", [] { nn_case(64, 1, 256, 1, false); }},  // (sixteen waves alone, eight in a pipelined call)
      {"nn_tiles_default_path", [] { nn_case(1024, -1, 256, 1, true); }},
      {"nn_layers", [] { nn_case(64, 2, 256, 1, false); }},
      {"nn_layers_timed", [] { nn_case(64, 2, 256, 1, true); }},
      {"nn_layers_w4", [] { nn_case(128, 2, 1, 1, false); }},
      {"nn_layers_two_models", [] { nn_case(64, 2, 256, 2, false); }},
      {"nn_layers_two_models_timed", [] { nn_case(64, 2, 256, 2, true); }},
      {"nn_one_three_models", [] { nn_case(64, 0, 256, 3, true); }},
      {"masked",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_masked(g_b, d_out(), d_in(), d_vad(), d_gains(), d_mask(), 0, nullptr));
         CALL(rnnoise_batch_process_device_masked(g_b, d_out(), d_in(), d_vad(), d_gains(), d_mask(), 3, caller_stream()));
         CALL(rnnoise_batch_process_device_masked_s16(g_b, (short *)d_out(), (const short *)d_in(), nullptr, nullptr, d_mask(), 1, nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 4, nullptr));  // (per-stream phase stays)
         CALL(rnnoise_batch_reset(g_b));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 1, nullptr));
         close_batch();
       }},
      {"list",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_set_nn_path(g_b, 2));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 1, nullptr));  // (the layer images are valid now)
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), d_vad(), d_gains(), d_list(), 5, nullptr, 3, caller_stream()));
         CALL(rnnoise_batch_process_device_list_s16(g_b, (short *)d_out(), (const short *)d_in(), nullptr, d_gains(), d_list(), 7, d_mask(), 1, nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 1, nullptr));
         CALL(rnnoise_batch_set_nn_path(g_b, 0));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), d_vad(), nullptr, d_list(), 64, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 0, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, nullptr, 0, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(nullptr, d_out(), d_in(), nullptr, nullptr, nullptr, 0, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, nullptr, 3, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 65, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), -1, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 0, nullptr, -2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, nullptr, d_in(), nullptr, nullptr, d_list(), 4, nullptr, 1, nullptr));
         close_batch();
       }},
      {"layout_channels_link",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_set_pcm_layout(g_b, 64 * 512, 512));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), 3, nullptr));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 480, 480 * 2));  // (stream-contiguous: two frames fit, three do not)
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 3, nullptr));
         CALL(batch_process_device_impl(g_b, {.out = d_out(), .in = d_in(), .n_frames = 3, .packed = true}));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 0, 0));
         CALL(rnnoise_batch_set_pcm_channels(g_b, 2));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 6, nullptr, 1, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 5, nullptr, 1, nullptr));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 64 * 480, 960));
         CALL(rnnoise_batch_process_device_s16(g_b, (short *)d_out(), (const short *)d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 0, 0));
         CALL(rnnoise_batch_set_pcm_channels(g_b, 1));
         CALL(rnnoise_batch_set_gain_link(g_b, 2));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), d_vad(), d_gains(), 2, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 6, nullptr, 1, nullptr));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 5, nullptr, 1, nullptr));
         CALL(rnnoise_batch_set_pcm_channels(g_b, 4));
         CALL(rnnoise_batch_process_device_list(g_b, d_out(), d_in(), nullptr, nullptr, d_list(), 6, nullptr, 1, nullptr));
         close_batch();
       }},
      {"tables",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_set_stream_out_rates_device(g_b, d_table(), nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_set_stream_out_formats_device(g_b, d_table(), nullptr));
         CALL(rnnoise_batch_process_device_s16(g_b, (short *)d_out(), (const short *)d_in(), d_vad(), nullptr, 1, nullptr));
         CALL(rnnoise_batch_set_pcm_rate(g_b, 48000));  // (drops both)
         CALL(rnnoise_batch_set_stream_rates_device(g_b, d_table(), nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         CALL(rnnoise_batch_set_stream_formats_device(g_b, d_table(), nullptr));
         CALL(rnnoise_batch_process_device_s16(g_b, (short *)d_out(), (const short *)d_in(), nullptr, nullptr, 1, nullptr));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 1, nullptr));
         CALL(rnnoise_batch_set_pcm_rate(g_b, 16000));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 3, nullptr));
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 500, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_set_stream_out_formats_device(g_b, d_table(), nullptr));
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 500, nullptr, nullptr, nullptr, nullptr));
         close_batch();
       }},
      {"host_fed_ring",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_set_schedule(g_b, 1));
         RecIo io;
         for (int F : {1, 2, 9})
           CALL(batch_process_device_impl(g_b, {.out = d_out(), .in = d_in(), .vad = d_vad(), .gains = d_gains(), .n_frames = F,
                                               .stream = caller_stream(), .hooks = &io}));
         CALL(rnnoise_batch_set_pcm_channels(g_b, 2));  // (the ring never sees channels, a link or a layout)
         CALL(rnnoise_batch_set_gain_link(g_b, 2));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 64 * 512, 1024));
         CALL(batch_process_device_impl(g_b, {.out = d_out(), .in = d_in(), .n_frames = 4, .s16 = true, .hooks = &io}));
         close_batch();
       }},
      {"split_sched0", [] { split_case(0, false, false, true, false); }},
      {"split_sched0_timed", [] { split_case(0, false, true, true, true); }},
      {"split_sched1", [] { split_case(1, false, false, false, false); }},
      {"split_sched9", [] { split_case(9, false, false, true, false); }},
      {"split_sched9_s16_strided", [] { split_case(9, true, true, false, false); }},
      {"split_sched0_s16_strided", [] { split_case(0, true, true, true, false); }},
      {"chunks",
       [] {
         open_batch(64);
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 700, d_vad(), d_gains(), d_frames(), caller_stream()));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, d_list(), 8, d_vad(), nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_s16(g_b, (short *)d_out(), (const short *)d_in(), d_counts(), 480, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 2000, nullptr, nullptr, nullptr, nullptr));  // (grows)
         CALL(rnnoise_batch_process_device_chunks_list_s16(g_b, (short *)d_out(), (const short *)d_in(), d_counts(), 100, d_list(), 64, nullptr, nullptr, d_frames(), nullptr));
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, d_list(), 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), nullptr, d_counts(), 700, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), -1, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list_s16(nullptr, (short *)d_out(), (const short *)d_in(), d_counts(), 7, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, nullptr, 3, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, d_list(), 65, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), nullptr, 700, nullptr, nullptr, nullptr, nullptr));
         int fill[64];
         CALL(rnnoise_batch_chunk_fill(g_b, fill));
         CALL(rnnoise_batch_set_gain_link(g_b, 2));  // (chunk calls do not combine with it: the no-op rule sees that too)
         CALL(rnnoise_batch_process_device_chunks(g_b, d_out(), d_in(), d_counts(), 700, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_device_chunks_list(g_b, d_out(), d_in(), d_counts(), 700, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_reset(g_b));
         close_batch();
       }},
      {"chunks_host",
       [] {
         open_batch(8);
         std::vector<float> in(8 * 700, 0.f), out(8 * 700, 0.f), vad(2 * 8), gains(2 * 8 * 32);
         std::vector<int> counts(8, 700), frames(8), list = {3, 1, 7};
         g_host = {{"in", (const char *)in.data(), in.size() * 4}, {"out", (const char *)out.data(), out.size() * 4},
                   {"vad", (const char *)vad.data(), vad.size() * 4}, {"gains", (const char *)gains.data(), gains.size() * 4},
                   {"counts", (const char *)counts.data(), counts.size() * 4}, {"frames", (const char *)frames.data(), frames.size() * 4},
                   {"list", (const char *)list.data(), list.size() * 4}};
         CALL(rnnoise_batch_process_chunks(g_b, out.data(), in.data(), counts.data(), 700, vad.data(), gains.data(), frames.data()));
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, list.data(), 3, vad.data(), nullptr, nullptr));
         CALL(rnnoise_batch_process_chunks_list_s16(g_b, (short *)out.data(), (const short *)in.data(), counts.data(), 700, list.data(), 3, nullptr, nullptr, frames.data()));
         CALL(rnnoise_batch_process_chunks_s16(g_b, (short *)out.data(), (const short *)in.data(), counts.data(), 700, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, nullptr, 0, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), nullptr, counts.data(), 700, nullptr, 0, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, list.data(), 0, nullptr, nullptr, nullptr));
         list[2] = 3;  // (a stream twice)
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, list.data(), 3, nullptr, nullptr, nullptr));
         list[2] = 8;  // (outside the batch)
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, list.data(), 3, nullptr, nullptr, nullptr));
         list[2] = 7;
         counts[1] = 701;
         CALL(rnnoise_batch_process_chunks_list(g_b, out.data(), in.data(), counts.data(), 700, list.data(), 3, nullptr, nullptr, nullptr));
         CALL(rnnoise_batch_process_chunks(g_b, out.data(), in.data(), counts.data(), 700, nullptr, nullptr, nullptr));
         counts[1] = 0;
         CALL(rnnoise_batch_process_chunks(g_b, out.data(), in.data(), counts.data(), 0, nullptr, nullptr, nullptr));
         close_batch();
       }},
      {"staged",
       [] {
         open_batch(8);
         CALL(rnnoise_batch_set_pcm_channels(g_b, 2));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 4 * 1024, 1024));
         const int F = 3;
         std::vector<float> in(F * 4 * 1024, 0.f), out(F * 4 * 1024, 0.f), vad(F * 8), gains(F * 8 * 32);
         std::vector<unsigned char> mask(F * 8, 1);
         std::vector<int> list = {6, 7, 2, 3};
         g_host = {{"in", (const char *)in.data(), in.size() * 4}, {"out", (const char *)out.data(), out.size() * 4},
                   {"vad", (const char *)vad.data(), vad.size() * 4}, {"gains", (const char *)gains.data(), gains.size() * 4},
                   {"mask", (const char *)mask.data(), mask.size()}, {"list", (const char *)list.data(), list.size() * 4}};
         CALL(rnnoise_batch_process_masked(g_b, out.data(), in.data(), vad.data(), gains.data(), mask.data(), F));
         CALL(rnnoise_batch_process_masked_s16(g_b, (short *)out.data(), (const short *)in.data(), nullptr, nullptr, mask.data(), 1));
         CALL(batch_process_staged(g_b, {.out = out.data(), .in = in.data(), .vad = vad.data(), .n_frames = F}));  // (no mask: out stays down)
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), vad.data(), gains.data(), list.data(), 4, nullptr, 2));
         CALL(rnnoise_batch_process_list_s16(g_b, (short *)out.data(), (const short *)in.data(), nullptr, nullptr, list.data(), 4, mask.data(), 1));
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), nullptr, nullptr, list.data(), 3, nullptr, 1));  // (half a group)
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), nullptr, nullptr, list.data(), 0, nullptr, 1));
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), nullptr, nullptr, nullptr, 2, nullptr, 1));
         list[1] = 6;
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), nullptr, nullptr, list.data(), 4, nullptr, 1));
         list[1] = 8;
         CALL(rnnoise_batch_process_list(g_b, out.data(), in.data(), nullptr, nullptr, list.data(), 4, nullptr, 1));
         CALL(rnnoise_batch_process_masked(g_b, out.data(), in.data(), nullptr, nullptr, mask.data(), 0));
         CALL(rnnoise_batch_process_masked(g_b, out.data(), in.data(), nullptr, nullptr, mask.data(), -1));
         CALL(rnnoise_batch_process_masked(g_b, out.data(), in.data(), nullptr, nullptr, nullptr, 1));  // (host_io.cpp's)
         CALL(rnnoise_batch_set_pcm_layout(g_b, 0, 0));
         CALL(rnnoise_batch_set_pcm_channels(g_b, 1));
         CALL(rnnoise_batch_set_stream_out_rates_device(g_b, d_table(), nullptr));
         CALL(batch_process_staged(g_b, {.out = out.data(), .in = in.data(), .n_frames = 1}));  // (an out-rate table: out goes up)
         close_batch();
       }},
      {"staged_split",
       [] {
         open_batch(8);
         const int T = 3;
         std::vector<float> in(T * 8 * 480, 0.f), out(T * 8 * 480, 0.f), feat(8 * T * 65 + 7), gains(8 * T * 32), vad(8 * T);
         std::vector<int> sil(T * 8);
         g_host = {{"in", (const char *)in.data(), in.size() * 4}, {"out", (const char *)out.data(), out.size() * 4},
                   {"feat", (const char *)feat.data(), feat.size() * 4}, {"gains", (const char *)gains.data(), gains.size() * 4},
                   {"vad", (const char *)vad.data(), vad.size() * 4}, {"sil", (const char *)sil.data(), sil.size() * 4}};
         const RNNoiseRows fr{65, 65L * T}, gr{32, 32L * T}, vr{1, T};
         CALL(rnnoise_batch_analyze(g_b, feat.data(), &fr, sil.data(), in.data(), T));
         CALL(rnnoise_batch_process_masked(g_b, out.data(), in.data(), nullptr, nullptr, (const unsigned char *)sil.data(), 1));
         CALL(rnnoise_batch_synthesize(g_b, out.data(), gains.data(), &gr, vad.data(), &vr, T));
         CALL(rnnoise_batch_analyze_s16(g_b, feat.data(), nullptr, nullptr, (const short *)in.data(), 2));
         CALL(rnnoise_batch_synthesize_s16(g_b, (short *)out.data(), gains.data(), nullptr, vad.data(), nullptr, 2));
         CALL(rnnoise_batch_set_pcm_layout(g_b, 8 * 480, 480));
         CALL(rnnoise_batch_analyze(g_b, feat.data(), nullptr, sil.data(), in.data(), 1));
         CALL(rnnoise_batch_synthesize(g_b, out.data(), gains.data(), nullptr, vad.data(), nullptr, 1));
         CALL(rnnoise_batch_analyze(g_b, feat.data(), nullptr, sil.data(), nullptr, 1));
         CALL(rnnoise_batch_synthesize(g_b, nullptr, gains.data(), nullptr, vad.data(), nullptr, 0));
         close_batch();
       }},
      {"host_lists",
       [] {
         open_batch(8);
         std::vector<float> snaps(3 * RNNOISE_AMD_SNAP_FLOATS, 0.f), recs(3 * RN_CHUNK_REC, 0.f);
         std::vector<int> list = {5, 0, 5};
         g_host = {{"snaps", (const char *)snaps.data(), snaps.size() * 4}, {"recs", (const char *)recs.data(), recs.size() * 4},
                   {"list", (const char *)list.data(), list.size() * 4}};
         CALL(rnnoise_batch_save_streams(g_b, snaps.data(), list.data(), 3));  // (a save may name a stream twice)
         CALL(rnnoise_batch_load_streams(g_b, snaps.data(), list.data(), 3));  // (no magic: refused)
         CALL(rnnoise_batch_save_chunk_fifos(g_b, recs.data(), list.data(), 3));
         CALL(rnnoise_batch_load_chunk_fifos(g_b, recs.data(), list.data(), 3));
         for (int i = 0; i < 3; i++) {
           const int magic = RN_SNAP_MAGIC, hdr[3] = {0, 480, RN_CHUNK_MAGIC};
           memcpy(&snaps[(size_t)i * RN_SNAP_FLOATS + RN_SNAP_OFF_MAGIC], &magic, 4);
           memcpy(&recs[(size_t)i * RN_CHUNK_REC + RN_CHUNK_OFF_FILL], hdr, sizeof hdr);
         }
         CALL(rnnoise_batch_load_streams(g_b, snaps.data(), list.data(), 3));  // (a stream twice)
         CALL(rnnoise_batch_load_chunk_fifos(g_b, recs.data(), list.data(), 3));
         list[2] = 8;
         CALL(rnnoise_batch_save_streams(g_b, snaps.data(), list.data(), 3));  // (outside the batch)
         CALL(rnnoise_batch_save_chunk_fifos(g_b, recs.data(), list.data(), 3));
         CALL(rnnoise_batch_reset_streams(g_b, list.data(), 3));
         list[2] = 7;
         CALL(rnnoise_batch_load_streams(g_b, snaps.data(), list.data(), 3));
         CALL(rnnoise_batch_load_chunk_fifos(g_b, recs.data(), list.data(), 3));
         CALL(rnnoise_batch_load_streams(g_b, snaps.data(), nullptr, 3));  // (no list: the whole batch or nothing)
         list[2] = 5;
         CALL(rnnoise_batch_reset_streams(g_b, list.data(), 3));  // (a reset may name a stream twice)
         close_batch();
       }},
      {"train_features",
       [] {
         open_batch(8);
         std::vector<float> pcm(2 * 8 * 480, 0.f), vad(2 * 8), rec98(2 * 8 * 98);
         std::vector<int> ints(8, 0);
         CALL(rnnoise_batch_train_features_device(g_b, d_feat(), d_in(), d_in(), d_vad(), d_list(), d_list(), d_list(), 2, nullptr));
         CALL(rnnoise_batch_train_features_device(g_b, d_feat(), d_in(), d_in(), d_vad(), d_list(), d_list(), d_list(), 0, nullptr));
         CALL(rnnoise_batch_train_features(g_b, rec98.data(), pcm.data(), pcm.data(), vad.data(), ints.data(), ints.data(), ints.data(), 2));
         CALL(rnnoise_batch_train_features(g_b, rec98.data(), pcm.data(), pcm.data(), vad.data(), ints.data(), ints.data(), ints.data(), 0));
         CALL(rnnoise_batch_process_device(g_b, d_out(), d_in(), nullptr, nullptr, 2, nullptr));
         close_batch();
       }},
  };
  return all;
}

static void run_case(const Case &c) {
  g_trace.clear();
  g_host.clear();
  g_bump = 0;
  g_streams = g_events = 0;
  g_device = 0;
  c.run();
  g_host.clear();
}

int main(int argc, char **argv) {
  for (int k = 0; k < 3; k++) {
    g_models[k] = new RNNModel();
    g_models[k]->blob_len = k + 1;
  }
  const char *dump = argc == 3 && !strcmp(argv[1], "--dump") ? argv[2] : nullptr;
  if (argc != 1 && !dump) {
    fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]);
    return 2;
  }
  bool found = false;
  for (const Case &c : cases()) {
    if (dump && strcmp(dump, c.name)) continue;
    found = true;
    run_case(c);
    std::string text;
    for (const std::string &l : g_trace) text += l, text += '\n';
    if (dump) fputs(text.c_str(), stdout);
    else printf("%s %zu %s\n", c.name, g_trace.size(), sha256(text).c_str());
  }
  for (RNNModel *m : g_models) delete m;
  if (!found) {
    fprintf(stderr, "no such case: %s\n", dump);
    return 2;
  }
  return 0;
}
