// batch_tables.cpp -- the configuration of a batch's calls: PCM rate, strides and channels, and the per-stream tables (rates and
// formats of the input side and of the output side, models, controls).  Nothing here launches a kernel: the step (batch_step.cpp) reads
// what these calls leave in the batch.
#include "shim.h"

// ---- the per-stream tables ----
// A table is n rows of device memory that lives from its first set to the batch's end, and a field of b->g that points at it while
// a table is set.  Each has a host setter (synchronous: a call in flight keeps what it was launched with, and the table is in place
// when the setter returns), a device setter (a copy, not a kernel: ordered on the caller's stream between its calls; the kernels
// sanitise what they read) and a getter (synchronous).  The three of every table are its validation, one of the helpers below, and
// what that table alone does -- said in the comment at its host setter.  The callers have selected the batch's device.
namespace {
template <typename T>
int table_alloc(RNNoiseBatch *b, T *&buf, size_t row_bytes) {  // memory on first use
  if (!buf) HIP_OK(hipMalloc((void **)&buf, (size_t)b->n * row_bytes));
  return 0;
}
// the host set: drain the device, copy, drain again; rows == null (the table is being dropped) copies nothing.  `drained` is what
// the table alone does to device memory once nothing is in flight, ahead of the copy.
template <typename T, typename F>
int table_set_host(RNNoiseBatch *b, T *&buf, size_t row_bytes, const void *rows, F drained) {
  HIP_OK(hipDeviceSynchronize());
  if (drained()) return -1;
  if (rows) {
    if (table_alloc(b, buf, row_bytes)) return -1;
    HIP_OK(hipMemcpy(buf, rows, (size_t)b->n * row_bytes, hipMemcpyHostToDevice));
  }
  HIP_OK(hipDeviceSynchronize());
  return 0;
}
template <typename T>
int table_set_host(RNNoiseBatch *b, T *&buf, size_t row_bytes, const void *rows) {
  return table_set_host(b, buf, row_bytes, rows, [] { return 0; });
}
template <typename T>
int table_set_device(RNNoiseBatch *b, T *&buf, size_t row_bytes, const void *d_rows, hipStream_t st) {
  if (table_alloc(b, buf, row_bytes)) return -1;
  HIP_OK(hipMemcpyAsync(buf, d_rows, (size_t)b->n * row_bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}
// the get: `fill` in every byte when no table is live (live == null), else drain and copy; the caller normalises the entries
int table_get(RNNoiseBatch *b, const void *live, size_t row_bytes, void *rows, int fill) {
  if (!live) {
    memset(rows, fill, (size_t)b->n * row_bytes);
    return 0;
  }
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(rows, live, (size_t)b->n * row_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// PCM rate: K0 upsamples the caller's rows from the rate of code L, K3 downsamples its output back (rn_dev.h: RnGroupDev::rs_L).  48 kHz
// without a rate table leaves g.rs_hist / g.rs_L null: every launch is then the one of a batch that never saw these calls.
// the code of a rate the batch API takes (rn_dev.h: rn_rate_samples), 0 for any other
int rate_code(int hz) { return hz == 32000 ? RN_RATE_32K : (hz == 48000 || hz == 24000 || hz == 16000 || hz == 8000) ? 48000 / hz : 0; }
// the group's resampler fields from the batch's rate and whether it has a rate table (rn_dev.h: RnGroupDev::rs_Ls)
void rs_point(RNNoiseBatch *b, bool table) {
  const size_t N = b->n;
  const bool on = table || b->pcm_rate != 48000;
  b->g.rs_L = on ? rate_code(b->pcm_rate) : 0;
  b->g.rs_pitch = on ? rn_rate_samples(b->g.rs_L) : 0;
  b->g.rs_hist = on ? b->rs_buf : nullptr;
  b->g.rs_up = on ? b->rs_buf + N * RN_RS_HIST : nullptr;
  b->g.rs_dn = on ? b->rs_buf + N * (RN_RS_HIST + RN_FRAME_SIZE) : nullptr;
  b->g.rs_Ls = table ? b->rate_map : nullptr;
}
// [N][RN_RS_HIST] histories (zero), then the [N][480] planes rs_up and rs_dn (the 48 kHz frames between the filters and the bodies of
// K0 / K3), on first use; the zeroing is ordered on st
int rs_alloc(RNNoiseBatch *b, hipStream_t st) {
  if (b->rs_buf) return 0;
  if (table_alloc(b, b->rs_buf, (RN_RS_HIST + 2 * RN_FRAME_SIZE) * sizeof(float))) return -1;
  HIP_OK(hipMemsetAsync(b->rs_buf, 0, (size_t)b->n * RN_RS_HIST * sizeof(float), st));
  return 0;
}
// whether a byte of a rate table names a rate of a batch at code Lb: a code whose frame fits the batch's row, M_s <= M_b
bool rate_code_ok(int v, int Lb) {
  return (v == 1 || v == 2 || v == 3 || v == 6 || v == RN_RATE_32K) && rn_rate_samples(v) <= rn_rate_samples(Lb);
}
// a table as the kernels read it: an entry that names no rate of this batch is the batch's own code
void rates_as_read(unsigned char *rates, int n, int Lb) {
  for (int s = 0; s < n; s++)
    if (!rate_code_ok(rates[s], Lb)) rates[s] = (unsigned char)Lb;
}
// the [N] codes K0 reads now (input == true: the rate table, or Lb everywhere) or K3 reads now (the out-rate table, else the same);
// the caller has drained the device
int codes_now(RNNoiseBatch *b, bool input, std::vector<uint8_t> &cur) {
  const int Lb = rate_code(b->pcm_rate);
  const uint8_t *live = !input && b->out_Ls ? b->out_Ls : b->g.rs_Ls;
  cur.assign((size_t)b->n, (uint8_t)Lb);
  if (live) {
    HIP_OK(hipMemcpy(cur.data(), live, (size_t)b->n, hipMemcpyDeviceToHost));
    rates_as_read(cur.data(), b->n, Lb);
  }
  return 0;
}
// zero floats [first, first + count) of the history of every stream whose code in cur differs from its code in next: one strided
// memset per run of such streams, on the null stream
int restart_changed_halves(RNNoiseBatch *b, const std::vector<uint8_t> &cur, const std::vector<uint8_t> &next, size_t first, size_t count) {
  const size_t N = b->n;
  for (size_t s = 0; s < N;) {
    if (cur[s] == next[s]) {
      s++;
      continue;
    }
    size_t e = s + 1;
    while (e < N && cur[e] != next[e]) e++;
    HIP_OK(hipMemset2DAsync(b->rs_buf + s * RN_RS_HIST + first, RN_RS_HIST * sizeof(float), 0, count * sizeof(float), e - s, nullptr));
    s = e;
  }
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_set_pcm_rate(RNNoiseBatch *b, int hz) {
  if (!b || !rate_code(hz)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int old = b->pcm_rate;
  b->frame_stride = b->row_stride = 0;  // (a PCM layout is in samples of the old rate's frame: dropped by every call)
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous: nothing of the old rate is in flight)
  const bool out_rates = b->out_Ls != nullptr;
  b->out_Ls = b->out_fmt = nullptr;  // (the out tables go with the rate table: they describe rows of the old rate)
  if (hz == old && !b->g.rs_Ls && !out_rates) {  // (a rate table is dropped by every call: the rows are redefined)
    if (batch_chunk_restart_all(b)) return -1;  // (... and the sample FIFOs of the chunk calls restart with every call)
    HIP_OK(hipDeviceSynchronize());
    return old;
  }
  if (hz != 48000 && rs_alloc(b, nullptr)) return -1;
  if (b->rs_buf) HIP_OK(hipMemset(b->rs_buf, 0, (size_t)b->n * RN_RS_HIST * sizeof(float)));
  HIP_OK(hipDeviceSynchronize());
  b->pcm_rate = hz;
  rs_point(b, false);
  if (batch_chunk_restart_all(b)) return -1;  // (at the new frame length)
  HIP_OK(hipDeviceSynchronize());
  return old;
}

extern "C" int rnnoise_batch_pcm_rate(const RNNoiseBatch *b) { return b ? b->pcm_rate : -1; }

// ---- per-stream rates (include/rnnoise_amd.h) ----
// The [N] code bytes (a divisor, or RN_RATE_32K) live in rate_map; while a table is set (g.rs_Ls) the batch runs its resampling launches at 48 kHz too
// (rs_L = 1), and K0 / K3 and the snapshot kernels take each stream's divisor from it (rn_dev.h: rn_stream_L).
// This table alone: NULL drops the table (nothing to do without one).  A host set also allocates rs_buf, restarts from zero the
// history of exactly the streams whose divisor changes, and re-points the resampler fields (rs_point); rnnoise_batch_set_pcm_rate
// drops the table with both strides.  The device set allocates rs_buf with its zeroing on the caller's stream, leaves the histories
// to the caller (include/rnnoise_amd.h), and points the fields only if no table is live.  An entry that names no rate of this batch
// reads as the batch's own divisor -- the getter's default too.
extern "C" int rnnoise_batch_set_stream_rates(RNNoiseBatch *b, const unsigned char *rates) {
  if (!b) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int Lb = rate_code(b->pcm_rate);
  if (rates)
    for (int s = 0; s < b->n; s++)
      if (!rate_code_ok(rates[s], Lb)) return -1;
  if (!rates && !b->g.rs_Ls) return 0;
  ON_DEVICE(b->device);
  const size_t N = b->n;
  auto restart_changed = [&]() -> int {
    std::vector<uint8_t> cur(N, (uint8_t)Lb);  // (the divisors the kernels read now)
    if (b->g.rs_Ls) {
      HIP_OK(hipMemcpy(cur.data(), b->rate_map, N, hipMemcpyDeviceToHost));
      rates_as_read(cur.data(), b->n, Lb);
    }
    if (rs_alloc(b, nullptr)) return -1;
    if (b->out_Ls) {  // (an out-rate table owns the down halves: only the up half follows the input code)
      std::vector<uint8_t> next(N, (uint8_t)Lb);
      if (rates) next.assign(rates, rates + N);
      return restart_changed_halves(b, cur, next, 0, RN_RS_DOWN0);
    }
    // one memset per run of streams whose divisor changes
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
    return 0;
  };
  if (table_set_host(b, b->rate_map, 1, rates, restart_changed)) return -1;
  rs_point(b, rates != nullptr);
  return 0;
}

extern "C" int rnnoise_batch_set_stream_rates_device(RNNoiseBatch *b, const unsigned char *d_rates, void *hip_stream) {
  if (!b || !d_rates) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (rs_alloc(b, st) || table_set_device(b, b->rate_map, 1, d_rates, st)) return -1;
  if (!b->g.rs_Ls) rs_point(b, true);
  return 0;
}

extern "C" int rnnoise_batch_stream_rates(RNNoiseBatch *b, unsigned char *rates) {
  if (!b || !rates) return -1;
  const int Lb = rate_code(b->pcm_rate);
  if (table_get(b, b->g.rs_Ls, 1, rates, Lb)) return -1;
  rates_as_read(rates, b->n, Lb);
  return 0;
}

// ---- per-stream output rates (include/rnnoise_amd.h) ----
// The [N] code bytes live in out_rate_map; while a table is set (b->out_Ls) the step points K3's copy of the group at it in the place
// of the rate table (shim.h: batch_k3_group), so that K3 writes every stream at the table's code whatever K0 read it at, and the
// snapshot kernels get it beside the group (batch_state_group).  b->g is not touched: K0 and the plan's input side stay what they
// were.  The two halves of a stream's history then belong to two codes: [0, RN_RS_DOWN0) to its input code, the rest to its output
// code.
// This table alone: NULL drops the table (nothing to do without one): every stream's output code is its input code again.  A host set
// allocates rs_buf and restarts from zero the DOWN half of exactly the streams whose effective output code changes.  The device set
// allocates rs_buf with its zeroing on the caller's stream and leaves the histories to the caller.  An entry that names no rate of
// this batch reads as the batch's own code, as K3 reads every table -- the getter's answer too; without a table the getter gives the
// input codes.
extern "C" int rnnoise_batch_set_stream_out_rates(RNNoiseBatch *b, const unsigned char *rates) {
  if (!b) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int Lb = rate_code(b->pcm_rate);
  if (rates)
    for (int s = 0; s < b->n; s++)
      if (!rate_code_ok(rates[s], Lb)) return -1;
  if (!rates && !b->out_Ls) return 0;
  ON_DEVICE(b->device);
  const size_t N = b->n;
  auto restart_changed = [&]() -> int {
    std::vector<uint8_t> cur, next;
    if (codes_now(b, false, cur)) return -1;
    if (rates) next.assign(rates, rates + N);
    else if (codes_now(b, true, next)) return -1;
    if (rs_alloc(b, nullptr)) return -1;
    return restart_changed_halves(b, cur, next, RN_RS_DOWN0, RN_RS_HIST - RN_RS_DOWN0);
  };
  if (table_set_host(b, b->out_rate_map, 1, rates, restart_changed)) return -1;
  b->out_Ls = rates ? b->out_rate_map : nullptr;
  return 0;
}

extern "C" int rnnoise_batch_set_stream_out_rates_device(RNNoiseBatch *b, const unsigned char *d_rates, void *hip_stream) {
  if (!b || !d_rates) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (rs_alloc(b, st) || table_set_device(b, b->out_rate_map, 1, d_rates, st)) return -1;
  b->out_Ls = b->out_rate_map;
  return 0;
}

extern "C" int rnnoise_batch_stream_out_rates(RNNoiseBatch *b, unsigned char *rates) {
  if (!b || !rates) return -1;
  const int Lb = rate_code(b->pcm_rate);
  if (table_get(b, b->out_Ls ? b->out_Ls : b->g.rs_Ls, 1, rates, Lb)) return -1;
  rates_as_read(rates, b->n, Lb);
  return 0;
}

// ---- caller-defined PCM strides (include/rnnoise_amd.h) ----
// Two numbers of the batch.  A process call hands the row stride to K0 / K3 (rn_dev.h: RnGroupDev::pcm_pitch) and steps its frame
// pointers by the frame stride (batch_step.cpp: Step::begin); without a layout both keep their defaults and every launch is
// the one of a batch that never saw these calls.
extern "C" int rnnoise_batch_set_pcm_layout(RNNoiseBatch *b, long frame_stride, long row_stride) {
  if (!b || !rn_pcm_layout_ok(frame_stride, row_stride)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous: a call in flight keeps what it was launched with)
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
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int old = b->channels;
  if (channels == old) return old;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous: a call in flight keeps what it was launched with)
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

// ---- linked gains (include/rnnoise_amd.h) ----
// One number of the batch, with the rule of the channel count.  A process call hands it to K3 alone (rn_dev.h: RnGroupDev::link); at 1
// nothing is handed on and every launch is the one of a batch that never saw these calls.
extern "C" int rnnoise_batch_set_gain_link(RNNoiseBatch *b, int k) {
  if (!b || !rn_pcm_channels_ok(k, b->n)) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  const int old = b->link;
  if (k == old) return old;
  ON_DEVICE(b->device);
  HIP_OK(hipDeviceSynchronize());  // (synchronous: a call in flight keeps what it was launched with)
  b->link = k;
  return old;
}

extern "C" int rnnoise_batch_gain_link(const RNNoiseBatch *b) { return b ? b->link : -1; }

// ---- per-stream PCM formats (include/rnnoise_amd.h) ----
// The [N] format bytes live in fmt_map; while a table is set (g.pcm_fmt) K0 expands and K3 compresses the rows of the companded
// streams in every int16 call (rn_dev.h: rn_stream_fmt), and those calls plan K0 one wave per stream (dispatch.h).
// This table alone: NULL drops the table (nothing to do without one).  It is configuration: nothing is zeroed when it changes, and
// nothing but these two setters and the batch's end touches it.  The device set points g.pcm_fmt at once.  A byte that names no law
// reads as linear int16 rows -- the getter's default too.
extern "C" int rnnoise_batch_set_stream_formats(RNNoiseBatch *b, const unsigned char *formats) {
  if (!b) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (formats)
    for (int s = 0; s < b->n; s++)
      if (formats[s] > RNNOISE_AMD_PCM_ALAW) return -1;
  if (!formats && !b->g.pcm_fmt) return 0;
  ON_DEVICE(b->device);
  if (table_set_host(b, b->fmt_map, 1, formats)) return -1;
  b->g.pcm_fmt = formats ? b->fmt_map : nullptr;
  return 0;
}

extern "C" int rnnoise_batch_set_stream_formats_device(RNNoiseBatch *b, const unsigned char *d_formats, void *hip_stream) {
  if (!b || !d_formats) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  if (table_set_device(b, b->fmt_map, 1, d_formats, static_cast<hipStream_t>(hip_stream))) return -1;
  b->g.pcm_fmt = b->fmt_map;
  return 0;
}

extern "C" int rnnoise_batch_stream_formats(RNNoiseBatch *b, unsigned char *formats) {
  if (!b || !formats) return -1;
  if (table_get(b, b->g.pcm_fmt, 1, formats, RNNOISE_AMD_PCM_LINEAR)) return -1;
  for (int s = 0; s < b->n; s++)
    if (formats[s] > RNNOISE_AMD_PCM_ALAW) formats[s] = RNNOISE_AMD_PCM_LINEAR;  // (as the kernels read it)
  return 0;
}

// ---- per-stream output formats (include/rnnoise_amd.h) ----
// The [N] format bytes live in out_fmt_map; while a table is set (b->out_fmt) the step points K3's copy of the group at it in the
// place of the format table (shim.h: batch_k3_group): K0 expands what the format table says, K3 compresses what this one says.
// Configuration like the format table: nothing is zeroed, and nothing but these two setters, rnnoise_batch_set_pcm_rate and the
// batch's end touches it.  A byte that names no law reads as linear; without a table the getter gives the input formats.
extern "C" int rnnoise_batch_set_stream_out_formats(RNNoiseBatch *b, const unsigned char *formats) {
  if (!b) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (formats)
    for (int s = 0; s < b->n; s++)
      if (formats[s] > RNNOISE_AMD_PCM_ALAW) return -1;
  if (!formats && !b->out_fmt) return 0;
  ON_DEVICE(b->device);
  if (table_set_host(b, b->out_fmt_map, 1, formats)) return -1;
  b->out_fmt = formats ? b->out_fmt_map : nullptr;
  return 0;
}

extern "C" int rnnoise_batch_set_stream_out_formats_device(RNNoiseBatch *b, const unsigned char *d_formats, void *hip_stream) {
  if (!b || !d_formats) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  if (table_set_device(b, b->out_fmt_map, 1, d_formats, static_cast<hipStream_t>(hip_stream))) return -1;
  b->out_fmt = b->out_fmt_map;
  return 0;
}

extern "C" int rnnoise_batch_stream_out_formats(RNNoiseBatch *b, unsigned char *formats) {
  if (!b || !formats) return -1;
  if (table_get(b, b->out_fmt ? b->out_fmt : b->g.pcm_fmt, 1, formats, RNNOISE_AMD_PCM_LINEAR)) return -1;
  for (int s = 0; s < b->n; s++)
    if (formats[s] > RNNOISE_AMD_PCM_ALAW) formats[s] = RNNOISE_AMD_PCM_LINEAR;  // (as the kernels read it)
  return 0;
}

// ---- per-stream models (include/rnnoise_amd.h) ----
// The network of every step is launched once per slot (batch_step.cpp: batch_network_step); the launch of slot k owns the streams
// the [N] slot bytes of model_map put on k (rn_dev.h: rn_owns).
// This table alone: it exists from the first add_model on, which allocates and zeroes it and points g.model_of / g.n_models from then
// on; before that every stream is on slot 0, nothing is read, and both setters are no-ops (the host one still checks its entries).
// NULL is refused.  The kernels read an entry that names no slot as slot 0; the getter hands the bytes out as they are.
extern "C" int rnnoise_batch_add_model(RNNoiseBatch *b, RNNModel *model) {
  if (!b || !model || b->n_models >= RNNOISE_AMD_MAX_MODELS) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  RnModelDev md;
  if (model_on_device(model, b->device, md)) return -1;
  HIP_OK(hipDeviceSynchronize());  // (synchronous: a call in flight keeps the slots it was launched with)
  if (!b->model_map) {
    if (table_alloc(b, b->model_map, 1)) return -1;
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
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  for (int s = 0; s < b->n; s++)
    if (models[s] >= b->n_models) return -1;
  if (!b->model_map) return 0;
  ON_DEVICE(b->device);
  return table_set_host(b, b->model_map, 1, models);
}

extern "C" int rnnoise_batch_set_stream_models_device(RNNoiseBatch *b, const unsigned char *d_models, void *hip_stream) {
  if (!b || !d_models) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!b->model_map) return 0;
  ON_DEVICE(b->device);
  return table_set_device(b, b->model_map, 1, d_models, static_cast<hipStream_t>(hip_stream));
}

extern "C" int rnnoise_batch_stream_models(RNNoiseBatch *b, unsigned char *models) {
  if (!b || !models) return -1;
  return table_get(b, b->model_map, 1, models, 0);
}

// ---- per-stream suppression controls (include/rnnoise_amd.h) ----
// ctl_buf holds the [N][RN_CTL_FLOATS] table, then the [N] hold counters; g.ctl / g.gate_c point into it while a table is set, and
// K3 reads them (rn_dev.h: RnGroupDev::ctl).  Without a table both are null and every launch is the one of a batch that never saw
// these calls.
// This table alone: NULL drops g.ctl and g.gate_c, after the drain.  Either setter arms the counters (ctl_arm): they start at
// RN_CTL_NONE only when the batch goes from no table to a table, ordered on the null stream or on the caller's.  K3 sanitises what
// a device set hands it (NaN as 0, clamped, truncated); the getter hands the table out as it is, zeros without one.
static_assert(RN_CTL_FLOATS == RNNOISE_AMD_CTL_FLOATS, "one record size for the kernels and the API");
namespace {
constexpr size_t CTL_ROW_BYTES = RN_CTL_FLOATS * sizeof(float);
bool ctl_entry_ok(const float *e) {
  const float floor_gain = e[0], thr = e[1], hold = e[2];
  return std::isfinite(floor_gain) && std::isfinite(thr) && std::isfinite(hold) && floor_gain >= 0.f && floor_gain <= 1.f &&
         thr >= 0.f && thr <= 1.f && hold >= 0.f && hold <= 65535.f && hold == std::floor(hold);
}
int ctl_arm(RNNoiseBatch *b, hipStream_t st) {
  const size_t N = b->n;
  if (table_alloc(b, b->ctl_buf, CTL_ROW_BYTES + sizeof(int))) return -1;
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
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (ctl)
    for (int s = 0; s < b->n; s++)
      if (!ctl_entry_ok(ctl + (size_t)s * RN_CTL_FLOATS)) return -1;
  ON_DEVICE(b->device);
  if (table_set_host(b, b->ctl_buf, CTL_ROW_BYTES, ctl, [&] { return ctl ? ctl_arm(b, nullptr) : 0; })) return -1;
  if (!ctl) {
    b->g.ctl = nullptr;
    b->g.gate_c = nullptr;
  }
  return 0;
}

extern "C" int rnnoise_batch_set_stream_controls_device(RNNoiseBatch *b, const float *d_ctl, void *hip_stream) {
  if (!b || !d_ctl) return -1;
  if (batch_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  ON_DEVICE(b->device);
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (ctl_arm(b, st)) return -1;
  return table_set_device(b, b->ctl_buf, CTL_ROW_BYTES, d_ctl, st);
}

extern "C" int rnnoise_batch_stream_controls(RNNoiseBatch *b, float *ctl) {
  if (!b || !ctl) return -1;
  return table_get(b, b->g.ctl, CTL_ROW_BYTES, ctl, 0);
}
