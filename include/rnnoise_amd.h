/* rnnoise_amd.h -- additive batched C API of the MI355X RNNoise back end.
 *
 * The reference API (include/rnnoise.h of xiph/rnnoise, mirrored by our include/rnnoise.h)
 * is one-frame / one-stream / synchronous (rnnoise.h:94); thousands of concurrent streams
 * cannot be expressed through it.  These entry points are what a maintainer's
 * FFI would bind for the throughput path.  Plain C ABI: pointers and sizes only.
 *
 * A "batch" is N independent 48 kHz mono streams resident on one GPU, advancing in
 * lock-step one 480-sample frame per step.  Frame buffers are stream-major:
 *     in / out : [n_frames][n_streams][480] float, int16-scaled like rnnoise_demo.c:56
 *     vad      : [n_frames][n_streams]      (return value of rnnoise_process_frame)
 *     gains    : [n_frames][n_streams][32]  raw band gains (the `g[]` local of
 *                src/denoise.c:465 right after compute_rnn; 0 on silent frames), optional
 */
#ifndef RNNOISE_AMD_H
#define RNNOISE_AMD_H

#include "rnnoise.h"
#include "rn_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RNNoiseBatch RNNoiseBatch;

/* Number of visible HIP devices (0 if none / runtime unavailable). */
RNNOISE_EXPORT int rnnoise_amd_device_count(void);

/* The reference's x86 tanh / sigmoid divide through `rcpps` (src/vec_avx.h:413,442,484,505), whose low bits depend on
 * the CPU family: its output is a function of the host it runs on.  The library reproduces one family at a time from a
 * 4096-entry table (rnnoise_amd/csrc/rcp_profiles.h):
 *   "host"      (default, alias "auto") the table is captured from the CPU this process runs on, so the bits are those the
 *               reference library produces on this same machine;
 *   "intel"     Intel Xeon (the committed goldens);  "amd-zen5" (alias "amd")  AMD EPYC 9005.
 * Process-wide: $RNNOISE_AMD_RCP_PROFILE at first use, or this call at any time (devices are drained and their table
 * replaced; every model and batch follows).  0, or -1 for an unknown name.  rnnoise_amd_rcp_profile() names the active
 * profile: "intel", "amd-zen5", "host=intel", "host=amd-zen5", "host=captured" (a CPU whose table equals neither). */
RNNOISE_EXPORT int rnnoise_amd_set_rcp_profile(const char *name);
RNNOISE_EXPORT const char *rnnoise_amd_rcp_profile(void);

/* The reference's one libm call on the path is log10 of the band energies in double, rounded to float (src/denoise.c:383): which
 * double comes out is a property of the HOST's libm.  The kernels restate GNU libc's algorithm (>= 2.28, the FMA build every AVX2
 * host selects) operation for operation (rnnoise_amd/csrc/log10_glibc.h) -- bit-identical to that libm for every float band energy
 * (swept exhaustively) -- after checking at first use that this process's libm is that one.  $RNNOISE_AMD_LOG10 = host (default) |
 * glibc-fma | ocml (the device library's log10).  Names the model in use: "host=glibc-fma", "glibc-fma", "ocml", or
 * "host=unknown:ocml" (a different libm: said on stderr once). */
RNNOISE_EXPORT const char *rnnoise_amd_log10_model(void);

/* Create N zero-initialised streams on `device`, all using `model` (must outlive the
 * batch, like rnnoise_create()).  NULL on error (no GPU, bad model, out of memory).
 * model==NULL fails here (the drop-in entry points rnnoise_create / rnnoise_init fall back
 * to $RNNOISE_AMD_DEFAULT_MODEL; the batched API wants the model spelled out). */
RNNOISE_EXPORT RNNoiseBatch *rnnoise_batch_create(RNNModel *model, int n_streams, int device);
RNNOISE_EXPORT void rnnoise_batch_destroy(RNNoiseBatch *b);
RNNOISE_EXPORT int rnnoise_batch_size(const RNNoiseBatch *b);

/* Back to the state rnnoise_init() produces (all zeros). 0 / -1. */
RNNOISE_EXPORT int rnnoise_batch_reset(RNNoiseBatch *b);

/* Host buffers; synchronous.  vad and gains may be NULL.  in may alias out. 0 / -1.
 * Pinned host memory (hipHostMalloc / hipHostRegister) is read and written by DMA in place, frame by frame, through a
 * six-slot ring in HBM beside ONE pipelined multi-frame device call: a call pays one frame's upload before and one frame's
 * download after its kernels whatever its length (use 16 frames or more per call when throughput matters).  Where the runtime
 * offers two free copy engines, uploads and downloads run on two NAMED SDMA engines at once (underneath HIP; DESIGN section 4,
 * $RNNOISE_AMD_HOSTIO_COPY): 65,536 streams 30.9 M frames/s with int16 PCM, 21.2 M with floats.  Pageable
 * memory goes through the library's pinned bounce buffers in ~32 MB chunks, two in flight.  A call that fails part of the way
 * drains the device and resets the batch (every stream back to its initial state) before it returns -1. */
RNNOISE_EXPORT int rnnoise_batch_process(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains,
                                         int n_frames);

/* Device-resident buffers (same shapes, memory of the batch's device, 16-byte aligned: the
 * kernels read and write them 16 bytes per lane); asynchronous on `hip_stream` (a hipStream_t,
 * NULL = default stream).  This is the throughput path. */
RNNOISE_EXPORT int rnnoise_batch_process_device(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad,
                                                float *d_gains, int n_frames, void *hip_stream);

/* The same two calls with 16-bit PCM at both ends: in / out : [n_frames][n_streams][480] int16.  The conversions are those
 * of the reference's only caller (examples/rnnoise_demo.c:56,58: x[i] = tmp[i] going in, tmp[i] = x[i] -- the C float -> short
 * conversion as x86 compiles it, truncation toward zero -- coming out) done inside the first and the last kernel of the step,
 * so a frame moves 2 x 960 bytes instead of 2 x 1,920 over HBM and PCIe.  Bits are those of the float calls followed by
 * that cast.  Device buffers 8-byte aligned.  The float and s16 calls may be mixed on one batch. */
RNNOISE_EXPORT int rnnoise_batch_process_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                             int n_frames);
RNNOISE_EXPORT int rnnoise_batch_process_device_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                    float *d_gains, int n_frames, void *hip_stream);

/* Masked calls: streams that skip frames.  active : [n_frames][n_streams] unsigned char, nonzero = the stream has this frame.
 * For every stream the result is that of rnnoise_process_frame() on its PRESENT frames only, in order: a present frame gives
 * out / vad / gains and state bit for bit as the unmasked call; on an absent frame the stream's state is not touched, its row of
 * `out` is not written (the caller's bytes stay), vad reads 0 and its gains row 32 zeros, as on a silent frame, and the rows of
 * `in` are not read.  active == NULL: every stream present -- exactly rnnoise_batch_process*.  Buffer shapes as in the unmasked
 * calls.  The first masked call switches the batch to per-stream frame phase (each stream's pitch ring and spectra slots follow
 * its own frame count); it stays there until rnnoise_batch_reset, and every call keeps working in it, but the analysis then runs
 * one stream per workgroup at every batch size (the cost) and rnnoise_batch_train_features* returns -1.
 * rnnoise_batch_debug_last reports silence = 2 for a stream that was absent from the last frame.
 * Device forms: device buffers as rnnoise_batch_process_device, asynchronous on hip_stream.  Host forms: the convenience path --
 * synchronous, staged through device memory with plain copies (no pinned ring or copy engines).  0 / -1. */
RNNOISE_EXPORT int rnnoise_batch_process_device_masked(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad,
                                                       float *d_gains, const unsigned char *d_active, int n_frames,
                                                       void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_device_masked_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                           float *d_gains, const unsigned char *d_active, int n_frames,
                                                           void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_masked(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains,
                                                const unsigned char *active, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_process_masked_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                                    const unsigned char *active, int n_frames);

/* Stream-list calls: advance ONLY the listed streams, with compact buffers.  Their cost follows n_rows, not the batch size.
 * Buffers are indexed by list position i, not by stream: in / out [n_frames][n_rows][480 / L] (float or int16, at the batch's PCM
 * rate 48000 / L), vad [n_frames][n_rows], gains [n_frames][n_rows][32] or NULL.  streams[i] is the batch stream of row i, in any
 * order.  active: optional [n_frames][n_rows] unsigned char, nonzero = row i has this frame; NULL = every listed stream has every frame.
 * A listed stream gets exactly what the masked call would give it with the same frames present in full-size buffers: out, vad,
 * gains and state, bit for bit.  An unlisted stream is not touched -- not its state, resampler history, gate counter or phase.  An
 * absent frame's vad reads 0 and its gains row 32 zeros; its out row is not written.  The first list call switches the batch to
 * per-stream frame phase, as the first masked call does (rnnoise_batch_train_features* then returns -1 until rnnoise_batch_reset).
 * List calls work together with lock-step, masked and list calls on the same batch, every PCM rate and int16, model slots (the
 * network runs once per slot, over the listed rows only), suppression controls and rnnoise_batch_reset_streams[_device].
 * Device forms: asynchronous on hip_stream, device buffers as the masked device calls; d_streams is int32 in the batch's device
 * memory.  An entry outside [0, n_streams) makes its row absent.  Duplicate entries are the caller's error: the affected streams'
 * results are unspecified, and no other stream changes.  Host forms: the masked calls' convenience path (synchronous, staged
 * through device memory with plain copies); the list is checked first, and an out-of-range or duplicate entry returns -1 with
 * nothing changed.  n_rows == 0 is a successful no-op; n_rows < 0, n_rows > n_streams, or a NULL list with n_rows > 0 return -1.
 * After a list call rnnoise_batch_debug_last defines only the entries of the streams listed in the last frame.  0 / -1. */
RNNOISE_EXPORT int rnnoise_batch_process_device_list(RNNoiseBatch *b, float *d_out, const float *d_in, float *d_vad,
                                                     float *d_gains, const int *d_streams, int n_rows,
                                                     const unsigned char *d_active, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_device_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, float *d_vad,
                                                         float *d_gains, const int *d_streams, int n_rows,
                                                         const unsigned char *d_active, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_list(RNNoiseBatch *b, float *out, const float *in, float *vad, float *gains,
                                              const int *streams, int n_rows, const unsigned char *active, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_process_list_s16(RNNoiseBatch *b, short *out, const short *in, float *vad, float *gains,
                                                  const int *streams, int n_rows, const unsigned char *active, int n_frames);

/* Back to rnnoise_init()'s state for the listed streams only; every other stream is untouched.  Host list: synchronous, -1 if an
 * index is out of range (nothing is reset then).  Device list (int32 in the batch's device memory): asynchronous on hip_stream,
 * out-of-range entries ignored.  Duplicates are harmless; n == 0 does nothing.  0 / -1. */
RNNOISE_EXPORT int rnnoise_batch_reset_streams(RNNoiseBatch *b, const int *streams, int n);
RNNOISE_EXPORT int rnnoise_batch_reset_streams_device(RNNoiseBatch *b, const int *d_streams, int n, void *hip_stream);

/* PCM rate of the batch's calls: 48000 (default), 32000, 24000, 16000 or 8000.  Returns the previous rate, or -1 for any other
 * value (nothing changes then).  Synchronous.  Changing the rate zeroes every stream's resampler history; the
 * DenoiseState of every stream is untouched.
 * At rate R the in / out buffers of every rnnoise_batch_process* call are [n_frames][n_streams][M], M = 480 R / 48000 samples per
 * 10 ms frame (320, 240, 160 or 80), float or int16 as before; vad and gains stay per 10 ms frame.  Each
 * stream is upsampled to 48 kHz, run through rnnoise_process_frame() frame by frame, and downsampled back to R (int16: the input
 * converted exactly, the downsampled float output with the truncating cast of the 48 kHz calls).  For the divisors L = 48000 / R
 * (2, 3 or 6) the filters are one Kaiser-windowed sinc per L of 48 L taps (rnnoise_amd/resample.py defines them and their arithmetic
 * bit for bit); up followed by down is a pure delay of RNNOISE_AMD_RESAMPLE_DELAY = 47 low-rate samples.  32 kHz divides nothing: it
 * is 2:3 through a common 96 kHz grid, over the filter of L = 3 read at that grid (again 48 taps per 48 kHz sample on the way up, 72
 * per 32 kHz sample on the way down; frames map to frames, no phase is carried between them).  Up followed by down is a delay of the
 * same 47 samples at 32 kHz, but not an exact one: the 2:1 step in the middle aliases at the filter's stop-band level (70 dB down).
 * Device-buffer calls stay asynchronous and
 * pipelined; host-buffer calls at R != 48000 are synchronous and staged through device memory (the convenience path of the masked
 * host calls).  An absent frame of a masked call leaves the stream's resampler history untouched; rnnoise_batch_reset,
 * rnnoise_batch_reset_streams[_device] and rnnoise_batch_import_state zero it.  rnnoise_batch_train_features* returns -1 at
 * R != 48000.  The per-frame API of rnnoise.h stays 48 kHz only. */
#define RNNOISE_AMD_RESAMPLE_DELAY 47
#define RNNOISE_AMD_RATE_32K 32 /* the code of a 32 kHz stream where the other rates have their divisor: rate tables, snapshot records */
RNNOISE_EXPORT int rnnoise_batch_set_pcm_rate(RNNoiseBatch *b, int hz);
RNNOISE_EXPORT int rnnoise_batch_pcm_rate(const RNNoiseBatch *b);

/* Mixed-rate batches: a PCM rate per stream.  rates[n_streams] is the rate CODE L_s of every stream: the divisor 48000 / rate -- 1, 2,
 * 3 or 6 (48, 24, 16, 8 kHz) -- or RNNOISE_AMD_RATE_32K for 32 kHz, which divides nothing.  M_s is the stream's samples per frame: 480
 * / L_s, 320 at 32 kHz.  The batch's own rate (rnnoise_batch_set_pcm_rate, code Lb, frame M_b) keeps defining the ROW PITCH of every
 * PCM buffer: in / out rows stay M_b samples apart in every call form (lock-step, masked, list; float and int16; host and device).  A
 * stream runs at the batch's rate or below it, M_s <= M_b, so that its frame fits its row: a batch at 48 kHz takes all five rates, one
 * at 32 kHz takes 32, 24, 16 and 8 kHz, one at 16 kHz takes 16 and 8 kHz.  Stream s uses the FIRST M_s samples of its row; the rest of
 * its `in` row is not read and the rest
 * of its `out` row is not written (the caller's bytes stay).  vad and gains stay per 10 ms frame.  Every stream gives, bit for bit in
 * out, vad, gains and exported state, what it gives in a uniform batch at its own rate -- for L_s = 1 the plain 48 kHz path: no
 * filter, no added delay -- whatever the rates of its neighbours.  Without a table a batch launches exactly what it launched before
 * these calls existed.
 * rnnoise_batch_set_stream_rates (host array): synchronous, like rnnoise_batch_set_stream_models; -1 and no change if any entry is
 * no code or has M_s > M_b (code 32 in a batch at 24 kHz or below, a divisor below Lb).  The resampler history of every stream whose divisor CHANGES is zeroed; a stream whose divisor
 * stays keeps its history and continues bit for bit.  No stream's DenoiseState, gate counter, model slot, controls or frame phase is
 * touched.  rates == NULL drops the table: every stream is at the batch's rate again (history zeroed for the streams that were not)
 * and the batch is back to the launches of one that never had a table.
 * rnnoise_batch_set_stream_rates_device (n_streams bytes in the batch's device memory): a copy ordered on hip_stream (no kernel, no
 * host synchronisation; the first table of a batch allocates its memory).  Entries are not checked: the kernel that reads one maps
 * anything that is no code, or that has M_s > M_b, to Lb (so byte 32 reads as 32 kHz in a batch at 48 or 32 kHz, and as the batch's
 * rate in one at 24 kHz or below).  It does NOT touch histories: a stream whose divisor it changes must
 * be reset (rnnoise_batch_reset_streams_device) or loaded from a snapshot on the same stream before its next frame -- which is what
 * recycling a slot for a new call does anyway; otherwise that stream's first frames start from the old rate's history (finite
 * samples, confined to that stream, gone after 47 of its input samples and 47 L_s of its 48 kHz output samples).
 * rnnoise_batch_stream_rates reads the divisors back as the kernels read them (synchronous; Lb everywhere when there is no table).
 * rnnoise_batch_set_pcm_rate drops the table.  rnnoise_batch_reset, reset_streams[_device] and import_state zero histories as before
 * and leave the table alone.  rnnoise_batch_train_features* returns -1 while a table is set.  Snapshots: save writes the stream's own
 * divisor into the record, load copies the history when the record's divisor equals the DESTINATION stream's current one and zeroes
 * it otherwise.  Host-buffer process calls on a batch with a table take the staged convenience path of the low-rate batches, also at
 * Lb = 1.  With a table K0 runs one wave per stream at every batch size, as in a low-rate batch (the cost).
 * 0 / -1; a NULL batch or buffer returns -1 without touching the device. */
RNNOISE_EXPORT int rnnoise_batch_set_stream_rates(RNNoiseBatch *b, const unsigned char *rates);
RNNOISE_EXPORT int rnnoise_batch_set_stream_rates_device(RNNoiseBatch *b, const unsigned char *d_rates, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_rates(RNNoiseBatch *b, unsigned char *rates);

/* Per-stream G.711: a PCM format per stream.  formats[n_streams] says what the rows of every `_s16` call hold for each stream:
 * RNNOISE_AMD_PCM_LINEAR int16 samples (the meaning of those calls without a table), RNNOISE_AMD_PCM_ULAW or RNNOISE_AMD_PCM_ALAW one
 * G.711 byte per sample.  The table describes every _s16 call form -- lock-step, masked and list; device and host --; the float calls
 * ignore it.  The ROW PITCH does not change: rows stay 480 / Lb int16 (960 / Lb bytes) apart, Lb the batch's divisor.  A companded
 * stream with M = 480 / L_s samples per frame (L_s from the rate table, else Lb) uses the FIRST M bytes of its row; the rest of its `in`
 * row is not read and the rest of its `out` row is not written (the caller's bytes stay) -- the rate table's rule applied to bytes, so
 * that an 8 kHz G.711 leg (80 bytes) sits beside a 48 kHz linear leg (960 bytes) in one buffer.  Any format goes with any rate.
 * The codec is the 14-bit mu-law / 13-bit A-law form that rnnoise_amd/g711.py states, equal for every input to CPython's audioop at
 * width 2.  >> is an arithmetic shift, x the int16 sample, b the byte:
 *   mu-law  encode  p = x >> 2; neg = p < 0; p = min((neg ? -p : p) + 33, 8191); seg = floor(log2(p)) - 5;
 *                   b = ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF)
 *           decode  u = ~b & 0xFF; t = (((u & 15) << 3) + 132) << ((u >> 4) & 7); x = (u & 0x80) ? 132 - t : t - 132
 *   A-law   encode  i = x >> 3; neg = i < 0; if (neg) i = ~i; seg = i < 32 ? 0 : floor(log2(i)) - 4;
 *                   m = seg < 2 ? (i >> 1) & 15 : (i >> seg) & 15; b = ((seg << 4) | m) ^ (neg ? 0x55 : 0xD5)
 *           decode  a = b ^ 0x55; t = (a & 15) << 4; seg = (a >> 4) & 7; t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
 *                   x = (a & 0x80) ? t : -t
 * Result, bit for bit: a companded stream's vad, gains and complete state (snapshot) are those of the same stream fed decode(bytes)
 * through the same _s16 call on a batch without a format table, and its output bytes are encode() of that call's int16 output (the
 * truncating conversion of the _s16 calls, then the code).  Every other stream of the batch is unchanged in every bit.  This holds in
 * every call form, at every rate, with masks, lists, model slots and controls, and across rnnoise_batch_reset_streams[_device] and
 * snapshot save / load.
 * rnnoise_batch_set_stream_formats (host array): synchronous, like rnnoise_batch_set_stream_models; -1 and no change if any entry is
 * above 2.  formats == NULL drops the table: the batch then launches exactly what a batch that never had one launches.
 * rnnoise_batch_set_stream_formats_device (n_streams bytes in the batch's device memory): a copy ordered on hip_stream (no kernel, no
 * host synchronisation; the first table of a batch allocates its n_streams bytes).  Entries are not checked: the kernel that reads one
 * takes anything that is not 1 or 2 as linear.
 * rnnoise_batch_stream_formats reads the table back as the kernels read it (synchronous; zeros when there is none).
 * A format is configuration, not state: it has no history, nothing is zeroed when it changes, and it does not appear in snapshots.
 * rnnoise_batch_reset, reset_streams[_device], import_state, load_streams, set_pcm_rate, set_stream_rates, set_nn_path and
 * set_schedule leave the table alone (set_pcm_rate too: no entry can become invalid at another rate).  A slot recycled for a leg of
 * another codec: set_stream_rates_device + set_stream_formats_device + reset_streams_device on one stream.
 * Host-buffer _s16 calls on a batch with a table take the staged convenience path, as with a rate table.
 * rnnoise_batch_train_features* is a float call and ignores the table.  While a table is set the _s16 calls run K0 one wave per
 * stream at every batch size, as with a rate table -- at 48 kHz without a rate table that replaces the lane-per-stream K0 of batches
 * above 2,048 streams, whose cost has not been measured yet; float calls launch what they launched before.
 * 0 / -1; a NULL batch or buffer returns -1 without touching the device.  The per-frame API of rnnoise.h stays linear float. */
#define RNNOISE_AMD_PCM_LINEAR 0   /* int16: the _s16 calls without a table */
#define RNNOISE_AMD_PCM_ULAW   1
#define RNNOISE_AMD_PCM_ALAW   2
RNNOISE_EXPORT int rnnoise_batch_set_stream_formats(RNNoiseBatch *b, const unsigned char *formats);
RNNOISE_EXPORT int rnnoise_batch_set_stream_formats_device(RNNoiseBatch *b, const unsigned char *d_formats, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_formats(RNNoiseBatch *b, unsigned char *formats);

/* Per-stream OUTPUT rates and formats: legs that leave in another shape than they came in -- 48 kHz linear in and 8 kHz mu-law out
 * towards the PSTN, G.711 in and 16 kHz linear out towards a recogniser.  The two tables above describe a stream's `in` and `out`
 * rows with one entry; these two describe the `out` rows alone, with the same codes: rates[n_streams] of 1, 2, 3, 6 or
 * RNNOISE_AMD_RATE_32K, formats[n_streams] of RNNOISE_AMD_PCM_LINEAR / _ULAW / _ALAW.
 * WITHOUT an out table a stream's output code is its input code -- its entry of the rate table, or the batch's code Lb without one;
 * the same for formats -- and the batch launches exactly what it launched before these calls existed.  WITH one, stream s's `out`
 * rows are written at the out table's code L_out (format F_out) whatever its input code L_in (F_in) is.
 * Rows: the ROW PITCH stays that of the batch's rate, M_b samples, in `in` and in `out`.  Stream s reads the first M_in samples (a
 * companded stream: bytes) of its `in` row and writes the first M_out samples (bytes) of its `out` row; the rest of either row is
 * neither read nor written.  So an out code must be a code with M_out <= M_b, the rule of the rate table.
 * Result, bit for bit: the stream's vad, gains and DenoiseState are those of the same stream in a uniform batch at L_in and F_in; its
 * output is Down(L_out) of the 48 kHz denoised signal -- the 48 kHz signal itself, written in place, for L_out = 1 --, in the _s16
 * calls followed by the truncating cast and then F_out's encoder.  rnnoise_amd/resample.py (Up, Down) and rnnoise_amd/g711.py define
 * every stage.  The delay is the sum of the two stages' delays, Up(L_in)'s in input samples plus Down(L_out)'s in 48 kHz samples; for
 * L_in != L_out it is in general no whole number of output samples, and there is no call that reports it.  Float calls ignore both
 * format tables.
 * Histories: the up half of a stream's resampler history belongs to L_in, the down half to L_out.
 * rnnoise_batch_set_stream_out_rates (host array): synchronous; -1 and no change if any entry is no code or has M_out > M_b.  The DOWN
 * half of exactly the streams whose effective output code changes is zeroed; the up half and every DenoiseState stay.  NULL drops the
 * table (the down half of the streams whose output code thereby changes is zeroed).  While an out-rate table is set,
 * rnnoise_batch_set_stream_rates zeroes only the UP half of the streams whose input code changes; without one it does what it did.
 * rnnoise_batch_set_stream_out_rates_device (n_streams bytes in the batch's device memory): a copy ordered on hip_stream, no kernel,
 * no check, no history touched (the rules of rnnoise_batch_set_stream_rates_device).  K3 reads this table where it would read the
 * rate table, with that table's rule: a byte that is no code, or has M_out > M_b, reads as the batch's code Lb -- which is the
 * stream's input code wherever the rate table does not say otherwise.
 * rnnoise_batch_set_stream_out_formats[_device]: configuration like the format table; nothing is zeroed; -1 for an entry above 2 (host),
 * anything that is not 1 or 2 reads as linear (device).
 * rnnoise_batch_stream_out_rates / _out_formats read the codes back as K3 reads them (synchronous): without an out table, what
 * rnnoise_batch_stream_rates / _formats answer.
 * rnnoise_batch_set_pcm_rate drops both out tables along with the rate table.  rnnoise_batch_reset, reset_streams[_device] and
 * import_state zero both halves of the history and leave the tables alone.  A slot recycled for another leg: the device setters of
 * the tables that change + reset_streams_device, on one stream.
 * Snapshots: save writes the output code beside the stream's own code while the batch has an out-rate table (0 otherwise: a record
 * of a batch without one is what it was); load copies the up half when the record's code is the destination stream's input code and
 * the down half when the record's output code (0: its code) is the destination's effective output code, and zeroes a half otherwise.
 * Works with every call form (lock-step, masked, list; float and int16; host and device), model slots, controls, linked gains, PCM
 * layouts and channels; the channel rule holds per side: within a group all outputs are linear or all are companded.  Host-buffer
 * calls with an out table take the staged convenience path.  Chunk calls return -1 with nothing launched while either out table is
 * set; rnnoise_batch_train_features* returns -1 while an out-rate table is set and ignores the out-format table.
 * K0 never reads an out table: a batch whose inputs are all 48 kHz linear keeps the lane-per-stream K0 above 2,048 streams whatever
 * its outputs are.  0 / -1; a NULL batch or buffer returns -1 without touching the device. */
RNNOISE_EXPORT int rnnoise_batch_set_stream_out_rates(RNNoiseBatch *b, const unsigned char *rates);
RNNOISE_EXPORT int rnnoise_batch_set_stream_out_rates_device(RNNoiseBatch *b, const unsigned char *d_rates, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_out_rates(RNNoiseBatch *b, unsigned char *rates);
RNNOISE_EXPORT int rnnoise_batch_set_stream_out_formats(RNNoiseBatch *b, const unsigned char *formats);
RNNOISE_EXPORT int rnnoise_batch_set_stream_out_formats_device(RNNoiseBatch *b, const unsigned char *d_formats, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_out_formats(RNNoiseBatch *b, unsigned char *formats);

/* Caller-defined PCM strides: where the frames of `in` and `out` lie.  By default every rnnoise_batch_process* call takes PCM as
 * [n_frames][n_rows][M], M = 480 / Lb samples (Lb the batch's divisor; n_rows = n_streams, or the list length of a list call): frame f
 * of row r starts at sample (f * n_rows + r) * M.  With a layout set it starts at
 *     f * frame_stride + r * row_stride
 * in `in` and in `out`, both strides in SAMPLES of the call's own type (float, or int16 in the _s16 calls -- a companded row keeps
 * its int16 stride and holds its bytes at the front of its slot).  So a [B][T] tensor or one contiguous jitter buffer per call leg is
 * passed where it lies: frame_stride = M, row_stride = samples between the buffers.
 * rnnoise_batch_set_pcm_layout: (0, 0) is the default and drops the layout -- the batch then launches exactly what a batch that never
 * saw the call launches.  Any other pair must have both strides > 0 and multiples of 4 samples (80, 160, 240 and 480 all are: the 16-byte
 * alignment of the float kernels and the 8-byte alignment of the int16 ones stay; the buffers themselves must be aligned as before);
 * otherwise -1 and nothing changes.  Synchronous, like rnnoise_batch_set_pcm_rate.
 * Every process call of a batch with a layout: the frames must not overlap --
 *     row-major:          row_stride >= M  and  frame_stride >= n_rows * row_stride,   or
 *     stream-contiguous:  frame_stride >= M  and  row_stride >= n_frames * frame_stride
 * (rnnoise_amd_pcm_layout_fits: 1 / 0) -- else the call returns -1 with nothing launched and nothing changed.  A stream reads and writes
 * the first 480 / L_s samples (a companded one: bytes) of its frame slot and nothing else: not the rest of the slot, not the padding
 * between rows or frames.  vad, gains and active keep their [n_frames][n_rows] shapes; `in` may alias `out`.  Everything else -- out,
 * vad, gains, complete state, histories, gate counters -- is bit for bit what the same frames give in the default layout.
 * The layout applies to every call form: lock-step, masked and list; float and int16; device and host.  Host-buffer calls with a layout
 * take the staged convenience path (strided copies of the frame slots into the default layout in device memory and back); the
 * pinned-ring path of rnnoise_batch_process[_s16] serves the default layout only.
 * A layout is configuration, not state: rnnoise_batch_reset, reset_streams[_device], import_state, load_streams and the model, control,
 * rate and format tables leave it alone, and it does not appear in snapshots.  rnnoise_batch_set_pcm_rate drops it (its strides are in
 * samples of the old M).  rnnoise_batch_train_features* returns -1 while a layout is set.
 * rnnoise_batch_pcm_layout writes the strides in force, the default as (0, 0).  0 / -1; a NULL batch returns -1 without touching the
 * device. */
RNNOISE_EXPORT int rnnoise_batch_set_pcm_layout(RNNoiseBatch *b, long frame_stride, long row_stride);
RNNOISE_EXPORT int rnnoise_batch_pcm_layout(const RNNoiseBatch *b, long *frame_stride, long *row_stride);
RNNOISE_EXPORT int rnnoise_amd_pcm_layout_fits(long frame_stride, long row_stride, int frame_samples, int n_rows, int n_frames);

/* Interleaved multichannel PCM: a channel count for the rows.  With C = channels > 1 the rows of every rnnoise_batch_process* call
 * are taken C at a time: row r = C * g + c is channel c of group g (r: the list position in a list call, the stream index in every
 * other call), and sample i of frame f of row r lies at
 *     f * frame_stride + g * row_stride + i * C + c
 * in `in` and in `out`, in SAMPLES of the call's own type, M = 480 / Lb samples per row and frame (Lb the batch's divisor).  Each
 * channel is a stream of its own -- state, model slot, controls, rate, format, mask bit and list entry are per row as before; only
 * where its samples lie changes.  So stereo LRLR... from a WAV file or a capture device, or a [B][T][C] tensor, is passed where it
 * lies, with no de-interleaving pass before the call and no re-interleaving pass after it.  (One
 * suppression for the channels of a group: rnnoise_batch_set_gain_link, below.)
 * Without a layout row_stride = M * C and frame_stride = (n_rows / C) * M * C: each frame is [n_rows / C][M][C].  With a layout
 * (rnnoise_batch_set_pcm_layout, in either order with this call) the caller's two strides apply and row_stride is the distance between
 * GROUPS: a [G][T][C] tensor is frame_stride = M * C, row_stride = n_frames * M * C.  Stride validity is unchanged (positive multiples
 * of 4 samples: every group slot stays 16 / 8-byte aligned), and the no-overlap rule is rnnoise_amd_pcm_layout_fits with the slot
 * size M * C and n_rows / C groups (rnnoise_amd_pcm_channels_fit: 1 / 0, host only; for channels == 1 it equals
 * rnnoise_amd_pcm_layout_fits; 0 when n_rows % channels != 0) -- a call whose slots overlap returns -1 with nothing launched.
 * A stream below the batch's rate uses the positions i * C + c for i < 480 / L_s only; a companded stream holds one BYTE at byte
 * offset i * C + c of its group slot -- so the channels of one group must all be linear or all be companded (either law, any rates):
 * next to a linear channel's int16 samples those bytes would share positions, and what such a group gives is undefined.
 * Every other position of the slot, and all padding, is neither read nor written: a masked or
 * list call in which a channel of a group is absent leaves that channel's samples in `out` as they were and writes its siblings'.
 * vad, gains and active keep their [n_frames][n_rows] shapes, one entry per row; `in` may alias `out`.  Every stream gives bit for
 * bit -- out, vad, gains, complete state -- what it gives when the same samples are passed planar, in every call form: lock-step,
 * masked and list; float and int16; device and host; with a rate table, a format table, model slots, controls, resets, snapshots.
 * rnnoise_batch_set_pcm_channels returns the previous count; -1 with nothing changed for a NULL batch, channels < 1, channels >
 * RNNOISE_AMD_MAX_CHANNELS or n_streams % channels != 0.  Synchronous, like rnnoise_batch_set_pcm_layout.  channels == 1 drops the
 * feature: the batch then launches exactly what a batch that never saw the call launches.  A list call whose n_rows % C != 0
 * returns -1 with nothing launched.  Host-buffer calls with C > 1 take the staged convenience path (whole group slots copied to
 * device memory and back); the pinned-ring path of rnnoise_batch_process[_s16] serves C == 1 only.
 * A channel count is configuration, not state: rnnoise_batch_reset, reset_streams[_device], import_state, load_streams and every table
 * setter leave it alone, and it is in no snapshot.  rnnoise_batch_set_pcm_rate leaves it alone too (a count does not depend on M;
 * that call still drops the layout).  rnnoise_batch_train_features* returns -1 while C > 1.
 * rnnoise_batch_pcm_channels: the count in force, 1 by default; -1 for a NULL batch, without touching the device. */
#define RNNOISE_AMD_MAX_CHANNELS 8
RNNOISE_EXPORT int rnnoise_batch_set_pcm_channels(RNNoiseBatch *b, int channels);
RNNOISE_EXPORT int rnnoise_batch_pcm_channels(const RNNoiseBatch *b);
RNNOISE_EXPORT int rnnoise_amd_pcm_channels_fit(long frame_stride, long row_stride, int frame_samples, int channels, int n_rows,
                                                int n_frames);

/* Linked gains: one suppression per group of rows (the "link channels" switch of a stereo denoiser).  Each channel is a stream of its
 * own, so by default it gets its own band gains and its own VAD gate: the noise floor of a stereo pair then moves by different
 * amounts left and right and the image wanders.  With a link count K > 1 the rows of every rnnoise_batch_process* call are taken K at a
 * time -- rows K * j .. K * j + K - 1 are a link group; a row is the stream index, or the list position in a list call, as for
 * channels -- and per frame and group:
 *   participants   the rows of the group whose stream has this frame and whose frame is not silent (the reference's E < 0.04
 *                  short-cut).  A masked-out row, a list entry naming no stream and a silent row do not participate.
 *   linked gain    per band b = 0 .. 31 a fold over the participants in ascending row order: m = the first participant's raw network
 *                  gain g[b]; for each further participant's x: m = (x < m) ? x : m.  A NaN never replaces m; a NaN first value stays.
 *   linked VAD     the same fold with (x > m) ? x : m over the participants' VADs; 0 without a participant.
 * A participant uses the linked gain wherever the reference uses the network's gain after its network call: the pitch filter's r[],
 * the decay cap and the lastg update (both stay per row, on the row's own lastg and energies), the floor of the controls and the
 * per-bin interpolation.  What is linked is the network's decision; the release smoothing is not.  Every present row of the group,
 * silent ones included, uses the linked VAD in place of its own in the `voice` decision of the controls (above), with its own thr
 * and hold: rows that share thr and hold open and close together.  A silent row is otherwise processed as ever, an absent row is not
 * touched at all.  The returned vad and gains stay each row's own raw values.
 * K is independent of the channel count of rnnoise_batch_set_pcm_channels (planar callers link too; a stereo file sets both to 2), of
 * rate, format, model slot, controls, layout, masks, lists and per-stream frame phase.  The drop-in API (rnnoise.h) and
 * rnnoise_batch_train_features* ignore it.
 * rnnoise_batch_set_gain_link returns the previous count; -1 with nothing changed for a NULL batch, k < 1, k > RNNOISE_AMD_MAX_CHANNELS
 * or n_streams % k != 0.  Synchronous, like rnnoise_batch_set_pcm_channels.  k == 1 (the default) drops the feature: the batch then
 * launches exactly what a batch that never saw the call launches.  A list call whose n_rows % K != 0 returns -1 with nothing
 * launched.  Host-buffer calls with K > 1 take the staged convenience path; the pinned-ring path of rnnoise_batch_process[_s16] serves
 * K == 1 only.
 * A link count is configuration, not state: no state word is added and nothing goes into snapshots; rnnoise_batch_reset,
 * reset_streams[_device], import_state, load_streams, every table setter, rnnoise_batch_set_pcm_rate and
 * rnnoise_batch_set_pcm_channels leave it alone.
 * rnnoise_batch_gain_link: the count in force, 1 by default; -1 for a NULL batch, without touching the device. */
RNNOISE_EXPORT int rnnoise_batch_set_gain_link(RNNoiseBatch *b, int k);
RNNOISE_EXPORT int rnnoise_batch_gain_link(const RNNoiseBatch *b);

/* Several models in one batch: every stream runs with the model of its SLOT.  Slot 0 is the model the batch was created with;
 * rnnoise_batch_add_model puts another one into the next free slot (1 .. RNNOISE_AMD_MAX_MODELS - 1) and returns that slot: -1 on a
 * NULL batch or model, a full table, or a model that cannot be put on the batch's device.  Synchronous.  The model must outlive the
 * batch.  Every stream stays on slot 0 until told otherwise.
 * models[n_streams] is the slot of every stream.  rnnoise_batch_set_stream_models (host array): synchronous, like
 * rnnoise_batch_reset_streams; -1 and no change if any entry names no slot.  rnnoise_batch_set_stream_models_device (n_streams bytes
 * in the batch's device memory): a stream-ordered copy on hip_stream (no kernel, no host synchronisation); an entry >= the number of
 * slots reads as slot 0.  rnnoise_batch_stream_models reads the map back (synchronous).  0 / -1.
 * A stream's frame runs with the weights of its slot at the time of that frame.  Changing a stream's slot keeps its whole state --
 * DenoiseState, resampler history, frame phase --: its next frame gives what the reference gives when the stream's state is carried
 * into a state initialised with the new model.  rnnoise_batch_reset, reset_streams[_device], import_state, set_pcm_rate, set_nn_path
 * and masked calls leave the map alone; masked calls, every PCM rate, int16 and the host-fed calls work as on a one-model batch.
 * The network runs once per slot in every step (the launch of a slot works on its own streams only): a map that puts whole
 * 64-stream groups on one slot costs little more than one model, an interleaved map about one network per extra slot (DESIGN.md
 * section 4.11).  rnnoise_batch_train_features* runs no network and ignores the map.  The per-frame API of rnnoise.h has one model
 * per state, as before. */
#define RNNOISE_AMD_MAX_MODELS 8
RNNOISE_EXPORT int rnnoise_batch_add_model(RNNoiseBatch *b, RNNModel *model);
RNNOISE_EXPORT int rnnoise_batch_set_stream_models(RNNoiseBatch *b, const unsigned char *models);
RNNOISE_EXPORT int rnnoise_batch_set_stream_models_device(RNNoiseBatch *b, const unsigned char *d_models, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_models(RNNoiseBatch *b, unsigned char *models);

/* Per-stream suppression controls: how hard each stream is suppressed.  ctl[n_streams][RNNOISE_AMD_CTL_FLOATS] = {floor, thr, hold}:
 *   floor  a floor on the band gains, linear in [0, 1] (0: none) -- an attenuation limit of L dB is floor = 10^(-L/20);
 *   thr    a VAD gate threshold in [0, 1] (0: no gate);
 *   hold   frames the gate stays open after the last voice frame, a whole number in [0, 65535].
 * Each stream counts c, the frames since its last voice frame.  On every frame the stream has (an absent frame of a masked call
 * touches nothing), with vad the value the call returns for it (0 on a silent frame): c = (thr == 0 || vad >= thr) ? 0 :
 * min(c + 1, 65536) -- a NaN vad is no voice.  That vad belongs to the frame after the one being synthesised: one frame of look-ahead.
 * Non-silent frames: after the decay cap of the band gains and its memory update (src/denoise.c:479-487, on the raw gains), every
 * band gain below floor is raised to floor (a NaN gain stays NaN); the per-bin gains are interpolated from the result.  When thr > 0
 * and c > hold, the gate is closed: the spectrum to be synthesised is zero (silent frames too), so the frame's output is the previous
 * frame's synthesis tail and the new synthesis tail is zero.  The returned vad and gains stay the raw network values, and of the
 * exported state only synthesis_mem can differ from that of a stream without controls.  All zeros: the reference's bits exactly.
 * A new stream starts with c = 65536 ("no voice yet": a gated stream stays muted until its first voice frame); rnnoise_batch_reset,
 * reset_streams[_device], import_state and a host-fed call that fails (it resets the batch) put it back there.  set_pcm_rate,
 * set_nn_path, set_schedule, the model map and a new table leave it alone.  rnnoise_batch_train_features* ignores the controls.
 * rnnoise_batch_set_stream_controls (host array): synchronous; -1 and no change if any entry is non-finite, out of range, or has a
 * fractional hold.  ctl == NULL drops the table and the counters: the batch then launches exactly what a batch that never had one
 * launches, and the next table set restarts every counter at 65536.
 * rnnoise_batch_set_stream_controls_device (n_streams records in the batch's device memory): a copy ordered on hip_stream (no kernel,
 * no host synchronisation; the first table of a batch allocates its memory).  Entries are not checked: the kernel that reads one maps
 * NaN to 0, clamps each value into its range and truncates hold.
 * rnnoise_batch_stream_controls reads the table back (synchronous; zeros when there is none).  0 / -1.
 * Cost: with a table the synthesis kernel reads 20 more bytes per stream and frame (record, counter, VAD) and writes 4; without
 * one, nothing.
 * The per-frame API of rnnoise.h has no controls. */
#define RNNOISE_AMD_CTL_FLOATS 3
RNNOISE_EXPORT int rnnoise_batch_set_stream_controls(RNNoiseBatch *b, const float *ctl);
RNNOISE_EXPORT int rnnoise_batch_set_stream_controls_device(RNNoiseBatch *b, const float *d_ctl, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_stream_controls(RNNoiseBatch *b, float *ctl);

/* Portable per-stream state: RN_STATE_FLOATS 32-bit words laid out as in rn_layout.h
 * (the 25,128 live bytes of the reference's DenoiseState).  Import requires
 * analysis_mem == the last 480 samples of pitch_buf, which every state produced by the
 * reference or by export satisfies; -1 otherwise.  Import zeroes the stream's resampler history
 * (rnnoise_batch_set_pcm_rate): the portable state carries none.  One stream per call, each call a device drain: to move
 * streams with their history and gate counter, many at a time and ordered on a stream, see rnnoise_batch_save_streams below. */
RNNOISE_EXPORT int rnnoise_batch_export_state(RNNoiseBatch *b, int stream, float *state);
RNNOISE_EXPORT int rnnoise_batch_import_state(RNNoiseBatch *b, int stream, const float *state);

/* Stream snapshots: save and load the COMPLETE state of many streams at once -- to move a call leg to another batch or GPU, to
 * compact or grow a batch, to checkpoint.  A snapshot is RNNOISE_AMD_SNAP_FLOATS 32-bit words (rn_layout.h: RN_SNAP_*): the
 * portable state exactly as rnnoise_batch_export_state writes it (a snapshot's first RN_STATE_FLOATS words can be handed to
 * import_state or the reference unchanged), a header of int32 words -- magic / version, the PCM-rate divisor L = 48000 / rate the
 * history belongs to, the VAD-gate counter (65536 without a control table), the code of the history's down half where the batch has an out-rate
 * table (0 without one: the same L), two reserved zeros -- and the 336 floats of
 * resampler history (zeros at 48 kHz).  It holds state, not configuration: the stream's model slot, its controls record, the
 * batch's rate and network path have their own setters and are set on the destination by the caller; frame phase never appears.
 * snap is [n][RNNOISE_AMD_SNAP_FLOATS], indexed by list position; streams[i] is the batch stream of row i, in any order.
 * streams == NULL with n == n_streams: stream i = row i (the whole batch); a NULL list with any other n > 0 returns -1.
 * save leaves the batch untouched.  load writes every field of the listed streams: what import_state writes, placed at the
 * DESTINATION stream's own frame phase, then the history -- copied when the record's L is the destination stream's current one (the batch's, or the stream's own under a rate table), zeroed otherwise
 * (what import_state does) -- and the counter, clamped to [0, 65536], when the batch has a control table.  analysis_mem is implied
 * by pitch_buf and ignored.  A moved stream continues bit for bit as if it had stayed.  Neither call changes the batch's mode: a
 * lock-step batch stays lock-step, one in per-stream frame phase stays there; model slots, controls, rate, network path and
 * schedule are left alone.
 * Device forms: asynchronous on hip_stream, no host synchronisation and no copy to the host; ordered after every earlier call of the
 * batch on that stream and before every later one, like rnnoise_batch_reset_streams_device.  d_snap (16-byte aligned; -1 otherwise)
 * and d_streams (int32) are in the batch's device memory.  save: an entry outside [0, n_streams) gets an empty record (magic word 0,
 * the row's other words are not written).  load: a row whose magic word is not RN_SNAP_MAGIC or whose entry is out of range touches
 * nothing.  Duplicate entries in a load are the caller's error: those streams are unspecified and no other stream changes; in a save
 * they are harmless.
 * Host forms: synchronous, staged through device memory in bounded chunks.  The list is checked first: an out-of-range entry, and
 * in a load a duplicate entry, a bad magic word or analysis_mem != the last 480 samples of pitch_buf in any record, return -1 with
 * nothing changed.
 * n == 0 is a successful no-op.  A NULL batch, a NULL buffer with n > 0, n < 0 or n > n_streams return -1 without touching the
 * device.  Cost: one launch per call (two for a load while the layer-wise network is in use), moving about 60 KB per stream at a
 * large fraction of the device's copy rate.  0 / -1. */
#define RNNOISE_AMD_SNAP_FLOATS RN_SNAP_FLOATS
RNNOISE_EXPORT int rnnoise_batch_save_streams_device(RNNoiseBatch *b, float *d_snap, const int *d_streams, int n, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_load_streams_device(RNNoiseBatch *b, const float *d_snap, const int *d_streams, int n,
                                                     void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_save_streams(RNNoiseBatch *b, float *snap, const int *streams, int n);
RNNOISE_EXPORT int rnnoise_batch_load_streams(RNNoiseBatch *b, const float *snap, const int *streams, int n);

/* Chunked calls: any number of samples per stream and call.  Audio that does not arrive in 10 ms frames -- AAC blocks of 1024,
 * capture callbacks of 64 .. 2048 samples, 7.5 ms Bluetooth frames, legs whose packet sizes differ inside one batch -- goes through
 * two FIFOs per stream that live on the device, so the caller re-blocks nothing.  M = 480 * rate / 48000, the batch's frame.
 * Every stream s owns an input FIFO of r_s pending samples, 0 <= r_s < M, and an output FIFO of M - r_s samples; after create,
 * rnnoise_batch_reset and every restart below r_s = 0 and the output FIFO holds M zeros.  A chunk call gives stream s
 * counts[s] = n_s new samples, 0 <= n_s <= max_count, and returns exactly n_s output samples.  With x the concatenation of all input
 * ever pushed to the stream and y that of all output ever returned:  y[t] = 0 for t < M, and y[t] = z[t - M] otherwise, where z is what
 * the lock-step call returns for x cut into frames -- bit for bit, float and int16 (the int16 forms: the float call on the exactly
 * converted input, then the truncating cast of the int16 calls).  The constant latency is one frame, the smallest that lets every
 * push return as many samples as it took.  A push completes k_s = (r_s + n_s) / M frames and leaves (r_s + n_s) % M samples pending.
 * Buffers: in / out are [n_streams][max_count], rows max_count samples apart and aligned as their element only (a row of 441 or 1023
 * samples is legal); in may be out.  Stream s reads and writes the first counts[s] samples of its row; the rest of the row is neither
 * read nor written.  vad is [F][n_streams], gains [F][n_streams][32], F = rnnoise_amd_chunk_frames(M, max_count), the most frames a
 * push can complete: rows j < k_s of a stream hold what the lock-step call gives for those frames, bit for bit, rows k_s <= j < F
 * vad 0 and 32 zero gains, as absent frames of a masked call.  frames is [n_streams] and receives k_s.  The three may be NULL.
 * rnnoise_amd_chunk_frames: (frame_samples - 1 + max_count) / frame_samples; 0 for max_count == 0; -1 for frame_samples <= 0 or
 * max_count < 0.  Host only.
 * Device forms: asynchronous on hip_stream, three steps on it -- the caller's rows and the pending samples into whole frames in a
 * staging buffer of the batch, the masked float call on those frames (F frames are launched whatever the counts, which only the
 * device knows), the frames' output and the output FIFO into the caller's rows.  d_counts is int32 in device memory; a negative
 * entry reads as 0, an entry above max_count as max_count.  The FIFOs (3.9 KB per stream) and the staging buffer (F frames of the
 * batch) are allocated at the first chunk call; a later call with a larger F grows the staging buffer, and that one call
 * synchronises with the device.  Host forms: the convenience path -- synchronous, plain copies; a count out of range returns -1 with
 * nothing changed.  max_count == 0 is a successful no-op; max_count < 0, a NULL batch or NULL counts / in / out return -1.
 * Works with every batch rate (rnnoise_batch_set_pcm_rate), float and int16, model slots, stream controls and
 * rnnoise_batch_reset_streams[_device].  Returns -1 with nothing launched while the batch has a rate table, a format table, an out-rate or
 * out-format table, a PCM layout, channels > 1 or a gain link > 1.  The first chunk call switches the batch to per-stream frame phase, as the first masked
 * call does.  rnnoise_batch_reset, rnnoise_batch_reset_streams[_device], rnnoise_batch_import_state and
 * rnnoise_batch_load_streams[_device] restart the FIFOs of the streams they touch, rnnoise_batch_set_pcm_rate those of every stream.
 * Snapshots do not carry FIFO contents (RNNOISE_AMD_SNAP_FLOATS and the record stay): move a stream at a frame boundary --
 * rnnoise_batch_chunk_fill writes r_s of every stream into fill[n_streams], synchronously; at r_s = 0 only the M output samples
 * still in the FIFO are lost with the move --, or take its FIFO record along (rnnoise_batch_save_chunk_fifos below), which moves
 * it anywhere in a frame with nothing lost.  The other call forms on the same batch neither read nor change the
 * FIFOs.  0 / -1. */
RNNOISE_EXPORT int rnnoise_amd_chunk_frames(int frame_samples, int max_count);
RNNOISE_EXPORT int rnnoise_batch_process_device_chunks(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts,
                                                       int max_count, float *d_vad, float *d_gains, int *d_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_device_chunks_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                           int max_count, float *d_vad, float *d_gains, int *d_frames,
                                                           void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_chunks(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count,
                                                float *vad, float *gains, int *frames);
RNNOISE_EXPORT int rnnoise_batch_process_chunks_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts, int max_count,
                                                    float *vad, float *gains, int *frames);
RNNOISE_EXPORT int rnnoise_batch_chunk_fill(RNNoiseBatch *b, int *fill);

/* Chunk calls on a stream list: the chunk call for the n_rows streams streams[i] only, at a cost that follows n_rows -- packets of
 * different legs do not arrive on one clock, and a tick usually carries pushes for a small part of the batch.  Every buffer is
 * indexed by list position i, not by stream: in / out are [n_rows][max_count] (rows max_count samples apart, aligned as their
 * element only; in may be out), counts [n_rows], vad [F][n_rows], gains [F][n_rows][32], frames [n_rows] (the three may be NULL),
 * F = rnnoise_amd_chunk_frames(M, max_count); streams[i] is the batch stream of row i, in any order.
 * A listed stream gets, bit for bit in output samples, vad, gains, frames, state and FIFOs, what the full-size chunk call gives it
 * with the same count and a count of 0 for every unlisted stream.  An unlisted stream is not touched: state, both FIFOs and their
 * fill, resampler history, gate counter and frame phase stay.  The two forms work on the same FIFOs: a stream may be pushed through
 * either form from one call to the next.
 * Device forms: three steps on hip_stream, all sized by n_rows -- the listed rows and their pending samples into a compact staging
 * buffer [F][n_rows][M], the stream-list call (rnnoise_batch_process_device_list) on it with the mask the first step wrote, the
 * frames' output and the output FIFOs into the listed rows.  The staging buffer is the full-size form's; a call that fits what is
 * allocated neither frees nor grows it, one that does not synchronises with the device once.  An entry outside [0, n_streams)
 * makes its row absent: its mask column is zero, frames[i] = 0, its out row is not written and no FIFO is touched.  A negative count
 * reads as 0, one above max_count as max_count.  Duplicate entries are the caller's error: those streams are unspecified, no other
 * stream changes and no access leaves its row or record.
 * Host forms: the list and the counts are checked first; an out-of-range or duplicate entry or a count out of range returns -1 with
 * nothing changed.
 * n_rows == 0 or max_count == 0 is a successful no-op.  n_rows < 0, n_rows > n_streams, a NULL list with n_rows > 0, a NULL batch,
 * in, out or counts, max_count < 0, and every configuration the chunk calls refuse (rate table, format table, PCM layout,
 * channels > 1, gain link > 1) return -1 with nothing launched.  The first call allocates the FIFOs and switches the batch to
 * per-stream frame phase, exactly as the first chunk call does.  0 / -1. */
RNNOISE_EXPORT int rnnoise_batch_process_device_chunks_list(RNNoiseBatch *b, float *d_out, const float *d_in, const int *d_counts,
                                                            int max_count, const int *d_streams, int n_rows, float *d_vad,
                                                            float *d_gains, int *d_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_device_chunks_list_s16(RNNoiseBatch *b, short *d_out, const short *d_in, const int *d_counts,
                                                                int max_count, const int *d_streams, int n_rows, float *d_vad,
                                                                float *d_gains, int *d_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_chunks_list(RNNoiseBatch *b, float *out, const float *in, const int *counts, int max_count,
                                                     const int *streams, int n_rows, float *vad, float *gains, int *frames);
RNNOISE_EXPORT int rnnoise_batch_process_chunks_list_s16(RNNoiseBatch *b, short *out, const short *in, const int *counts,
                                                         int max_count, const int *streams, int n_rows, float *vad, float *gains,
                                                         int *frames);

/* FIFO records: the two sample FIFOs of a stream that is fed in chunks, to move a leg that is not at a frame boundary -- a leg fed by
 * 1024-sample AAC blocks almost never is.  A snapshot (rnnoise_batch_save_streams) carries no FIFO contents; a FIFO record carries
 * nothing else.  rec is [n][RNNOISE_AMD_CHUNK_REC_FLOATS] 32-bit words, by list position: words [0, r) the pending input samples
 * and zeros up to 480; words [480, 480 + M - r) the output FIFO and zeros up to 960; word 960 r, word 961 M (the frame length the
 * record belongs to), word 962 RNNOISE_AMD_CHUNK_MAGIC, word 963 zero, as int32.  Samples move as bits (a NaN payload survives),
 * and saving the same stream twice gives identical bytes.  The list, streams == NULL with n == n_streams, and the NULL / n rules
 * are those of rnnoise_batch_save_streams; no alignment is asked of rec.
 * save leaves the batch untouched; on a batch that has made no chunk call it allocates nothing and writes restarted records (r = 0,
 * M zeros to give out).  load takes a row whose magic word matches, whose word 961 is the batch's current M and whose r is in
 * [0, M), and writes the stream's two FIFOs and their fill -- nothing else: no state, no history, no counter, no frame phase, no
 * mode; on a batch without FIFOs it allocates them as the first chunk call does.
 * Device forms: asynchronous on hip_stream, one launch.  save: an entry outside [0, n_streams) gets magic word 0 and the rest of its
 * row is not written.  load: a row that is not taken and an entry out of range touch nothing; duplicate entries are the caller's
 * error.  Host forms: synchronous; a load checks every row first, and one bad row or a duplicate or out-of-range entry returns -1
 * with nothing changed.
 * ORDER OF A MOVE.  rnnoise_batch_load_streams[_device] restarts the FIFOs of the streams it touches, so the FIFO records go in
 * behind the snapshots: (1) save_streams and save_chunk_fifos on the source, (2) load_streams on the destination,
 * (3) load_chunk_fifos on the destination.  A leg moved that way continues bit for bit as if it had stayed, output samples
 * included.  0 / -1. */
#define RNNOISE_AMD_CHUNK_REC_FLOATS 964
#define RNNOISE_AMD_CHUNK_MAGIC 0x464b4301 /* "\1CKF": record version 1 */
RNNOISE_EXPORT int rnnoise_batch_save_chunk_fifos_device(RNNoiseBatch *b, float *d_rec, const int *d_streams, int n, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_load_chunk_fifos_device(RNNoiseBatch *b, const float *d_rec, const int *d_streams, int n,
                                                         void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_save_chunk_fifos(RNNoiseBatch *b, float *rec, const int *streams, int n);
RNNOISE_EXPORT int rnnoise_batch_load_chunk_fifos(RNNoiseBatch *b, const float *rec, const int *streams, int n);

/* Network implementation: 0 = vector path (v_dot4 / FMA chains), 1 = batched MFMA path -- one kernel per 16-stream tile
 * below 10,240 streams, layer by layer (64 streams per GRU workgroup, five launches) from there up --, 2 = the layer-wise
 * MFMA schedule whatever the batch size (tests, A/B runs).  All produce identical bits and share all state: the path may
 * be switched between calls.  Default: 0 up to 512 streams (there path 0 runs as a latency-oriented kernel, one workgroup per
 * stream, which finishes before a 16-stream MFMA tile does), 1 beyond.
 * Returns the previous value, or -1 if unsupported. */
RNNOISE_EXPORT int rnnoise_batch_set_nn_path(RNNoiseBatch *b, int path);

/* Stream schedule of multi-frame rnnoise_batch_process_device calls: 0 = default (three-stream frame pipeline: high-pass
 * up to two frames ahead, analysis of frame t+1 beside network + synthesis of frame t), 9 = every kernel on the caller's
 * stream (stand-alone kernel timings), 1 = only the high-pass on a side stream.  Same bits in every mode.
 * Returns the previous value, or -1. */
RNNOISE_EXPORT int rnnoise_batch_set_schedule(RNNoiseBatch *b, int schedule);

/* Weight bytes one frame touches (SURVEY 8d "W"): the numerator of the HBM-roofline
 * fraction reported by bench.py. */
RNNOISE_EXPORT long rnnoise_model_weight_bytes(RNNModel *model);

/* GPU-native packed model "RNPK" (SURVEY 8f row f2): the layers already in their device layouts (int8 blocks + column
 * tables, zero-filled MFMA A-fragment order, row sums), behind a header {magic "RNPK", version, architecture dims, W,
 * per-layer offsets}.  rnnoise_model_from_buffer / _file / _filename accept a pack wherever they accept a "DNNw" blob
 * (reference format: src/write_weights.c:46-69); loading one skips the blob walk and the re-layout.
 * Returns the pack size in bytes; writes it only if cap suffices (out == NULL sizes the buffer).  -1 on a bad model.
 * Host-only: no GPU needed.  `python -m rnnoise_amd.blob pack in.blob out.rnpk` is the command-line form. */
RNNOISE_EXPORT long rnnoise_amd_model_pack(RNNModel *model, void *out, long cap);

/* Training-feature extraction (the inner loop of the reference's src/dump_features.c:466-491, a
 * TRAINING=1 build of denoise.c): per frame and stream, Ey from the CLEAN frame, the 65 features
 * from the NOISY frame (no silence short-cut), the 32 band-gain targets and the VAD target passed
 * through: records[n_frames][n_streams][98] = features | gains | vad.  Mixing, filtering and
 * augmentation of the signals are the calls below (RNNoiseTrainMix), whose outputs have the layouts
 * this call takes; a caller with a mixer of their own passes its frames here.  lowpass[n_streams] is the
 * first zeroed FFT bin (481 = none, src/denoise.c:340-343), band_lp[n_streams] the last band with a
 * valid target (32 = all), noise_free[n_streams] = (noise_gain==0 && fgnoise_gain==0).
 * The batch's per-stream analysis state tracks the noisy signal; a batch used for extraction
 * should not be mixed with rnnoise_batch_process calls.  Host-buffer and device-buffer variants. */
RNNOISE_EXPORT int rnnoise_batch_train_features(RNNoiseBatch *b, float *records, const float *clean,
                                                const float *noisy, const float *vad, const int *lowpass,
                                                const int *band_lp, const int *noise_free, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_train_features_device(RNNoiseBatch *b, float *d_records, const float *d_clean,
                                                       const float *d_noisy, const float *d_vad, const int *d_lowpass,
                                                       const int *d_band_lp, const int *d_noise_free, int n_frames,
                                                       void *hip_stream);

/* Training sequences (the caller-side half of the reference's feature dumper, src/dump_features.c:408-465): from three int16
 * corpora on the device -- speech, noise, foreground noise -- to the clean / noisy frames rnnoise_batch_train_features_device
 * takes, one sequence of n_frames frames per stream of the batch (n_seq = the batch size), bit for bit what the reference
 * computes from the same draws in its pinned build (-O2 -ffp-contract=off).  RNNoiseTrainMix holds one sequence's draws
 * (:367-399, :454, :460): the first sample of the sequence in each corpus (in samples; odd values too), the three gains as they
 * stand after :395-396 (before the level normalisation), the six filter coefficient pairs of rand_resp (:397-399) and the two
 * augmentation flags.  Four calls, in this order (or three: the levels call with the VAD in it, then the mix):
 *   rnnoise_amd_train_mix_check        host only: 1 when every position lies in [0, len - 480 * n_frames], every gain and
 *                                      coefficient is finite and the flags are 0 or 1 (n_seq, n_frames >= 1); 0 otherwise.
 *   rnnoise_batch_train_levels_device  d_energy[n_seq][n_frames]: the speech energy per frame (:409-412);
 *                                      d_rms[n_seq][3]: weighted_rms (:283-293) of each signal after its two biquads (:420-431).
 *   rnnoise_amd_train_vad              host only, on the energies copied back: viterbi_vad (:199-254) per row with n_frames for
 *                                      its 2000 frames, then the first start_pos[s] / 480 frames cleared (:437; start_pos NULL:
 *                                      none) -> vad[n_seq][n_frames] bytes.  Its log, pow and sqrt in double are the host libm's,
 *                                      as in the reference.  0 / -1.
 *   rnnoise_batch_train_levels_vad_device  the levels call and, in the same launch, d_vad[n_seq][n_frames] = what
 *                                      rnnoise_amd_train_vad(energy, n_seq, n_frames, start_pos, vad) gives on those energies, byte
 *                                      for byte: no copy to the host, no host work between levels and mix.  start_pos: a host
 *                                      array of n_seq ints, or NULL; it goes up with `mix`, in the same copy.  The device
 *                                      evaluates the host libm's log and pow, restated operation for operation for GNU libc >=
 *                                      2.28 on an x86-64 with FMA, so the call exists only on such a host:
 *   rnnoise_amd_train_vad_device_available  1 when this process's log and pow equal the restated ones on a short sweep (run on
 *                                      first use, cached), 0 when they do not (said once on stderr).  At 0 the device call
 *                                      returns -1 with nothing enqueued, as it does for a NULL d_vad and for everything the
 *                                      levels call refuses; use the levels call and rnnoise_amd_train_vad there.
 *   rnnoise_batch_train_mix_device     the biquads again, clear_vad (:256-281) on the speech with d_vad[n_seq][n_frames] bytes,
 *                                      the level normalisation with d_rms (:440-442), the mix (:443-448), clipping (:457) and
 *                                      quantisation (:463) where the flags say so ->
 *                                      d_clean, d_noisy [n_frames][n_seq][480] (16-byte aligned), d_vad_target [n_frames][n_seq],
 *                                      d_noise_free [n_seq] (noise_gain == 0 && fgnoise_gain == 0 as :477 sees them).
 * RIR filtering (-rir_list, :449-453) is not part of it: it sits between mix and clip, so a caller who wants it passes
 * clip = quantize = 0 here and hands the real flags to rnnoise_batch_train_rir_device (RNNoiseTrainRir, below) -- or filters with a
 * convolution of their own and clips / quantises afterwards.
 * The device calls enqueue on hip_stream; `mix` is a host array of n_seq entries, copied into a buffer the batch owns
 * (allocated on first use) by a copy ordered on hip_stream.  `mix` (and `start_pos`) is read before the call returns and may be freed then: for
 * pageable memory that means the call waits until the stream has reached the copy; the kernel runs asynchronously after it.  A
 * batch has one such buffer: issue its training-mix calls on one stream, or order them yourself.  They run the check first; a failed check, a NULL argument or n_frames < 1 returns -1 with
 * nothing launched.  They read and write no per-stream state, ignore the rate, format, layout, channel, model and control
 * tables, work in lock-step and in per-stream frame phase, and write nothing but the named outputs.  *_len: corpus lengths in
 * samples.  Cost: DESIGN.md section 4.20. */
typedef struct RNNoiseTrainMix {
  long long speech_pos, noise_pos, fgnoise_pos;
  float speech_gain, noise_gain, fgnoise_gain;
  float a_sig[2], b_sig[2], a_noise[2], b_noise[2], a_fgnoise[2], b_fgnoise[2];
  int clip, quantize;
} RNNoiseTrainMix;
RNNOISE_EXPORT int rnnoise_amd_train_mix_check(const RNNoiseTrainMix *mix, int n_seq, long long speech_len, long long noise_len,
                                               long long fgnoise_len, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_train_levels_device(RNNoiseBatch *b, float *d_energy, float *d_rms, const short *d_speech,
                                                     const short *d_noise, const short *d_fgnoise, long long speech_len,
                                                     long long noise_len, long long fgnoise_len, const RNNoiseTrainMix *mix,
                                                     int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_amd_train_vad(const float *energy, int n_seq, int n_frames, const int *start_pos, unsigned char *vad);
RNNOISE_EXPORT int rnnoise_amd_train_vad_device_available(void);
RNNOISE_EXPORT int rnnoise_batch_train_levels_vad_device(RNNoiseBatch *b, float *d_energy, float *d_rms, unsigned char *d_vad,
                                                         const short *d_speech, const short *d_noise, const short *d_fgnoise,
                                                         long long speech_len, long long noise_len, long long fgnoise_len,
                                                         const RNNoiseTrainMix *mix, const int *start_pos, int n_frames,
                                                         void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_train_mix_device(RNNoiseBatch *b, float *d_clean, float *d_noisy, float *d_vad_target,
                                                  int *d_noise_free, const short *d_speech, const short *d_noise,
                                                  const short *d_fgnoise, long long speech_len, long long noise_len,
                                                  long long fgnoise_len, const RNNoiseTrainMix *mix, const float *d_rms,
                                                  const unsigned char *d_vad, int n_frames, void *hip_stream);

/* Room impulse responses for training sequences (the reference's -rir_list option, src/dump_features.c:51-144 and :449-465), between
 * rnnoise_batch_train_mix_device (called with clip = quantize = 0) and rnnoise_batch_train_features_device, bit for bit what the
 * reference computes in its pinned build: overlap-save in blocks of 32,768 samples with its 65,536-point kiss_fft, whose output is
 * HALF the convolution (signal and response are both scaled by 1/65536 going forward, the product by 32768) -- kept.
 *   rnnoise_batch_train_rir_load_device  load_rir (:63-88) for n_rirs responses: d_rir[n_rirs][32768] floats on the device, of
 *                                      which the first lens[r] count (host array, 1 <= len <= 32768) ->
 *                                      d_spectra[n_rirs][2][65536][2] floats: [r][0] the whole response, [r][1] the early one
 *                                      (samples 480..719 faded out, nothing from 720 on).
 *   rnnoise_batch_train_rir_device     per sequence s of the batch (n_seq = the batch size) with rir[s].rir_id >= 0:
 *                                      rir_filter_sequence (:119-144) for any n_frames, on d_clean with the early spectrum and on
 *                                      d_noisy with the whole one, in place, in the [n_frames][n_seq][480] layout; then, for every
 *                                      sequence (rir_id = -1: not filtered), clipping (:457) and quantisation (:463) of d_noisy
 *                                      where rir[s] says so.
 *   rnnoise_amd_train_rir_work_bytes   host only: the bytes of d_work for n_units transform pairs in flight (one unit = one
 *                                      block of one signal of one sequence; 1 MiB each).  The filter call works through its
 *                                      2 * ceil(480 * n_frames / 32768) * (filtered sequences) units in slabs of as many as
 *                                      work_bytes holds; the result does not depend on that number.
 *   rnnoise_amd_train_rir_check        host only: 1 when every rir_id lies in [-1, n_rirs) and the flags are 0 or 1; else 0.
 * `rir` and `lens` are host arrays, read before the call returns (for pageable memory the call waits until hip_stream has reached
 * its table copy, as the training-mix calls do); a batch has one table buffer and one loader scratch, so issue these calls of one
 * batch on one stream.  The twiddles are the host libm's cos and sin, built on the first call and owned by the batch.  -1 with
 * nothing enqueued: a NULL argument, n_frames < 1, n_rirs < 1 or a length outside [1, 32768] (load), a failed check, work_bytes
 * below one unit, a buffer that is not 16-byte aligned.  The calls read and write no per-stream state and ignore every table of the
 * batch.  Cost: DESIGN.md section 4.21. */
typedef struct RNNoiseTrainRir {
  int rir_id, clip, quantize;
} RNNoiseTrainRir;
RNNOISE_EXPORT int rnnoise_amd_train_rir_check(const RNNoiseTrainRir *rir, int n_seq, int n_rirs);
RNNOISE_EXPORT long long rnnoise_amd_train_rir_work_bytes(long long n_units);
RNNOISE_EXPORT int rnnoise_batch_train_rir_load_device(RNNoiseBatch *b, float *d_spectra, const float *d_rir, const int *lens,
                                                       int n_rirs, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_train_rir_device(RNNoiseBatch *b, float *d_clean, float *d_noisy, const float *d_spectra,
                                                  int n_rirs, const RNNoiseTrainRir *rir, void *d_work, long long work_bytes,
                                                  int n_frames, void *hip_stream);

/* Feature calls: the network alone (the reference's compute_rnn, src/rnn.c:44) on features that already exist, and the same walk over
 * training records scored with the reference trainer's loss -- what a blob costs, quantised and sparsified as it ships, on records
 * that may still lie in device memory behind rnnoise_batch_train_features_device.
 *
 * ROWS.  Frame t of stream s lies at  base + t * frame_stride + s * row_stride  (in floats); 0, 0 is [frame][n_streams][row], and
 * any two positive strides whose slots are disjoint do: [frame][n_streams][98] reads the features out of records where they lie,
 * n_streams sequences one after the other -- the file format of dump_features -- are frame_stride = 98, row_stride = T * 98.  No
 * alignment beyond the float's 4 bytes and no multiple of anything is asked of pointers or strides.
 *
 * rnnoise_batch_process_features[_device]: for t = 0 .. n_frames - 1 the 65 features of every stream go through the stream's
 * network state; gains[t][s][32] and vad[t][s] receive what compute_rnn returns (either may be NULL).  Every frame runs the
 * network: the call has no silence decision.
 *
 * rnnoise_batch_eval_records[_device]: rows are records of 98 floats -- 65 features, 32 gain targets, 1 VAD target -- and
 * `records` is the base of the sequences (record 0).  The call runs frames t0 .. t0 + n_frames - 1.  The reference network looks one
 * frame ahead (two `valid` convolutions, torch/rnnoise/rnnoise.py), so the output of step t belongs to the targets of record t - 1:
 * step t is scored against record t - 1 for every t >= max(first, 1) -- first = 4 is the trainer's own cut (train_rnnoise.py:147-148),
 * and step 0 has no record.  A call with t0 > 0 therefore reads record t0 - 1, which must lie there; a file walked in segments
 * gives the sums of one call bit for bit.  sums is [n_streams][RNNOISE_AMD_EVAL_SUMS] doubles, per stream {sum of gain terms, sum of
 * VAD terms, frames scored, 0}; the call ADDS to it, so zero it first.  Per scored frame, in double, with g the record's gain targets,
 * v its VAD target, p the network's gains and q its VAD (train_rnnoise.py:149-155):
 *     tg = max(g, 0);  tg *= tanh(8 tg)^2
 *     gain terms, one per band   (1 + 5 v) * min(g + 1, 1) * (p^gamma - tg^gamma)^2
 *     VAD term                   |2 v - 1| * (-v log(.01 + q) - (1 - v) log(1.01 - q))
 * The trainer's three means over a set of streams are then, with G, V, F the sums of the three columns over the set:
 *     gain_loss = G / (32 F),   vad_loss = V / F,   loss = gain_loss + .001 vad_loss
 * A stream's additions happen in an order that depends on (stream, frame, band) alone: the sums are the same doubles whatever the
 * batch size, the network path and the cut of the frames into calls.  cfg: NULL or a zeroed struct is {gamma .25, first 4}; any
 * other struct is taken as it stands (so gamma = 0 beside first != 0 is refused, and first = 0 beside a gamma scores from step 1).
 * gains / vad as in process_features, over the call's n_frames frames.
 *
 * rnnoise_amd_eval_records_check (host only): 1 when the calls accept the arguments -- a finite gamma > 0 and first >= 0 (or the
 * defaults), t0 >= 0, n_frames >= 0, and the n_streams x (t0 + n_frames) slots of row_floats floats (65 or 98 above) disjoint: rows
 * inside a frame or frames inside a row, as rnnoise_amd_pcm_layout_fits has it with the record as the row.  The calls return -1
 * where it returns 0, and for a NULL batch, rows or sums, with nothing launched.
 *
 * STATE.  The calls advance the network state of every stream -- conv histories, GRU states -- as rnnoise_batch_process does, and
 * nothing else: the DSP state of such a batch (pitch ring, spectra, synthesis memory, frame phase) is NOT advanced, so a batch
 * used for them should not be mixed with PCM calls without a reset between.  rnnoise_batch_reset and rnnoise_batch_reset_streams
 * restart a sequence.  The model map is honoured (one record set under several blobs in one batch: put the same rows on streams of
 * different slots); masks, lists, chunk FIFOs, controls and the PCM tables are not read.  The network path and its forms are those of
 * rnnoise_batch_process_device for a whole batch; rnnoise_batch_kernel_ms counts the network launches under ms[1].  Device forms:
 * asynchronous on hip_stream, n_frames + 1 small launches around the network's.  Host forms: synchronous; everything from the base
 * to the last slot goes up in one copy.  Cost: DESIGN.md section 4.28. */
#define RNNOISE_AMD_EVAL_SUMS 4
typedef struct RNNoiseEvalConfig {
  float gamma; /* perceptual exponent of the gain term; the trainer's default .25 */
  int first;   /* first step that is scored; the trainer's 4 */
} RNNoiseEvalConfig;
RNNOISE_EXPORT int rnnoise_amd_eval_records_check(const RNNoiseEvalConfig *cfg, long frame_stride, long row_stride, int row_floats,
                                                  int n_streams, int t0, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_process_features_device(RNNoiseBatch *b, float *d_gains, float *d_vad, const float *d_features,
                                                         long frame_stride, long row_stride, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_process_features(RNNoiseBatch *b, float *gains, float *vad, const float *features,
                                                  long frame_stride, long row_stride, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_eval_records_device(RNNoiseBatch *b, double *d_sums, float *d_gains, float *d_vad,
                                                     const float *d_records, long frame_stride, long row_stride, int t0,
                                                     int n_frames, const RNNoiseEvalConfig *cfg, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_eval_records(RNNoiseBatch *b, double *sums, float *gains, float *vad, const float *records,
                                              long frame_stride, long row_stride, int t0, int n_frames,
                                              const RNNoiseEvalConfig *cfg);

/* Score calls: the scoring of rnnoise_batch_eval_records with the network taken out -- the trainer's loss on predictions of the
 * caller's, so that a float checkpoint evaluated in torch and the blob exported from it (python -m rnnoise_amd.cli export) are
 * scored by one piece of code, in double, in one order of additions.
 *
 * rnnoise_batch_score_records[_device]: gains / vad hold the predictions of steps t0 .. t0 + n_frames - 1 of n_rows sequences; step t
 * of row s lies at  base + (t - t0) * frame_stride + s * row_stride  (gains: 32 floats, vad: 1).  records is record 0, record t of
 * row s at  records + t * rec_frame_stride + s * rec_row_stride  (98 floats), as in eval_records.  Step t is scored against record
 * t - 1 for every t >= max(first, 1), with the terms of "Feature calls" above; a call with t0 > 0 reads record t0 - 1.  Of a record
 * only its 33 targets are read.  sums[n_rows][RNNOISE_AMD_EVAL_SUMS] is ADDED to, column for column as eval_records adds: scoring the
 * gains / vad that eval_records returned gives the doubles eval_records gave, whatever the cut of the frames into calls.
 * band_sums[n_rows][32], or NULL: band b's gain terms are ADDED to band_sums[s][b] in frame order -- where in the spectrum a blob
 * loses; the doubles do not depend on the cut either.  A pair of strides 0, 0 is [frame][n_rows][row] for that buffer.
 *
 * STATE.  None is read or written: not the network's, not the DSP's, no table, no pending split frame.  The batch only names the
 * device, n_rows is not tied to its size, and the calls work while split frames are pending.
 *
 * rnnoise_amd_score_records_check (host only): 1 when the calls accept the arguments -- cfg as rnnoise_amd_eval_records_check has
 * it, n_rows >= 1, t0 >= 0, n_frames >= 0, and for each of the three buffers strides that keep its slots disjoint (records: n_rows x
 * (t0 + n_frames) slots of 98; gains, vad: n_rows x n_frames slots of 32 and of 1); no alignment beyond the float's.  The calls
 * return -1 where it returns 0, and for a NULL batch, records, gains, vad or sums, with nothing launched.  Device form: asynchronous
 * on hip_stream, ONE launch whatever n_frames is (one wave per row walks its frames in order).  Host form: synchronous; each buffer
 * goes up from its base to its last slot read.  Cost: DESIGN.md section 4.30. */
RNNOISE_EXPORT int rnnoise_amd_score_records_check(const RNNoiseEvalConfig *cfg, long rec_frame_stride, long rec_row_stride,
                                                   long gain_frame_stride, long gain_row_stride, long vad_frame_stride,
                                                   long vad_row_stride, int n_rows, int t0, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_score_records_device(RNNoiseBatch *b, double *d_sums, double *d_band_sums, const float *d_gains,
                                                      long gain_frame_stride, long gain_row_stride, const float *d_vad,
                                                      long vad_frame_stride, long vad_row_stride, const float *d_records,
                                                      long rec_frame_stride, long rec_row_stride, int n_rows, int t0, int n_frames,
                                                      const RNNoiseEvalConfig *cfg, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_score_records(RNNoiseBatch *b, double *sums, double *band_sums, const float *gains,
                                               long gain_frame_stride, long gain_row_stride, const float *vad, long vad_frame_stride,
                                               long vad_row_stride, const float *records, long rec_frame_stride, long rec_row_stride,
                                               int n_rows, int t0, int n_frames, const RNNoiseEvalConfig *cfg);

/* Split calls: the two DSP halves of the frame step as calls of their own, around a network that is the caller's --
 *     rnnoise_batch_analyze  ->  any network: 65 features in, 32 band gains and a VAD out  ->  rnnoise_batch_synthesize
 * so that a float checkpoint, a model of other dimensions or another architecture is heard through the DSP this library restates to
 * the bit: pitch filter, decay cap, interpolation, resampling, the G.711 ends.  With the batch's own network in the middle
 * (rnnoise_batch_process_features on the exported rows) the chain gives the bits of rnnoise_batch_process, on streams without silent
 * frames: the full call skips the network on a silent frame, process_features has no silence decision.
 *
 * ROWS.  RNNoiseRows places the rows of a buffer as the feature calls place theirs: frame t of stream s at
 * base + t * frame_stride + s * row_stride, in floats.  NULL or {0, 0} is [frame][n_streams][row] -- what process_features reads, so
 * analyze's output plugs straight into it; {65, T * 65} is the trainer's batch-first [n_streams][T][65].  Any two positive strides
 * with disjoint rows do, and no alignment beyond the float's is asked.  rnnoise_amd_split_rows_check (host only): 1 when the calls
 * accept the strides for rows of row_floats floats (65 features, 32 gains, 1 vad).
 *
 * rnnoise_batch_analyze[_s16][_device] runs the high-pass and the analysis of n_frames frames of every stream -- the launches of
 * rnnoise_batch_process_device with its plan, the high-pass ahead on a side stream -- and writes exactly 65 floats per stream and
 * frame to `features`, and the frame's silence word (0: not silent) to silence[t][s] (int32, [n_frames][n_streams]; may be NULL).
 * It advances what the analysis side owns (high-pass memory, pitch rings, pitch state, up-resampler history, frame counters) and
 * leaves n_frames frames PENDING in the batch: per stream and frame the X and P spectra, the band energies and the silence word,
 * rnnoise_amd_split_frame_bytes(n_streams) bytes of device memory per frame.  That store is the batch's own:
 * rnnoise_batch_split_reserve makes room for max_frames frames (synchronous); a call that needs more grows it, synchronising once.
 *
 * rnnoise_batch_synthesize[_s16][_device] runs the synthesis of the pending frames -- n_frames must equal
 * rnnoise_batch_split_pending -- with gains (rows of 32 floats) and vad (one float per row) in place of the network's.  Values are
 * taken as they are, NaN included.  On a silent frame (silence word != 0) the caller's rows are NOT read: the frame is synthesised
 * as the full call synthesises a silent frame and its vad reads 0, for the controls' gate and the link fold too.  (Not read by the
 * device: the host forms copy every row of the call up, silent frames' too, so there the rows must be readable memory.)  Afterwards the
 * batch is where rnnoise_batch_process would have left it, and the next call of any kind continues bit for bit.
 *
 * Float and int16 PCM, every batch rate, rate / format / out tables, PCM layout and channels, controls and gain link apply as in
 * rnnoise_batch_process_device[_s16].  The network state, the model slots and the model map are not touched.
 *
 * PENDING FRAMES.  While frames are pending every PCM call (analyze included), chunk call and training call, state export / import,
 * save / load, rnnoise_batch_reset_streams[_device] and every setter return -1 with nothing launched and nothing changed;
 * process_features*, eval_records* and the getters work.  rnnoise_batch_reset drops the pending frames.  Pending frames are in no
 * snapshot.  Both calls return -1 on a batch in per-stream frame phase (after a masked, list or chunk call), for a NULL batch or
 * buffer, for rows that overlap, and synthesize for n_frames != pending.  Device forms: asynchronous on hip_stream, one small
 * launch per frame beside the DSP kernels.  Host forms: synchronous, staged.  Cost: DESIGN.md section 4.29. */
#define RNNOISE_AMD_FEATURES 65
typedef struct RNNoiseRows {
  long frame_stride, row_stride; /* in elements; NULL or {0, 0}: [frame][n_streams][row] */
} RNNoiseRows;
RNNOISE_EXPORT long rnnoise_amd_split_frame_bytes(int n_streams);
RNNOISE_EXPORT int rnnoise_amd_split_rows_check(const RNNoiseRows *r, int row_floats, int n_streams, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_split_reserve(RNNoiseBatch *b, int max_frames);
RNNOISE_EXPORT int rnnoise_batch_split_pending(const RNNoiseBatch *b);
RNNOISE_EXPORT int rnnoise_batch_analyze_device(RNNoiseBatch *b, float *d_features, const RNNoiseRows *feat_rows, int *d_silence,
                                                const float *d_in, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_analyze_device_s16(RNNoiseBatch *b, float *d_features, const RNNoiseRows *feat_rows, int *d_silence,
                                                    const short *d_in, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_analyze(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence,
                                         const float *in, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_analyze_s16(RNNoiseBatch *b, float *features, const RNNoiseRows *feat_rows, int *silence,
                                             const short *in, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_synthesize_device(RNNoiseBatch *b, float *d_out, const float *d_gains, const RNNoiseRows *gain_rows,
                                                   const float *d_vad, const RNNoiseRows *vad_rows, int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_synthesize_device_s16(RNNoiseBatch *b, short *d_out, const float *d_gains,
                                                       const RNNoiseRows *gain_rows, const float *d_vad, const RNNoiseRows *vad_rows,
                                                       int n_frames, void *hip_stream);
RNNOISE_EXPORT int rnnoise_batch_synthesize(RNNoiseBatch *b, float *out, const float *gains, const RNNoiseRows *gain_rows,
                                            const float *vad, const RNNoiseRows *vad_rows, int n_frames);
RNNOISE_EXPORT int rnnoise_batch_synthesize_s16(RNNoiseBatch *b, short *out, const float *gains, const RNNoiseRows *gain_rows,
                                                const float *vad, const RNNoiseRows *vad_rows, int n_frames);

/* Test taps for the last processed frame step: per-stream feature vectors [N][65],
 * silence flags [N] and final pitch periods [N] (host buffers, any may be NULL). */
RNNOISE_EXPORT int rnnoise_batch_debug_last(RNNoiseBatch *b, float *features, int *silence, int *pitch);

/* Average device time per launch of each kernel over the calls since the last query, in
 * milliseconds, measured with HIP events on the launch stream when timing is enabled.
 * ms[0]=analysis (K1), ms[1]=network (K2), ms[2]=synthesis (K3), ms[3]=high-pass + pitch LPC (K0). */
RNNOISE_EXPORT int rnnoise_batch_enable_timing(RNNoiseBatch *b, int on);
RNNOISE_EXPORT int rnnoise_batch_kernel_ms(RNNoiseBatch *b, double ms[4], long *launches);

#ifdef __cplusplus
}
#endif
#endif
