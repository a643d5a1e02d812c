/* rnnoise_amd_fnet.h -- librnnoise_amd_fnet.so: the float network of a trainer checkpoint as a streaming runtime on the device, any
 * cond_size / gru_size the GRU cell takes, served from C.
 *
 * A library of its own beside the product and the other side libraries (it links none of them and none links it): six kernels,
 * rn_fnet_reset_kernel, rn_fnet_gather_kernel, rn_fnet_conv1_kernel, rn_fnet_conv2_kernel, rn_fnet_gru_kernel and
 * rn_fnet_heads_kernel, and the calls below.  It knows no batch: it maps rows of 65 features to rows of 32 gains and one VAD value,
 * placed as rnnoise_amd.h's RNNoiseRows places the rows of rnnoise_batch_analyze and rnnoise_batch_synthesize, so it sits between the
 * two (tools/fnet_serve.c).  rnnoise_amd/fnet.py binds it (FloatNetRuntime).  It reads no environment variable.
 *
 * THE NETWORK is rnnoise_amd/float_net.py's FloatNet in its streaming view (FloatNet.forward), C = cond_size, H = gru_size, x[t] the
 * row's feature frame t counted from its last reset:
 *     c1[t]  = tanh(conv1.bias + sum_{tap, ch} conv1.weight[.][ch][tap] x[t - 2 + tap][ch])        C values, 3 x 65 inputs
 *     c2[t]  = tanh(conv2.bias + sum_{tap, c} conv2.weight[.][c][tap] c1[t - 2 + tap][c])          H values, 3 x C inputs
 *     y_0[t] = GRU(gru1; input c2[t], state y_0[t-1]),  y_1[t] = GRU(gru2; y_0[t], y_1[t-1]),  y_2[t] = GRU(gru3; y_1[t], y_2[t-1])
 *              torch's gate order r, z, n and the formulas of rnnoise_amd_gru_stack.h, the input projection w_ih . input + b_ih included
 *     cat[t] = [c2[t] | y_0[t] | y_1[t] | y_2[t]]                                                   4H values
 *     gains[t] = sigmoid(dense_out.bias + dense_out.weight . cat[t]),  vad[t] = sigmoid(vad_dense.bias + vad_dense.weight . cat[t])
 * Output frame t of a row has seen that row's frames t - 4 .. t.  WARM-UP: for t < 4 (the row's first four frames after a reset)
 * the 32 + 1 outputs are zeros and the row's three GRU states stay zero -- FloatNet.forward does not run its GRUs on those frames --
 * whatever the other rows of the runtime are doing.  The silence word of rnnoise_batch_analyze is not looked at.
 *
 * LIMITS.  cond_size: a multiple of 16 in 16 .. 1024.  gru_size: a multiple of 16 in 16 .. 4096 (the cell's range).  n_rows:
 * 1 .. 1048560.  max_frames: 1 .. 4096 -- the frames a piece of a call holds in the workspace; a call of more frames cuts itself
 * into pieces, and no float depends on the cut.
 *
 * ROWS.  RNNoiseFnetRows places the rows of a buffer: frame t of row s at base + t * frame_stride + s * row_stride, in floats.  NULL
 * or {0, 0} is [frame][n_rows][row] -- what rnnoise_batch_analyze writes and rnnoise_batch_synthesize reads by default; {65, T * 65}
 * is torch's batch-first [n_rows][T][65].  Any two positive strides that keep the rows (65, 32 or 1 floats) disjoint in one of the two
 * orders do; no alignment beyond the float's is asked.
 *
 * THE ORDER OF EVERY SUM.  The floats of a row depend on the row's own features, the weights and the row's frames since its reset,
 * and on nothing else: not on n_rows, the row's position, max_frames, or how the frames are cut into calls.
 *   - conv1, conv2 and the heads: one wave owns 16 outputs x 16 rows of one frame and adds the whole product with the exact float32
 *     matrix instruction (v_mfma_f32_16x16x4_f32: four products per issue, added onto the accumulator in ascending order of the lane
 *     group that feeds them), one accumulator from 0.0; then (sum + bias) and the activation.
 *       conv1: k = 65 tap + ch, K = 195 padded to 196 with a zero weight AND a zero input; issue i adds k = 4 i, 4 i + 1, 4 i + 2, 4 i + 3.
 *       conv2: k = C tap + c, K = 3C;  heads: k over cat, K = 4H.  Both in chunks of 16 k, ascending; issue j = 0 .. 3 of a chunk that
 *       begins at k0 adds k0 + j, k0 + 4 + j, k0 + 8 + j, k0 + 12 + j.
 *   - the GRUs: the cell of the gru libraries, in the form that projects its own input, for all three layers.  A workgroup of four
 *     waves owns 16 units x 16 rows of one layer; a product over k = 0 .. H-1 is cut into the quarters w = 0 .. 3 of H/4 consecutive
 *     k, P^hh_w over y_l[t-1] and P^ih_w over the layer's input;  Q_w = P^hh_w + P^ih_w for r and z,  S_g = ((Q_0 + Q_1) + Q_2) + Q_3,
 *     r = sigmoid(S_r + (b_ih_r + b_hh_r)), z likewise;  hn = S^hh_n + b_hh_n and gi_n = S^ih_n + b_ih_n are sums of their own (each
 *     ((P_0 + P_1) + P_2) + P_3);  n = tanh(gi_n + r hn);  y = (1 - z) n + z y[t-1].
 *   - sigmoid(x) = 1 / (1 + expf(-x)); tanhf.  A row is a column of the matrix instruction's second operand and of its result: what
 *     one row holds, a NaN included, never reaches another row.
 *
 * LAUNCHES.  Plain launches from a loop inside the call; the kernel boundary is the only ordering (no atomics, no workgroup waits
 * for another, no persistent kernel, no graph).  A piece of T <= max_frames frames makes, in this order: one gather launch (the
 * row's last four feature frames and the piece's T into the workspace), one conv1 launch (T + 2 frames: two are recomputed from the
 * history), one conv2 launch, the GRU launches, one heads launch (which also keeps the three states of the piece's last frame).
 * With `seen` the frames every row has had since the last rnnoise_amd_fnet_reset (or the creation) when the piece begins and
 * G = T - min(T, max(0, 4 - seen)) -- the frames of the piece on which some row may be past its warm-up -- the GRUs take G + 2
 * launches, none where G = 0: launch s runs layer l at the piece's frame T - G + s - l, on the diagonal schedule of
 * rnnoise_amd_gru_stack.h.  So a piece makes 4 + (G > 0 ? G + 2 : 0) launches and a call the sum over its ceil(n_frames /
 * max_frames) pieces.  In a GRU launch the workgroup that owns 16 units x 16 rows writes zeros, after the cell's stores, over the
 * rows of its tile that are still warming up at that frame, so their states stay zero beside rows that are running.
 *
 * ORDER OF CALLS.  A runtime holds per-row state; its reset and process calls take effect in the order in which they are issued,
 * which the caller keeps by issuing them on one stream (or by ordering the streams itself).  The host forms wait for their own work.
 *
 * OUT OF SCOPE: saving and loading a runtime's per-row state; masks and lists of rows that skip a frame (every row of a runtime
 * advances in every call); int8; anything backward.
 */
#ifndef RNNOISE_AMD_FNET_H
#define RNNOISE_AMD_FNET_H

#ifndef RNNOISE_EXPORT
#if defined(__GNUC__)
#define RNNOISE_EXPORT __attribute__((visibility("default")))
#else
#define RNNOISE_EXPORT
#endif
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RNNOISE_AMD_FNET_FEATURES 65      /* floats of a feature row */
#define RNNOISE_AMD_FNET_BANDS 32         /* floats of a gain row */
#define RNNOISE_AMD_FNET_LOOKAHEAD 4      /* frames of a row's warm-up after a reset */
#define RNNOISE_AMD_FNET_MIN_COND 16      /* cond_size: a multiple of 16 in this range */
#define RNNOISE_AMD_FNET_MAX_COND 1024
#define RNNOISE_AMD_FNET_MIN_GRU 16       /* gru_size: a multiple of 16 in this range */
#define RNNOISE_AMD_FNET_MAX_GRU 4096
#define RNNOISE_AMD_FNET_MAX_ROWS 1048560 /* 16 * 65535: the row tiles are the grid's second dimension */
#define RNNOISE_AMD_FNET_MAX_FRAMES 4096  /* largest max_frames */

typedef struct RNNoiseFnet RNNoiseFnet;

typedef struct RNNoiseFnetRows {
  long frame_stride, row_stride; /* in floats; NULL or {0, 0}: [frame][n_rows][row] */
} RNNoiseFnetRows;

/* The trainer's state dict, HOST pointers, float32, dense, in torch's own layouts (C = cond_size, H = gru_size). */
typedef struct RNNoiseFnetWeights {
  int cond_size, gru_size;
  const float *conv1_weight, *conv1_bias;         /* [C][65][3], [C] */
  const float *conv2_weight, *conv2_bias;         /* [H][C][3], [H] */
  const float *gru_weight_ih[3], *gru_weight_hh[3]; /* gru1 .. gru3: weight_ih_l0, weight_hh_l0 [3H][H] */
  const float *gru_bias_ih[3], *gru_bias_hh[3];   /* bias_ih_l0, bias_hh_l0 [3H] */
  const float *dense_out_weight, *dense_out_bias; /* [32][4H], [32] */
  const float *vad_dense_weight, *vad_dense_bias; /* [1][4H], [1] */
} RNNoiseFnetWeights;

/* Host only: 0 when rnnoise_amd_fnet_create accepts the arguments, -1 when it refuses them: a NULL w; cond_size not a multiple of
 * 16 or outside 16 .. 1024; gru_size not a multiple of 16 or outside 16 .. 4096; n_rows < 1 or above RNNOISE_AMD_FNET_MAX_ROWS;
 * max_frames < 1 or above RNNOISE_AMD_FNET_MAX_FRAMES; any of the twenty tensor pointers NULL or not 4-byte aligned.  Nothing is
 * dereferenced. */
RNNOISE_EXPORT int rnnoise_amd_fnet_check(const RNNoiseFnetWeights *w, int n_rows, int max_frames);

/* Host only: 1 when the process calls accept the strides for rows of row_floats floats (65 features, 32 gains, 1 vad), 0 when they
 * refuse them: a stride that is negative, or zero beside a non-zero one; rows that overlap in both orders (neither row_stride >=
 * row_floats and frame_stride >= n_rows * row_stride, nor frame_stride >= row_floats and row_stride >= n_frames * frame_stride); a
 * last row beyond LONG_MAX floats; row_floats < 1, n_rows < 1, n_frames < 0.  r NULL or {0, 0} is accepted. */
RNNOISE_EXPORT int rnnoise_amd_fnet_rows_check(const RNNoiseFnetRows *r, int row_floats, int n_rows, int n_frames);

/* Host only: the device bytes a runtime of that shape holds, or -1 outside the limits above.  With C = cond_size, H = gru_size,
 * N = n_rows, M = max_frames:
 *     weights    4 * (196 C + C + 3 C H + H + 18 H H + 18 H + 48 * 4 H + 48)
 *                conv1 (K padded to 196), conv2, three GRUs (w_ih, w_hh, b_ih, b_hh), the 33 head rows padded to 48
 *     state      4 * (65 (M + 4) N + 3 N H) + 8 N
 *                a row's feature frames (the last four are its history), its three GRU states, and the frame of its last reset
 *     workspace  4 * ((M + 2) N C + 4 M N H + 12 N H + N)
 *                conv1's frames, cat of the piece's frames, the cell's gate scratch, a row list
 * The host form of the process call stages through device memory of its own for the time of the call, which is not counted. */
RNNOISE_EXPORT long long rnnoise_amd_fnet_bytes(int cond_size, int gru_size, int n_rows, int max_frames);

/* A runtime of n_rows rows on HIP device `device`: uploads (and repacks) the weights, every row at the start of a sequence.
 * Synchronous; the weights are not referenced afterwards.  NULL where the check refuses, where the device cannot be selected and
 * where the device memory cannot be had. */
RNNOISE_EXPORT RNNoiseFnet *rnnoise_amd_fnet_create(int device, const RNNoiseFnetWeights *w, int n_rows, int max_frames);
/* Waits for the device, then frees everything.  NULL is allowed. */
RNNOISE_EXPORT void rnnoise_amd_fnet_destroy(RNNoiseFnet *f);

/* Every row starts a new sequence: zero history, zero states, a frame count of 0.  Asynchronous on hip_stream (a hipStream_t, NULL:
 * the default stream), one launch.  -1 for a NULL runtime or a failed launch. */
RNNOISE_EXPORT int rnnoise_amd_fnet_reset(RNNoiseFnet *f, void *hip_stream);

/* Only the n listed rows start a new sequence; every other row is untouched.  d_rows: n ints in device memory, 0 <= n <= n_rows; an
 * entry outside 0 .. n_rows - 1 is skipped, a row may be listed twice.  Asynchronous on hip_stream, one launch (none for n = 0).
 * -1, with nothing launched, for a NULL runtime, a NULL list with n > 0, and n outside 0 .. n_rows. */
RNNOISE_EXPORT int rnnoise_amd_fnet_reset_rows_device(RNNoiseFnet *f, const int *d_rows, int n, void *hip_stream);
/* The same for a list in host memory: synchronous, on the default stream. */
RNNOISE_EXPORT int rnnoise_amd_fnet_reset_rows(RNNoiseFnet *f, const int *rows, int n);

/* n_frames frames of every row: reads d_features, WRITES d_gains (rows of 32) and d_vad (rows of 1); every pointer is memory of the
 * runtime's device.  Asynchronous on hip_stream; the launches are LAUNCHES above.  n_frames may exceed max_frames.  0 for
 * n_frames = 0, with nothing launched, read or written.  -1, with nothing launched, for a NULL runtime or buffer, a buffer that is not
 * 4-byte aligned, n_frames < 0, and strides rnnoise_amd_fnet_rows_check refuses; -1 where a launch fails. */
RNNOISE_EXPORT int rnnoise_amd_fnet_process_device(RNNoiseFnet *f, float *d_gains, const RNNoiseFnetRows *gain_rows, float *d_vad,
                                                   const RNNoiseFnetRows *vad_rows, const float *d_features,
                                                   const RNNoiseFnetRows *feat_rows, int n_frames, void *hip_stream);
/* Host form: every buffer is host memory; synchronous, on the default stream, staged through the device in pieces of max_frames
 * frames.  The floats are the device form's. */
RNNOISE_EXPORT int rnnoise_amd_fnet_process(RNNoiseFnet *f, float *gains, const RNNoiseFnetRows *gain_rows, float *vad,
                                            const RNNoiseFnetRows *vad_rows, const float *features, const RNNoiseFnetRows *feat_rows,
                                            int n_frames);

#ifdef __cplusplus
}
#endif
#endif
