// nn_mfma.hip -- K2, batched MFMA path: the network (src/rnn.c:44-60) recast as
// (16 streams x K) . (K x outputs) matrix products, one workgroup (4 waves) per tile of 16
// streams.
//
//   int8 layers (conv2, 6 GRU matrices): v_mfma_i32_16x16x64_i8 on the block-sparse weights
//     zero-filled to dense and pre-swizzled into A-fragment order (model.cpp: stage_linear), the
//     activations quantised exactly like the x86 path (u8, src/vec_avx.h:326-341) and
//     re-centred to s8 = u8-128; acc_x86 = acc_mfma + 128*rowsum(w).  Integer => exact.
//   float layers (conv1, dense_out): v_mfma_f32_16x16x4_f32, which on gfx950 is bitwise a
//     k-ordered fmaf chain (tools/mfma_probe.hip, cdna_hip_programming.md section 3) = the AVX2
//     sgemv order (src/vec_avx.h:672-730).  vad_dense is the unfused scalar tail
//     (vec_avx.h:732-736) and stays on the VALU, lane = stream.
//
// Fragment maps (verified on hardware by the probe): A lane l -> row l&15, k-group l>>4;
// B lane l -> column (stream) l&15, k-group l>>4; C/D lane l, reg r -> row 4*(l>>4)+r, col l&15.
// Results are bit-identical to the vector path and to the oracle.
#include "nn_common.h"
#include "dispatch.h"
#include <stdlib.h>

#define CHUNK 256      // inputs per staged chunk of the dense_out / vad chains
#define CH_STRIDE 260  // floats per stream and chunk in LDS (16-byte aligned rows, 2-way bank conflicts at most)

struct MfmaLds {
  uint16_t lut[4096];             // rcpps table (rn_dev.h: rcp16)
  float vadw[RN_CAT];             // vad_dense weights: the lane = stream chain of wave 2 must not wait for L2 at every step
  union {
    struct {
      float tmp1[TS][197];          // conv1 input [t-2|t-1|t], padded row
      int8_t xq[2][KT * 64 * 16];   // quantised layer input, B-fragment order (double buffer)
      int8_t hq[KT * 64 * 16];      // quantised recurrent state
    };
    float stage[2][TS][CH_STRIDE];  // dense_out / vad phase: f32 activations, 128 inputs per chunk, double buffer
  };
};

// one int8 output-row tile: 6 MFMAs over K=384, A straight from the pre-swizzled weights
// (B fragments are re-read from LDS per use -- conflict-free 16-byte reads -- rather than held in 48 VGPRs)
__device__ __forceinline__ v4i int8_tile(const int8_t *__restrict__ wmf, int rt, int lane, const int8_t *bq) {
  v4i acc = {0, 0, 0, 0};
  const v4i *a = reinterpret_cast<const v4i *>(wmf) + (size_t)rt * KT * 64 + lane;
  const v4i *b = reinterpret_cast<const v4i *>(bq) + lane;
#pragma unroll
  for (int kt = 0; kt < KT; kt++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[kt * 64], b[kt * 64], acc, 0, 0, 0);
  return acc;
}

// The whole network for one tile.  Large batches run it layer by layer instead (nn_layers.hip): rn_nn_front_kernel below
// (conv1, conv2; leaves the quantised conv2 output as a B-fragment image in act_q[0]), then three launches of the
// 64-stream GRU layer kernel, then the 64-stream dense kernel on the f32 activations the others left in HBM.
// Two workgroups per CU (4 waves per SIMD, <= 128 VGPRs) is what the 47 KB of LDS is sized for; left to itself the
// allocator drifts between 121 and 162 VGPRs with unrelated edits, and above 128 only one workgroup fits.
// "At least 4" costs 8 spilled registers, "exactly 4" 36.  (Forcing <= 64 VGPRs for 4 workgroups per CU is slower: measured.)
extern "C" __global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(4)))
rn_nn_mfma_kernel(RnGroupDev g, RnModelDev m, RnTablesDev tb) {
  __shared__ __attribute__((aligned(16))) MfmaLds L;
#define RN_NN_LIST 1  // (rows through g.list when it is set: nn_tile_body.inc)
#include "nn_tile_body.inc"
#undef RN_NN_LIST
}
// The same with SIXTEEN waves per tile, for one-frame calls on batches in which every tile has a CU to itself (n_tiles <= CUs: up to
// 4,096 streams on MI355X).  The tile is a chain of barrier-separated phases, each as long as its slowest wave: the GRU phases give a
// wave 24 / NWAVES unit tiles (36 MFMAs each, every weight fragment an L2 round trip), conv2 as many row tiles -- 3 with eight waves,
// 2 with sixteen (waves 8..15 one).  1,024 threads = 4 waves per SIMD at the same <= 128 VGPRs: the workgroup takes every register of
// its CU, so inside a pipelined multi-frame call -- where at these sizes the analysis and synthesis waves of the neighbouring frames
// live on the CU's other half -- it is the slower form (4,096 streams: 21.5 against 25.3 M frames/s), and alone the faster one
// (0.0750 -> 0.0686 ms, one frame per call 0.237 -> 0.2305 ms per step; profiles/r6_late_ab.txt).  Same arithmetic per element, same
// bits (tests/test_gpu_parity.py runs both forms at every small size).
#undef NWAVES
#define NWAVES 16
extern "C" __global__ void __launch_bounds__(NTHREADS) rn_nn_mfma16_kernel(RnGroupDev g, RnModelDev m, RnTablesDev tb) {
  __shared__ __attribute__((aligned(16))) MfmaLds L;
#define RN_NN_LIST 1  // (rows through g.list when it is set: nn_tile_body.inc)
#include "nn_tile_body.inc"
#undef RN_NN_LIST
}
#undef NWAVES
#define NWAVES 8
// ---- the front of the layer-wise network: conv1 and conv2 for 64 streams (FM tiles of 16) per workgroup --------------------
// The tile body above fetches every weight fragment for ONE MFMA and copies the rcpps table once per 16 streams: fine for the
// small batches it serves, but at 4,096 tiles per launch the front read ~1 GB of weights and table from L2 to move 0.35 GB of
// HBM data.  Here a workgroup takes four tiles, like the GRU layer kernel (nn_gru.h: int8_gates): the table is copied once,
// and every weight fragment feeds four MFMAs -- one per tile, into four accumulators whose chains are independent and
// interleave in the matrix pipe.  Per accumulator the MFMAs, their operands and their order are the tile body's, and so
// are the activations and the quantiser per element: the same bits (tests/test_front_tiles_gpu.py against the tile kernel).
//
// LDS: the table, and ONE 49 KB arena that is first the f32 conv1 input of the 64 streams and then -- conv1's results wait
// in registers for the barrier behind which nobody reads that input any more -- the four conv2 input images and the four
// output images.  57 KB, static, two workgroups per CU (<= 128 VGPRs).
#define FM 4  // 16-stream tiles per front workgroup (= GM of the layer kernels)
struct FrontLds {
  uint16_t lut[4096];               // rcpps table (rn_dev.h: rcp16)
  union {
    float tmp1[FM * TS][197];       // conv1 input [t-2|t-1|t] per stream, padded row; dead behind the barrier after conv1
    struct {
      int8_t xq[FM][KT * 64 * 16];  // conv2 input images, B-fragment order: [conv2 history (256) | conv1 output (128)]
      int8_t oq[FM][KT * 64 * 16];  // conv2 output images, on their way to act_q[0]
    };
  };
};
static_assert(sizeof(FrontLds) <= 64 * 1024 && 2 * sizeof(FrontLds) <= 160 * 1024, "static LDS; two workgroups per CU");

extern "C" __global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(4)))
rn_nn_front_kernel(RnGroupDev g, RnModelDev m, RnTablesDev tb) {
  __shared__ __attribute__((aligned(16))) FrontLds L;
  static_assert(NWAVES == 8 && NTHREADS == 512, "one conv1 row tile per wave; the trip counts below");
  constexpr int GS = FM * TS;  // streams per workgroup
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, gq = lane >> 4;
  const int N = g.n_streams, s0 = blockIdx.x * GS, n_tiles = (N + TS - 1) / TS;
  // Rows s0 .. s0 + 63.  A row past the batch's end is loaded from the last stream and gets no store; neither does a row of another
  // model slot (rn_dev.h: RnGroupDev::model_of) -- its slot's launch writes it -- and a silent row keeps its conv state
  // (src/denoise.c:474).  Bit r of livem: row r gets state stores.  Lane l forms row l's bit, so every wave holds the same masks
  // and a workgroup without an owned row leaves -- uniformly -- before any barrier.
#define ROW_S(r) ((r) < N ? (r) : N - 1)
  const int sl = ROW_S(s0 + lane);
  const int sil_l = g.silence[sl];  // (sl is clamped: loaded unconditionally, not behind the range test's branch)
  const bool own_l = s0 + lane < N && rn_owns(g, sl);
#define LIVE(r) ((livem >> (r)) & 1ull)
  const uint16_t *lut = L.lut;
#if RN_INSTRUMENT
  float *dbg = (g.debug && tid == 0) ? g.debug + (size_t)s0 * RN_DBG_FLOATS + RN_DBG_CLK2 : nullptr;
#else
  float *const dbg = nullptr;
#endif
  unsigned long long clk_prev = (RN_INSTRUMENT && g.debug) ? __builtin_amdgcn_s_memtime() : 0;
#define CLK_TAP(idx)                                           \
  do {                                                         \
    if (RN_INSTRUMENT && g.debug) {                            \
      unsigned long long now_ = __builtin_amdgcn_s_memtime();  \
      if (dbg) dbg[idx] = (float)(now_ - clk_prev);            \
      clk_prev = now_;                                         \
    }                                                          \
  } while (0)

  // ---- prologue: every global load of the thread is issued before its first dependent store (constant trip counts, fully
  // unrolled: as run-time loops each trip waited out its own HBM round trip) ----
  uint32_t lw[2048 / NTHREADS];
#pragma unroll
  for (int j = 0; j < 2048 / NTHREADS; j++) lw[j] = reinterpret_cast<const uint32_t *>(tb.rcp16)[tid + j * NTHREADS];
  // conv1 input: [conv1_state(130) | features(65) | 0] per stream.  Wave w takes rows w, w + 8, ..., lane l the inputs l, l + 64,
  // l + 128 and -- lanes 0..3 -- l + 192 (195 is the zero pad): a row is wave-uniform, the addresses one base and constants.
  constexpr int HC = GS / NWAVES;  // rows per wave
  float t1v[HC][4];
#pragma unroll
  for (int c = 0; c < HC; c++) {
    const int s = ROW_S(s0 + wave + c * NWAVES);
    const float *cs = g.conv1_state + (size_t)s * 130, *ft = g.features + (size_t)s * 68;
    t1v[c][0] = cs[lane];
    t1v[c][1] = cs[lane + 64];
    t1v[c][2] = *(lane < 2 ? cs + 128 + lane : ft + (lane - 2));
    t1v[c][3] = lane < 3 ? ft[62 + lane] : 0.f;
  }
  constexpr int C1WD = 4;  // conv1 weight groups (of four chain steps) in flight
  const v4f *c1wq = reinterpret_cast<const v4f *>(m.conv1.fwm) + (size_t)wave * 13 * 64 + lane;
  v4f c1w[C1WD];
#pragma unroll
  for (int u = 0; u < C1WD; u++) c1w[u] = c1wq[u * 64];
  // conv2 history: wave w reads the 1 KB rows w, w + 8, ...; lane l holds old[4 l .. 4 l + 3], which is quantised for the input
  // image (k = 0..255) and, for k >= 128, becomes the new history's first half
  v4f hist[HC];
#pragma unroll
  for (int c = 0; c < HC; c++) hist[c] = *reinterpret_cast<const v4f *>(g.conv2_state + (size_t)ROW_S(s0 + wave + c * NWAVES) * 256 + 4 * lane);
  // (the masks only here: formed first, their round trip stood in front of every other load)
  if (!__ballot(own_l)) return;
  const unsigned long long livem = __ballot(own_l && !sil_l);
#pragma unroll
  for (int j = 0; j < 2048 / NTHREADS; j++) reinterpret_cast<uint32_t *>(L.lut)[tid + j * NTHREADS] = lw[j];
#pragma unroll
  for (int c = 0; c < HC; c++) {
    float *row = L.tmp1[wave + c * NWAVES];
    row[lane] = t1v[c][0];
    row[lane + 64] = t1v[c][1];
    row[lane + 128] = t1v[c][2];
    if (lane < 4) row[lane + 192] = t1v[c][3];
  }
  int hq_[HC];  // (the image they belong to lies on tmp1: they wait in registers)
#pragma unroll
  for (int c = 0; c < HC; c++) hq_[c] = pack4(hist[c][0], hist[c][1], hist[c][2], hist[c][3]);
  // the state stores behind the barrier overwrite what other threads load above: every load has landed before anybody passes it
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // state shifts (src/nnet.c:122): conv1 history <- tmp1[65..194]; conv2 history[0..127] <- old[128..255]
#pragma unroll
  for (int c = 0; c < HC; c++) {
    const int q = wave + c * NWAVES;
    if (LIVE(q)) {  // (wave-uniform)
      const float *row = L.tmp1[q] + 65;
      float *cs = g.conv1_state + (size_t)(s0 + q) * 130;
      cs[lane] = row[lane];
      cs[lane + 64] = row[lane + 64];
      if (lane < 2) cs[lane + 128] = row[lane + 128];
    }
  }
#pragma unroll
  for (int c = 0; c < HC; c++)
    if (lane >= 32 && LIVE(wave + c * NWAVES)) *reinterpret_cast<v4f *>(g.conv2_state + (size_t)(s0 + wave + c * NWAVES) * 256 + 4 * lane - 128) = hist[c];

  CLK_TAP(0);  // loads, history quantisation, state shifts
  // ---- conv1: f32 MFMA, 195(+1) -> 128 = 8 row tiles, one per wave, four stream tiles per weight operand ----
  // Weights in MFMA operand order (model.cpp: stage_linear): 16 bytes = this lane's operands of four steps, C1WD groups ahead of
  // their MFMAs.  Accumulator t is the 49-step chain of tile t, step for step the tile body's.
  const int row1 = 16 * wave + 4 * gq;  // this lane's four conv1 outputs
  int c1q[FM];
  // conv2 weight fragments of this wave's row tile i: a whole row tile ahead of their MFMAs (each register is refilled for row tile
  // i + 1 as soon as its MFMAs of row tile i are issued)
  v4i a2[KT];
  const v4i *a2q = reinterpret_cast<const v4i *>(m.conv2.wmf) + (size_t)wave * KT * 64 + lane;
  {
    v4f acc[FM];
#pragma unroll
    for (int t = 0; t < FM; t++) acc[t] = v4f{0, 0, 0, 0};
    const float *bx = &L.tmp1[n][gq];
#pragma unroll
    for (int u = 0; u < 12; u++) {  // steps 0..47
      const v4f a = c1w[u % C1WD];
      if (u + C1WD < 13) c1w[u % C1WD] = c1wq[(u + C1WD) * 64];
      __builtin_amdgcn_sched_barrier(0);  // (else the scheduler sinks the fetch to its use: every weight group an exposed L2 trip)
#pragma unroll
      for (int e = 0; e < 4; e++)
#pragma unroll
        for (int t = 0; t < FM; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bx[t * TS * 197 + 16 * u + 4 * e], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < FM; t++)  // step 48: inputs 192..194 (+ the zero pad)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c1w[12 % C1WD][0], bx[t * TS * 197 + 192], acc[t], 0, 0, 0);
#pragma unroll
    for (int kt = 0; kt < KT; kt++) a2[kt] = a2q[kt * 64];  // (in flight through the activations and the two barriers below)
    const v4f bs = *reinterpret_cast<const v4f *>(m.conv1.bias + row1);
#pragma unroll
    for (int t = 0; t < FM; t++) {
      v4f c1;
#pragma unroll
      for (int r = 0; r < 4; r++) c1[r] = tanh_x86(acc[t][r] + bs[r], lut);
      c1q[t] = pack4(c1[0], c1[1], c1[2], c1[3]);
      if (LIVE(TS * t + n)) *reinterpret_cast<v4f *>(g.conv2_state + (size_t)(s0 + TS * t + n) * 256 + 128 + row1) = c1;
    }
  }
  __syncthreads();  // nobody reads tmp1 any more: the images take its place
#pragma unroll
  for (int c = 0; c < HC; c++) {
    const int q = wave + c * NWAVES;
    *reinterpret_cast<int *>(L.xq[q >> 4] + frag_off(q & 15, 4 * lane)) = hq_[c];
  }
#pragma unroll
  for (int t = 0; t < FM; t++) *reinterpret_cast<int *>(L.xq[t] + frag_off(n, 256 + row1)) = c1q[t];
  __syncthreads();

  CLK_TAP(1);  // conv1
  // ---- conv2: int8 dense 384 -> 384, tanh; wave w owns row tiles w, w + 8, w + 16; one A fragment from L2 feeds four MFMAs ----
#pragma unroll
  for (int i = 0; i < 24 / NWAVES; i++) {
    // (the row constants in front of the next row tile's fragments: vmcnt retires in order)
    const int row0 = 16 * (wave + NWAVES * i) + 4 * gq;
    const v4i rs = *reinterpret_cast<const v4i *>(m.conv2.rowsum128 + row0);
    const v4f sc = *reinterpret_cast<const v4f *>(m.conv2.scale + row0);
    const v4f sb = *reinterpret_cast<const v4f *>(m.conv2.bias + row0);
    __builtin_amdgcn_sched_barrier(0);
    v4i acc[FM];
#pragma unroll
    for (int t = 0; t < FM; t++) acc[t] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int kt = 0; kt < KT; kt++) {
#pragma unroll
      for (int t = 0; t < FM; t++)
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2[kt], reinterpret_cast<const v4i *>(L.xq[t])[kt * 64 + lane], acc[t], 0, 0, 0);
      if (i + 1 < 24 / NWAVES) a2[kt] = a2q[((i + 1) * NWAVES * KT + kt) * 64];
      __builtin_amdgcn_sched_barrier(0);  // (else the scheduler sinks the fetch to its use: every A fragment an exposed L2 trip)
    }
#pragma unroll
    for (int t = 0; t < FM; t++) {
      v4f o;
#pragma unroll
      for (int r = 0; r < 4; r++) o[r] = tanh_x86((float)(acc[t][r] + rs[r]) * sc[r] + sb[r], lut);  // (nn_common.h: int8_finish)
      if (s0 + TS * t + n < N) *reinterpret_cast<v4f *>(g.nn_act + (size_t)(s0 + TS * t + n) * RN_GRU + row0) = o;  // f32 copy for dense_out
      *reinterpret_cast<int *>(L.oq[t] + frag_off(n, row0)) = pack4(o[0], o[1], o[2], o[3]);
    }
  }
  CLK_TAP(2);  // conv2
  __syncthreads();
  {  // hand the images of the tiles that exist to the layer kernels: tile t's at act_q[0] + t * 6144
    constexpr int NI = FM * KT * 64;  // 16-byte pieces
    static_assert(NI % NTHREADS == 0, "whole trips");
    v4i *dst = reinterpret_cast<v4i *>(g.act_q[0] + (size_t)blockIdx.x * (NI * 16));
#pragma unroll
    for (int j = 0; j < NI / NTHREADS; j++) {
      const int i = tid + j * NTHREADS;
      if (blockIdx.x * FM + i / (KT * 64) < n_tiles) dst[i] = reinterpret_cast<const v4i *>(L.oq[0])[i];
    }
  }
#undef CLK_TAP
#undef LIVE
#undef ROW_S
}
// the tile kernel in the form the step's plan chose (dispatch.h: RN_NN_TILE8 | RN_NN_TILE16)
extern "C" hipError_t rn_launch_nn_mfma(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *tb, RnNnForm form, hipStream_t st,
                                        hipEvent_t e0, hipEvent_t e1) {
  if (!m->conv2.wmf || !g->nn_act || !m->dense_out.fwm || !m->conv1.fwm) return hipErrorNotSupported;
  const int n_tiles = (rn_launch_rows(g) + TS - 1) / TS;  // (a list call: tiles of listed rows)
  if (form == RN_NN_TILE16)
    RN_LAUNCH(rn_nn_mfma16_kernel, dim3(n_tiles), dim3(1024), 0, st, e0, e1, *g, *m, *tb);
  else
    RN_LAUNCH(rn_nn_mfma_kernel, dim3(n_tiles), dim3(NTHREADS), 0, st, e0, e1, *g, *m, *tb);
  return hipGetLastError();
}
extern "C" hipError_t rn_launch_nn_gru_layer(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *tb, int layer, RnGruForm form,
                                             const hipError_t lds_opt_in[2], hipStream_t st, hipEvent_t e0, hipEvent_t e1);
extern "C" hipError_t rn_launch_nn_dense(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *tb, hipStream_t st, hipEvent_t e0,
                                         hipEvent_t e1);
// the network layer by layer (front, three GRU layers at 64 streams per workgroup in the form `gru`, dense); lds_opt_in: the batch's
// opt-ins of the two GRU forms (rnnoise_batch_create); ev[i] = the optional (start, stop) events of launch i: each kernel is timed on its
// own, the durations add up to the network's
extern "C" hipError_t rn_launch_nn_layers(const RnGroupDev *g, const RnModelDev *m, const RnTablesDev *tb, RnGruForm gru,
                                          const hipError_t lds_opt_in[2], hipStream_t st, hipEvent_t ev[5][2]) {
  if (!m->conv2.wmf || !g->nn_act || !m->dense_out.fwm || !m->conv1.fwm || !g->act_q[0] || g->n_streams != g->n_stride) return hipErrorNotSupported;
  if ((size_t)g->n_streams * RN_GRU * 4 >= (1ull << 32)) return hipErrorNotSupported;  // 32-bit offsets in nn_layers.hip
  const dim3 grid(((g->n_streams + TS - 1) / TS + FM - 1) / FM);
  RN_LAUNCH(rn_nn_front_kernel, grid, dim3(NTHREADS), 0, st, ev[0][0], ev[0][1], *g, *m, *tb);
  for (int k = 0; k < 3; k++) {
    hipError_t e = rn_launch_nn_gru_layer(g, m, tb, k, gru, lds_opt_in, st, ev[1 + k][0], ev[1 + k][1]);
    if (e != hipSuccess) return e;
  }
  return rn_launch_nn_dense(g, m, tb, st, ev[4][0], ev[4][1]);
}
