// hp_kernel.hip -- K0: the per-stream serial front end (high-pass, pitch-buffer decimation, 5-lag autocorrelation,
// Levinson), transposed to lane = stream.  Compiled WITHOUT the SLP vectoriser since round 5: with it (~9 % fewer
// instructions) the autocorrelation chains became v_pk_mul_f32 / v_pk_add_f32 with op_sel operand selects, and those take the
// wrong operand half in lanes 48..63 whenever a wave issuing v_mfma_i32_16x16x64_i8 shares the SIMD (profiles/r5_gru_race.txt;
// tests/test_kernel_budgets_cpu.py keeps every such instruction out of the library).
// Numerics contract as in dsp_kernels.hip: -ffp-contract=off, reference order of every float sum.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "rn_dev.h"
#include "dispatch.h"
#define RN_RS_CONST static __constant__
#include "rs_coeffs.h"

#define WAVE 64

// ---------------------------------------------------------------------------------------------
// Upsampling of a low-rate stream (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate; rs_coeffs.h, rnnoise_amd/resample.py):
// u[L q + p] = sum_{k<48} hup[p][k] x[q - k], four chains over k mod 4 combined as (a0 + a1) + (a2 + a3).  A prologue of both K0
// kernels: one wave forms one stream's 480 samples at 48 kHz into the stream's row of RnGroupDev::rs_up, from its row staged in LDS
// -- xs[0 .. 46] the history x[-47 .. -1], xs[47 ..] the frame's 480 / L samples -- and the taps staged beside it (hu: [L][48]);
// lane l forms outputs l, l + 64, ...  (rn_hp_one_kernel only: rn_launch_hp.)  L is the batch's, or the stream's own where the batch
// has a rate table (rn_dev.h: rn_stream_L) -- one wave serves one stream, so it stays wave-uniform.  The kernel's 48 kHz float body then reads rs_up as its input: the body is not compiled a
// second time (a second copy of it, even with nothing else changed, took 6 SGPRs more than the kernel's budget), and L is a run-time
// value with four accumulators per lane, so that the prologue fits inside the registers of the body.
// 32 kHz (L = RN_RATE_32K) is 2:3 over the taps of L = 3: u[J] = sum_{k<48} hup3[p][k] x[q - k] with q = floor(2 J / 3), p = 2 J mod 3 --
// the same loop with the index pair formed from 2 n and 3 instead of n and L; frames are 320 samples, the history the same 47.
// ---------------------------------------------------------------------------------------------
#define RN_RS_LDS (RN_RS_XS + RN_RS_TAPS * 6)  // LDS floats of the prologue: the staged row, then the taps
__device__ __forceinline__ const float *rs_up_taps(int L) {
  return L == 2 ? &rn_rs_up2[0][0] : L == 6 ? &rn_rs_up6[0][0] : &rn_rs_up3[0][0];  // (L = 3, and 32 kHz)
}
// the wave's LDS hand-offs (one wave per workgroup: no s_barrier needed)
__device__ __forceinline__ void rs_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// IN: 0 float rows, 1 int16 rows, 2 companded rows (rn_dev.h: RnGroupDev::pcm_fmt) -- G.711 bytes of law `fmt` in the first M bytes
// of the row, which keeps its int16 pitch; each is expanded to the int16 value the linear path would have read (g711.h)
template <int IN>
__device__ __forceinline__ void rs_up_stream(const RnGroupDev &g, const void *in, int s, int row, float *xs, int L, int fmt = 0) {
  // (M: the stream's samples per frame; its row starts at row * rs_pitch -- M of the batch's rate, which a stream of a rate table may
  //  fill only in part: rn_dev.h RnGroupDev::rs_Ls -- or at row * pcm_pitch in a caller-defined layout; with interleaved channels its
  //  samples are pr.step apart from pr.slot + pr.c on: rn_dev.h rn_pcm_row.  Lane l reads samples l, l + 64, ...: one load of the
  //  wave covers 64 * step consecutive elements, every cache line of the group slot once)
  // (P: phases of the up filter, the divisor of the index pair below; n * mul its dividend)
  const int lane = threadIdx.x & (WAVE - 1), M = rn_rate_samples(L), P = L == RN_RATE_32K ? 3 : L, mul = L == RN_RATE_32K ? 2 : 1;
  const RnPcmRow pr = rn_pcm_row(g, row, g.rs_pitch);
  const size_t row0 = pr.slot + pr.c;
  float *hu = xs + RN_RS_XS;
  float *hist = g.rs_hist + (size_t)s * RN_RS_HIST;
  // (loads and LDS stores at clamped indices, without a branch: a lane past the end rewrites the last element with its own value)
  constexpr int NX = (RN_RATE_32K_SAMPLES + WAVE - 1) / WAVE, NT = (RN_RS_TAPS * 6 + WAVE - 1) / WAVE;
  const float rh = hist[min(lane, RN_RS_UP_HIST - 1)];
  float rx[NX], rt[NT];
#pragma unroll
  for (int i = 0; i < NX; i++) {
    const int m = min(lane + WAVE * i, M - 1);
    const size_t q = row0 + (size_t)(m * pr.step);  // (row: the caller's row of stream s, RnStreamAt::i)
    if (IN == 2) rx[i] = (float)rn_g711_decode(fmt, static_cast<const uint8_t *>(in)[pr.slot * sizeof(short) + pr.c + (size_t)(m * pr.step)]);
    else rx[i] = IN == 1 ? (float)static_cast<const short *>(in)[q] : static_cast<const float *>(in)[q];
  }
  const float *ht = rs_up_taps(L);
#pragma unroll
  for (int i = 0; i < NT; i++) rt[i] = ht[min(lane + WAVE * i, RN_RS_TAPS * P - 1)];
  rs_wsync();  // (the previous stream's reads of xs are behind us)
  xs[min(lane, RN_RS_UP_HIST - 1)] = rh;
#pragma unroll
  for (int i = 0; i < NX; i++) xs[RN_RS_UP_HIST + min(lane + WAVE * i, M - 1)] = rx[i];
#pragma unroll
  for (int i = 0; i < NT; i++) hu[min(lane + WAVE * i, RN_RS_TAPS * P - 1)] = rt[i];
  rs_wsync();
  float *dst = g.rs_up + (size_t)s * RN_FRAME_SIZE;
  const unsigned inv = (65536u + P - 1) / P;  // j / P = (j * inv) >> 16, exact for j < 960
  for (int n = lane; n < RN_FRAME_SIZE; n += WAVE) {
    const int j = n * mul, q = (int)(((unsigned)j * inv) >> 16), p = j - q * P;
    const float *xq = xs + RN_RS_UP_HIST + q, *hp = hu + p * RN_RS_TAPS;
    float a0 = hp[0] * xq[0], a1 = hp[1] * xq[-1], a2 = hp[2] * xq[-2], a3 = hp[3] * xq[-3];
#pragma unroll 2
    for (int k = 4; k < RN_RS_TAPS; k += 4) {
      a0 = a0 + hp[k] * xq[-k];
      a1 = a1 + hp[k + 1] * xq[-(k + 1)];
      a2 = a2 + hp[k + 2] * xq[-(k + 2)];
      a3 = a3 + hp[k + 3] * xq[-(k + 3)];
    }
    dst[n] = (a0 + a1) + (a2 + a3);
  }
  // the new up history: the row's last 47 samples (all of the frame's own, M >= 80)
  if (lane < RN_RS_UP_HIST) hist[lane] = xs[M + lane];
}

// ---------------------------------------------------------------------------------------------
// K0: rnn_biquad (src/denoise.c:409-419, coefficients :469-470), transposed: lane = stream.
// The recurrence is strictly serial per stream (every step rounds its state to float), so the
// wave-per-frame kernel would idle 63 of 64 lanes for 480 steps; here 64 streams advance in
// lock-step instead.  Output goes straight into the stream's pitch ring (slot `slot`).
// a0*yi and a1*yi are products of two 24-bit significands, exact in double, so
// fma(-a, yi, b*xi) rounds once exactly like the reference's (b*xi - a*yi).
// ---------------------------------------------------------------------------------------------
#define RN_HP_BLK 8   // float4 per block and stream: 8 = one 128-byte line
// The body is compiled once per (high-pass applied, int16 input): as run-time flags the two were tested inside the block loop, per
// float4, and behind those joins the compiler could no longer count the loads in flight -- it waited with vmcnt(0) in front of every
// block's arithmetic, i.e. for the NEXT block's loads it had just issued: the one-block prefetch hid nothing (round 6, last day).
template <bool HP_ON, bool IN_S16, bool PHASED = false>
__device__ __forceinline__ void hp_body(const RnGroupDev &g, const float *__restrict__ in, int slot, int mode) {
  // mode: bit 0 = apply the high-pass (inference); bit 1 = `in` holds int16 samples, converted as the reference's only caller
  // does (examples/rnnoise_demo.c:56: x[i] = tmp[i], short -> float, exact)
  constexpr bool apply_hp = HP_ON, in_s16 = IN_S16;
  // bits 12-13: streams per wave = 64 >> k (rn_launch_hp passes 0: 64 streams per wave)
  const int spw = WAVE >> ((mode >> 12) & 3);
  // (one wave per workgroup, which is what rn_launch_hp launches; or four whole waves: blockDim.x = 256)
  const int s = blockDim.x > WAVE ? blockIdx.x * blockDim.x + threadIdx.x : blockIdx.x * spw + threadIdx.x;
  if ((blockDim.x == WAVE && (int)threadIdx.x >= spw) || s >= g.n_streams) return;
  if (PHASED) {  // per-stream frame phase (rn_dev.h: RnGroupDev::phase): the lane's own ring slot; an absent stream writes nothing
    bool present;
    slot = rn_stream_phase(g, s, s, present) % RN_RING_SLOTS;
    if (!present) return;
  }
  const float a0 = -1.99599f, a1 = 0.99600f, b0 = -2.f;
  const double na0 = -(double)a0, na1 = -(double)a1, b0d = (double)b0;
  float m0 = g.mem_hp[2 * s], m1 = g.mem_hp[2 * s + 1];
  // (the lane's row of the caller's buffer: one 64-bit product per lane, here, outside the block loop; the pitch is wave-uniform and a
  //  multiple of 4 samples, so the float4 / short4 loads keep their alignment -- rn_dev.h: RnGroupDev::pcm_pitch)
  const size_t row0 = (size_t)s * rn_pcm_pitch(g, RN_FRAME_SIZE);
  const float4 *x = reinterpret_cast<const float4 *>(in + row0);
  float4 *y = reinterpret_cast<float4 *>(g.pitch_ring + (size_t)s * RN_RING_SIZE + slot * RN_FRAME_SIZE);
  // the slot's 240 decimated samples (rn_dev.h: RN_XRING_SLOT) are formed from the filtered frame as it leaves the registers; the
  // first one needs the last sample of the previous slot
  float4 *y2 = reinterpret_cast<float4 *>(g.xlp_ring + (size_t)s * RN_XRING_SIZE + slot * RN_XRING_SLOT);
  const float *ring = g.pitch_ring + (size_t)s * RN_RING_SIZE;
  const float *xring = g.xlp_ring + (size_t)s * RN_XRING_SIZE;
  const int ring0 = RN_RING0(slot), x0 = ring0 / 2;
  float left = ring[(slot * RN_FRAME_SIZE + RN_RING_SIZE - 1) % RN_RING_SIZE];
  // x_lp[0] has no left neighbour (src/pitch.c:166): formed here from pitch_buf[0], pitch_buf[1]
  const float2 pb01 = *reinterpret_cast<const float2 *>(ring + ring0);
  const float xlp0 = .5f * (.5f * (pb01.y) + pb01.x);
  // BLK float4 (32 samples = one 128-byte line per stream at BLK = 8) per block, the next block's loads in flight while this one is
  // consumed: with one wave per SIMD nothing else hides the HBM round trip
  // (per-stream phase: half the blocks in flight.  Its slot-dependent addresses are per lane there, and at eight float4 per block the
  //  kernel's register budget -- four waves per SIMD, which the lock-step forms need -- spilled over)
  constexpr int BLK = PHASED ? RN_HP_BLK / 2 : RN_HP_BLK;  // float4 per block
  float4 cur[BLK], nxt[BLK];
  const short4 *x16 = reinterpret_cast<const short4 *>(reinterpret_cast<const short *>(in) + row0);
  auto load4 = [&](int idx) -> float4 {
    if (in_s16) {
      const short4 q = x16[idx];
      return make_float4((float)q.x, (float)q.y, (float)q.z, (float)q.w);
    }
    return x[idx];
  };

  // ---- the serial half of rnn_pitch_downsample (src/pitch.c:146-214) rides along: 5-lag autocorrelation of the 2x decimated
  // pitch_buf (src/celt_lpc.c:92-174), lag window, order-4 Levinson (src/celt_lpc.c:38-89) -> the 5 FIR taps.  In the wave-per-frame
  // kernel these 5 chains of 864 steps used 5 lanes of 64; here every lane runs them over its own stream, keeping the last 4
  // decimated samples in registers.  For sample t and lag k the product xlp[t-k]*xlp[t] is term i = t-k of the reference's sum for
  // lag k: terms i < 860 go to the main chain (rnn_pitch_xcorr over fastN), later ones to the tail chain `d`.
  // Order of the work (round 6): FIRST the 624 decimated samples that older frames left in the decimated ring (no dependence on
  // this frame: 156 float4 from x0, the ring size a multiple of 4 so that a float4 never straddles the wrap), THEN the frame itself,
  // block by block: biquad -> ring slot -> its 16 decimated samples -> decimated slot AND straight on into the chains.  The new
  // samples are never read back, and the frame's first block is requested while the last old block is consumed.
  float ac[5] = {0, 0, 0, 0, 0};
  float w1 = 0, w2 = 0, w3 = 0, w4 = 0;  // xlp[t-1..t-4]; zeros before the start add exact +0 products
#define AC_MAIN(xv)                      \
  {                                      \
    const float x0_ = (xv);              \
    ac[0] = ac[0] + x0_ * x0_;           \
    ac[1] = ac[1] + w1 * x0_;            \
    ac[2] = ac[2] + w2 * x0_;            \
    ac[3] = ac[3] + w3 * x0_;            \
    ac[4] = ac[4] + w4 * x0_;            \
    w4 = w3; w3 = w2; w2 = w1; w1 = x0_; \
  }
  // t = 860 + e: term i = t-k is < 860 for k > e, else it belongs to the tail
#define AC_TAIL(xv, e)                                                        \
  {                                                                           \
    const float x0_ = (xv);                                                   \
    d[0] = d[0] + x0_ * x0_;                                                  \
    if ((e) >= 1) d[1] = d[1] + x0_ * w1; else ac[1] = ac[1] + w1 * x0_;      \
    if ((e) >= 2) d[2] = d[2] + x0_ * w2; else ac[2] = ac[2] + w2 * x0_;      \
    if ((e) >= 3) d[3] = d[3] + x0_ * w3; else ac[3] = ac[3] + w3 * x0_;      \
    ac[4] = ac[4] + w4 * x0_;                                                 \
    w4 = w3; w3 = w2; w2 = w1; w1 = x0_;                                      \
  }
  constexpr int OLD4 = (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE) / 2 / 4;  // 156 float4 of old decimated samples
  constexpr int OLD_BLOCKS = (OLD4 + BLK - 1) / BLK, NEW_BLOCKS = RN_FRAME_SIZE / 4 / BLK;
  static_assert(RN_FRAME_SIZE / 4 % BLK == 0 && BLK % 2 == 0 && (RN_PITCH_BUF_SIZE / 2 - 860) == 4, "whole frame blocks; the tail terms are the frame's last two float4");
  auto old_block = [&](int b, float4 (&dst)[BLK]) {
#pragma unroll
    for (int j = 0; j < BLK; j++) {
      int p = x0 + 4 * min(BLK * b + j, OLD4 - 1);  // (a partial last block re-reads its last float4 and drops it)
      p = (p >= RN_XRING_SIZE) ? p - RN_XRING_SIZE : p;
      dst[j] = *reinterpret_cast<const float4 *>(xring + p);
    }
  };
  old_block(0, nxt);
  for (int b = 0; b < OLD_BLOCKS; b++) {
#pragma unroll
    for (int j = 0; j < BLK; j++) cur[j] = nxt[j];
    if (b + 1 < OLD_BLOCKS) {
      old_block(b + 1, nxt);
    } else {
#pragma unroll
      for (int j = 0; j < BLK; j++) nxt[j] = load4(j);
    }
#pragma unroll
    for (int j = 0; j < BLK; j++) {
      const int c = b * BLK + j;
      if (OLD4 % BLK == 0 || c < OLD4) {
        const float4 v = cur[j];
        AC_MAIN(c == 0 ? xlp0 : v.x) AC_MAIN(v.y) AC_MAIN(v.z) AC_MAIN(v.w)
      }
    }
  }
  for (int blk = 0; blk < NEW_BLOCKS; blk++) {
#pragma unroll
    for (int j = 0; j < BLK; j++) cur[j] = nxt[j];
    if (blk + 1 < NEW_BLOCKS) {
#pragma unroll
      for (int j = 0; j < BLK; j++) nxt[j] = load4((blk + 1) * BLK + j);
    }
#define HP_STEP(xi, yo)                                              \
    {                                                                \
      const float yi = (xi) + m0;                                    \
      const double xd = (double)(xi), yd = (double)yi;               \
      m0 = (float)((double)m1 + fma(na0, yd, b0d * xd));             \
      m1 = (float)fma(na1, yd, xd);                                  \
      (yo) = yi;                                                     \
    }
    float2 dec[BLK];
#pragma unroll
    for (int j = 0; j < BLK; j++) {
      const float4 v = cur[j];
      float4 o;
      if (apply_hp) {
        HP_STEP(v.x, o.x) HP_STEP(v.y, o.y) HP_STEP(v.z, o.z) HP_STEP(v.w, o.w)
      } else {
        o = v;  // training frames arrive already filtered by the caller's mixer (src/dump_features.c)
      }
      y[blk * BLK + j] = o;
      dec[j].x = .5f * (.5f * (left + o.y) + o.x);  // (src/pitch.c:155-160)
      dec[j].y = .5f * (.5f * (o.y + o.w) + o.z);
      left = o.w;
    }
#undef HP_STEP
#pragma unroll
    for (int j = 0; j < BLK; j += 2) y2[(blk * BLK + j) / 2] = make_float4(dec[j].x, dec[j].y, dec[j + 1].x, dec[j + 1].y);
    if (blk + 1 < NEW_BLOCKS) {
#pragma unroll
      for (int j = 0; j < BLK; j++) { AC_MAIN(dec[j].x) AC_MAIN(dec[j].y) }
    } else {  // the frame's last block ends with decimated samples 860..863
#pragma unroll
      for (int j = 0; j < BLK - 2; j++) { AC_MAIN(dec[j].x) AC_MAIN(dec[j].y) }
      float d[5] = {0, 0, 0, 0, 0};
      AC_TAIL(dec[BLK - 2].x, 0) AC_TAIL(dec[BLK - 2].y, 1) AC_TAIL(dec[BLK - 1].x, 2) AC_TAIL(dec[BLK - 1].y, 3)
#pragma unroll
      for (int k = 0; k < 5; k++) ac[k] = ac[k] + d[k];
    }
  }
#undef AC_MAIN
#undef AC_TAIL
  if (apply_hp) {
    g.mem_hp[2 * s] = m0;
    g.mem_hp[2 * s + 1] = m1;
  }
  {
    float taps[5];
    rn_fir_taps_from_ac(ac, taps);  // (lag window, Levinson, bandwidth expansion: rn_dev.h)
    float *o = g.lpc2 + ((size_t)slot * g.n_stride + s) * 8;  // one copy per ring slot: K0 runs up to 2 frames ahead of K1
#pragma unroll
    for (int k = 0; k < 5; k++) o[k] = taps[k];
    if (RN_INSTRUMENT && g.debug) {
#pragma unroll
      for (int k = 0; k < 5; k++) g.debug[(size_t)s * RN_DBG_FLOATS + RN_DBG_AC + k] = ac[k];
    }
  }
}
// ONE kernel for the four forms.  (Tried: a kernel of its own for int16 input, so that the float forms keep their 101 registers
// instead of the 128 of the hungriest form -- slower, 0.147 against 0.135 ms at 65,536 streams: inside the common kernel the scheduler
// works the float forms to the looser budget too, and that is the faster code.  profiles/r6_hp_specialised.txt)
// (bit 4 of mode: per-stream frame phase, the slot of each lane from RnGroupDev::phase -- it enters only the lane's addresses)
extern "C" __global__ void __launch_bounds__(4 * WAVE) rn_hp_kernel(RnGroupDev g, const float *__restrict__ in, int slot, int mode) {
  if (mode & 16) {
    if (mode & 2) hp_body<true, true, true>(g, in, slot, mode);
    else hp_body<true, false, true>(g, in, slot, mode);
  } else if (mode & 2) {
    if (mode & 1) hp_body<true, true>(g, in, slot, mode);
    else hp_body<false, true>(g, in, slot, mode);
  } else {
    if (mode & 1) hp_body<true, false>(g, in, slot, mode);
    else hp_body<false, false>(g, in, slot, mode);
  }
}
// ---------------------------------------------------------------------------------------------
// K0 for a handful of streams (the one-stream states behind rnnoise_process_frame, and batches of up to 64 streams): the
// same arithmetic with ONE WAVE PER STREAM instead of one lane, arranged for latency.  What is serial stays serial -- the
// biquad recurrence runs once per wave (every lane computes the same values from broadcast LDS reads), each autocorrelation
// lag is one lane's chain in the reference's order -- but the five lags run side by side on lanes 0-4 instead of one after
// the other in a lane, the 2x decimation is spread over the wave, and global memory is touched in coalesced rows only
// (frame and pitch_buf come in through LDS).  43 us -> 22 us for one stream (the biquad chain alone is ~8 us).
// ---------------------------------------------------------------------------------------------
// One array (6.9 KB per wave: 16 waves fit a CU and a 4,096-stream batch is ONE round):
//   pb[0 .. 623]      the 624 decimated samples of pitch_buf that older frames left in the decimated ring (rn_dev.h: RN_XRING_SLOT),
//   pb[624 .. 863]    the frame's own 240, formed once the biquad is through; + zeros up to 935 for the reads of the idle lanes of the
//                     lag chains;
//   pb[1248 .. 1727]  first the UNFILTERED frame, then the filtered one: the biquad runs in place (a block's samples are in registers,
//                     and the next block's too, before its outputs are stored).
// (Rounds 1-5 loaded the 1248 old samples of the pitch ring and decimated all 864 in place: 14 passes instead of 4.)
struct HpOneLds {
  float pb[RN_PITCH_BUF_SIZE];
};
static_assert(864 + 64 + 8 <= RN_PITCH_BUF_SIZE - RN_FRAME_SIZE, "the decimated signal and its pad stay below the new frame");
static_assert(RN_RS_LDS <= RN_PITCH_BUF_SIZE, "the upsampling prologue's LDS fits the body's");

// (the body once per input type, like hp_body above: behind the run-time test per load the frame's two loads and the three loads of
//  old samples were each followed by its own s_waitcnt vmcnt(0) -- five serial round trips, two of them to pinned host memory in the
//  one-frame API, in front of a kernel of ~20 us)
// IN: 0 a float row, 1 an int16 row, 2 a companded row -- 480 G.711 bytes of law `fmt` at the front of the int16 row (rn_dev.h:
// RnGroupDev::pcm_fmt), four codes per lane and load where the int16 row gives four samples, expanded in registers (g711.h)
// CH: interleaved channels (rn_dev.h: RnGroupDev::pcm_chan) -- in_row points at the row's first sample (a companded row's first byte)
// and its samples are `step` elements apart.  Lane l then takes samples l, l + 64, ... one element per load, so that one load of the
// wave covers 64 * step consecutive elements: every cache line of the group slot is requested once by this wave (its other elements are
// the sibling channels', whose waves find the line in L2), where four-sample runs per lane would request each line four times.  A
// body of its own, not a run-time stride in the body above: C = 1 keeps its float4 / short4 loads and its code
template <int IN, bool CH = false>
__device__ __forceinline__ void hp_one_body(HpOneLds &L, const RnGroupDev &g, const void *__restrict__ in_row,
                                            bool listed, int s, int slot, int fmt = 0, int step = 1) {
  constexpr bool in_s16 = IN == 1;
  const int lane = threadIdx.x;
  const float a0 = -1.99599f, a1 = 0.99600f, b0 = -2.f;
  const double na0 = -(double)a0, na1 = -(double)a1, b0d = (double)b0;
  float m0 = g.mem_hp[2 * s], m1 = g.mem_hp[2 * s + 1];
  float *ring = g.pitch_ring + (size_t)s * RN_RING_SIZE;
  const int ring0 = RN_RING0(slot);
  const float *xring = g.xlp_ring + (size_t)s * RN_XRING_SIZE;
  // what the decimated signal needs of the undecimated one: the last sample of the previous slot (left neighbour of the slot's first
  // decimated sample) and pitch_buf[0], pitch_buf[1] (x_lp[0] has no left neighbour: src/pitch.c:166)
  const float left = ring[(slot * RN_FRAME_SIZE + RN_RING_SIZE - 1) % RN_RING_SIZE];
  const float2 pb01 = *reinterpret_cast<const float2 *>(ring + ring0);
  {  // frame -> pb[1248..] (120 float4); the 624 decimated samples older frames left in the decimated ring -> pb[0..623] (156 float4 from
     // ring0 / 2, a multiple of 16; the decimated ring's size is a multiple of 4, so a float4 never straddles the wrap)
    const float4 *x = reinterpret_cast<const float4 *>(in_row);
    const short4 *x16 = reinterpret_cast<const short4 *>(in_row);
    const uint32_t *x8 = reinterpret_cast<const uint32_t *>(in_row);
    constexpr int OLD4 = (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE) / 2 / 4;
    constexpr int NE = (RN_FRAME_SIZE + 63) / 64;
    float4 f[2], o[3];
    float e[NE];
#pragma unroll
    for (int i = 0; CH && i < NE; i++) {
      const size_t q = (size_t)(min(lane + 64 * i, RN_FRAME_SIZE - 1) * step);  // (lanes past the end re-read the last sample)
      if (IN == 2) e[i] = (float)rn_g711_decode(fmt, static_cast<const uint8_t *>(in_row)[q]);
      else if (in_s16) e[i] = (float)static_cast<const short *>(in_row)[q];
      else e[i] = static_cast<const float *>(in_row)[q];
    }
#pragma unroll
    for (int i = 0; !CH && i < 2; i++) {
      const int q = min(lane + 64 * i, RN_FRAME_SIZE / 4 - 1);  // (lanes past the end re-read the last 16 bytes and drop them)
      if (IN == 2) {
        const uint32_t v = x8[q];
        f[i] = make_float4((float)rn_g711_decode(fmt, v & 255), (float)rn_g711_decode(fmt, (v >> 8) & 255),
                           (float)rn_g711_decode(fmt, (v >> 16) & 255), (float)rn_g711_decode(fmt, v >> 24));
      } else if (in_s16) {
        const short4 v = x16[q];
        f[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
      } else {
        f[i] = x[q];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int q = min(lane + 64 * i, OLD4 - 1);
      int p = ring0 / 2 + 4 * q;
      p = (p >= RN_XRING_SIZE) ? p - RN_XRING_SIZE : p;
      o[i] = *reinterpret_cast<const float4 *>(xring + p);
    }
    // (stores at the clamped index too, without a branch: a lane past the end holds the last float4 and rewrites it with its own value.
    //  Behind a branch per store the compiler sank every load to its store and waited for it there: five round trips one after the other)
#pragma unroll
    for (int i = 0; CH && i < NE; i++) L.pb[RN_PITCH_BUF_SIZE - RN_FRAME_SIZE + min(lane + 64 * i, RN_FRAME_SIZE - 1)] = e[i];
#pragma unroll
    for (int i = 0; !CH && i < 2; i++)
      reinterpret_cast<float4 *>(L.pb + (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE))[min(lane + 64 * i, RN_FRAME_SIZE / 4 - 1)] = f[i];
#pragma unroll
    for (int i = 0; i < 3; i++) reinterpret_cast<float4 *>(L.pb)[min(lane + 64 * i, OLD4 - 1)] = o[i];
  }
  __syncthreads();
  // rnn_biquad (src/denoise.c:409-419), once per wave: every lane reads the same samples and computes the same states
  {
    float4 *yo4 = reinterpret_cast<float4 *>(L.pb + (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE));
    const float4 *xi4 = yo4;  // (in place)
    constexpr int BLK = 8;
    float4 cur[BLK], nxt[BLK];
#pragma unroll
    for (int j = 0; j < BLK; j++) nxt[j] = xi4[j];
    for (int blk = 0; blk < RN_FRAME_SIZE / 4 / BLK; blk++) {
#pragma unroll
      for (int j = 0; j < BLK; j++) cur[j] = nxt[j];
      if (blk + 1 < RN_FRAME_SIZE / 4 / BLK) {
#pragma unroll
        for (int j = 0; j < BLK; j++) nxt[j] = xi4[(blk + 1) * BLK + j];
      }
#define HP_STEP(xi, yo)                                              \
      {                                                              \
        const float yi = (xi) + m0;                                  \
        const double xd = (double)(xi), yd = (double)yi;             \
        m0 = (float)((double)m1 + fma(na0, yd, b0d * xd));           \
        m1 = (float)fma(na1, yd, xd);                                \
        (yo) = yi;                                                   \
      }
#pragma unroll
      for (int j = 0; j < BLK; j++) {
        const float4 v = cur[j];
        float4 o;
        HP_STEP(v.x, o.x) HP_STEP(v.y, o.y) HP_STEP(v.z, o.z) HP_STEP(v.w, o.w)
        if (lane == ((blk * BLK + j) & 63)) yo4[blk * BLK + j] = o;  // (one writer per 16 bytes)
      }
#undef HP_STEP
    }
    if (lane == 0) {
      g.mem_hp[2 * s] = m0;
      g.mem_hp[2 * s + 1] = m1;
    }
  }
  __syncthreads();
  {  // the filtered frame -> its ring slot (coalesced); its 240 decimated samples (src/pitch.c:155-160) -> the decimated ring
     // (rn_dev.h: RN_XRING_SLOT), which the analysis kernel reads, and behind the 624 old ones in pb
    float4 *y = reinterpret_cast<float4 *>(ring + slot * RN_FRAME_SIZE);
    const float4 *src = reinterpret_cast<const float4 *>(L.pb + (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE));
#pragma unroll
    for (int i = 0; i < 2; i++)
      if (lane + 64 * i < RN_FRAME_SIZE / 4) y[lane + 64 * i] = src[lane + 64 * i];
    float *y2 = g.xlp_ring + (size_t)s * RN_XRING_SIZE + slot * RN_XRING_SLOT;
    const float *nb = L.pb + (RN_PITCH_BUF_SIZE - RN_FRAME_SIZE);
    float *xlp = L.pb;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int t = lane + 64 * i;
      if (t < RN_XRING_SLOT) {
        const float v = .5f * (.5f * ((t ? nb[2 * t - 1] : left) + nb[2 * t + 1]) + nb[2 * t]);
        y2[t] = v;
        xlp[(RN_PITCH_BUF_SIZE - RN_FRAME_SIZE) / 2 + t] = v;
      }
    }
    // a listed row whose analysis runs as a four-wave workgroup gets its 5 FIR taps there, on a spare wave, beside the
    // transform of X (rn_analysis_rows_kernel): the lags, a third of this kernel's time, are not formed here
    if (listed) return;
    if (lane == 0) xlp[0] = .5f * (.5f * pb01.y + pb01.x);
    if (lane < 8) xlp[864 + lane] = 0;
    xlp[872 + lane] = 0;
  }
  __syncthreads();
  // 5-lag autocorrelation (src/celt_lpc.c:92-174): lane k = lag k, terms in the reference's order; terms i >= 860 form the
  // tail chain d (rnn_pitch_xcorr runs over fastN = 860 terms, the rest is added afterwards)
  float acl = 0, dl = 0;
  {
    const float *xa = L.pb, *xb = L.pb + lane;
#pragma unroll 20
    for (int i = 0; i < 860; i++) acl = acl + xa[i] * xb[i];
#pragma unroll
    for (int i = 860; i < 864; i++)
      if (i + lane <= 863) dl = dl + xb[i] * xa[i];
    acl = acl + dl;
  }
  float ac[5];
#pragma unroll
  for (int k = 0; k < 5; k++) ac[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acl), k));  // (the builtin moves ints)
  float taps[5];
  rn_fir_taps_from_ac(ac, taps);  // (lag window, Levinson, bandwidth expansion: rn_dev.h; the same on every lane)
  if (lane == 0) {
    float *o = g.lpc2 + ((size_t)slot * g.n_stride + s) * 8;
#pragma unroll
    for (int k = 0; k < 5; k++) o[k] = taps[k];
    if (RN_INSTRUMENT && g.debug) {
#pragma unroll
      for (int k = 0; k < 5; k++) g.debug[(size_t)s * RN_DBG_FLOATS + RN_DBG_AC + k] = ac[k];
    }
  }
}
extern "C" __global__ void __launch_bounds__(WAVE)
rn_hp_one_kernel(RnGroupDev g, const float *__restrict__ in, int slot_arg, int in_s16, RnRows rows) {
  __shared__ __attribute__((aligned(16))) HpOneLds L;
  // (rows: the launch groups of the one-frame API, rn_dev.h -- the block's stream, ring slot and frame buffer come from the list)
  const RnStreamAt at = rn_stream_at(g, &rows, slot_arg, 0, 0);
  const int s = at.s;
  if (!at.present) return;  // an absent stream writes nothing
  const float *rs_row = nullptr;
  // a companded stream of an int16 call (rn_dev.h: RnGroupDev::pcm_fmt; never a row list): its row holds bytes
  const int fmt = (in_s16 & 1) ? rn_stream_fmt(g, s) : 0;
  if (in_s16 & 2) {  // low-rate rows (never a row list): upsampled into RnGroupDev::rs_up, staged in the body's LDS before the body uses it
    const int rs_L = rn_stream_L(g, s);  // (the batch's divisor, or the stream's own from the rate table)
    if (rs_L > 1) {
      if (fmt) rs_up_stream<2>(g, in, s, at.i, L.pb, rs_L, fmt);
      else if (in_s16 & 1) rs_up_stream<1>(g, in, s, at.i, L.pb, rs_L);
      else rs_up_stream<0>(g, in, s, at.i, L.pb, rs_L);
      __syncthreads();
      rs_row = g.rs_up + (size_t)s * RN_FRAME_SIZE;
      in_s16 = 0;
    } else {
      in_s16 &= 1;  // a 48 kHz stream of a rate table: its row is a whole frame (rows are 480 apart), read in place below
    }
  }
  // the caller's row i (rn_dev.h: RnStreamAt::i -- stream s's own row except in a list call), RnGroupDev::pcm_pitch samples of the
  // call's type from row i - 1 (a companded row keeps its int16 pitch: its byte base is row * pitch * sizeof(short))
  if (g.pcm_chan && !at.listed && !rs_row) {
    // interleaved channels (rn_dev.h: RnGroupDev::pcm_chan): row i is channel pr.c of its group's slot, its samples pr.step apart
    const RnPcmRow pr = rn_pcm_row(g, at.i, RN_FRAME_SIZE);
    if (in_s16 && fmt)
      hp_one_body<2, true>(L, g, reinterpret_cast<const uint8_t *>(in) + pr.slot * sizeof(short) + pr.c, false, s, at.ring, fmt, pr.step);
    else if (in_s16) hp_one_body<1, true>(L, g, reinterpret_cast<const short *>(in) + pr.slot + pr.c, false, s, at.ring, 0, pr.step);
    else hp_one_body<0, true>(L, g, in + pr.slot + pr.c, false, s, at.ring, 0, pr.step);
    return;
  }
  const size_t row0 = (size_t)at.i * rn_pcm_pitch(g, RN_FRAME_SIZE);
  const void *in_row = at.listed ? static_cast<const void *>(at.io + RN_ROW_IN)
                       : rs_row ? static_cast<const void *>(rs_row)
                       : (in_s16 & 1) ? static_cast<const void *>(reinterpret_cast<const short *>(in) + row0)
                                      : static_cast<const void *>(in + row0);
  if (in_s16 && fmt) hp_one_body<2>(L, g, in_row, at.listed, s, at.ring, fmt);
  else if (in_s16) hp_one_body<1>(L, g, in_row, at.listed, s, at.ring);
  else hp_one_body<0>(L, g, in_row, at.listed, s, at.ring);
}


#define RN_HP_SPW 64  // streams per wave of the lane = stream kernel
// K0 in the form the step's plan chose (dispatch.h: rn_plan)
extern "C" hipError_t rn_launch_hp(const RnGroupDev *g, const void *in, int in_s16, int slot, RnHpForm form, hipStream_t st, hipEvent_t e0,
                                   hipEvent_t done) {
  if (form == RN_HP_ONE_WAVE) {  // (low-rate rows: always this form, dispatch.h)
    RN_LAUNCH(rn_hp_one_kernel, dim3(rn_launch_rows(g)), dim3(WAVE), 0, st, e0, done, *g, static_cast<const float *>(in), slot,
              in_s16 | (g->rs_L ? 2 : 0), RnRows{});
    return hipGetLastError();
  }
  // (rounds 5-6 had a second build of this kernel with 16-sample blocks at 64 VGPRs -- rn_hp_lean_kernel, a wave of which fits a SIMD
  // beside four analysis waves: +0.5 % at 65,536 streams while the autocorrelation pass re-read the whole pitch ring.  Over the decimated
  // ring the 32-sample form is the faster one inside the pipeline too (profiles/r6_xlp_ring.txt), and with the chains fed from the
  // biquad's registers the 64-register budget spills: gone.)
  // one wave of RN_HP_SPW streams per workgroup
  RN_LAUNCH(rn_hp_kernel, dim3((g->n_streams + RN_HP_SPW - 1) / RN_HP_SPW), dim3(WAVE), 0, st, e0, done, *g, static_cast<const float *>(in), slot,
            1 | (in_s16 ? 2 : 0) | (g->phase ? 16 : 0));
  return hipGetLastError();
}
extern "C" hipError_t rn_launch_hp_passthrough(const RnGroupDev *g, const float *in, int slot, hipStream_t st) {
  hipLaunchKernelGGL(rn_hp_kernel, dim3((g->n_streams + WAVE - 1) / WAVE), dim3(WAVE), 0, st, *g, in, slot, 0);
  return hipGetLastError();
}
// K0 of a launch group of the one-frame API (rn_dev.h: RnRows): one wave per listed row, float frames from the pool's pinned blocks
extern "C" hipError_t rn_launch_hp_rows(const RnGroupDev *g, const RnRows *rows, hipStream_t st) {
  hipLaunchKernelGGL(rn_hp_one_kernel, dim3(rows->n), dim3(WAVE), 0, st, *g, static_cast<const float *>(nullptr), 0, 0, *rows);
  return hipGetLastError();
}
