// train_mix.hip -- the mixing stage of training-data generation (include/rnnoise_amd.h: RNNoiseTrainMix; the reference's
// src/dump_features.c:408-465 without the RIR): rnnoise_amd_train_mix_check, rnnoise_batch_train_levels_device,
// rnnoise_amd_train_vad, rnnoise_batch_train_levels_vad_device, rnnoise_batch_train_mix_device and their two kernels.  DESIGN.md
// sections 4.20 and 4.22.
//
// Every signal of a sequence is a strictly serial recurrence over 480 * n_frames samples (two biquads with double intermediates,
// src/denoise.c:409-419; a third one in the levels pass), so a lane owns one (sequence, signal) chain: a workgroup is three waves,
// wave k runs signal k (speech, noise, foreground noise) of 64 neighbouring sequences.  Each lane reads its corpus row 32 samples at
// a time as aligned 32-bit words, one chunk ahead of the chunk it computes (the rows are only 2-byte aligned: the words are
// funnel-shifted by the row's phase, and the row's first and last sample are read on their own where a word would reach across the
// row's end).  The mix kernel hands each chunk through LDS to all 192 threads, which add the three signals and store runs of 32
// floats per sequence as float4.
//
// tests/csrc/hip_emul compiles THIS FILE as host C++ against a stand-in for shim.h (tests/test_train_mix_cpu.py, under the address
// sanitizer): a HIP call, a builtin or a member of RNNoiseBatch that this file starts to use needs its counterpart there.
#include "train_common.h"
#include "rn_train_vad.h"  // (include/: the Viterbi VAD as device code, the epilogue of rn_train_levels)

#include <limits.h>
#include <atomic>

namespace {
constexpr int CH = 32;                              // samples per chunk: 480 = 15 * 32, a chunk never straddles a frame
constexpr int FRAME_CHUNKS = RN_FRAME_SIZE / CH;
constexpr int SEQS = 64;                            // sequences per workgroup: the lanes of a wave
constexpr int THREADS = 3 * SEQS;                   // wave k = signal k
constexpr int LDS_ROW = CH + 1;                     // a lane's chunk in LDS, padded: the lanes' writes fall into distinct banks
static_assert(RN_FRAME_SIZE % CH == 0, "a chunk must not straddle a frame");

struct TrainMixArgs {
  const RNNoiseTrainMix *mix;  // [n_seq] (the batch's device copy)
  const int16_t *corpus[3];
  int n_seq, n_frames;
  // levels
  float *energy, *rms_out;
  uint8_t *vad_out;      // [n_seq][n_frames], or null: no VAD epilogue
  const int *start_pos;  // [n_seq] behind the table in the batch's buffer (with vad_out)
  // mix
  float *clean, *noisy, *vad_target;
  int *noise_free;
  const float *rms;
  const uint8_t *vad;
};

// rnn_biquad (src/denoise.c:409-419), one sample: the products and sums in double, mem[] rounded to float
struct Biquad {
  float b0, b1, a0, a1, m0 = 0.f, m1 = 0.f;
  __device__ Biquad(float b0_, float b1_, float a0_, float a1_) : b0(b0_), b1(b1_), a0(a0_), a1(a1_) {}
  __device__ __forceinline__ float step(float xi) {
    const float yi = xi + m0;
    m0 = (float)((double)m1 + ((double)b0 * (double)xi - (double)a0 * (double)yi));
    m1 = (float)((double)b1 * (double)xi - (double)a1 * (double)yi);
    return yi;
  }
};

// 32 samples of a row as 17 words of the aligned word stream that starts at row - o (o = 1: the row is not 4-byte aligned, sample i
// is half i + 1 of the stream): chunk c is words 16c .. 16c + 16, the last one only with o = 1.  No byte outside the row is read.
struct Chunk {
  uint32_t w[17];
};
__device__ __forceinline__ void load_chunk(Chunk &k, const int16_t *row, int o, long long c, long long n_chunks) {
  const uint32_t *a = reinterpret_cast<const uint32_t *>(row - o) + c * (CH / 2);
#pragma unroll
  for (int j = 1; j < CH / 2; j++) k.w[j] = a[j];
  if (o) {
    k.w[0] = c == 0 ? (uint32_t)(uint16_t)row[0] << 16 : a[0];
    k.w[CH / 2] = c == n_chunks - 1 ? (uint32_t)(uint16_t)row[c * CH + CH - 1] : a[CH / 2];
  } else {
    k.w[0] = a[0];
    k.w[CH / 2] = 0;
  }
}

struct MixLds {
  float sig[2][3][SEQS * LDS_ROW];  // [chunk parity][signal][lane][sample]
  float ratio[RN_FRAME_SIZE];       // j / 480.f, the fades of clear_vad (src/dump_features.c:263, :271)
  int flags[SEQS];                  // clip | quantize << 1
};

// MIX = false: the levels pass -- per-frame speech energy (:409-412) and weighted_rms (:283-293) of each filtered signal.
// MIX = true: biquads, clear_vad, gains, mix, clip, quantise (:420-465).
template <bool MIX>
__device__ __forceinline__ void train_mix_body(const TrainMixArgs &a, MixLds *lds) {
  const int sig = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // (a wave's signal: uniform)
  const int seq0 = blockIdx.x * SEQS;
  const bool live = seq0 + lane < a.n_seq;
  const int seq = live ? seq0 + lane : a.n_seq - 1;  // lanes behind the last sequence repeat it and store nothing
  const RNNoiseTrainMix &p = a.mix[seq];
  const long long pos = sig == 0 ? p.speech_pos : sig == 1 ? p.noise_pos : p.fgnoise_pos;
  const float *fa = sig == 0 ? p.a_sig : sig == 1 ? p.a_noise : p.a_fgnoise;
  const float *fb = sig == 0 ? p.b_sig : sig == 1 ? p.b_noise : p.b_fgnoise;
  const int16_t *row = a.corpus[sig] + pos;
  const int o = (int)((reinterpret_cast<uintptr_t>(row) >> 1) & 1);
  const unsigned sh = 16u * o;
  const long long n_chunks = (long long)a.n_frames * FRAME_CHUNKS;

  Biquad hp(-2.f, 1.f, -1.99599f, 0.99600f);  // b_hp, a_hp (:298-299)
  Biquad flt(fb[0], fb[1], fa[0], fa[1]);
  Biquad wgt(-2.f, 1.f, -1.89f, .895f);       // weighting_b, weighting_a (:286-287)
  float mse = 1e-15f, E = 0.f;

  // mix only
  float g = 0.f;
  int act = 0, active = 0;                 // clear_vad: 0 keep, 1 zero, 2 fade in, 3 fade out
  unsigned v_prev = 0, v_cur = 0, v_next = 0, v_ahead = 0;
  const uint8_t *vad = nullptr;
  if constexpr (MIX) {
    for (int j = threadIdx.x; j < RN_FRAME_SIZE; j += THREADS) lds->ratio[j] = (float)j / (float)RN_FRAME_SIZE;
    if (threadIdx.x < SEQS) {
      const RNNoiseTrainMix &q = a.mix[min(seq0 + (int)threadIdx.x, a.n_seq - 1)];
      lds->flags[threadIdx.x] = (q.clip ? 1 : 0) | (q.quantize ? 2 : 0);
    }
    const float gain = sig == 0 ? p.speech_gain : sig == 1 ? p.noise_gain : p.fgnoise_gain;
    g = gain * (3000.f / (1.f + a.rms[(size_t)seq * 3 + sig]));  // (:440-442)
    if (sig == 0) {
      vad = a.vad + (size_t)seq * a.n_frames;
      v_cur = vad[0];
      v_next = a.n_frames > 1 ? vad[1] : 0;
      active = v_cur != 0;
      if (live) {
        const float gn = p.noise_gain * (3000.f / (1.f + a.rms[(size_t)seq * 3 + 1]));
        const float gf = p.fgnoise_gain * (3000.f / (1.f + a.rms[(size_t)seq * 3 + 2]));
        a.noise_free[seq] = gn == 0 && gf == 0;  // (:477, on the gains as they stand there)
      }
    }
    __syncthreads();
  }

  Chunk cur, nxt;
  load_chunk(cur, row, o, 0, n_chunks);
  int fc = 0, frame = 0;  // chunk of the frame, frame of the sequence
  for (long long c = 0; c < n_chunks; c++) {
    if (c + 1 < n_chunks) load_chunk(nxt, row, o, c + 1, n_chunks);
    if constexpr (MIX) {
      if (sig == 0 && fc == 0) {  // clear_vad (:256-275) for this frame
        v_ahead = frame + 2 < a.n_frames ? vad[frame + 2] : 0;
        if (!active) {
          if (v_next) {  // (v_next is 0 behind the last frame)
            act = 2;
            active = 1;
          } else {
            act = 1;
          }
        } else if (frame >= 1 && v_cur == 0 && v_prev == 0) {
          act = 3;
          active = 0;
        } else {
          act = 0;
        }
        if (live) a.vad_target[(size_t)frame * a.n_seq + seq] = (float)v_cur;
      }
    }
    float *out = nullptr;
    if constexpr (MIX) out = &lds->sig[c & 1][sig][lane * LDS_ROW];
#pragma unroll
    for (int j = 0; j < CH / 2; j++) {
      const uint32_t v = __builtin_amdgcn_alignbit(cur.w[j + 1], cur.w[j], sh);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float x = (float)(int16_t)(h ? v >> 16 : v & 0xffffu);
        if constexpr (!MIX) E += x * x;  // (every wave: the speech wave's is the one stored)
        float y = flt.step(hp.step(x));
        if constexpr (MIX) {
          // clear_vad: the noise waves stay at act = 0, whose factor 1.f changes no bit -- no branch inside the chain
          const float r = lds->ratio[fc * CH + 2 * j + h];
          const float m = act == 2 ? r : act == 3 ? 1.f - r : 1.f;
          y = act == 1 ? 0.f : y * m;
          out[2 * j + h] = y * g;
        } else {
          const float t = wgt.step(y);
          mse += t * t;
        }
      }
    }
    if constexpr (MIX) {
      __syncthreads();  // (two chunk buffers: the readers of chunk c are done before anybody passes the barrier of chunk c + 1)
      const size_t frame_base = (size_t)frame * a.n_seq + seq0;
      for (int q = threadIdx.x; q < SEQS * (CH / 4); q += THREADS) {
        const int s = q / (CH / 4), j4 = (q % (CH / 4)) * 4;
        if (seq0 + s >= a.n_seq) continue;
        const float *xs = &lds->sig[c & 1][0][s * LDS_ROW + j4], *ns = &lds->sig[c & 1][1][s * LDS_ROW + j4],
                    *fs = &lds->sig[c & 1][2][s * LDS_ROW + j4];
        const int fl = lds->flags[s];
        float cl[4], xn[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          cl[k] = xs[k];
          xn[k] = clip_quantize((xs[k] + ns[k]) + fs[k], fl & 1, fl & 2);   // (:447, :457, :463)
        }
        const size_t at = (frame_base + s) * RN_FRAME_SIZE + fc * CH + j4;
        *reinterpret_cast<float4 *>(a.clean + at) = make_float4(cl[0], cl[1], cl[2], cl[3]);
        *reinterpret_cast<float4 *>(a.noisy + at) = make_float4(xn[0], xn[1], xn[2], xn[3]);
      }
    }
    if (++fc == FRAME_CHUNKS) {
      fc = 0;
      if constexpr (!MIX) {
        if (sig == 0) {
          if (live) a.energy[(size_t)seq * a.n_frames + frame] = E;
          E = 0.f;
        }
      } else {
        v_prev = v_cur;
        v_cur = v_next;
        v_next = v_ahead;
      }
      frame++;
    }
#pragma unroll
    for (int j = 0; j <= CH / 2; j++) cur.w[j] = nxt.w[j];
  }
  if constexpr (!MIX) {
    // weighted_rms (:291-292): the mean in float, the root and the product with 0.9506 in double, rounded once
    if (live) a.rms_out[(size_t)seq * 3 + sig] = (float)(0.9506 * sqrt((double)(mse / (float)(RN_FRAME_SIZE * a.n_frames))));
    // The Viterbi VAD of the row of energies this lane has just written (include/rn_train_vad.h): the speech wave only, and
    // only for the call that asks for it -- both tests are uniform in the wave.
    if (a.vad_out && sig == 0 && live) {
      const int sp = a.start_pos[seq];
      const int lead = sp > 0 ? min(sp / RN_FRAME_SIZE, a.n_frames) : 0;
      rn_vad_row(a.energy + (size_t)seq * a.n_frames, a.n_frames, a.vad_out + (size_t)seq * a.n_frames, lead);
    }
  }
}

}  // namespace

// (tests/test_product_surface_cpu.py and tests/test_kernel_budgets_cpu.py pin the kernels of this file by name)
extern "C" __global__ __launch_bounds__(THREADS) void rn_train_levels(TrainMixArgs a) { train_mix_body<false>(a, nullptr); }

extern "C" __global__ __launch_bounds__(THREADS) void rn_train_mix(TrainMixArgs a) {
  __shared__ MixLds lds;
  train_mix_body<true>(a, &lds);
}

// ---- host ----
extern "C" int rnnoise_amd_train_mix_check(const RNNoiseTrainMix *mix, int n_seq, long long speech_len, long long noise_len,
                                           long long fgnoise_len, int n_frames) {
  if (!mix || n_seq < 1 || n_frames < 1 || n_frames > INT_MAX / RN_FRAME_SIZE) return 0;
  const long long span = (long long)RN_FRAME_SIZE * n_frames;
  for (int s = 0; s < n_seq; s++) {
    const RNNoiseTrainMix &p = mix[s];
    if (p.speech_pos < 0 || p.speech_pos > speech_len - span || p.noise_pos < 0 || p.noise_pos > noise_len - span || p.fgnoise_pos < 0 ||
        p.fgnoise_pos > fgnoise_len - span)
      return 0;
    const float f[] = {p.speech_gain, p.noise_gain, p.fgnoise_gain, p.a_sig[0], p.a_sig[1], p.b_sig[0], p.b_sig[1], p.a_noise[0],
                       p.a_noise[1], p.b_noise[0], p.b_noise[1], p.a_fgnoise[0], p.a_fgnoise[1], p.b_fgnoise[0], p.b_fgnoise[1]};
    for (float v : f)
      if (!isfinite(v)) return 0;
    if (!train_flag01(p.clip) || !train_flag01(p.quantize)) return 0;
  }
  return 1;
}

// ---- the Viterbi VAD of the speech energies (what src/dump_features.c:199-254 computes, for any number of frames) ----
// A two-state hidden Markov model over the frames, state 1 = speech: transitions keep their state with probability 0.99, the
// observation is the frame's log energy placed between a noise level and a speech level of the whole sequence, and the decoded
// path is widened by one frame on both sides.  The arithmetic is the reference's to the bit: every quantity it holds in a float is
// rounded to float here, every sub-expression it evaluates in double (a double constant or a libm call takes part) is evaluated in
// double -- spelled with casts, because C++ would pick the float overloads of sqrt and log where C promotes.
namespace {
constexpr float kStay = 0.99f, kSwitch = 0.01f;

struct VadLevels {
  float speech, noise;  // RMS of the frame energies; harmonic-mean-like level that the quiet frames dominate
};

VadLevels vad_levels(const float *energy, int n) {
  float sq = 1e-30, inv = 1e-30;
  for (int f = 0; f < n; f++) sq += energy[f] * energy[f];
  const float speech = sqrt((double)(sq / n));
  for (int f = 0; f < n; f++) inv += 1.f / (1e-8 * speech * speech + energy[f] * energy[f]);
  const float noise = 1.f / sqrt((double)(inv / n));
  return {speech, noise};
}

// probability that a frame of this energy is speech, from its energy alone: the position of its log energy between the two
// levels, limited to [.1, .9] (a NaN passes both limits), then flattened by a square root of the odds
float vad_observation(float energy, const VadLevels &lv) {
  volatile double odds_power = 0.5f;  // (volatile: pow() stays the libm call it is in the reference, whatever the compiler knows about 0.5)
  const double log_noise = log((double)lv.noise);
  float where = (log(1e-15 + energy) - log_noise) / (.01 + log((double)lv.speech) - log_noise);
  where = .1f > where ? .1f : where;
  where = .9f < where ? .9f : where;
  return 1.f / (1.f + pow((double)((1.f - where) / where), odds_power));
}

// one row: n frame energies -> n bytes; `from` is scratch for 2 * n predecessor states
void vad_decode(const float *energy, int n, unsigned char *vad, unsigned char *from) {
  const VadLevels lv = vad_levels(energy, n);
  float belief = 0.5;  // posterior of "speech" after the frames so far
  for (int f = 0; f < n; f++) {
    const float obs = vad_observation(energy[f], lv);
    const float quiet = 1 - belief;
    // the likelier way into each state (a tie goes to the state that is not kept), and its weight
    const bool speech_stays = belief * kStay > quiet * kSwitch, noise_stays = quiet * kStay > belief * kSwitch;
    from[2 * f + 1] = speech_stays ? 1 : 0;
    from[2 * f] = noise_stays ? 0 : 1;
    const float into_speech = (speech_stays ? belief * kStay : quiet * kSwitch) * obs;
    const float into_noise = (noise_stays ? quiet * kStay : belief * kSwitch) * (1 - obs);
    belief = into_speech / (into_speech + into_noise);
  }
  // back along the stored predecessors from the last frame's decision
  unsigned char state = belief > .5;
  for (int f = n - 1; f >= 0; f--) {
    vad[f] = state;
    state = from[2 * f + state];
  }
  // hangover: a frame next to a speech frame is speech -- first backwards in time, then forwards, each pass seeing its own results
  for (int f = 0; f + 1 < n; f++) vad[f] |= vad[f + 1];
  for (int f = n - 1; f > 0; f--) vad[f] |= vad[f - 1];
}
}  // namespace

extern "C" int rnnoise_amd_train_vad(const float *energy, int n_seq, int n_frames, const int *start_pos, unsigned char *vad) {
  if (!energy || !vad || n_seq < 1 || n_frames < 1) return -1;
  std::vector<unsigned char> from((size_t)2 * n_frames);
  for (int s = 0; s < n_seq; s++) {
    unsigned char *row = vad + (size_t)s * n_frames;
    vad_decode(energy + (size_t)s * n_frames, n_frames, row, from.data());
    // no speech target before the sequence's start position (:437): its first start_pos / 480 frames
    const int lead = start_pos && start_pos[s] > 0 ? std::min(start_pos[s] / RN_FRAME_SIZE, n_frames) : 0;
    memset(row, 0, lead);
  }
  return 0;
}

// ---- the device form of the VAD: rn_train_levels' epilogue evaluates the host libm's log() and pow() (pow_glibc.h) ----
// It is offered only where that is true of THIS process's libm: a short sweep of the restated functions against the running ones
// over the VAD's arguments, on first use, cached -- like the log10 model of the feature stage (tables.cpp), except that there is no
// second-best form to fall back to: a VAD with other arithmetic would make a record file depend on where it was written.
namespace {
std::atomic<int> g_vad_selfcheck{-1};  // -1: not run yet; 0: differs; 1: equal
#if RN_INSTRUMENT
std::atomic<int> g_vad_selfcheck_forced{-1};  // (rnnoise_amd_debug_train_vad_selfcheck: tests)
#endif

bool host_libm_is_the_restated_one() {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&s] {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  volatile double half = 0.5;  // (volatile: the libm calls are made, not folded)
  uint32_t w_lo, w_hi;
  const float lo = .1f, hi = .9f;
  memcpy(&w_lo, &lo, 4);
  memcpy(&w_hi, &hi, 4);
  for (int it = 0; it < 100000; it++) {
    const uint64_t r = rnd();
    uint32_t u = w_lo + (uint32_t)(r % (w_hi - w_lo + 1)), e = (uint32_t)((r >> 32) % 0x7f800000u);  // w of [.1f, .9f]; any energy
    float w, en;
    memcpy(&w, &u, 4);
    memcpy(&en, &e, 4);
    const volatile double x = (double)((1.f - w) / w), l = 1e-15 + (double)en;
    const double want_p = pow(x, half), got_p = rn_vad_pow_half(x), want_l = log(l), got_l = rn_vad_log(l);
    if (memcmp(&want_p, &got_p, 8) || memcmp(&want_l, &got_l, 8)) return false;
  }
  const volatile double zero = 0.0, one = 1.0;
  return log(zero) == rn_vad_log(zero) && pow(one, half) == rn_vad_pow_half(one);
}
}  // namespace

extern "C" int rnnoise_amd_train_vad_device_available(void) {
#if RN_INSTRUMENT
  if (g_vad_selfcheck_forced.load() >= 0) return g_vad_selfcheck_forced.load();
#endif
  int v = g_vad_selfcheck.load();
  if (v < 0) {
    v = host_libm_is_the_restated_one() ? 1 : 0;
    int expected = -1;
    if (g_vad_selfcheck.compare_exchange_strong(expected, v) && !v)  // (said once)
      fprintf(stderr, "[rnnoise_amd] this host's log and pow are not GNU libc >= 2.28 with FMA; the Viterbi VAD of training-data "
                      "generation stays on the host (rnnoise_amd_train_vad), rnnoise_batch_train_levels_vad_device refuses\n");
  }
  return v;
}
#if RN_INSTRUMENT
// include/rnnoise_amd_debug.h: 0 or 1 makes the self-check's answer, -1 gives it back to the sweep
extern "C" void rnnoise_amd_debug_train_vad_selfcheck(int forced) {
  g_vad_selfcheck_forced.store(forced < 0 ? -1 : forced != 0);
}
#endif

namespace {
// What both device calls do once their pointers are checked and their outputs are in `a`: the table checked and in the batch's
// buffer (train_common.h), the arguments both kernels read, the launch.
// The batch's buffer holds the table and, behind it, room for one int per sequence: the start positions of the call with the VAD
// (`with_start`: start_pos or, for null, zeros), which go up with the table in one copy.
int mix_launch(void (*kernel)(TrainMixArgs), TrainMixArgs a, RNNoiseBatch *b, const short *d_speech, const short *d_noise,
               const short *d_fgnoise, long long speech_len, long long noise_len, long long fgnoise_len, const RNNoiseTrainMix *mix,
               int n_frames, void *hip_stream, bool with_start = false, const int *start_pos = nullptr) {
  if (!rnnoise_amd_train_mix_check(mix, b->n, speech_len, noise_len, fgnoise_len, n_frames)) return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ON_DEVICE(b->device);
  const size_t bytes = (size_t)b->n * sizeof(RNNoiseTrainMix), capacity = bytes + (size_t)b->n * sizeof(int);
  if (with_start) {
    std::vector<unsigned char> both(capacity, 0);
    memcpy(both.data(), mix, bytes);
    if (start_pos) memcpy(both.data() + bytes, start_pos, capacity - bytes);
    if (train_upload(&b->train_mix_buf, capacity, both.data(), capacity, st)) return -1;
    a.start_pos = reinterpret_cast<const int *>(static_cast<const unsigned char *>(b->train_mix_buf) + bytes);
  } else if (train_upload(&b->train_mix_buf, capacity, mix, bytes, st)) {
    return -1;
  }
  a.mix = static_cast<const RNNoiseTrainMix *>(b->train_mix_buf);
  a.corpus[0] = d_speech;
  a.corpus[1] = d_noise;
  a.corpus[2] = d_fgnoise;
  a.n_seq = b->n;
  a.n_frames = n_frames;
  hipLaunchKernelGGL(kernel, dim3((b->n + SEQS - 1) / SEQS), dim3(THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int rnnoise_batch_train_levels_device(RNNoiseBatch *b, float *d_energy, float *d_rms, const short *d_speech,
                                                 const short *d_noise, const short *d_fgnoise, long long speech_len, long long noise_len,
                                                 long long fgnoise_len, const RNNoiseTrainMix *mix, int n_frames, void *hip_stream) {
  if (!b || !d_energy || !d_rms || !d_speech || !d_noise || !d_fgnoise || !mix || n_frames < 1) return -1;
  if (train_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  TrainMixArgs a{};
  a.energy = d_energy;
  a.rms_out = d_rms;
  return mix_launch(rn_train_levels, a, b, d_speech, d_noise, d_fgnoise, speech_len, noise_len, fgnoise_len, mix, n_frames, hip_stream);
}

extern "C" int rnnoise_batch_train_levels_vad_device(RNNoiseBatch *b, float *d_energy, float *d_rms, unsigned char *d_vad,
                                                     const short *d_speech, const short *d_noise, const short *d_fgnoise,
                                                     long long speech_len, long long noise_len, long long fgnoise_len,
                                                     const RNNoiseTrainMix *mix, const int *start_pos, int n_frames, void *hip_stream) {
  if (!b || !d_energy || !d_rms || !d_vad || !d_speech || !d_noise || !d_fgnoise || !mix || n_frames < 1) return -1;
  if (train_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!rnnoise_amd_train_vad_device_available()) return -1;
  TrainMixArgs a{};
  a.energy = d_energy;
  a.rms_out = d_rms;
  a.vad_out = d_vad;
  return mix_launch(rn_train_levels, a, b, d_speech, d_noise, d_fgnoise, speech_len, noise_len, fgnoise_len, mix, n_frames, hip_stream,
                    true, start_pos);
}

extern "C" int rnnoise_batch_train_mix_device(RNNoiseBatch *b, float *d_clean, float *d_noisy, float *d_vad_target, int *d_noise_free,
                                              const short *d_speech, const short *d_noise, const short *d_fgnoise, long long speech_len,
                                              long long noise_len, long long fgnoise_len, const RNNoiseTrainMix *mix, const float *d_rms,
                                              const unsigned char *d_vad, int n_frames, void *hip_stream) {
  if (!b || !d_clean || !d_noisy || !d_vad_target || !d_noise_free || !d_speech || !d_noise || !d_fgnoise || !mix || !d_rms || !d_vad ||
      n_frames < 1)
    return -1;
  if (train_split_busy(b)) return -1;  // (frames of a split call are pending: include/rnnoise_amd.h)
  if (!aligned16(d_clean) || !aligned16(d_noisy)) return -1;  // (stored as float4)
  TrainMixArgs a{};
  a.clean = d_clean;
  a.noisy = d_noisy;
  a.vad_target = d_vad_target;
  a.noise_free = d_noise_free;
  a.rms = d_rms;
  a.vad = d_vad;
  return mix_launch(rn_train_mix, a, b, d_speech, d_noise, d_fgnoise, speech_len, noise_len, fgnoise_len, mix, n_frames, hip_stream);
}
