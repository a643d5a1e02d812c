// g711.h -- the G.711 mappings of a companded stream's rows (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats), in the
// arithmetic form rnnoise_amd/g711.py defines them in: a handful of integer operations per sample inside K0's loads and K3's
// stores, floor(log2) a count of leading zeros, no table in LDS or constant memory.  Plain C++ in the host pass (no HIP in here), so
// that tests/csrc/g711_sweep.cpp runs the same text over all 65,536 inputs and all 256 codes without a GPU.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RN_G711_FN __host__ __device__ __forceinline__
#else
#define RN_G711_FN static inline
#endif

#define RN_PCM_LINEAR 0  // = RNNOISE_AMD_PCM_LINEAR: int16 rows
#define RN_PCM_ULAW 1    // = RNNOISE_AMD_PCM_ULAW
#define RN_PCM_ALAW 2    // = RNNOISE_AMD_PCM_ALAW

// x: an int16 value widened to int; the result is the byte
RN_G711_FN int rn_ulaw_encode(int x) {
  int p = x >> 2;
  const bool neg = p < 0;
  p = (neg ? -p : p) + 33;
  p = p < 8191 ? p : 8191;
  const int seg = 26 - __builtin_clz((unsigned)p);  // floor(log2(p)) - 5, p in [33, 8191]
  return ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF);
}
RN_G711_FN int rn_ulaw_decode(int b) {
  const int u = ~b & 0xFF;
  const int t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);
  return (u & 0x80) ? 132 - t : t - 132;
}
RN_G711_FN int rn_alaw_encode(int x) {
  int i = x >> 3;
  const bool neg = i < 0;
  i = neg ? ~i : i;
  const int seg = i < 32 ? 0 : 27 - __builtin_clz((unsigned)i);  // floor(log2(i)) - 4, i in [32, 4095]
  const int m = (i >> (seg < 2 ? 1 : seg)) & 15;
  return ((seg << 4) | m) ^ (neg ? 0x55 : 0xD5);
}
RN_G711_FN int rn_alaw_decode(int b) {
  const int a = (b & 0xFF) ^ 0x55;
  const int seg = (a >> 4) & 7;
  int t = (a & 15) << 4;
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
  return (a & 0x80) ? t : -t;
}
// fmt: RN_PCM_ULAW or RN_PCM_ALAW (the caller has dealt with linear rows)
RN_G711_FN int rn_g711_encode(int fmt, int x) { return fmt == RN_PCM_ULAW ? rn_ulaw_encode(x) : rn_alaw_encode(x); }
RN_G711_FN int rn_g711_decode(int fmt, int b) { return fmt == RN_PCM_ULAW ? rn_ulaw_decode(b) : rn_alaw_decode(b); }
