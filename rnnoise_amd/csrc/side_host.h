// side_host.h -- what the host halves of the side libraries (score/, train/, gru/, gru_stack/, stoi/) have in common: the argument
// checks on slots and buffers, and the device guard of their *_device calls.  Plain C++; every library still compiles it into its own
// object.  The device part needs HIP's names, so it is there under hipcc and behind a test shim that supplies them (RN_SIDE_HIP_SHIM:
// tests/csrc/gru_stack_shim.h); the including unit says who speaks in the messages:
//   #define RN_SIDE_LIB "rnnoise_amd_gru"
// The product (shim.h, train_common.h) keeps copies of its own: it is frozen by its surface tests and its HIP_OK is another macro.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

namespace {
// whether n_frames x n_rows slots of M floats, slot (f, s) at f * frame_stride + s * row_stride, are disjoint in one of the two
// orders, move in whole pieces of `piece` floats (4: 16-byte reads; 1: any stride), and end within LONG_MAX floats
inline bool slots_fit(long frame_stride, long row_stride, long M, int n_rows, long long n_frames, long piece) {
  if (frame_stride <= 0 || row_stride <= 0 || frame_stride % piece || row_stride % piece) return false;
  if (n_frames <= 0) return true;
  const __int128 fs = frame_stride, rs = row_stride;
  if ((n_frames - 1) * fs + (n_rows - 1) * rs + M > (__int128)LONG_MAX) return false;
  const bool rows_in_frame = rs >= M && fs >= n_rows * rs;
  const bool frames_in_row = fs >= M && rs >= n_frames * fs;
  return rows_in_frame || frames_in_row;
}

// whether two sets of slots of M floats (each of which fits) are apart: their extents do not meet, or they have the same strides and
// lie side by side within the smaller stride (every slot pitch is at least that), as slices of a concatenation buffer do
inline bool slots_apart(const float *a, long afs, long ars, const float *b, long bfs, long brs, long M, int n_rows, long long n_frames) {
  if (n_frames <= 0) return true;
  const __int128 ua = (__int128)reinterpret_cast<uintptr_t>(a), ub = (__int128)reinterpret_cast<uintptr_t>(b);
  const __int128 ea = ((n_frames - 1) * (__int128)afs + (n_rows - 1) * (__int128)ars + M) * 4;
  const __int128 eb = ((n_frames - 1) * (__int128)bfs + (n_rows - 1) * (__int128)brs + M) * 4;
  if (ua + ea <= ub || ub + eb <= ua) return true;
  if (afs != bfs || ars != brs) return false;
  const __int128 d = (ua < ub ? ub - ua : ua - ub) / 4, inner = afs < ars ? afs : ars;
  return d >= M && d + M <= inner;
}

// whether two buffers of `bytes` bytes do not meet
inline bool buffers_apart(const void *a, const void *b, uintptr_t bytes) {
  const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
  return (ua < ub ? ub - ua : ua - ub) >= bytes;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

#if defined(__HIPCC__) || defined(RN_SIDE_HIP_SHIM)
#define HIP_OK(expr)                                                                                                  \
  do {                                                                                                                \
    hipError_t e_ = (expr);                                                                                           \
    if (e_ != hipSuccess) {                                                                                           \
      fprintf(stderr, "[" RN_SIDE_LIB "] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                                                      \
    }                                                                                                                 \
  } while (0)

namespace {
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (prev == device) || hipSetDevice(device) == hipSuccess;
    if (prev == device) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
}  // namespace
#define ON_DEVICE(dev)                                                                                     \
  DeviceGuard guard_(dev);                                                                                 \
  if (!guard_.ok) {                                                                                        \
    fprintf(stderr, "[" RN_SIDE_LIB "] cannot select HIP device %d (%s:%d)\n", (dev), __FILE__, __LINE__); \
    return -1;                                                                                             \
  }
#endif
