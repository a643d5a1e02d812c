// train_common.h -- what the two training units, train_mix.hip and train_rir.hip, share and nobody else includes: the upload into a
// batch-owned device buffer, the argument tests both repeat, and the device clip-and-quantise of the noisy signal.
//
// tests/csrc/hip_emul compiles both units as host C++ against a stand-in for shim.h and copies this file beside them: a HIP call that
// this file starts to use needs its counterpart there.
#pragma once
#include "shim.h"

// A table of a call on the device: into a buffer the batch owns (*slot, one of RNNoiseBatch's train_* members, `capacity` bytes
// allocated on first use and freed with the batch), a copy ordered on the call's stream.  `host` is pageable memory that may die as
// soon as the call returns (capi.py hands in temporaries, the units build tables on their stack): the HIP runtime makes a pageable
// host-to-device copy host-synchronous -- it returns when the copy has run, that is, when the stream has reached it -- and the calls
// rely on that and say so in the header.  The kernels that follow stay asynchronous.  One buffer per batch and purpose: two training
// calls of one kind on one batch have to share a stream, or they race on it (include/rnnoise_amd.h).
// A buffer that was allocated here and whose copy failed is freed again: the slot stays null, and the next call starts over.
inline int train_upload(void **slot, size_t capacity, const void *host, size_t bytes, hipStream_t st) {
  const bool fresh = !*slot;
  if (fresh) HIP_OK(hipMalloc(slot, capacity));
  const auto upload_copy = hipMemcpyAsync(*slot, host, bytes, hipMemcpyHostToDevice, st);
  if (upload_copy != 0 && fresh) {
    hipFree(*slot);
    *slot = nullptr;
  }
  HIP_OK(upload_copy);
  return 0;
}

// The training calls are refused while frames of a split call are pending (include/rnnoise_amd.h: "PENDING FRAMES"): the library's
// own test (shim.h: batch_split_busy).  The host emulation of tests/csrc/hip_emul, which is not compiled by hipcc, has a stand-in
// batch without split calls: nothing can be pending there.
#ifdef __HIPCC__
inline bool train_split_busy(const RNNoiseBatch *b) { return batch_split_busy(b); }
#else
inline bool train_split_busy(const RNNoiseBatch *) { return false; }
#endif

// clip and quantize of a record are flags: 0 or 1
inline bool train_flag01(int v) { return v == 0 || v == 1; }

// (buffers that the kernels move as float4 or float2 pairs)
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// MIN16(32767.f, MAX16(-32767.f, xn)) (src/dump_features.c:457), floor(.5f + xn) (:463)
__device__ __forceinline__ float clip_quantize(float t, int clip, int quantize) {
  if (clip) {
    t = -32767.f > t ? -32767.f : t;
    t = 32767.f < t ? 32767.f : t;
  }
  if (quantize) t = floorf(.5f + t);
  return t;
}
