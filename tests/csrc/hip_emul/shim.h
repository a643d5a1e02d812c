// shim.h -- a host stand-in for rnnoise_amd/csrc/shim.h and the HIP runtime.  TEST INFRASTRUCTURE: tests/train_support.py
// (run_kernel_emul) copies a training unit -- rnnoise_amd/csrc/train_mix.hip or train_rir.hip -- and train_common.h next to this file
// and the unit's main (mix_main.cpp, rir_main.cpp) and compiles them as plain C++, so that the kernels' own source runs on the host:
// a workgroup is as many host threads as the launch asks for around a std::barrier, which run the workgroups of a grid one after the
// other; device memory is the heap.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <barrier>
#include <thread>
#include <vector>
#include "rnnoise_amd.h"
#define RN_FRAME_SIZE 480
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct Dim { unsigned x; };
static thread_local Dim threadIdx, blockIdx;
static std::barrier<> *g_bar;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline uint32_t __builtin_amdgcn_alignbit(uint32_t hi, uint32_t lo, unsigned sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31)); }
static inline unsigned __builtin_amdgcn_readfirstlane(unsigned v) { return v; }
using std::min;
struct float2 { float x, y; };
static inline float2 make_float2(float a, float b) { return {a, b}; }
struct alignas(16) float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
typedef void *hipStream_t;
struct dim3 { unsigned x; dim3(unsigned v) : x(v) {} };
struct RNNoiseBatch { int n, device; void *train_mix_buf = nullptr, *train_rir_tw = nullptr, *train_rir_buf = nullptr; };
#define ON_DEVICE(d)
#define HIP_OK(e) do { if (e) return -1; } while (0)
static inline int hipMalloc(void **p, size_t n) { *p = malloc(n); return 0; }
static inline int hipFree(void *p) { free(p); return 0; }
static inline int hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
#define hipMemcpyHostToDevice 0
static inline int hipGetLastError() { return 0; }
template <typename K, typename A>
static void emul_launch(K k, dim3 grid, dim3 block, A a) {
  std::barrier<> bar(block.x);
  g_bar = &bar;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < block.x; t++)
    th.emplace_back([=] {
      threadIdx.x = t;
      for (unsigned bl = 0; bl < grid.x; bl++) {  // (a kernel may return early: every thread of a block then does)
        blockIdx.x = bl;
        k(a);
        g_bar->arrive_and_wait();
      }
    });
  for (auto &x : th) x.join();
}
#define hipLaunchKernelGGL(k, grid, block, lds, st, a) emul_launch(k, grid, block, a)
