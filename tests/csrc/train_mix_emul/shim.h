// shim.h -- a host stand-in for rnnoise_amd/csrc/shim.h.  TEST INFRASTRUCTURE: tests/test_train_mix_cpu.py copies rnnoise_amd/csrc/train_mix.hip
// next to this file and main.cpp and compiles the three as plain C++, so that the kernels' own source runs on the host: a workgroup is
// 192 host threads around a std::barrier, one workgroup after the other; device memory is the heap.
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
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
using std::min;
static inline unsigned __builtin_amdgcn_readfirstlane(unsigned v) { return v; }
typedef void *hipStream_t;
struct dim3 { unsigned x; dim3(unsigned v) : x(v) {} };
struct RNNoiseBatch { int n, device; void *train_mix_buf = nullptr; };
#define ON_DEVICE(d)
#define HIP_OK(e) do { if (e) return -1; } while (0)
static inline int hipMalloc(void **p, size_t n) { *p = malloc(n); return 0; }
static inline int hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
#define hipMemcpyHostToDevice 0
static inline int hipGetLastError() { return 0; }
template <typename K, typename A>
static void emul_launch(K k, dim3 grid, dim3 block, A a) {
  for (unsigned bl = 0; bl < grid.x; bl++) {
    std::barrier<> bar(block.x);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = bl; k(a); });
    for (auto &x : th) x.join();
  }
}
#define hipLaunchKernelGGL(k, grid, block, lds, st, a) emul_launch(k, grid, block, a)
