// gru_stack_shim.h -- what the host halves of rnnoise_amd/csrc/gru_stack/gru_stack.hip (RN_STK_HOST) and rnnoise_amd/csrc/gru/gru_seq.hip
// (RN_GRU_HOST) need to compile as plain C++ (TEST INFRASTRUCTURE; its own, beside tests/csrc/train_loss_shim.h): the few HIP names
// the device calls and rnnoise_amd/csrc/side_host.h's device guard use, and a launch that hands the kernel's argument block to the
// test program instead of a device.
#pragma once
#define RN_SIDE_HIP_SHIM 1

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void *hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0 };

static int g_shim_device = 0;  // two devices, 0 and 1
static inline hipError_t hipGetDevice(int *d) { return *d = g_shim_device, hipSuccess; }
static inline hipError_t hipSetDevice(int d) { return d < 0 || d > 1 ? 1 : (g_shim_device = d, hipSuccess); }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline const char *hipGetErrorString(hipError_t) { return "shim error"; }

struct RnStackStep;
struct RnStackGradStep;
struct RnGruStep;
struct RnGruGradStep;
// (defined in gru_stack_main.cpp, behind the units' own text)
static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t stream, const RnStackStep &a);
static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t stream, const RnStackGradStep &a);
static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t stream, const RnGruStep &a);
static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t stream, const RnGruGradStep &a);
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, arg) rn_stk_host_launch((grid), (block), (stream), (arg))
