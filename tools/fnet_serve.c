/* fnet_serve.c -- serving a float network from C: rnnoise_batch_analyze_device -> rnnoise_amd_fnet_process_device ->
 * rnnoise_batch_synthesize_device on one stream, against include/rnnoise_amd.h and include/rnnoise_amd_fnet.h alone (and HIP's C
 * API for the memory).  The DSP's batch is built on a weight blob (argv[1]); the float network's tensors would come from the
 * trainer's checkpoint -- here they are small pseudo-random numbers, so that the example stands alone.  INTEGRATION.md section 2.
 *
 *   cc tools/fnet_serve.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lrnnoise_amd -lrnnoise_amd -lrnnoise_amd_fnet \
 *      -L/opt/rocm/lib -lamdhip64 -lm -o fnet_serve && ./fnet_serve weights_blob.bin */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "rnnoise_amd.h"
#include "rnnoise_amd_fnet.h"

enum { N = 3, T = 8, CALLS = 2, COND = 16, GRU = 16, FRAME = 480 };

static unsigned lcg = 12345u;
static float *tensor(size_t n, float scale) { /* n floats in [-scale, scale) */
  float *p = (float *)malloc(n * sizeof(float));
  for (size_t i = 0; p && i < n; i++) lcg = lcg * 1664525u + 1013904223u, p[i] = scale * ((float)(lcg >> 8) / 8388608.f - 1.f);
  return p;
}

#define OK(expr)                                             \
  do {                                                       \
    if (!(expr)) {                                           \
      fprintf(stderr, "fnet_serve: %s failed\n", #expr);     \
      return 1;                                              \
    }                                                        \
  } while (0)

int main(int argc, char **argv) {
  OK(argc == 2);
  RNNModel *model = rnnoise_model_from_filename(argv[1]);
  OK(model != NULL);
  RNNoiseBatch *batch = rnnoise_batch_create(model, N, 0);
  OK(batch != NULL);

  /* the trainer's state dict, in torch's layouts */
  RNNoiseFnetWeights w = {COND, GRU};
  w.conv1_weight = tensor(COND * 65 * 3, .1f), w.conv1_bias = tensor(COND, .1f);
  w.conv2_weight = tensor(GRU * COND * 3, .2f), w.conv2_bias = tensor(GRU, .1f);
  for (int l = 0; l < 3; l++) {
    w.gru_weight_ih[l] = tensor(3 * GRU * GRU, .25f), w.gru_weight_hh[l] = tensor(3 * GRU * GRU, .25f);
    w.gru_bias_ih[l] = tensor(3 * GRU, .1f), w.gru_bias_hh[l] = tensor(3 * GRU, .1f);
  }
  w.dense_out_weight = tensor(32 * 4 * GRU, .2f), w.dense_out_bias = tensor(32, .1f);
  w.vad_dense_weight = tensor(4 * GRU, .2f), w.vad_dense_bias = tensor(1, .1f);
  OK(rnnoise_amd_fnet_check(&w, N, T) == 0);
  printf("a runtime of %d rows holds %lld bytes on the device\n", N, rnnoise_amd_fnet_bytes(COND, GRU, N, T));
  RNNoiseFnet *net = rnnoise_amd_fnet_create(0, &w, N, T); /* uploads: the host tensors may go */
  OK(net != NULL);

  hipStream_t stream;
  float *d_pcm, *d_out, *d_feat, *d_gains, *d_vad;
  OK(hipStreamCreate(&stream) == hipSuccess);
  OK(hipMalloc((void **)&d_pcm, sizeof(float) * T * N * FRAME) == hipSuccess && hipMalloc((void **)&d_out, sizeof(float) * T * N * FRAME) == hipSuccess);
  OK(hipMalloc((void **)&d_feat, sizeof(float) * T * N * 65) == hipSuccess && hipMalloc((void **)&d_gains, sizeof(float) * T * N * 32) == hipSuccess);
  OK(hipMalloc((void **)&d_vad, sizeof(float) * T * N) == hipSuccess);
  OK(rnnoise_batch_split_reserve(batch, T) == 0);

  static float pcm[T][N][FRAME], out[T][N][FRAME], gains[T][N][32], vad[T][N];
  for (int call = 0; call < CALLS; call++) {
    for (int t = 0; t < T; t++) /* [frame][stream][480], int16-scaled: a tone per stream under some noise */
      for (int s = 0; s < N; s++)
        for (int i = 0; i < FRAME; i++) {
          lcg = lcg * 1664525u + 1013904223u;
          pcm[t][s][i] = 6000.f * sinf(.02f * (float)(s + 2) * (float)(((call * T + t) * FRAME) + i)) + (float)(lcg >> 20) - 2048.f;
        }
    OK(hipMemcpyAsync(d_pcm, pcm, sizeof pcm, hipMemcpyHostToDevice, stream) == hipSuccess);
    /* rows where they lie: NULL is [frame][stream][row] on both sides */
    OK(rnnoise_batch_analyze_device(batch, d_feat, NULL, NULL, d_pcm, T, stream) == 0);
    OK(rnnoise_amd_fnet_process_device(net, d_gains, NULL, d_vad, NULL, d_feat, NULL, T, stream) == 0);
    OK(rnnoise_batch_synthesize_device(batch, d_out, d_gains, NULL, d_vad, NULL, T, stream) == 0);
    OK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, stream) == hipSuccess);
    OK(hipMemcpyAsync(gains, d_gains, sizeof gains, hipMemcpyDeviceToHost, stream) == hipSuccess);
    OK(hipMemcpyAsync(vad, d_vad, sizeof vad, hipMemcpyDeviceToHost, stream) == hipSuccess);
    OK(hipStreamSynchronize(stream) == hipSuccess);
    double peak = 0;
    for (int t = 0; t < T; t++)
      for (int s = 0; s < N; s++) {
        const int warm = t < RNNOISE_AMD_FNET_LOOKAHEAD && (call == 0 || s == 1); /* a row's first four frames: zeros */
        for (int b = 0; b < 32; b++) OK(warm ? gains[t][s][b] == 0.f : gains[t][s][b] > 0.f && gains[t][s][b] < 1.f);
        OK(warm ? vad[t][s] == 0.f : vad[t][s] > 0.f && vad[t][s] < 1.f);
        for (int i = 0; i < FRAME; i++) {
          OK(isfinite(out[t][s][i]));
          if (fabs(out[t][s][i]) > peak) peak = fabs(out[t][s][i]);
        }
      }
    printf("call %d: %d frames of %d streams, vad of stream 0 at the last frame %.4f, output peak %.1f\n", call, T, N, vad[T - 1][0], peak);
    if (call == 0) OK(rnnoise_amd_fnet_reset_rows(net, (const int[]){1}, 1) == 0); /* a call leg ends, another begins: row 1 alone */
  }
  rnnoise_amd_fnet_destroy(net);
  rnnoise_batch_destroy(batch);
  rnnoise_model_free(model);
  printf("ok\n");
  return 0;
}
