/* vad_libm_sweep.c -- test helper: rnnoise_amd/csrc/pow_glibc.h compiled for the host against the running libm, over the domains
 * the Viterbi VAD of training-data generation uses (include/rn_train_vad.h).  Built with -fopenmp; a range is split among threads.
 *   vad_libm_sweep <mode> [stride]     prints "<arguments> <mismatches> <first bad argument or 0>"
 *   mode pow:   pow(x, .5) for x = (double)((1.f - w) / w), EVERY float w of [.1f, .9f], and NaN
 *        loge:  log(1e-15 + (double)E) for every stride-th finite float E >= 0 (stride 1: all 2^31 - 2^23 of them)
 *        logf:  log((double)f) for every stride-th float f from +0 to +Inf: subnormals, zero and Inf (always) included
 *        spec:  the special arguments of log: +-0, Inf, NaN, negative */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../rnnoise_amd/csrc/pow_glibc.h"

static const double log_tab[256] = {RN_LOG_TAB_VALUES};
static const double pow_log_tab[384] = {RN_POW_LOG_TAB_VALUES};
static const uint64_t exp_tab[256] = {RN_EXP_TAB_VALUES};
static volatile double half = 0.5; /* (volatile: pow() stays the libm call, as in the reference's build) */

static int same(double a, double b) { return rn_log_bits(a) == rn_log_bits(b) || (a != a && b != b); }
static float f_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t u_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "pow";
  const long long stride = argc > 2 ? atoll(argv[2]) : 1;
  long long n = 0, bad = 0;
  uint32_t first = 0;
  if (!strcmp(mode, "pow")) {
    const uint32_t lo = u_of(.1f), hi = u_of(.9f);
    const double y = half;
#pragma omp parallel for reduction(+ : n, bad) reduction(max : first) schedule(static)
    for (long long u = lo; u <= (long long)hi + 1; u++) {
      const float w = u <= hi ? f_of((uint32_t)u) : f_of(0x7fc00000u);
      const double x = (double)((1.f - w) / w);
      n++;
      if (!same(rn_pow_glibc_fma(x, y, pow_log_tab, exp_tab), pow(x, y))) bad++, first = first > (uint32_t)u ? first : (uint32_t)u;
    }
  } else if (!strcmp(mode, "loge") || !strcmp(mode, "logf")) {
    const int e = mode[3] == 'e';
    const long long last = e ? 0x7f7fffffll : 0x7f800000ll;
#pragma omp parallel for reduction(+ : n, bad) reduction(max : first) schedule(static)
    for (long long k = 0; k <= last / stride + 1; k++) {
      const long long u = k * stride < last ? k * stride : last; /* (the last value of the range whatever the stride) */
      const double x = e ? 1e-15 + (double)f_of((uint32_t)u) : (double)f_of((uint32_t)u);
      n++;
      if (!same(rn_log_glibc_full(x, log_tab), log(x))) bad++, first = first > (uint32_t)u ? first : (uint32_t)u;
    }
  } else {
    const double xs[] = {0.0, -0.0, 1.0 / 0.0, -1.0 / 0.0, 0.0 / 0.0, -(0.0 / 0.0), -1.0, -0x1p-1060, 1.0, 0x1p-1022, 0x1.fffffffffffffp1023};
    for (unsigned i = 0; i < sizeof(xs) / sizeof(xs[0]); i++, n++) {
      volatile double x = xs[i];
      if (!same(rn_log_glibc_full(x, log_tab), log(x))) bad++, first = i + 1;
    }
  }
  printf("%lld %lld %#x\n", n, bad, first);
  return 0;
}
