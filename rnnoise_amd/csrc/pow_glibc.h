// pow_glibc.h -- (double) pow and log exactly as the reference's host computes them, for the one use the Viterbi VAD of training-data
// generation makes of them (src/dump_features.c:199-254; include/rn_train_vad.h): GNU libc >= 2.28 on an x86-64 with FMA.
//
// Like log10, pow and log are not correctly rounded: which double comes out is a property of the libm in use, and the VAD rounds
// the results to float and compares them.  So the device evaluates THE HOST'S algorithm, operation for operation, as log10_glibc.h
// does -- every operation below is an IEEE double add, multiply or fused multiply-add, which gfx950 and x86 round identically:
//
//   pow(x, y) = e_pow.c (__pow, ARM's optimized routines): log_inline(x) -> hi + lo with the 128-entry __pow_log_data, then
//               exp_inline(y hi, y lo + the product's error) with the 128-entry __exp_data, in the build every AVX2 host selects
//               (sysdeps/x86_64/fpu/multiarch/e_pow-fma.c, __pow_fma: compiled with -mfma -mavx2, __FP_FAST_FMA defined, so the
//               source's own fma branches are taken AND the compiler fused a*b+c where the expression tree allows).  WHICH sums are
//               fused is taken from the machine code of libm.so.6 (GNU libc 2.35, Ubuntu 22.04), instruction by instruction -- the
//               comments give the x86 instruction each line restates.
//   log(x)    = rn_log_glibc_fma of log10_glibc.h as it is, with the special arguments of __log around it.
//
// RESTATED: the main path of __pow for a positive normal finite x and an ordinary y (|y log x| in [2^-54, 512): the VAD calls
// pow((double)((1.f - w) / w), 0.5) with a float w limited to [.1f, .9f], so x lies in [1/9, 9]), its path for a product below 2^-54
// (x = 1: 1.0 + y log x), and NaN in, NaN out.  NOT RESTATED: zero, subnormal, negative and infinite x, an infinite, NaN, zero, huge
// or tiny y, integer-y sign handling, overflow and underflow of the result -- rn_pow_glibc_fma must not be given such arguments.
//
// Pinned: tests/test_train_vad_cpu.py compiles this header for the host and compares it with the running libm over the VAD's whole
// domain (every float w of [.1f, .9f]; every float energy); the library's self-check (train_mix.hip) does a short sweep on first use
// and refuses the device VAD on a host whose libm is a different one; tests/test_train_vad_gpu.py sweeps the device code.
#pragma once
#include "log10_glibc.h"
#include "pow_glibc_data.h"

// log_inline of e_pow.c, FMA build: log(x) = hi + *tail for a positive normal finite x.  tab = {invc, logc, logctail} x 128
// (RN_POW_LOG_TAB_VALUES)
RN_HD double rn_pow_log_inline(uint64_t ix, double *tail, const double *tab) {
  const uint64_t tmp = ix - 0x3fe6955500000000ull;
  const int i = (int)((tmp >> 45) & 127);
  const int k = (int)((int64_t)tmp >> 52);
  const uint64_t iz = ix - (tmp & 0xfff0000000000000ull);
  const double z = rn_log_dbl(iz);
  const double kd = (double)k;                                                          // vcvtsi2sd
  const double invc = tab[3 * i], logc = tab[3 * i + 1], logctail = tab[3 * i + 2];
  const double t1 = __builtin_fma(kd, RN_POW_LN2HI, logc);                              // vfmadd213sd  k ln2hi + log c
  const double r = __builtin_fma(z, invc, -1.0);                                        // vfmadd132sd  z/c - 1
  const double ar = r * RN_POW_A0;                                                      // vmulsd
  const double lo1 = __builtin_fma(kd, RN_POW_LN2LO, logctail);                         // vfmadd213sd  k ln2lo + logctail
  const double p12 = __builtin_fma(r, RN_POW_A2, RN_POW_A1);                            // vfmadd213sd  A1 + r A2
  const double p34 = __builtin_fma(r, RN_POW_A4, RN_POW_A3);                            // vfmadd213sd  A3 + r A4
  const double t2 = r + t1;                                                             // vaddsd
  const double ar2 = r * ar;                                                            // vmulsd
  const double d12 = t1 - t2;                                                           // vsubsd
  const double ar3 = r * ar2;                                                           // vmulsd
  const double lo3 = __builtin_fma(ar, r, -ar2);                                        // vfmsub132sd  the product's error
  const double lo2 = d12 + r;                                                           // vaddsd
  const double p56 = __builtin_fma(r, RN_POW_A6, RN_POW_A5);                            // vfmadd132sd  A5 + r A6
  const double hi = t2 + ar2;                                                           // vaddsd
  const double dh = t2 - hi;                                                            // vsubsd
  const double p36 = __builtin_fma(p56, ar2, p34);                                      // vfmadd132sd
  const double lo4 = dh + ar2;                                                          // vaddsd
  const double p = __builtin_fma(ar2, p36, p12);                                        // vfmadd132sd
  double lo = lo1 + lo2;                                                                // vaddsd
  lo = lo + lo3;                                                                        // vaddsd
  lo = lo + lo4;                                                                        // vaddsd
  lo = __builtin_fma(ar3, p, lo);                                                       // vfmadd231sd
  const double y = hi + lo;                                                             // vaddsd
  const double dy = hi - y;                                                             // vsubsd
  *tail = dy + lo;                                                                      // vaddsd
  return y;
}

// __pow of e_pow.c, FMA build, on the domain named at the top.  log_tab = RN_POW_LOG_TAB_VALUES, exp_tab = RN_EXP_TAB_VALUES
RN_HD double rn_pow_glibc_fma(double x, double y, const double *log_tab, const uint64_t *exp_tab) {
  const uint64_t ix = rn_log_bits(x);
  if (2 * ix - 1 >= 0xffdfffffffffffffull) return x * x;  // NaN (and, not needed here, zero and Inf with y > 0)  vmulsd
  double lo;
  const double hi = rn_pow_log_inline(ix, &lo, log_tab);
  const double ehi = y * hi;                                                            // vmulsd
  const double ee = __builtin_fma(hi, y, -ehi);                                         // vfmsub132sd  the product's error
  const double elo = __builtin_fma(y, lo, ee);                                          // vfmadd132sd
  // exp_inline(ehi, elo, 0)
  const unsigned abstop = (unsigned)(rn_log_bits(ehi) >> 52) & 0x7ff;
  if (abstop < 0x3c9) return ehi + 1.0;  // |y log x| < 2^-54 (x = 1)                      vaddsd
  const double kd0 = __builtin_fma(ehi, RN_EXP_INVLN2N, RN_EXP_SHIFT);                  // vfmadd132sd  z + Shift, z never rounded
  const uint64_t ki = rn_log_bits(kd0);
  const double kd = kd0 - RN_EXP_SHIFT;                                                 // vsubsd
  const double r0 = __builtin_fma(kd, RN_EXP_NEGLN2HIN, ehi);                           // vfmadd231sd
  const double r1 = __builtin_fma(kd, RN_EXP_NEGLN2LON, r0);                            // vfmadd132sd
  const unsigned idx = 2 * (unsigned)(ki & 127);
  const uint64_t sbits = exp_tab[idx + 1] + (ki << 45);
  const double r = elo + r1;                                                            // vaddsd
  const double c23 = __builtin_fma(r, RN_EXP_C3, RN_EXP_C2);                            // vfmadd213sd  C2 + r C3
  const double tr = r + rn_log_dbl(exp_tab[idx]);                                       // vaddsd       tail + r
  const double r2 = r * r;                                                              // vmulsd
  const double c45 = __builtin_fma(r, RN_EXP_C5, RN_EXP_C4);                            // vfmadd132sd  C4 + r C5
  const double t = __builtin_fma(c23, r2, tr);                                          // vfmadd132sd
  const double r4 = r2 * r2;                                                            // vmulsd
  const double tmp = __builtin_fma(c45, r4, t);                                         // vfmadd132sd
  const double scale = rn_log_dbl(sbits);
  return __builtin_fma(tmp, scale, scale);                                              // vfmadd132sd  scale + scale tmp
}

// __log of e_log.c with its special arguments (the wrapper's domain handling folded in, as in rn_log10_glibc_fma): the VAD takes
// log(+0) = -Inf on digital silence.  A SUBNORMAL double is not restated: the VAD's arguments are floats widened to double, or
// 1e-15 + such a one -- a float subnormal is a normal double.  tab = RN_LOG_TAB_VALUES
RN_HD double rn_log_glibc_full(double x, const double *tab) {
  const uint64_t ix = rn_log_bits(x);
  if ((ix << 1) == 0) return -1.0 / 0.0;                        // log(+-0) = -1 / 0
  if (ix == 0x7ff0000000000000ull) return x;                    // log(Inf) = Inf
  if (ix >= 0x7ff0000000000000ull) return (x - x) / (x - x);    // negative, NaN: NaN
  return rn_log_glibc_fma(x, tab);
}
