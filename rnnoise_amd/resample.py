"""Polyphase resampling of the batch API's low-rate PCM (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate).

At R = 48000 / L (L = 2, 3, 6) a stream's low-rate samples are upsampled to 48 kHz in front of the denoiser and its 48 kHz
output is downsampled back to R behind it.  This module holds the filter of each L, which the library carries as
rnnoise_amd/csrc/rs_coeffs.h, and restates the two filters as a streaming CPU reference in plain float32 numpy.

  design     one linear-phase FIR per L of N = 48 L taps: a Kaiser-windowed sinc, beta = 0.1102 (75 - 8.7), cutoff 0.45 R,
             unit DC gain, rounded to float32 -> h[k].  The up filter's 48 taps of phase p: hup[p][k] = (float)(L (double)h[L k + p]).
  up         u[L q + p] = sum_{k=0..47} hup[p][k] x[q - k]                  (x = low-rate input, x[m < 0] = 0 after a reset)
  down       y[m] = sum_{k=0..N-1} h[k] v[L m + L - 1 - k]                   (v = 48 kHz output of the denoiser)
  arithmetic float32, every product and sum rounded; each sum is four partial sums a_j over k = j (mod 4), each in ascending k and
             starting from its first product, combined as (a0 + a1) + (a2 + a3).
  delay      up followed by down is a pure delay of DELAY = 47 low-rate samples.

32 kHz is the one rate that is no divisor of 48 kHz: 2:3 through a common 96 kHz grid, where the prototype (144 taps, cutoff 0.45 * 32 kHz
= 0.15 cycles per sample) is h of L = 3 as it stands.  Its code where an L is expected is RATE_32K = 32; frames are 320 samples.
  up         u[J] = sum_{k=0..47} hup3[p][k] x[q - k],  q = floor(2 J / 3), p = 2 J mod 3      (history: 47 samples at 32 kHz)
  down       y[m] = sum_{k=0..71} hd[e][k] v[n0 - k],  e = m & 1, n0 = (3 m + 2) >> 1, hd[e][k] = 2 h3[2 k + e]   (history: 70 at 48 kHz)
  delay      up followed by down is again a delay of 47 samples at 32 kHz, but not an exact one: the 2:1 step in the middle aliases at the
             stop-band level.

The table below is the committed one: `design()` recomputes it with this machine's libm, which may move a last bit, so nothing
regenerates it at build time.  `python -m rnnoise_amd.resample --header` prints the C header from the table.
"""
from __future__ import annotations

import sys

import numpy as np

RATE_32K = 32  # the code of 32 kHz wherever a divisor L is expected (include/rnnoise_amd.h: RNNOISE_AMD_RATE_32K)
RATES = {48000: 1, 32000: RATE_32K, 24000: 2, 16000: 3, 8000: 6}
TAPS_PER_PHASE = 48
DOWN32_TAPS = 72  # taps per phase of the 32 kHz down filter
DELAY = 47  # low-rate samples
UP_HIST = TAPS_PER_PHASE - 1  # low-rate samples of history per stream


def frame_samples(L: int) -> int:
    """samples per 10 ms frame at the rate of code L"""
    return 320 if L == RATE_32K else 480 // L


def down_hist(L: int) -> int:
    """48 kHz samples of down-filter history per stream (N - L; 70 at 32 kHz: y[0] reaches v[1 - 71])."""
    return DOWN32_TAPS - 2 if L == RATE_32K else TAPS_PER_PHASE * L - L


def design(L: int) -> np.ndarray:
    """The filter of ratio L recomputed in float64 and rounded to float32 (what the committed table was generated from)."""
    N = TAPS_PER_PHASE * L
    fc = 0.45 / L  # cutoff in cycles per 48 kHz sample
    n = np.arange(N, dtype=np.float64) - (N - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * n) * np.kaiser(N, 0.1102 * (75 - 8.7))
    return (h / h.sum()).astype(np.float32)


# the committed table: h[k] of each L as float32 hex floats
_H_HEX = {
    2: """
-0x1.cfcb5e0000000p-16 0x1.883a660000000p-17 0x1.3f032c0000000p-14 0x1.20a5000000000p-17
-0x1.3479400000000p-13 -0x1.44f3a40000000p-14 0x1.d90c100000000p-13 0x1.cdca0e0000000p-13
-0x1.232ab00000000p-12 -0x1.db72100000000p-12 0x1.0641a80000000p-12 0x1.9538480000000p-11
-0x1.3b2eca0000000p-14 -0x1.2b1aaa0000000p-10 -0x1.4c4be40000000p-12 0x1.83528e0000000p-10
0x1.00799c0000000p-10 -0x1.b293fe0000000p-10 -0x1.f762020000000p-10 0x1.8ec5cc0000000p-10
0x1.94b5680000000p-9 -0x1.d3b6760000000p-11 -0x1.1c74160000000p-8 -0x1.96c54e0000000p-12
0x1.64c3380000000p-8 0x1.3d22c00000000p-9 -0x1.8e15ba0000000p-8 -0x1.54fce80000000p-8
0x1.7ed8840000000p-8 0x1.19cfec0000000p-7 -0x1.1b6d3c0000000p-8 -0x1.9346da0000000p-7
0x1.23922c0000000p-10 0x1.03844a0000000p-6 0x1.10ce180000000p-8 -0x1.2f8f960000000p-6
-0x1.835c3c0000000p-7 0x1.3f5e400000000p-6 0x1.6bfea40000000p-6 -0x1.1f56de0000000p-6
-0x1.27038a0000000p-5 0x1.5f71d40000000p-7 0x1.c38fde0000000p-5 0x1.60c83e0000000p-8
-0x1.6399920000000p-4 -0x1.8b6a680000000p-5 0x1.714db20000000p-3 0x1.a736be0000000p-2
0x1.a736be0000000p-2 0x1.714db20000000p-3 -0x1.8b6a680000000p-5 -0x1.6399920000000p-4
0x1.60c83e0000000p-8 0x1.c38fde0000000p-5 0x1.5f71d40000000p-7 -0x1.27038a0000000p-5
-0x1.1f56de0000000p-6 0x1.6bfea40000000p-6 0x1.3f5e400000000p-6 -0x1.835c3c0000000p-7
-0x1.2f8f960000000p-6 0x1.10ce180000000p-8 0x1.03844a0000000p-6 0x1.23922c0000000p-10
-0x1.9346da0000000p-7 -0x1.1b6d3c0000000p-8 0x1.19cfec0000000p-7 0x1.7ed8840000000p-8
-0x1.54fce80000000p-8 -0x1.8e15ba0000000p-8 0x1.3d22c00000000p-9 0x1.64c3380000000p-8
-0x1.96c54e0000000p-12 -0x1.1c74160000000p-8 -0x1.d3b6760000000p-11 0x1.94b5680000000p-9
0x1.8ec5cc0000000p-10 -0x1.f762020000000p-10 -0x1.b293fe0000000p-10 0x1.00799c0000000p-10
0x1.83528e0000000p-10 -0x1.4c4be40000000p-12 -0x1.2b1aaa0000000p-10 -0x1.3b2eca0000000p-14
0x1.9538480000000p-11 0x1.0641a80000000p-12 -0x1.db72100000000p-12 -0x1.232ab00000000p-12
0x1.cdca0e0000000p-13 0x1.d90c100000000p-13 -0x1.44f3a40000000p-14 -0x1.3479400000000p-13
0x1.20a5000000000p-17 0x1.3f032c0000000p-14 0x1.883a660000000p-17 -0x1.cfcb5e0000000p-16
""",
    3: """
-0x1.49652e0000000p-16 -0x1.aff1760000000p-17 0x1.2556ec0000000p-16 0x1.a2ccce0000000p-15
0x1.7f954e0000000p-15 -0x1.a9ac940000000p-17 -0x1.75f6940000000p-14 -0x1.c74c4e0000000p-14
-0x1.80e36a0000000p-16 0x1.0337dc0000000p-13 0x1.abe6fc0000000p-13 0x1.cd5f560000000p-14
-0x1.0cbcfc0000000p-13 -0x1.527a540000000p-12 -0x1.1707540000000p-12 0x1.1ae36c0000000p-14
0x1.cb5ae00000000p-12 0x1.04cc9c0000000p-11 0x1.9e4d3a0000000p-14 -0x1.07c9100000000p-11
-0x1.9dc7700000000p-11 -0x1.a9cfaa0000000p-12 0x1.db3b700000000p-12 0x1.1fa9e20000000p-10
0x1.c9308e0000000p-11 -0x1.bff5820000000p-13 -0x1.604ca20000000p-10 -0x1.844c700000000p-10
-0x1.2beef60000000p-12 0x1.740ebc0000000p-10 0x1.1cb5960000000p-9 0x1.1e46ce0000000p-10
-0x1.389b640000000p-10 -0x1.72c08e0000000p-9 -0x1.20f9de0000000p-9 0x1.1608400000000p-11
0x1.ade54e0000000p-9 0x1.d2450c0000000p-9 0x1.62c7800000000p-11 -0x1.b1f2900000000p-9
-0x1.47c0ec0000000p-8 -0x1.4597380000000p-9 0x1.5f99340000000p-9 0x1.9cc7d00000000p-8
0x1.3ecc8a0000000p-8 -0x1.303cdc0000000p-10 -0x1.d3179a0000000p-8 -0x1.f796f40000000p-8
-0x1.7d54b60000000p-10 0x1.d0c0500000000p-8 0x1.5e39120000000p-7 0x1.5b9e9a0000000p-8
-0x1.77a8760000000p-8 -0x1.ba1b3a0000000p-7 -0x1.56f0da0000000p-7 0x1.496ae20000000p-9
0x1.fe4e9e0000000p-7 0x1.1659f80000000p-6 0x1.abf1920000000p-9 -0x1.09c1b20000000p-6
-0x1.9a0db80000000p-6 -0x1.a300ea0000000p-7 0x1.d55ac20000000p-7 0x1.20c4040000000p-5
0x1.d9a0b40000000p-6 -0x1.e824460000000p-8 -0x1.9e06160000000p-5 -0x1.fd68100000000p-5
-0x1.ce69ac0000000p-7 0x1.6f3dbc0000000p-4 0x1.ac9b2e0000000p-3 0x1.27e7d00000000p-2
0x1.27e7d00000000p-2 0x1.ac9b2e0000000p-3 0x1.6f3dbc0000000p-4 -0x1.ce69ac0000000p-7
-0x1.fd68100000000p-5 -0x1.9e06160000000p-5 -0x1.e824460000000p-8 0x1.d9a0b40000000p-6
0x1.20c4040000000p-5 0x1.d55ac20000000p-7 -0x1.a300ea0000000p-7 -0x1.9a0db80000000p-6
-0x1.09c1b20000000p-6 0x1.abf1920000000p-9 0x1.1659f80000000p-6 0x1.fe4e9e0000000p-7
0x1.496ae20000000p-9 -0x1.56f0da0000000p-7 -0x1.ba1b3a0000000p-7 -0x1.77a8760000000p-8
0x1.5b9e9a0000000p-8 0x1.5e39120000000p-7 0x1.d0c0500000000p-8 -0x1.7d54b60000000p-10
-0x1.f796f40000000p-8 -0x1.d3179a0000000p-8 -0x1.303cdc0000000p-10 0x1.3ecc8a0000000p-8
0x1.9cc7d00000000p-8 0x1.5f99340000000p-9 -0x1.4597380000000p-9 -0x1.47c0ec0000000p-8
-0x1.b1f2900000000p-9 0x1.62c7800000000p-11 0x1.d2450c0000000p-9 0x1.ade54e0000000p-9
0x1.1608400000000p-11 -0x1.20f9de0000000p-9 -0x1.72c08e0000000p-9 -0x1.389b640000000p-10
0x1.1e46ce0000000p-10 0x1.1cb5960000000p-9 0x1.740ebc0000000p-10 -0x1.2beef60000000p-12
-0x1.844c700000000p-10 -0x1.604ca20000000p-10 -0x1.bff5820000000p-13 0x1.c9308e0000000p-11
0x1.1fa9e20000000p-10 0x1.db3b700000000p-12 -0x1.a9cfaa0000000p-12 -0x1.9dc7700000000p-11
-0x1.07c9100000000p-11 0x1.9e4d3a0000000p-14 0x1.04cc9c0000000p-11 0x1.cb5ae00000000p-12
0x1.1ae36c0000000p-14 -0x1.1707540000000p-12 -0x1.527a540000000p-12 -0x1.0cbcfc0000000p-13
0x1.cd5f560000000p-14 0x1.abe6fc0000000p-13 0x1.0337dc0000000p-13 -0x1.80e36a0000000p-16
-0x1.c74c4e0000000p-14 -0x1.75f6940000000p-14 -0x1.a9ac940000000p-17 0x1.7f954e0000000p-15
0x1.a2ccce0000000p-15 0x1.2556ec0000000p-16 -0x1.aff1760000000p-17 -0x1.49652e0000000p-16
""",
    6: """
-0x1.4b50880000000p-17 -0x1.7137600000000p-17 -0x1.3386cc0000000p-17 -0x1.02d4f60000000p-18
0x1.2c05b20000000p-18 0x1.dfae9c0000000p-17 0x1.8553a60000000p-16 0x1.dc5b900000000p-16
0x1.cb68280000000p-16 0x1.3be1c60000000p-16 0x1.a7e3ec0000000p-19 -0x1.1f8a6e0000000p-16
-0x1.3cb0380000000p-15 -0x1.bf6ed00000000p-15 -0x1.ecd7920000000p-15 -0x1.a753320000000p-15
-0x1.d2c7900000000p-16 0x1.a2572c0000000p-18 0x1.7bb4a20000000p-15 0x1.5115240000000p-14
0x1.abf4680000000p-14 0x1.add5e00000000p-14 0x1.46e48e0000000p-14 0x1.fba1640000000p-16
-0x1.11b1860000000p-15 -0x1.99e6fe0000000p-14 -0x1.39755a0000000p-13 -0x1.6b25da0000000p-13
-0x1.4d06a60000000p-13 -0x1.b516780000000p-14 -0x1.18ce0a0000000p-16 0x1.6dcfa60000000p-14
0x1.83da5c0000000p-13 0x1.085c000000000p-12 0x1.19871a0000000p-12 0x1.d473340000000p-13
0x1.f527d80000000p-14 -0x1.b470540000000p-16 -0x1.8175760000000p-13 -0x1.4d65620000000p-12
-0x1.9ce2060000000p-12 -0x1.94f51c0000000p-12 -0x1.2d0b200000000p-12 -0x1.c966500000000p-14
0x1.e2fff60000000p-14 0x1.627b040000000p-12 0x1.09e1000000000p-11 0x1.2e56540000000p-11
0x1.1052a40000000p-11 0x1.5f46d00000000p-12 0x1.bbdd900000000p-15 -0x1.1c7bd40000000p-12
-0x1.28f3a80000000p-11 -0x1.8ebc460000000p-11 -0x1.a278700000000p-11 -0x1.5744740000000p-11
-0x1.6a3c380000000p-12 0x1.374c060000000p-14 0x1.0f6b3c0000000p-11 0x1.cfb2060000000p-11
0x1.1bab6a0000000p-10 0x1.12fa0c0000000p-10 0x1.94339a0000000p-11 0x1.2fb1220000000p-12
-0x1.3d44480000000p-12 -0x1.ccde660000000p-11 -0x1.56330c0000000p-10 -0x1.81531e0000000p-10
-0x1.57c89a0000000p-10 -0x1.b760fc0000000p-11 -0x1.131e620000000p-13 0x1.5d9bda0000000p-11
0x1.69deaa0000000p-10 0x1.e1f43e0000000p-10 0x1.f5d2e60000000p-10 0x1.9880860000000p-10
0x1.abe4c40000000p-11 -0x1.6d194a0000000p-13 -0x1.3c22700000000p-10 -0x1.0c3f740000000p-9
-0x1.4619f00000000p-9 -0x1.3a281c0000000p-9 -0x1.cb0d9c0000000p-10 -0x1.56f0700000000p-11
0x1.6450280000000p-11 0x1.0171ac0000000p-9 0x1.7c68420000000p-9 0x1.aa52380000000p-9
0x1.7aa7a20000000p-9 0x1.e1e5d40000000p-10 0x1.2c8a920000000p-12 -0x1.7c7e600000000p-10
-0x1.8879ec0000000p-9 -0x1.0486880000000p-8 -0x1.0e7a060000000p-8 -0x1.b732a20000000p-9
-0x1.caf8d80000000p-10 0x1.86d1d40000000p-12 0x1.51d2a00000000p-9 0x1.1e3fd60000000p-8
0x1.5b9d440000000p-8 0x1.4ea4380000000p-8 0x1.e8d0280000000p-9 0x1.6d2e680000000p-10
-0x1.7b95760000000p-10 -0x1.127d320000000p-8 -0x1.961d520000000p-8 -0x1.c7ed840000000p-8
-0x1.95dc020000000p-8 -0x1.02f9640000000p-8 -0x1.4418fe0000000p-11 0x1.9bec460000000p-9
0x1.aad4000000000p-8 0x1.1ccf500000000p-7 0x1.2973740000000p-7 0x1.e642360000000p-8
0x1.0001fc0000000p-8 -0x1.b7b4b80000000p-11 -0x1.7fb4b60000000p-8 -0x1.4896a60000000p-7
-0x1.93c2b20000000p-7 -0x1.89d1b00000000p-7 -0x1.23d87a0000000p-7 -0x1.bb2c840000000p-9
0x1.d502760000000p-9 0x1.5a01de0000000p-7 0x1.05bb180000000p-6 0x1.2d3b800000000p-6
0x1.13b7940000000p-6 0x1.6b05f20000000p-7 0x1.d693560000000p-10 -0x1.3730e80000000p-7
-0x1.5165040000000p-6 -0x1.da41180000000p-6 -0x1.06f4780000000p-5 -0x1.cd05500000000p-6
-0x1.07a5040000000p-6 0x1.f41b840000000p-9 0x1.ecf9b40000000p-6 0x1.ec6d620000000p-5
0x1.729d5c0000000p-4 0x1.e1529a0000000p-4 0x1.1a24cc0000000p-3 0x1.305a040000000p-3
0x1.305a040000000p-3 0x1.1a24cc0000000p-3 0x1.e1529a0000000p-4 0x1.729d5c0000000p-4
0x1.ec6d620000000p-5 0x1.ecf9b40000000p-6 0x1.f41b840000000p-9 -0x1.07a5040000000p-6
-0x1.cd05500000000p-6 -0x1.06f4780000000p-5 -0x1.da41180000000p-6 -0x1.5165040000000p-6
-0x1.3730e80000000p-7 0x1.d693560000000p-10 0x1.6b05f20000000p-7 0x1.13b7940000000p-6
0x1.2d3b800000000p-6 0x1.05bb180000000p-6 0x1.5a01de0000000p-7 0x1.d502760000000p-9
-0x1.bb2c840000000p-9 -0x1.23d87a0000000p-7 -0x1.89d1b00000000p-7 -0x1.93c2b20000000p-7
-0x1.4896a60000000p-7 -0x1.7fb4b60000000p-8 -0x1.b7b4b80000000p-11 0x1.0001fc0000000p-8
0x1.e642360000000p-8 0x1.2973740000000p-7 0x1.1ccf500000000p-7 0x1.aad4000000000p-8
0x1.9bec460000000p-9 -0x1.4418fe0000000p-11 -0x1.02f9640000000p-8 -0x1.95dc020000000p-8
-0x1.c7ed840000000p-8 -0x1.961d520000000p-8 -0x1.127d320000000p-8 -0x1.7b95760000000p-10
0x1.6d2e680000000p-10 0x1.e8d0280000000p-9 0x1.4ea4380000000p-8 0x1.5b9d440000000p-8
0x1.1e3fd60000000p-8 0x1.51d2a00000000p-9 0x1.86d1d40000000p-12 -0x1.caf8d80000000p-10
-0x1.b732a20000000p-9 -0x1.0e7a060000000p-8 -0x1.0486880000000p-8 -0x1.8879ec0000000p-9
-0x1.7c7e600000000p-10 0x1.2c8a920000000p-12 0x1.e1e5d40000000p-10 0x1.7aa7a20000000p-9
0x1.aa52380000000p-9 0x1.7c68420000000p-9 0x1.0171ac0000000p-9 0x1.6450280000000p-11
-0x1.56f0700000000p-11 -0x1.cb0d9c0000000p-10 -0x1.3a281c0000000p-9 -0x1.4619f00000000p-9
-0x1.0c3f740000000p-9 -0x1.3c22700000000p-10 -0x1.6d194a0000000p-13 0x1.abe4c40000000p-11
0x1.9880860000000p-10 0x1.f5d2e60000000p-10 0x1.e1f43e0000000p-10 0x1.69deaa0000000p-10
0x1.5d9bda0000000p-11 -0x1.131e620000000p-13 -0x1.b760fc0000000p-11 -0x1.57c89a0000000p-10
-0x1.81531e0000000p-10 -0x1.56330c0000000p-10 -0x1.ccde660000000p-11 -0x1.3d44480000000p-12
0x1.2fb1220000000p-12 0x1.94339a0000000p-11 0x1.12fa0c0000000p-10 0x1.1bab6a0000000p-10
0x1.cfb2060000000p-11 0x1.0f6b3c0000000p-11 0x1.374c060000000p-14 -0x1.6a3c380000000p-12
-0x1.5744740000000p-11 -0x1.a278700000000p-11 -0x1.8ebc460000000p-11 -0x1.28f3a80000000p-11
-0x1.1c7bd40000000p-12 0x1.bbdd900000000p-15 0x1.5f46d00000000p-12 0x1.1052a40000000p-11
0x1.2e56540000000p-11 0x1.09e1000000000p-11 0x1.627b040000000p-12 0x1.e2fff60000000p-14
-0x1.c966500000000p-14 -0x1.2d0b200000000p-12 -0x1.94f51c0000000p-12 -0x1.9ce2060000000p-12
-0x1.4d65620000000p-12 -0x1.8175760000000p-13 -0x1.b470540000000p-16 0x1.f527d80000000p-14
0x1.d473340000000p-13 0x1.19871a0000000p-12 0x1.085c000000000p-12 0x1.83da5c0000000p-13
0x1.6dcfa60000000p-14 -0x1.18ce0a0000000p-16 -0x1.b516780000000p-14 -0x1.4d06a60000000p-13
-0x1.6b25da0000000p-13 -0x1.39755a0000000p-13 -0x1.99e6fe0000000p-14 -0x1.11b1860000000p-15
0x1.fba1640000000p-16 0x1.46e48e0000000p-14 0x1.add5e00000000p-14 0x1.abf4680000000p-14
0x1.5115240000000p-14 0x1.7bb4a20000000p-15 0x1.a2572c0000000p-18 -0x1.d2c7900000000p-16
-0x1.a753320000000p-15 -0x1.ecd7920000000p-15 -0x1.bf6ed00000000p-15 -0x1.3cb0380000000p-15
-0x1.1f8a6e0000000p-16 0x1.a7e3ec0000000p-19 0x1.3be1c60000000p-16 0x1.cb68280000000p-16
0x1.dc5b900000000p-16 0x1.8553a60000000p-16 0x1.dfae9c0000000p-17 0x1.2c05b20000000p-18
-0x1.02d4f60000000p-18 -0x1.3386cc0000000p-17 -0x1.7137600000000p-17 -0x1.4b50880000000p-17
""",
}


def _parse(s: str) -> np.ndarray:
    return np.array([float.fromhex(t) for t in s.split()], dtype=np.float32)


_H = {L: _parse(s) for L, s in _H_HEX.items()}


def h(L: int) -> np.ndarray:
    """Down filter of ratio L (N = 48 L float32 taps)."""
    return _H[L].copy()


def hup(L: int) -> np.ndarray:
    """Up filter of ratio L: [L][48] float32, hup[p][k] = (float)(L * (double)h[L k + p])."""
    hh = _H[L].astype(np.float64)
    return np.array([[np.float32(L * hh[L * k + p]) for k in range(TAPS_PER_PHASE)] for p in range(L)], dtype=np.float32)


def hd32() -> np.ndarray:
    """Down filter of 32 kHz: [2][72] float32, hd[e][k] = 2 h3[2 k + e] (an exact doubling)."""
    return np.ascontiguousarray((np.float32(2) * _H[3]).reshape(DOWN32_TAPS, 2).T)


def _fir4(taps: np.ndarray, window) -> np.ndarray:
    """sum_k taps[k] * window(k) in the library's order: four float32 chains over k mod 4, then (a0 + a1) + (a2 + a3).
    window(k) returns the float32 operand vector of tap k (one entry per output)."""
    a = [None] * 4
    for k in range(len(taps)):
        prod = np.float32(taps[k]) * window(k)
        j = k & 3
        a[j] = prod if a[j] is None else (a[j] + prod).astype(np.float32)
    return ((a[0] + a[1]).astype(np.float32) + (a[2] + a[3]).astype(np.float32)).astype(np.float32)


class Up:
    """Streaming upsampler of one or more streams: frames of shape [..., M] at R in, [..., M * L] at 48 kHz out (L = RATE_32K: M a
    multiple of 2, [..., M * 3 / 2] out)."""

    def __init__(self, L: int, shape=()):
        self.L = L
        self.hist = np.zeros(tuple(shape) + (UP_HIST,), np.float32)
        self.taps = hup(3 if L == RATE_32K else L)

    def __call__(self, x: np.ndarray) -> np.ndarray:
        x = np.asarray(x, np.float32)
        M, L = x.shape[-1], self.L
        xs = np.concatenate([self.hist, x], axis=-1)  # xs[..., UP_HIST + q] = x[q]
        if L == RATE_32K:  # three outputs per two inputs: J = 3 i + r reads from q = 2 i + floor(2 r / 3) on, phase 2 r mod 3
            assert M % 2 == 0
            i = np.arange(M // 2)
            u = np.empty(x.shape[:-1] + (M // 2, 3), np.float32)
            for r in range(3):
                u[..., r] = _fir4(self.taps[2 * r % 3], lambda k: xs[..., UP_HIST + 2 * i + 2 * r // 3 - k])
            self.hist = xs[..., -UP_HIST:].copy()
            return u.reshape(x.shape[:-1] + (M // 2 * 3,))
        q = np.arange(M)
        u = np.empty(x.shape[:-1] + (M, L), np.float32)
        for p in range(L):
            u[..., p] = _fir4(self.taps[p], lambda k: xs[..., UP_HIST + q - k])
        self.hist = xs[..., -UP_HIST:].copy()
        return u.reshape(x.shape[:-1] + (M * L,))


class Down:
    """Streaming downsampler: frames [..., M * L] at 48 kHz in, [..., M] at R out (L = RATE_32K: a multiple of 3 in, two thirds out)."""

    def __init__(self, L: int, shape=()):
        self.L = L
        self.D = down_hist(L)
        self.hist = np.zeros(tuple(shape) + (self.D,), np.float32)
        self.taps = hd32() if L == RATE_32K else h(L)

    def __call__(self, v: np.ndarray) -> np.ndarray:
        v = np.asarray(v, np.float32)
        L, D = self.L, self.D
        vs = np.concatenate([self.hist, v], axis=-1)  # vs[..., D + n] = v[n]
        if L == RATE_32K:  # outputs m = 2 i + e: phase e from n0 = 3 i + 1 + e on
            assert v.shape[-1] % 3 == 0
            i = np.arange(v.shape[-1] // 3)
            y = np.empty(v.shape[:-1] + (len(i), 2), np.float32)
            for e in range(2):
                y[..., e] = _fir4(self.taps[e], lambda k: vs[..., D + 3 * i + 1 + e - k])
            self.hist = vs[..., -D:].copy()
            return y.reshape(v.shape[:-1] + (2 * len(i),))
        M = v.shape[-1] // L
        m = np.arange(M)
        y = _fir4(self.taps, lambda k: vs[..., D + L * m + L - 1 - k])
        self.hist = vs[..., -D:].copy()
        return y


def up(x: np.ndarray, L: int) -> np.ndarray:
    """Whole signal(s) [..., T] from a zero history -> [..., T * L]."""
    return Up(L, np.shape(x)[:-1])(x)


def down(v: np.ndarray, L: int) -> np.ndarray:
    """Whole signal(s) [..., T * L] from a zero history -> [..., T]."""
    return Down(L, np.shape(v)[:-1])(v)


def up32(x: np.ndarray) -> np.ndarray:
    """Whole signal(s) [..., T] at 32 kHz from a zero history -> [..., T * 3 / 2] at 48 kHz."""
    return up(x, RATE_32K)


def down32(v: np.ndarray) -> np.ndarray:
    """Whole signal(s) [..., T] at 48 kHz from a zero history -> [..., T * 2 / 3] at 32 kHz."""
    return down(v, RATE_32K)


def to_s16(y: np.ndarray) -> np.ndarray:
    """The library's float -> int16 output conversion (examples/rnnoise_demo.c:58 as x86 compiles it: cvttss2si, low 16 bits)."""
    y = np.asarray(y, np.float32)
    ok = (y >= -2147483648.0) & (y < 2147483648.0)
    q = np.where(ok, np.trunc(np.where(ok, y, 0)).astype(np.int64), -2147483648)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


def _hex(v: np.ndarray) -> list:
    return [float(x).hex() for x in np.asarray(v, np.float32)]


def header_text() -> str:
    """rnnoise_amd/csrc/rs_coeffs.h from the committed table."""
    out = ["// rs_coeffs.h -- GENERATED by `python -m rnnoise_amd.resample --header` from the table of rnnoise_amd/resample.py; do not edit.",
           "// The polyphase resampler of rnnoise_batch_set_pcm_rate (include/rnnoise_amd.h), per L = 48000 / R:",
           "//   rn_rs_h<L>[48 L]     down filter h[k]",
           "//   rn_rs_up<L>[L][48]   up filter, phase p: (float)(L * (double)h[L k + p])",
           "//   rn_rs_h_all[528]     rn_rs_h2, rn_rs_h3, rn_rs_h6 back to back",
           "//   rn_rs_hd32[2][72]    down filter of 32 kHz (2:3 over rn_rs_h3; its up filter is rn_rs_up3), phase e: 2 * h3[2 k + e]",
           "// RN_RS_CONST is defined by the includer (__constant__ in device code).",
           "#pragma once",
           "#ifndef RN_RS_CONST",
           "#define RN_RS_CONST static const",
           "#endif"]
    for L in (2, 3, 6):
        out.append(f"RN_RS_CONST float rn_rs_h{L}[{TAPS_PER_PHASE * L}] = {{")
        hx = _hex(_H[L])
        for i in range(0, len(hx), 6):
            out.append("    " + ", ".join(x + "f" for x in hx[i:i + 6]) + ",")
        out.append("};")
        out.append(f"RN_RS_CONST float rn_rs_up{L}[{L}][{TAPS_PER_PHASE}] = {{")
        for row in hup(L):
            hx = _hex(row)
            out.append("    {" + ", ".join(x + "f" for x in hx) + "},")
        out.append("};")
    # the three down filters once more, back to back (offsets 0, 96, 240): one base address for a kernel that picks L at run time
    out.append(f"RN_RS_CONST float rn_rs_h_all[{TAPS_PER_PHASE * 11}] = {{")
    hx = _hex(np.concatenate([_H[2], _H[3], _H[6]]))
    for i in range(0, len(hx), 6):
        out.append("    " + ", ".join(x + "f" for x in hx[i:i + 6]) + ",")
    out.append("};")
    out.append(f"RN_RS_CONST float rn_rs_hd32[2][{DOWN32_TAPS}] = {{")
    for row in hd32():
        out.append("    {" + ", ".join(x + "f" for x in _hex(row)) + "},")
    out.append("};")
    return "\n".join(out) + "\n"


def parse_header(text: str) -> dict:
    """{name: float32 array} of the arrays of a header as header_text() writes it."""
    import re
    arrays = {}
    for m in re.finditer(r"float (rn_rs_\w+)(?:\[\d+\])+ = \{(.*?)\};", text, re.S):
        vals = re.findall(r"(-?0x[0-9a-fA-F.]+p[-+]?\d+)f", m.group(2))
        arrays[m.group(1)] = np.array([float.fromhex(v) for v in vals], dtype=np.float32)
    return arrays


if __name__ == "__main__":
    if sys.argv[1:] == ["--header"]:
        sys.stdout.write(header_text())
    else:
        sys.exit("usage: python -m rnnoise_amd.resample --header")
