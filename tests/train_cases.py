"""One set of streams for the tests of training-feature extraction (plain helper module: tests/test_train_cases_cpu.py checks what the
set covers, tests/test_train_features_gpu.py runs it, tests/test_train_features.py pins a part of it to the reference).

`cases()` is D = 97 distinct streams x T = 16 frames: per stream a clean and a noisy signal, a VAD target per frame, and the three
per-stream parameters of rnnoise_batch_train_features (include/rnnoise_amd.h).  The GPU tests lay a batch out as copies of it (stream i
takes case i mod D); D is prime, so the copies shift against the 64 streams of a wave of the pass-through high-pass kernel.

The categories (`Cases.labels`), each aimed at one rule of src/dump_features.c:466-491 on a TRAINING=1 build of src/denoise.c:
  pitch      test_gpu_parity.fuzz_pcm as the noisy signal (pitch 60 .. 767), a scaled copy plus a second fuzz stream as clean; band
             limits, band_lp and noise_free drawn per stream
  louder     noisy = 0.5 * clean: the clamp g > 1 -> 1 (dump_features.c:474) fires wherever a target is valid
  threshold  white noise around the TRAINING build's silence rule E < 0.1 (denoise.c:389,397), from below the inference build's 0.04
             up; the clean signal is loud, so that a frame that is not silent has valid targets
  empty      both signals band-limited: bands in which Ey < 5e-2 && Ex < 5e-2 (dump_features.c:476) beside valid ones in live frames
  zeros      exact-zero frames in clean only, in noisy only and in both, at and across the call boundaries the GPU tests use; one
             stream is zero throughout
  vad        wide-band signals with VAD targets 0, -0.0, 0.5 and 1 (the record passes them through; the rule is vad == 0 exactly,
             dump_features.c:477): streams in pairs that differ only in noise_free, and pairs that differ only in band_lp (32 / 16)
  recipe     make_case of tests/test_train_features.py

Every signal is a function of numpy's bit generators, +, * and rounding to integers only where a transcendental or a transform is
involved, so that every host regenerates the same bits (tests/golden/reference_pins.npz holds reference outputs for some of them).
No NaN or Inf anywhere: the poisoned-stream test writes its own.
"""
from __future__ import annotations

import functools
import os
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np

from rnnoise_amd import synth
from test_gpu_parity import fuzz_pcm
from test_train_features import make_case

D = 97                                    # distinct streams: prime
T = 16                                    # frames
STEP = 37                                 # a fixed permutation spreads the categories: position p holds stream (p * STEP) % D of _layout()
FREQ_SIZE, NB_BANDS, REC = 481, 32, 98
TARGETS = slice(65, 97)                   # the band-gain targets of a record; [64] is the pitch feature, [97] the VAD target

# sigma of the "threshold" streams, from a sweep on the oracle: white noise is silent in the inference build (E < 0.04) below about
# 0.45, silent in the TRAINING build (E < 0.1) in every frame up to 0.65 and in none but the first from 0.76; between, it flips
THRESHOLD_SIGMA = (0.30, 0.50, 0.60, 0.66, 0.68, 0.69, 0.70, 0.71, 0.72, 0.74, 0.78, 0.90)
# exact-zero frames [a, b) of (clean, noisy) per "zeros" stream.  A spectrum is zero when the frame and the one before it are; the
# runs start and end at the call boundaries 1, 7, 8 of the GPU tests' calls (1, 6, 1, 6) and (1, 7), and inside calls
_ZEROS = [
    ([(1, 4)], []),
    ([], [(1, 4), (7, 9)]),
    ([(0, 2), (6, 8)], [(0, 2), (6, 8)]),
    ([(2, 5)], [(3, 7)]),
    ([(7, 8), (10, 16)], [(4, 5), (8, 14)]),
    ([(0, T)], [(0, T)]),
]
# VAD targets of the "vad" streams, cycled from a stream-dependent start
_VADS = np.array([0.0, 1.0, 0.5, 0.0, -0.0, 1.0, 0.0, 0.5, 1.0], np.float32)


class Cases(NamedTuple):
    clean: np.ndarray        # (T, n, 480) float32
    noisy: np.ndarray        # (T, n, 480) float32
    vad: np.ndarray          # (T, n) float32
    lowpass: np.ndarray      # (n,) int32
    band_lp: np.ndarray      # (n,) int32
    noise_free: np.ndarray   # (n,) int32
    labels: tuple            # (n,) category names

    @property
    def n(self):
        return self.clean.shape[1]

    def args(self, frames=slice(None)):
        """the arguments of capi.Batch.train_features for these frames"""
        return self.clean[frames], self.noisy[frames], self.vad[frames], self.lowpass, self.band_lp, self.noise_free


def _frames(x):
    return np.asarray(x, np.float32).reshape(T, 480)


def _band_limited(rng, cutoff, sigma):
    """white noise of T frames with nothing from bin `cutoff` (of 481 per 960 samples) up, rounded to integers: in the bands above
    the cutoff only the rounding is left, about 3e-4 per bin"""
    n = T * 480
    X = np.fft.rfft(rng.standard_normal(n))
    X[int(cutoff * n / 960):] = 0
    x = np.fft.irfft(X, n)
    return _frames(np.rint(x * (sigma / x.std())))


def _layout() -> Cases:
    """the D streams category by category, before the permutation"""
    clean, noisy, vad, lp, blp, nf, labels = [], [], [], [], [], [], []

    def add(label, c, x, v=1.0, lowpass=FREQ_SIZE, band_lp=NB_BANDS, noise_free=0):
        clean.append(_frames(c)), noisy.append(_frames(x))
        vad.append(np.broadcast_to(np.asarray(v, np.float32), (T,)).copy())
        lp.append(lowpass), blp.append(band_lp), nf.append(noise_free), labels.append(label)

    rng = np.random.default_rng([D, T])
    # pitch: 36 streams
    a, b = fuzz_pcm(36, T, 11), fuzz_pcm(36, T, 12)
    for s in range(36):
        add("pitch", 0.7 * a[:, s] + 0.25 * b[:, s], a[:, s], v=(rng.random(T) < 0.7),
            lowpass=(FREQ_SIZE, int(rng.integers(1, FREQ_SIZE)))[s % 2], band_lp=int(rng.integers(0, NB_BANDS + 1)),
            noise_free=int(rng.integers(0, 2)))
    # louder: 8
    for s in range(8):
        c = synth.stream_pcm(40 + s, T).astype(np.float32) + 40.0 * rng.standard_normal(T * 480)
        add("louder", c, 0.5 * _frames(c))
    # threshold: 12
    for sigma in THRESHOLD_SIGMA:
        add("threshold", 30.0 * rng.standard_normal(T * 480), sigma * rng.standard_normal(T * 480))
    # empty: 8
    for s in range(8):
        c = _band_limited(rng, (40, 90, 150, 230)[s % 4], 300.0)
        x = c + _band_limited(rng, (25, 120, 60, 300)[s % 4], (100.0, 600.0)[s // 4])
        add("empty", c, x)
    # zeros: 6
    for zc, zx in _ZEROS:
        c = _frames(synth.stream_pcm(60 + len(clean), T).astype(np.float32) + 20.0 * rng.standard_normal(T * 480))
        x = c + _frames(200.0 * rng.standard_normal(T * 480))
        for a0, b0 in zc:
            c[a0:b0] = 0
        for a0, b0 in zx:
            x[a0:b0] = 0
        add("zeros", c, x, v=(np.arange(T) % 4 != 1), noise_free=len(clean) % 2)
    # vad: 11 pairs
    for p in range(11):
        c = _frames(synth.stream_pcm(80 + p, T).astype(np.float32) * 0.5 + 100.0 * rng.standard_normal(T * 480))
        x = c + _frames((150.0 + 100.0 * p) * rng.standard_normal(T * 480))
        v = _VADS[(np.arange(T) + p) % len(_VADS)]
        if p < 7:      # the pair differs in noise_free only
            add("vad", c, x, v, band_lp=(32, 31)[p % 2], noise_free=0)
            add("vad", c, x, v, band_lp=(32, 31)[p % 2], noise_free=1)
        else:          # the pair differs in band_lp only
            add("vad", c, x, v, band_lp=32, noise_free=p % 2)
            add("vad", c, x, v, band_lp=16, noise_free=p % 2)
    # recipe: 5, with the parameters of test_gpu_train_features_bit_exact
    rng6 = np.random.default_rng(6)
    for s, (l, bl, f) in enumerate([(481, 32, 0), (200, 24, 0), (481, 32, 1), (90, 16, 1), (300, 28, 0)]):
        c, x, v = make_case(s, T, rng6)
        add("recipe", c, x, v, l, bl, f)
    assert len(labels) == D and all(D % k for k in range(2, int(D ** 0.5) + 1))
    return Cases(np.stack(clean, 1), np.stack(noisy, 1), np.stack(vad, 1), np.array(lp, np.int32), np.array(blp, np.int32),
                 np.array(nf, np.int32), tuple(labels))


@functools.lru_cache(None)
def cases() -> Cases:
    """the D streams, read-only.  Neighbouring streams -- the lanes of one wave of the high-pass kernel -- are of different categories"""
    out = take(_layout(), (np.arange(D) * STEP) % D)
    assert np.isfinite(out.clean).all() and np.isfinite(out.noisy).all()
    for arr in out[:6]:
        arr.setflags(write=False)
    return out


def pairs(c: Cases, field: str):
    """(i, j) for every two "vad" streams that differ in `field` ("noise_free" or "band_lp") and in nothing else"""
    other = "band_lp" if field == "noise_free" else "noise_free"
    same = lambda i, j: (getattr(c, other)[i] == getattr(c, other)[j] and c.lowpass[i] == c.lowpass[j]
                         and all(a[:, i].tobytes() == a[:, j].tobytes() for a in (c.clean, c.noisy, c.vad)))
    v = [s for s in range(c.n) if c.labels[s] == "vad"]
    return [(i, j) for i in v for j in v if i < j and getattr(c, field)[i] != getattr(c, field)[j] and same(i, j)]


def take(c: Cases, idx, frames=slice(None), **params) -> Cases:
    """the streams idx of c (any order, repeats allowed) over `frames` as a batch; lowpass= / band_lp= / noise_free= replace the
    streams' own parameters"""
    idx = np.asarray(idx)
    p = {k: np.ascontiguousarray(params.get(k, getattr(c, k)[idx]), np.int32) for k in ("lowpass", "band_lp", "noise_free")}
    assert all(v.shape == idx.shape for v in p.values())
    return Cases(np.ascontiguousarray(c.clean[frames][:, idx]), np.ascontiguousarray(c.noisy[frames][:, idx]),
                 np.ascontiguousarray(c.vad[frames][:, idx]), p["lowpass"], p["band_lp"], p["noise_free"],
                 tuple(c.labels[i] for i in idx))


def cycled(n, frames=slice(None), **params) -> Cases:
    """a batch of n streams: stream i takes case i mod D"""
    return take(cases(), np.arange(n) % D, frames, **params)


def oracle_records(c: Cases) -> np.ndarray:
    """(T, n, 98): one oracle.binding.TrainOracle per stream over all frames of c, several streams at a time (the oracle's C calls
    release the GIL)"""
    from oracle.binding import TrainOracle
    Tn = c.clean.shape[0]

    def one(s):
        o = TrainOracle()
        return np.stack([o.frame(c.clean[t, s], c.noisy[t, s], int(c.lowpass[s]), int(c.band_lp[s]), float(c.vad[t, s]),
                                 int(c.noise_free[s])) for t in range(Tn)])

    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(workers) as pool:
        return np.stack(list(pool.map(one, range(c.n))), axis=1)


# ---- the part of the set that tests/golden/reference_pins.npz pins to the reference (tests/golden/make_golden.py --pins) ----
EDGE_LOWPASS = (0, 1, 63, 64, 65, 480, 481, 482, 3006)   # 3006: the largest value src/dump_features.c:400 can draw
EDGE_BAND_LP = (0, 15, 31, 32, 33)


def edge_subset() -> Cases:
    """14 streams: the first and the second stream of every category, with the band limits of EDGE_LOWPASS and EDGE_BAND_LP going
    round and noise_free alternating"""
    c = cases()
    kinds = list(dict.fromkeys(c.labels))
    idx = [[s for s in range(c.n) if c.labels[s] == k][r] for r in (0, 1) for k in kinds]
    i = np.arange(len(idx))
    return take(c, idx, lowpass=np.array(EDGE_LOWPASS)[i % len(EDGE_LOWPASS)], band_lp=np.array(EDGE_BAND_LP)[i % len(EDGE_BAND_LP)],
                noise_free=(i // 2) % 2)
