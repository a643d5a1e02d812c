"""The oracle of the RIR calls (tests/csrc/rir_oracle.c): built once per process (train_support.c_library), bound by ctypes.  TEST
INFRASTRUCTURE.  load() is load_rir from memory, filter() rir_filter_sequence for any number of frames; batch() applies a table of
capi.RIR_DTYPE records to frames in the layout of the device calls.  signal() and responses() are the seeded inputs the CPU and the
GPU tests share."""
import ctypes as C
import os

import numpy as np

from train_support import c_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "rir_oracle.c")
FRAME, NFFT, RIR_MAX = 480, 65536, 32768
BLOCK = NFFT // 2
# the lengths at which load_rir changes: one sample, around the early form's fade (480 .. 719) and its end, long, full
RIR_LENS = (1, 480, 481, 600, 719, 720, 721, 1500, 32768)
_lib = None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def lib():
    global _lib
    if _lib is None:
        L = c_library(SRC, flags=["-Wall"])
        fp = C.POINTER(C.c_float)
        L.riro_twiddles.argtypes = [fp]
        L.riro_bitrev.argtypes = [C.POINTER(C.c_int)]
        L.riro_fft.argtypes = [fp, fp, C.c_int]
        L.riro_load.argtypes = [fp, C.c_int, C.c_int, fp]
        L.riro_filter.argtypes = [fp, C.c_int, fp]
        L.riro_clip_quantize.argtypes = [fp, C.c_long, C.c_int, C.c_int]
        _lib = L
    return _lib


def twiddles():
    tw = np.empty((NFFT, 2), np.float32)
    lib().riro_twiddles(_fp(tw))
    return tw


def bitrev():
    r = np.empty(NFFT, np.int32)
    lib().riro_bitrev(r.ctypes.data_as(C.POINTER(C.c_int)))
    return r


def fft(x, inverse=False):
    """rnn_fft_c / rnn_ifft_c on (65536, 2) float32"""
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape == (NFFT, 2)
    y = np.empty_like(x)
    lib().riro_fft(_fp(x), _fp(y), int(inverse))
    return y


def load(rir, early):
    """load_rir of the samples of `rir` (at most 32768) -> (65536, 2)"""
    rir = np.ascontiguousarray(rir, np.float32)
    assert rir.ndim == 1 and 1 <= len(rir) <= RIR_MAX
    spec = np.empty((NFFT, 2), np.float32)
    lib().riro_load(_fp(rir), len(rir), int(early), _fp(spec))
    return spec


def spectra(rirs):
    """[whole, early] of every response: (n, 2, 65536, 2), the layout of rnnoise_batch_train_rir_load_device"""
    return np.stack([np.stack([load(r, 0), load(r, 1)]) for r in rirs])


def filter(audio, spec):
    """rir_filter_sequence on a copy of audio (480 * n_frames,)"""
    y = np.array(audio, np.float32).ravel()
    assert y.size % FRAME == 0
    spec = np.ascontiguousarray(spec, np.float32)
    lib().riro_filter(_fp(y), y.size // FRAME, _fp(spec))
    return y.reshape(np.shape(audio))


def clip_quantize(x, clip, quantize):
    y = np.array(x, np.float32)
    lib().riro_clip_quantize(_fp(y.reshape(-1)), y.size, int(clip), int(quantize))
    return y


def batch(clean, noisy, spec, table):
    """what rnnoise_batch_train_rir_device leaves in clean, noisy (T, n, 480) for spec = spectra(...) and a table of n records"""
    clean, noisy = np.array(clean, np.float32), np.array(noisy, np.float32)
    for s, rec in enumerate(table):
        if rec["rir_id"] >= 0:
            clean[:, s] = filter(clean[:, s], spec[rec["rir_id"], 1])
            noisy[:, s] = filter(noisy[:, s], spec[rec["rir_id"], 0])
        noisy[:, s] = clip_quantize(noisy[:, s], rec["clip"], rec["quantize"])
    return clean, noisy


def response(length, seed, decay=None):
    """a room-like response: a direct path, then noise under an exponential decay (to 1e-3 at its end unless `decay` samples is given)"""
    rng = np.random.default_rng([*np.ravel(seed), length])
    t = np.arange(length)
    h = rng.standard_normal(length) * .2 * np.exp(-t / (decay or max(length / 6.9, 1)))
    h[0] = 1
    return h.astype(np.float32)


def denormal_tail_response():
    """full length and so quiet that load_rir's scaling by 1/65536 takes nearly all of its samples below the smallest normal float,
    1.18e-38, and hardly any to zero: a transform that flushes denormals gives another spectrum (tests/test_train_rir_cpu.py)"""
    h = (response(RIR_MAX, 99, decay=RIR_MAX / 9.2).astype(np.float64) * 1e-33).astype(np.float32)
    scaled = np.float32(1 / 65536) * h
    assert ((scaled != 0) & (np.abs(scaled) < 1.17e-38)).sum() > 32000 and (np.abs(h) > 1.2e-38).sum() > 20000
    return h


def responses():
    """the responses of RIR_LENS and the one with the denormal tail"""
    return [response(n, 7) for n in RIR_LENS] + [denormal_tail_response()]


def signal(n_frames, seed, level=3000.0):
    """n_frames of noise under a slow envelope with silences (not in the first five frames), around `level`"""
    rng = np.random.default_rng([*np.ravel(seed), n_frames])
    steps = rng.choice([0.0, .1, 1.0, 2.5], -(-n_frames // 5))
    steps[0] = 1.0
    env = np.repeat(steps, 5 * FRAME)[:n_frames * FRAME]
    return (rng.standard_normal(n_frames * FRAME) * env * level).astype(np.float32)
