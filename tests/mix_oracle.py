"""The oracle of the training-mix calls (tests/csrc/mix_oracle.c): built once per process (train_support.c_library), bound by
ctypes.  TEST INFRASTRUCTURE.  sequence() runs one sequence through levels, VAD and mix; batch() lays the sequences of a table out as
the device calls do."""
import ctypes as C
import os

import numpy as np

from rnnoise_amd import capi
from train_support import c_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "mix_oracle.c")
FRAME = 480
_lib = None


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def lib():
    global _lib
    if _lib is None:
        L = c_library(SRC, [os.path.join(ROOT, "include")], ["-Wall"])
        fp, ip, sp, up, vp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_short), C.POINTER(C.c_ubyte), C.c_void_p
        L.mixo_biquad.argtypes = [fp, fp, fp, fp, fp, C.c_int]
        L.mixo_weighted_rms.argtypes = [fp, C.c_int]
        L.mixo_weighted_rms.restype = C.c_float
        L.mixo_viterbi.argtypes = [fp, C.c_int, ip]
        L.mixo_clear_vad.argtypes = [fp, ip, C.c_int]
        L.mixo_levels.argtypes = [sp, sp, sp, vp, C.c_int, fp, fp]
        L.mixo_vad.argtypes = [fp, C.c_int, C.c_int, up]
        L.mixo_mix.argtypes = [sp, sp, sp, vp, fp, up, C.c_int, fp, fp, fp, ip]
        _lib = L
    return _lib


def biquad(x, b, a):
    """rnn_biquad from zero memory over the whole of x"""
    x = np.ascontiguousarray(x, np.float32)
    y, mem = np.empty_like(x), np.zeros(2, np.float32)
    b, a = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(a, np.float32)
    lib().mixo_biquad(_p(y, C.c_float), _p(mem, C.c_float), _p(x, C.c_float), _p(b, C.c_float), _p(a, C.c_float), len(x))
    return y


def weighted_rms(x):
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(lib().mixo_weighted_rms(_p(x, C.c_float), len(x)))


def viterbi(E):
    E = np.ascontiguousarray(E, np.float32)
    vad = np.zeros(len(E), np.int32)
    lib().mixo_viterbi(_p(E, C.c_float), len(E), _p(vad, C.c_int))
    return vad


def clear_vad(x, vad):
    x = np.array(x, np.float32)
    vad = np.ascontiguousarray(vad, np.int32)
    assert len(x) == FRAME * len(vad)
    lib().mixo_clear_vad(_p(x, C.c_float), _p(vad, C.c_int), len(vad))
    return x


def levels(corpora, rec, n_frames):
    """one sequence (rec: one capi.MIX_DTYPE record) -> energy (n_frames,), rms (3,)"""
    rec = np.ascontiguousarray(rec, capi.MIX_DTYPE).reshape(1)
    energy, rms = np.empty(n_frames, np.float32), np.empty(3, np.float32)
    lib().mixo_levels(*[_p(c, C.c_short) for c in corpora], rec.ctypes.data, n_frames, _p(energy, C.c_float), _p(rms, C.c_float))
    return energy, rms


def vad(energy, start_pos=0):
    energy = np.ascontiguousarray(energy, np.float32)
    v = np.empty(len(energy), np.uint8)
    lib().mixo_vad(_p(energy, C.c_float), len(energy), int(start_pos), _p(v, C.c_ubyte))
    return v


def mix(corpora, rec, rms, v, n_frames):
    """one sequence -> clean (n_frames, 480), noisy (n_frames, 480), vad_target (n_frames,), noise_free"""
    rec = np.ascontiguousarray(rec, capi.MIX_DTYPE).reshape(1)
    rms, v = np.ascontiguousarray(rms, np.float32), np.ascontiguousarray(v, np.uint8)
    clean, noisy = np.empty((n_frames, FRAME), np.float32), np.empty((n_frames, FRAME), np.float32)
    target, nf = np.empty(n_frames, np.float32), C.c_int(0)
    lib().mixo_mix(*[_p(c, C.c_short) for c in corpora], rec.ctypes.data, _p(rms, C.c_float), _p(v, C.c_ubyte), n_frames,
                   _p(clean, C.c_float), _p(noisy, C.c_float), _p(target, C.c_float), C.byref(nf))
    return clean, noisy, target, nf.value


def batch(corpora, table, n_frames, start_pos=None, vad_tracks=None):
    """every sequence of `table` through levels, VAD (or the given vad_tracks (n, n_frames)) and mix, in the layouts of the device
    calls: dict(energy (n, T), rms (n, 3), vad (n, T) uint8, clean / noisy (T, n, 480), vad_target (T, n), noise_free (n,) int32)"""
    n, T = len(table), n_frames
    corpora = [np.ascontiguousarray(c, np.int16) for c in corpora]
    r = dict(energy=np.empty((n, T), np.float32), rms=np.empty((n, 3), np.float32), vad=np.empty((n, T), np.uint8),
             clean=np.empty((T, n, FRAME), np.float32), noisy=np.empty((T, n, FRAME), np.float32),
             vad_target=np.empty((T, n), np.float32), noise_free=np.empty(n, np.int32))
    for s in range(n):
        r["energy"][s], r["rms"][s] = levels(corpora, table[s], T)
        r["vad"][s] = vad(r["energy"][s], 0 if start_pos is None else start_pos[s]) if vad_tracks is None else vad_tracks[s]
        r["clean"][:, s], r["noisy"][:, s], r["vad_target"][:, s], r["noise_free"][s] = mix(corpora, table[s], r["rms"][s], r["vad"][s], T)
    return r
