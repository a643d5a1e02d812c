"""The oracle of the split calls (tests/csrc/split_oracle.c: rno_split_analyze, rno_split_synthesize): built once per process with the
flags of oracle/Makefile's liboracle.so (train_support.c_library), bound by ctypes.  TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

from oracle import binding
from oracle.binding import FRAME, NB_BANDS, NB_FEATURES, STATE_FLOATS
from train_support import c_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "split_oracle.c")
C_NONE = 65536  # the gate counter of a stream that has had no voice frame yet
_lib = None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def lib():
    global _lib
    if _lib is None:
        L = c_library(SRC, [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "rnnoise_amd", "csrc")], ["-mfma"])
        fp = C.POINTER(C.c_float)
        L.rno_model_from_blob.restype = C.c_void_p
        L.rno_model_from_blob.argtypes = [C.c_char_p, C.c_int]
        L.rno_compute_rnn.argtypes = [C.c_void_p] + [fp] * 4
        L.rno_split_analyze.argtypes = [fp, C.c_void_p, fp, fp]
        L.rno_split_synthesize.argtypes = [fp, C.c_void_p, C.POINTER(C.c_int), C.c_float, C.c_float, C.c_float, fp, fp, fp]
        L.rno_set_rcp_profile.argtypes = [C.c_char_p]
        _lib = L
    # (a library of its own: its rcpps table follows the one the test put the oracle on)
    prof = binding.rcp_profile()
    _lib.rno_set_rcp_profile({"other": "host"}.get(prof, prof).encode())
    return _lib


class SplitStream:
    """one stream's DenoiseState, gate counter and pending frames.  ctl: (floor, thr, hold) or None for no controls"""

    def __init__(self, ctl=None):
        self.L = lib()
        self.state = np.zeros(STATE_FLOATS, np.float32)
        self.c = C.c_int(C_NONE)
        self.ctl = (0.0, 0.0, 0.0) if ctl is None else tuple(float(v) for v in ctl)
        self.rec_bytes = self.L.rno_split_pending_bytes()
        self.pending = []

    def analyze(self, pcm):
        """pcm (T, 480) -> (features (T, 65), silence (T,)); the T frames stay pending"""
        pcm = np.ascontiguousarray(pcm, np.float32).reshape(-1, FRAME)
        feats = np.zeros((len(pcm), NB_FEATURES), np.float32)
        sil = np.zeros(len(pcm), np.int32)
        for t in range(len(pcm)):
            p = C.create_string_buffer(self.rec_bytes)
            sil[t] = self.L.rno_split_analyze(_fp(self.state), p, _fp(feats[t]), _fp(pcm[t]))
            self.pending.append(p)
        return feats, sil

    def synthesize(self, gains, vad):
        """gains (T, 32), vad (T,) for the T pending frames -> out (T, 480)"""
        gains = np.ascontiguousarray(gains, np.float32).reshape(-1, NB_BANDS)
        vad = np.ascontiguousarray(vad, np.float32).reshape(-1)
        assert len(gains) == len(vad) == len(self.pending)
        out = np.zeros((len(vad), FRAME), np.float32)
        for t, p in enumerate(self.pending):
            self.L.rno_split_synthesize(_fp(self.state), p, C.byref(self.c), *self.ctl, _fp(out[t]), _fp(gains[t]), _fp(vad[t:t + 1]))
        self.pending = []
        return out

    def run_with_model(self, blob, pcm, pair=1):
        """analyze -> the oracle's own compute_rnn on this state (not on silent frames) -> synthesize, `pair` frames at a time ->
        dict(out, vad, gains, features, silence) as Oracle.run gives them"""
        model = self.L.rno_model_from_blob(blob, len(blob))  # (never freed: a handful per process)
        assert model, "oracle: blob rejected"
        pcm = np.ascontiguousarray(pcm, np.float32).reshape(-1, FRAME)
        res = dict(out=[], vad=[], gains=[], features=[], silence=[])
        for t0 in range(0, len(pcm), pair):
            feats, sil = self.analyze(pcm[t0:t0 + pair])
            g, v = np.zeros((len(sil), NB_BANDS), np.float32), np.zeros(len(sil), np.float32)
            for t in range(len(sil)):
                if not sil[t]:
                    self.L.rno_compute_rnn(model, _fp(self.state), _fp(g[t]), _fp(v[t:t + 1]), _fp(feats[t]))
            out = self.synthesize(g, v)
            for k, a in (("out", out), ("vad", v), ("gains", g), ("features", feats), ("silence", sil)):
                res[k].append(a)
        return {k: np.concatenate(a) for k, a in res.items()}
