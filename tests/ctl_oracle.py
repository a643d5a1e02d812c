"""The oracle of the per-stream suppression controls (tests/csrc/ctl_oracle.c: rno_process_frame_ctl): built once per process with the
flags of oracle/Makefile's liboracle.so (train_support.c_library), bound by ctypes.  TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

from oracle import binding
from oracle.binding import FRAME, NB_BANDS, STATE_FLOATS, Record
from train_support import c_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "ctl_oracle.c")
C_NONE = 65536  # the counter of a stream that has had no voice frame yet
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
        L.rno_model_free.argtypes = [C.c_void_p]
        L.rno_process_frame.restype = C.c_float
        L.rno_process_frame.argtypes = [C.c_void_p, fp, fp, fp, C.POINTER(Record)]
        L.rno_process_frame_ctl.restype = C.c_float
        L.rno_process_frame_ctl.argtypes = [C.c_void_p, fp, C.POINTER(C.c_int), C.c_float, C.c_float, C.c_float, fp, fp,
                                            C.POINTER(Record)]
        L.rno_set_rcp_profile.argtypes = [C.c_char_p]
        _lib = L
    # (a library of its own: its rcpps table follows the one the test put the oracle on)
    prof = binding.rcp_profile()
    _lib.rno_set_rcp_profile({"other": "host"}.get(prof, prof).encode())
    return _lib


class CtlOracle:
    """one stream: its DenoiseState and its counter; ctl = (floor, thr, hold) per frame, or None for the plain oracle"""

    def __init__(self, blob: bytes):
        self.L = lib()
        self._blob = blob
        self.model = self.L.rno_model_from_blob(blob, len(blob))
        assert self.model, "oracle: blob rejected"
        self.state = np.zeros(STATE_FLOATS, np.float32)
        self.c = C_NONE

    def __del__(self):
        if getattr(self, "model", None):
            self.L.rno_model_free(self.model)
            self.model = None

    def reset(self):
        self.state[:] = 0
        self.c = C_NONE

    def process(self, frame, ctl=None):
        frame = np.ascontiguousarray(frame, np.float32)
        out = np.zeros(FRAME, np.float32)
        rec = Record()
        if ctl is None:
            v = self.L.rno_process_frame(self.model, _fp(self.state), _fp(out), _fp(frame), C.byref(rec))
        else:
            c = C.c_int(self.c)
            v = self.L.rno_process_frame_ctl(self.model, _fp(self.state), C.byref(c), float(ctl[0]), float(ctl[1]), float(ctl[2]),
                                             _fp(out), _fp(frame), C.byref(rec))
            self.c = c.value
        return out, np.float32(v), np.frombuffer(rec.gains, np.float32).copy()

    def run(self, pcm, ctl=None):
        """pcm: (T, 480) -> dict(out (T, 480), vad (T,), gains (T, 32))"""
        T = pcm.shape[0]
        r = dict(out=np.zeros((T, FRAME), np.float32), vad=np.zeros(T, np.float32), gains=np.zeros((T, NB_BANDS), np.float32))
        for t in range(T):
            r["out"][t], r["vad"][t], r["gains"][t] = self.process(pcm[t], ctl)
        return r
