"""The oracle of linked gains (tests/csrc/link_oracle.c: rno_link_group_frame): built once per process with the flags of
oracle/Makefile's liboracle.so (train_support.c_library), bound by ctypes.  TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

from oracle import binding
from oracle.binding import FRAME, NB_BANDS, STATE_FLOATS, Record
from train_support import c_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "link_oracle.c")
C_NONE = 65536  # the counter of a stream that has had no voice frame yet
_lib = None
_models = {}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def lib():
    global _lib
    if _lib is None:
        L = c_library(SRC, [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "rnnoise_amd", "csrc")], ["-mfma"])
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.rno_model_from_blob.restype = C.c_void_p
        L.rno_model_from_blob.argtypes = [C.c_char_p, C.c_int]
        L.rno_model_free.argtypes = [C.c_void_p]
        L.rno_link_fold.argtypes = [C.c_int, fp, fp, fp, fp]
        L.rno_link_group_frame.argtypes = [C.c_int, C.POINTER(C.c_void_p), fp, ip, fp, ip, fp, fp, C.POINTER(Record), fp, fp, fp]
        L.rno_set_rcp_profile.argtypes = [C.c_char_p]
        _lib = L
    # (a library of its own: its rcpps table follows the one the test put the oracle on)
    prof = binding.rcp_profile()
    _lib.rno_set_rcp_profile({"other": "host"}.get(prof, prof).encode())
    return _lib


def fold(gains, vads):
    """the two folds over n participants in row order: gains (n, 32), vads (n,) -> (g_link (32,), vad_link)"""
    gains = np.ascontiguousarray(gains, np.float32).reshape(-1, NB_BANDS)
    vads = np.ascontiguousarray(vads, np.float32).reshape(-1)
    assert len(gains) == len(vads)
    g, v = np.zeros(NB_BANDS, np.float32), np.zeros(1, np.float32)
    lib().rno_link_fold(len(vads), _fp(gains), _fp(vads), _fp(g), _fp(v))
    return g, v[0]


class LinkGroup:
    """the K rows of one link group: their DenoiseStates and gate counters.  blobs: one model blob for every row, or one per row;
    ctl: (K, 3) = floor, thr, hold per row, or None for no controls"""

    def __init__(self, blobs, K, ctl=None):
        self.L, self.K = lib(), K
        blobs = [blobs] * K if isinstance(blobs, (bytes, bytearray)) else list(blobs)
        assert len(blobs) == K
        # (one parsed model per blob and process, never freed: a test builds hundreds of groups on two or three blobs)
        for b in blobs:
            if b not in _models:
                _models[b] = self.L.rno_model_from_blob(b, len(b))
                assert _models[b], "oracle: blob rejected"
        self.models = (C.c_void_p * K)(*[_models[b] for b in blobs])
        self.state = np.zeros((K, STATE_FLOATS), np.float32)
        self.c = np.full(K, C_NONE, np.int32)
        self.ctl = np.zeros((K, 3), np.float32) if ctl is None else np.ascontiguousarray(ctl, np.float32).reshape(K, 3)

    def process(self, frames, present=None):
        """frames (K, 480); present (K,) or None for all -> dict(out (K, 480), vad (K,), gains (K, 32) -- each row's own raw ones --,
        silence (K,), n: participants, g_link (32,), vad_link).  Rows that are absent keep out = 0 here and their state"""
        K = self.K
        frames = np.ascontiguousarray(frames, np.float32).reshape(K, FRAME)
        pres = np.ones(K, np.int32) if present is None else np.ascontiguousarray(np.asarray(present) != 0, np.int32).astype(np.int32)
        out = np.zeros((K, FRAME), np.float32)
        vad = np.zeros(K, np.float32)
        rec = (Record * K)()
        g_link, vad_link = np.zeros(NB_BANDS, np.float32), np.zeros(1, np.float32)
        n = self.L.rno_link_group_frame(K, self.models, _fp(self.state), _ip(self.c), _fp(self.ctl), _ip(pres), _fp(out), _fp(frames),
                                        rec, _fp(vad), _fp(g_link), _fp(vad_link))
        assert n >= 0
        gains = np.stack([np.frombuffer(rec[k].gains, np.float32).copy() for k in range(K)])
        silence = np.array([rec[k].silence if pres[k] else 2 for k in range(K)])
        features = np.stack([np.frombuffer(rec[k].features, np.float32).copy() for k in range(K)])
        pitch = np.array([rec[k].pitch for k in range(K)], np.int32)
        return dict(out=out, vad=vad, gains=gains, silence=silence, n=n, g_link=g_link, vad_link=vad_link[0], present=pres,
                    features=features, pitch=pitch)

    def reset_row(self, k, counter=True):
        """row k back to a new stream's state and gate counter (include/rnnoise_amd.h: rnnoise_batch_reset_streams); counter=False
        leaves the counter, which no reset of the product does"""
        self.state[k] = 0
        if counter:
            self.c[k] = C_NONE

    def run(self, pcm, active=None):
        """pcm (T, K, 480), active (T, K) or None -> dict of (T, ...) arrays of process()'s entries"""
        T = pcm.shape[0]
        rows = [self.process(pcm[t], None if active is None else active[t]) for t in range(T)]
        return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
